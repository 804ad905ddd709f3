/*
 * cudecomp_halo_fold.h -- halo folding: sum the ghost cells beyond the non-periodic edges of the domain into their mirror images.
 * An extension of the cuDecomp API a solver may use, accepted by this library only (cudecomp_amd.h, cudecomp_amd_fill.h and
 * cudecomp_amd_reflect.h have the others).
 *
 * The halo extensions come in pairs of a gather and its adjoint scatter: cudecompUpdateHalos{X,Y,Z} (neighbour -> ghost) has
 * cudecompAmdAccumulateHalos{X,Y,Z} (ghost -> owner, summed).  cudecompAmdReflectHalos{X,Y,Z} (cudecomp_amd_reflect.h) writes the
 * ghost cells at a non-periodic edge of the domain as the even or odd mirror image of the interior; the fold is ITS adjoint.  A
 * wall-bounded solver that scatters onto the grid (particle deposition, force spreading, adjoint stencils in a channel) folds
 * what has landed in the ghost cells beyond a wall back onto the mirror-image interior cells: with the same sign at a symmetry
 * plane, with the opposite sign at an odd wall.  The library knows the memory order, the halo widths, the padding and which ranks
 * sit on the domain's edge; the caller names the mirror.
 */
#ifndef CUDECOMP_HALO_FOLD_H
#define CUDECOMP_HALO_FOLD_H

#include "cudecomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which sides.  The sides folded are exactly the sides cudecompAmdReflectHalos{X,Y,Z} writes for the same grid_desc,
 * halo_extents, halo_periods, dim and padding: the low halo where cudecompGetShiftedRank gives NO low neighbour, the high halo
 * where it gives no high one.  Each slab spans the other two dims INCLUDING their halos and excludes padding.  With
 * halo_periods[dim] true, or on a rank away from the domain's edge, there is nothing to do and the call succeeds.
 *
 * Definition.  With h = halo_extents[dim], n = the pencil's extent along `dim` without padding, c = centering and s = parity,
 * for k in [0, h), the low side first, then the high side:
 *   low side:   cell(h + k + c)         += s * cell(h - 1 - k)
 *   high side:  cell(n - h - 1 - k - c) += s * cell(n - h + k)
 * along `dim`, at every position of the other two dims: the transpose of the reflection's two assignments.
 *
 * Parity.  s = -1: the addend is the ghost cell's bytes with the sign bit of every real component inverted, and it is ADDED.
 * The sign bit is flipped first, so nothing is ever subtracted and a ghost +0 contributes -0.
 *
 * Arithmetic.  As cudecomp_amd.h states it for the accumulation: the addition of the call's data type, binary16 for
 * CUDECOMP_AMD_HALF, for CUDECOMP_AMD_BFLOAT16 the round-to-nearest-even of the fp32 sum, complex types component-wise.  Which
 * NaN comes out of two NaNs is unspecified.
 *
 * Overlapping sides.  A cell that is a destination of both sides -- on a rank that is alone along the dim with n < 4 h + 2 c --
 * receives the low addend first, then the high one.  Results are bit-identical from run to run.
 *
 * clear.  With clear == 1 every ghost cell that was read holds zero bytes afterwards, written by the same launches.  With
 * clear == 0 the ghost cells are only read.
 *
 * Touches nothing else.  Only the destination cells named above change, and with clear == 1 the ghost cells read.  The halo of
 * the other side, padding, the cells between rows and everything beyond the pencil are neither read nor written: the kernels
 * never take a whole-line form.
 *
 * Local and asynchronous.  No workspace, no communication: the call is not collective, a rank may call it alone.  It is
 * enqueued on `stream`, never blocks the host on GPU work, and can be captured into a hipGraph.
 *
 * Validation.  An argument tuple that cudecompAmdReflectHalos* refuses is refused here with the same result code and kind of
 * CUDECOMP:ERROR message: what the fill refuses, a parity that is not +1 or -1 or a centering that is not 0 or 1 -- also when
 * h == 0 -- and a side that would be folded with h + centering > n - 2 h.  In addition, and checked after parity and centering, a
 * `clear` that is not 0 or 1 is CUDECOMP_RESULT_INVALID_USAGE.  Otherwise the call succeeds; without a usable device the result
 * is CUDECOMP_RESULT_CUDA_ERROR only when there are cells to fold.
 *
 * Sequences.  Within one dim the fold and the accumulation read disjoint sides' ghost cells, so they may be called in either
 * order; where their destinations coincide the two orders differ in rounding order only.  Calling (accumulation, fold) for dims
 * 2, 1, 0 in that order is the transpose of (update, reflection) for dims 0, 1, 2.  Let S be that forward sequence, applied to
 * an x that is zero outside the interior, and S^T the reverse one with clear == 0: then <S x, y> summed over all non-padding
 * cells equals <x, S^T y> summed over the interior cells.  A scatter loop calls (cudecompAmdAccumulateAndClearHalos*, fold with
 * clear == 1) for dims 2, 1, 0 and finds every ghost cell zero again.
 */
cudecompResult_t cudecompAmdFoldHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                       cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t clear,
                                       const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                       const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdFoldHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                       cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t clear,
                                       const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                       const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdFoldHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                       cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t clear,
                                       const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                       const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_HALO_FOLD_H */
