/*
 * cudecomp_amd_reflect.h -- halo reflection: mirror ghost cells at the non-periodic edges of the domain.  An extension of the
 * cuDecomp API a solver may use, accepted by this library only (cudecomp_amd.h and cudecomp_amd_fill.h have the others).
 *
 * cudecompUpdateHalos{X,Y,Z} writes the ghost cells that have a neighbour behind them; on a non-periodic edge of the domain it
 * writes nothing.  A wall-bounded solver (a channel flow: periodic in two directions, walls in the third) sets those cells from
 * its boundary condition.  The two conditions that are mirror images of the interior are served here: the even mirror (zero
 * gradient, symmetry planes) and the odd mirror (homogeneous Dirichlet for a cell-centred quantity, no-slip walls).  The library
 * knows the memory order, the halo widths, the padding and which ranks sit on the domain's edge; the caller names the mirror.
 * Per dim a solver calls the update and the reflection: together they write every ghost cell along that dim exactly once.
 */
#ifndef CUDECOMP_AMD_REFLECT_H
#define CUDECOMP_AMD_REFLECT_H

#include "cudecomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which cells.  With h = halo_extents[dim] and n = the pencil's extent along `dim` without padding: the low halo L = [0, h) is
 * written only where cudecompGetShiftedRank gives NO low neighbour, the high halo H = [n - h, n) only where it gives no high
 * neighbour (periodic wrap per halo_periods[dim]).  This is the exact complement, along `dim`, of the cells
 * cudecompAmdFillHalos{X,Y,Z} (cudecomp_amd_fill.h) names for the same grid_desc, halo_extents, halo_periods, dim and padding.
 * With halo_periods[dim] true, or on a rank away from the domain's edge, there is nothing to do and the call succeeds.  A rank
 * that is alone along a non-periodic dim writes both sides.  Each slab spans the other two dims INCLUDING their halos and
 * excludes padding, like the faces of the update.
 *
 * Definition.  With c = centering and s = parity, for k in [0, h):
 *   low side:   cell(h - 1 - k) = s * cell(h + k + c)
 *   high side:  cell(n - h + k) = s * cell(n - h - 1 - k - c)
 * along `dim`, at every position of the other two dims.  centering 0 mirrors about the face between the last ghost cell and the
 * first interior cell (cell-centred quantities; numpy.pad's "symmetric").  centering 1 mirrors about the first / last interior
 * cell itself (node-centred quantities; numpy.pad's "reflect").  parity +1 copies the bytes.  parity -1 copies them with the sign
 * bit of every real component inverted: one bit per real, two per complex element, for any of the four types of cudecomp.h and
 * the three of cudecomp_amd.h.  -0 becomes +0; NaN payloads and infinities keep every other bit.  Nothing is ever converted or
 * rounded.  `input` is aligned as its element type requires, the complex types as their real type; like the update, the call
 * does not check that.
 *
 * Sequences.  The source cells lie in the interior along `dim`, so within one dim the update and the reflection may be called
 * in either order.  Calling (update, reflection) for dims 0, 1, 2 in that order fills every ghost cell, edges and corners
 * included: a cell reached through r reflected dims carries s^r.
 *
 * Touches nothing else.  Only the named ghost cells are written and only their source cells are read.  Interior cells, the halo
 * of the other side, padding and everything beyond the pencil are neither read nor written: the kernels never take a whole-line
 * form that would rewrite the cells between rows.
 *
 * Local and asynchronous.  No workspace, no communication: the call is not collective, a rank may call it alone.  It is
 * enqueued on `stream`, never blocks the host on GPU work, and can be captured into a hipGraph.
 *
 * Validation.  An argument tuple that cudecompAmdFillHalos* refuses (its value aside) is refused here with the same result code
 * and kind of CUDECOMP:ERROR message.  A tuple the fill accepts is CUDECOMP_RESULT_INVALID_USAGE when parity is not +1 or -1 or
 * centering is not 0 or 1 -- also when h == 0 -- and when a side that would be written has h + centering > n - 2 h: the sources
 * would leave the rank's interior.  Otherwise the call succeeds; without a usable device the result is
 * CUDECOMP_RESULT_CUDA_ERROR only when there are cells to write.
 */
cudecompResult_t cudecompAmdReflectHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                          cudecompDataType_t dtype, int32_t parity, int32_t centering,
                                          const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                          const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdReflectHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                          cudecompDataType_t dtype, int32_t parity, int32_t centering,
                                          const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                          const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdReflectHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                          cudecompDataType_t dtype, int32_t parity, int32_t centering,
                                          const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                          const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_AMD_REFLECT_H */
