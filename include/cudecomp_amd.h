/*
 * cudecomp_amd.h -- extensions of the cuDecomp API a solver may use.
 *
 * cudecomp.h stays the drop-in boundary (exactly the reference's API); cudecomp_ext.h is for test harnesses and
 * tools.  What is declared here is accepted by this library only.
 *
 * 2-byte element types.  Every entry point that takes a cudecompDataType_t accepts these values in addition to the
 * four of cudecomp.h: cudecompGetDataTypeSize, the four transposes, the three halo updates and
 * cudecompGridDescAutotuneOptions_t::dtype.  Data movement is bit-exact: no value is ever converted, so NaN payloads,
 * -0, subnormals and infinities arrive exactly as they were sent.
 *
 * Halo accumulation (cudecompAmdAccumulateHalos{X,Y,Z}): the transpose of cudecompUpdateHalos{X,Y,Z} -- ghost cells are
 * summed back into the cells that own them; see the declarations below.
 *
 * The values are 1..3: the reference's enumerators are -1..-4, which makes [-4, 3] the range of values of the enum in
 * C++, so these are valid cudecompDataType_t values in C and C++ alike and cannot collide with the reference's.
 */
#ifndef CUDECOMP_AMD_H
#define CUDECOMP_AMD_H

#include "cudecomp.h"

#define CUDECOMP_AMD_HALF ((cudecompDataType_t)1)         /* IEEE binary16, 2 bytes */
#define CUDECOMP_AMD_BFLOAT16 ((cudecompDataType_t)2)     /* bfloat16, 2 bytes */
#define CUDECOMP_AMD_HALF_COMPLEX ((cudecompDataType_t)3) /* interleaved binary16 (re, im), 4 bytes */

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Halo accumulation: ghost -> owner with a sum, the transpose (adjoint) of cudecompUpdateHalos{X,Y,Z}.  For solvers that
 * SCATTER onto a decomposed grid (particle deposition, force spreading, assembly, adjoint stencils): a rank deposits into
 * its halo cells, and this adds those contributions into the interior cells of the ranks that own them.
 *
 * Arguments, NULL conventions, validation order, error codes and messages are those of cudecompUpdateHalos*; `work` is
 * sized by cudecompGetHaloWorkspaceSize; the transport is the descriptor's halo_comm_backend.  Collective, asynchronous on
 * `stream`, never blocks the host on GPU work, capturable into a hipGraph wherever cudecompUpdateHalos* is.
 *
 * Along `dim`, with h = halo_extents[dim] and n = the pencil's extent along `dim` without padding, a pencil has four slabs,
 * each spanning the other two dims INCLUDING their halos and excluding padding:
 *     low halo L = [0, h)    low face LF = [h, 2h)    high face HF = [n - 2h, n - h)    high halo H = [n - h, n).
 * cudecompUpdateHalos* does  L <- HF(low neighbour),  H <- LF(high neighbour).  Accumulation does
 *     LF += H(low neighbour)   then   HF += L(high neighbour),
 * in that order, element by element.  Neighbours are those of cudecompGetShiftedRank (periodic wrap per halo_periods[dim]);
 * on a non-periodic edge nothing is added on that side; a rank that is its own neighbour adds its own halos.
 *   - The halo cells along `dim` (L, H) and all padding cells are only READ: a call changes cells of LF and HF and nothing
 *     else.  (LF and HF span the other two dims with their halos, so they contain halo cells of the OTHER dims; those change
 *     too -- that is what carries edge and corner contributions from one call to the next.)
 *   - h == 0: success, nothing happens.  h larger than the rank's own interior extent along `dim` (LF / HF would reach
 *     into halo cells) or larger than a neighbour's: CUDECOMP_RESULT_INVALID_USAGE.  Empty pencils: not supported, as
 *     for the updates.  When LF and HF overlap (interior < 2h) the stated order still holds.
 *   - Calling dims 2, 1, 0 IN THAT ORDER folds edges and corners: afterwards interior cell g holds its old value plus the old
 *     values of every ghost cell, on any rank, that cudecompUpdateHalos* along 0, 1, 2 would fill from g.  With U the
 *     update along 0, 1, 2 and A the accumulation along 2, 1, 0:  <U x, y> over all cells == <x, A y> over interior cells
 *     for x zero outside the interior.
 *   - Arithmetic: CUDECOMP_FLOAT / CUDECOMP_DOUBLE IEEE addition; CUDECOMP_AMD_HALF IEEE binary16 addition (round to
 *     nearest even); CUDECOMP_AMD_BFLOAT16 round-to-nearest-even to bfloat16 of the fp32 sum of the two widened operands;
 *     the complex types add component-wise.  Subnormals are kept.  Which NaN comes out of a NaN operand is unspecified.
 *     A cell always receives its addends in the order above: results are deterministic and bit-identical run to run.
 * The halos are not zeroed afterwards; only sums; halos wider than a neighbour's slab are refused.
 */
cudecompResult_t cudecompAmdAccumulateHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                             void* work, cudecompDataType_t dtype, const int32_t halo_extents[],
                                             const bool halo_periods[], int32_t dim, const int32_t padding[],
                                             hipStream_t stream);
cudecompResult_t cudecompAmdAccumulateHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                             void* work, cudecompDataType_t dtype, const int32_t halo_extents[],
                                             const bool halo_periods[], int32_t dim, const int32_t padding[],
                                             hipStream_t stream);
cudecompResult_t cudecompAmdAccumulateHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                             void* work, cudecompDataType_t dtype, const int32_t halo_extents[],
                                             const bool halo_periods[], int32_t dim, const int32_t padding[],
                                             hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_AMD_H */
