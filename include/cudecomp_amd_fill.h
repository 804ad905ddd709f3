/*
 * cudecomp_amd_fill.h -- halo fill: set the ghost cells a halo update would write.  An extension of the cuDecomp API a solver
 * may use, accepted by this library only (cudecomp_amd.h has the others).
 *
 * A solver that SCATTERS onto a decomposed grid runs, every time step:  clear the ghost cells -- deposit -- accumulate
 * (cudecompAmdAccumulateHalos{X,Y,Z}).  This is the first of the three.  The library knows which cells of a pencil are ghost
 * cells (memory order, halo widths, padding, which sides have a neighbour); the caller names a value.
 */
#ifndef CUDECOMP_AMD_FILL_H
#define CUDECOMP_AMD_FILL_H

#include "cudecomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which cells.  Exactly the cells cudecompUpdateHalos{X,Y,Z} would write when called with the same grid_desc, halo_extents,
 * halo_periods, dim and padding.  In the words of cudecomp_amd.h, with h = halo_extents[dim] and n = the pencil's extent along
 * `dim` without padding: the low halo L = [0, h) and the high halo H = [n - h, n) along `dim`, each slab spanning the other two
 * dims INCLUDING their halos and excluding padding.  A side is written only where cudecompGetShiftedRank gives a neighbour
 * (periodic wrap per halo_periods[dim]); a rank that is its own neighbour counts as having one; on a non-periodic edge of the
 * domain nothing is written on that side.  A caller who wants EVERY ghost cell set, those at physical boundaries included,
 * passes halo_periods all true.  Calling dims 0, 1 and 2 covers every ghost cell, edges and corners included; the order does
 * not matter.
 *
 * Value.  Every written cell receives the bytes of *value: one element of `dtype` (any of the four types of cudecomp.h and the
 * three of cudecomp_amd.h), read on the host before the call returns -- the caller may free or change it afterwards.
 * value == NULL means all-zero bytes (+0).  The bytes are stored as given, nothing is converted: NaN payloads, -0, infinities
 * and sentinels arrive as they are.  `input` is aligned as its element type requires, the complex types as their real type
 * (half the element); like the update, the call does not check that.
 *
 * Touches nothing else.  Every byte outside those cells -- interior cells, halo cells of the other side, padding, anything
 * beyond the pencil -- is neither written nor read, and the cells themselves are not read either: the kernels issue no loads
 * from the pencil, so the caller may write neighbouring cells from another stream meanwhile.
 *
 * Local and asynchronous.  No workspace, no communication: the call is not collective, a rank may call it alone.  It is
 * enqueued on `stream`, never blocks the host on GPU work, and can be captured into a hipGraph; the value travels in the
 * kernel arguments, so a captured call keeps the value it was captured with.
 *
 * Validation.  For any argument tuple the result code, the order of the checks and the kind of CUDECOMP:ERROR message are those
 * of cudecompUpdateHalos* for the same tuple with a non-NULL `work`: h == 0 is success with no effect, empty pencils are
 * CUDECOMP_RESULT_NOT_SUPPORTED, a halo wider than a neighbour's slab is refused as the update refuses it, and without a usable
 * device (and with cells to write) the result is CUDECOMP_RESULT_CUDA_ERROR.
 *
 */
cudecompResult_t cudecompAmdFillHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                       cudecompDataType_t dtype, const void* value, const int32_t halo_extents[],
                                       const bool halo_periods[], int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdFillHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                       cudecompDataType_t dtype, const void* value, const int32_t halo_extents[],
                                       const bool halo_periods[], int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdFillHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                       cudecompDataType_t dtype, const void* value, const int32_t halo_extents[],
                                       const bool halo_periods[], int32_t dim, const int32_t padding[], hipStream_t stream);

/*
 * Accumulate-and-clear: the second and the first part of the scatter step for the NEXT time step in one call -- ghost cells are
 * summed into their owners and left as zero bytes, in the launches of the accumulation.  The argument list is that of
 * cudecompAmdAccumulateHalos{X,Y,Z} (cudecomp_amd.h).
 *
 * Definition.  After the call every byte of the pencil -- interior, faces, both halos, padding and everything beyond -- is what it
 * would be after this sequence with the same arguments:
 *   1. cudecompAmdAccumulateHalos*(handle, grid_desc, input, work, dtype, halo_extents, halo_periods, dim, padding, stream);
 *   2. cudecompAmdFillHalos*(handle, grid_desc, input, dtype, NULL, halo_extents, halo_periods, dim, padding, stream).
 *
 * What is cleared.  The low halo L and the high halo H along `dim` (the slabs named above) end as all-zero bytes, on the sides
 * that have a neighbour; a rank that is its own neighbour counts as having one.  What is not cleared: a side on a non-periodic
 * edge of the domain is neither added nor cleared.
 *
 * Addend order.  That of accumulation: LF += H(low neighbour), then HF += L(high neighbour), LF and HF the low and high faces
 * of cudecomp_amd.h.  The sums are bit-identical to those of the two-call form.
 *
 * Sequences over dims.  Calling dims 2, 1, 0 leaves the whole pencil equal, byte for byte, to accumulation along 2, 1, 0
 * followed by fills (value NULL) along 0, 1, 2: a ghost cell cleared by an earlier call of the sequence is only ever added into
 * cells that are themselves cleared by the end, and adding +0 instead of the cell's value changes nothing that survives.  A
 * solver therefore clears once, before its first step, and never calls the fill again.
 *
 * Collective, workspace, transport, asynchrony.  Exactly those of cudecompAmdAccumulateHalos*: every rank of the communicator
 * along `dim` calls it, `work` is sized by cudecompGetHaloWorkspaceSize, the transport is the descriptor's halo_comm_backend, the
 * call is enqueued on `stream`, never blocks the host on GPU work and is capturable wherever accumulation is.  The contents of
 * `work` after the call are unspecified.
 *
 * Validation.  For any argument tuple the result code, the order of the checks and the kind of CUDECOMP:ERROR message are those
 * of cudecompAmdAccumulateHalos* for the same tuple.
 *
 * Touches nothing else.  Only cells of LF, HF, L and H are written: the kernels never take a whole-line form that would rewrite
 * the cells between rows.
 *
 * The three prototypes are in cudecomp_amd_accumulate_clear.h, which this header includes below: every extension keeps a header of
 * its own, so that the ones before it stay as they were.
 */
#ifdef __cplusplus
}
#endif

#include "cudecomp_amd_accumulate_clear.h"

#endif /* CUDECOMP_AMD_FILL_H */
