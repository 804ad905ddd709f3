/*
 * cudecomp_halo_accumulate_fields.h -- multi-field halo accumulation: several pencils in one exchange.  An extension of the cuDecomp
 * API a solver may use, accepted by this library only (cudecomp_halo_fields.h has the update side of the same idea; cudecomp_amd.h
 * and cudecomp_amd_fill.h have the single accumulation and its clearing form).
 *
 * The scatter half of a particle or immersed-boundary code never holds one field: a current deposit is Jx, Jy, Jz and usually
 * rho, a force spread is three components.  Accumulating their halos one by one pays a pack launch, an exchange and one or two
 * addition launches per field to send messages that are small already.  cudecompAmdAccumulateFieldHalos{X,Y,Z} takes the list of
 * fields, packs all their ghost slabs in one launch, sends ONE message per direction and adds what arrived in one launch.  The
 * clearing form is built in (`clear`), because a scatter loop zeroes its ghost cells every step.
 */
#ifndef CUDECOMP_HALO_ACCUMULATE_FIELDS_H
#define CUDECOMP_HALO_ACCUMULATE_FIELDS_H

#include "cudecomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most fields one call takes: a 256-byte table of pointers in the kernel arguments */
#define CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS 32

/*
 * Arguments.  `inputs` is a HOST array of n_fields device pointers, each to a pencil of grid_desc along the axis in the function's
 * name; all fields have the same dtype, halo_extents and padding.  The array is read before the call returns: it may be a
 * temporary, and the call may be captured into a hipGraph.  `clear` is 0 or 1.  The remaining arguments are those of
 * cudecompAmdAccumulateHalos{X,Y,Z} (cudecomp_amd.h).
 *
 * Result.  clear == 0: afterwards every field is byte for byte what cudecompAmdAccumulateHalos{X,Y,Z} with the same remaining
 * arguments would have made of it alone; the addend order stated in cudecomp_amd.h holds (low face += the low neighbour's high
 * halo, then high face += the high neighbour's low halo), also where the two faces overlap.  clear == 1: every field is byte for
 * byte the result of cudecompAmdAccumulateAndClearHalos{X,Y,Z} (cudecomp_amd_fill.h) on it alone: the ghost cells that were read
 * are zero bytes afterwards.  Every cell a single call leaves alone is untouched.  All seven element types are accepted (the four
 * of cudecomp.h and the three of cudecomp_amd.h, whose values may be passed without including that header).
 *
 * Workspace.  `work` holds n_fields x cudecompGetHaloWorkspaceSize(...) elements of dtype; there is no query of its own.  Cells of
 * `work` beyond what the plan uses are never touched.  The workspace rules of the descriptor's halo_comm_backend apply as they do
 * to the accumulation.
 *
 * Validation.  The order, result codes and CUDECOMP:ERROR messages of the accumulation, with the list checked where the
 * accumulation checks `input`: inputs == NULL, n_fields < 1 or > CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS, a NULL entry and two
 * equal entries are each CUDECOMP_RESULT_INVALID_USAGE, found on the host before anything is launched.  A `clear` other than 0 or
 * 1 is CUDECOMP_RESULT_INVALID_USAGE, checked right after halo_extents (also when every halo is zero).  Fields that overlap partly
 * are the caller's error and are not detected.  A call whose three halo_extents are all zero succeeds before the list is looked at;
 * halo_extents[dim] == 0 succeeds and does nothing; halos wider than the rank's own interior or a neighbour's slab and
 * decompositions with empty pencils are refused as the accumulation refuses them.
 *
 * Collective and asynchronous.  Every rank calls with the same n_fields and clear.  The call is enqueued on `stream`, travels over
 * the transport of the descriptor's halo_comm_backend and can be captured into a hipGraph wherever the accumulation can.
 *
 * One field.  n_fields == 1 IS the single call: the same plan, kernels and launches.
 *
 * Two fields or more.  One pack launch, one message of n_fields slabs per direction, one addition launch -- one per side, the low
 * side first, where the rank's interior along `dim` is narrower than two halos.  A rank that is its own neighbour on both sides
 * adds all fields' wraps in one launch (two in that narrow case) and exchanges nothing.  The performance report does not sample
 * these calls.
 */
cudecompResult_t cudecompAmdAccumulateFieldHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                  int32_t n_fields, void* work, cudecompDataType_t dtype,
                                                  const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                                  const int32_t padding[], int32_t clear, hipStream_t stream);
cudecompResult_t cudecompAmdAccumulateFieldHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                  int32_t n_fields, void* work, cudecompDataType_t dtype,
                                                  const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                                  const int32_t padding[], int32_t clear, hipStream_t stream);
cudecompResult_t cudecompAmdAccumulateFieldHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                                  int32_t n_fields, void* work, cudecompDataType_t dtype,
                                                  const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                                  const int32_t padding[], int32_t clear, hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_HALO_ACCUMULATE_FIELDS_H */
