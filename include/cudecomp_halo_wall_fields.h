/*
 * cudecomp_halo_wall_fields.h -- multi-field wall halos: the reflection and the fold of several pencils in one launch, each field
 * with a parity of its own.  An extension of the cuDecomp API a solver may use, accepted by this library only
 * (cudecomp_amd_reflect.h and cudecomp_halo_fold.h have the single calls; cudecomp_halo_fields.h and
 * cudecomp_halo_accumulate_fields.h the same idea for the exchanging halo calls).
 *
 * The wall is where the fields of one solver step differ most: at a no-slip wall the tangential velocities are odd (parity -1),
 * the pressure or a scalar at the same wall is even (parity +1).  A channel-flow step therefore makes one reflection per field per
 * wall-normal dim, a scatter step as many folds, and each of them is a launch of a few tens of microseconds that moves a slab a
 * few cells thick.  cudecompAmdReflectFieldHalos{X,Y,Z} and cudecompAmdFoldFieldHalos{X,Y,Z} take the list of fields and the list
 * of their parities and do all of them in one launch.
 */
#ifndef CUDECOMP_HALO_WALL_FIELDS_H
#define CUDECOMP_HALO_WALL_FIELDS_H

#include "cudecomp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most fields one call takes: a 256-byte table of pointers in the kernel arguments, one bit per field in the mask of signs */
#define CUDECOMP_AMD_MAX_HALO_WALL_FIELDS 32

/*
 * Arguments.  `inputs` is a HOST array of n_fields device pointers, each to a pencil of grid_desc along the axis in the function's
 * name; `parities` is a HOST array of n_fields values, each +1 or -1: entry f is the parity of field f.  Both arrays are read
 * before the call returns: they may be temporaries, and the call may be captured into a hipGraph.  All fields share dtype,
 * halo_extents, padding, `centering` and (fold) `clear`.  One centering per call is deliberate: it changes the offsets, the
 * refusals and the ordering rule, so a staggered solver groups its fields by centering.  The remaining arguments are those of
 * cudecompAmdReflectHalos{X,Y,Z} (cudecomp_amd_reflect.h) and cudecompAmdFoldHalos{X,Y,Z} (cudecomp_halo_fold.h).
 *
 * Result.  Afterwards every field f is byte for byte what the single call with parity = parities[f] and the same remaining
 * arguments would have made of it alone.  For the fold that includes its rule "flip the sign bits, then add in the type's
 * arithmetic", where the two sides add onto the same cells "the low addend first, then the high one", and with clear == 1 that
 * exactly the ghost cells that were read hold zero bytes afterwards.  Nothing else is read or written: no cells between rows, no
 * padding, no cell of a side the rank does not own an edge of.  All seven element types are accepted (the four of cudecomp.h and
 * the three of cudecomp_amd.h, whose values may be passed without including that header).
 *
 * Validation.  The order, result codes and CUDECOMP:ERROR messages of the single calls, with the lists checked where the single
 * calls check `input`: inputs == NULL, n_fields < 1 or > CUDECOMP_AMD_MAX_HALO_WALL_FIELDS, a NULL entry, two equal entries and
 * then parities == NULL are each CUDECOMP_RESULT_INVALID_USAGE, found on the host before anything is launched.  The entries of
 * `parities` are checked where the single calls check `parity` -- after what the halo fill refuses, before `centering` and
 * `clear`: any entry other than +1 or -1 is CUDECOMP_RESULT_INVALID_USAGE.  Every refusal of the single calls holds unchanged: a
 * `centering` other than 0 or 1, a `clear` other than 0 or 1, and halo_extents[dim] + centering > n - 2 * halo_extents[dim] on a
 * side that would be written (n: the rank's extent along `dim` with its halos).  Fields that overlap partly are the caller's error
 * and are not detected.  A call whose three halo_extents are all zero looks at `parities`, n_fields, the parities, `centering` and
 * `clear` only and succeeds; halo_extents[dim] == 0, a periodic dim and a rank away from the edges of the domain succeed, write
 * nothing and need no device.
 *
 * Local and asynchronous.  No exchange, no workspace, not collective: only the ranks at a non-periodic edge of the domain launch
 * anything.  The call is enqueued on `stream`.
 *
 * One field.  n_fields == 1 IS the single call with parities[0]: the same plan, kernels and launches.
 *
 * Two fields or more.  A reflection is ONE launch, also on a rank that writes both sides (their cells are disjoint).  A fold is
 * one launch -- one per side, the low side first, where a rank alone along `dim` has n < 4 * halo_extents[dim] + 2 * centering,
 * so that the two sides add onto the same cells.  The parities are no part of the cached plan: calls that differ only in them
 * share it.  The performance report does not sample these calls.
 */
cudecompResult_t cudecompAmdReflectFieldHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                               int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                               int32_t centering, const int32_t halo_extents[], const bool halo_periods[],
                                               int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdReflectFieldHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                               int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                               int32_t centering, const int32_t halo_extents[], const bool halo_periods[],
                                               int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdReflectFieldHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                               int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                               int32_t centering, const int32_t halo_extents[], const bool halo_periods[],
                                               int32_t dim, const int32_t padding[], hipStream_t stream);

cudecompResult_t cudecompAmdFoldFieldHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                            int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                            int32_t centering, int32_t clear, const int32_t halo_extents[],
                                            const bool halo_periods[], int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdFoldFieldHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                            int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                            int32_t centering, int32_t clear, const int32_t halo_extents[],
                                            const bool halo_periods[], int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdFoldFieldHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                            int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                            int32_t centering, int32_t clear, const int32_t halo_extents[],
                                            const bool halo_periods[], int32_t dim, const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_HALO_WALL_FIELDS_H */
