/*
 * cudecomp_halo_wall_value_fields.h -- multi-field wall values: the affine wall ghosts (ghost = +-mirror + a) of several pencils in
 * one launch, each field with a parity and addends of its own.  An extension of the cuDecomp API a solver may use, accepted by this
 * library only (cudecomp_halo_wall_values.h has the single call and the definition; cudecomp_halo_wall_fields.h the same idea for
 * the homogeneous wall conditions, the reflection and the fold).
 *
 * A channel step with a moving wall, a heated wall or a prescribed flux sets the wall ghosts of u, v, w, p and T one after the
 * other: five launches of a few tens of microseconds that each move a slab a few cells thick.  The fields differ in parity (odd
 * velocities, even pressure at one wall) and in their data (the wall's velocity, its temperature, a flux).
 * cudecompAmdSetWallFieldHalos{X,Y,Z} takes the list of fields, the list of their parities and one vector of addends per field
 * and side.
 */
#ifndef CUDECOMP_HALO_WALL_VALUE_FIELDS_H
#define CUDECOMP_HALO_WALL_VALUE_FIELDS_H

#include "cudecomp_halo_wall_values.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most fields one call takes: a 256-byte table of pointers in the kernel arguments, one bit per field in the mask of signs */
#define CUDECOMP_AMD_MAX_WALL_VALUE_FIELDS 32

/*
 * Arguments.  `inputs` is a HOST array of n_fields device pointers, each to a pencil of grid_desc along the axis in the function's
 * name; `parities` is a HOST array of n_fields values, each +1 or -1: entry f is the parity of field f.  values_low and values_high
 * are HOST arrays, field-major: with h = halo_extents[dim] and nc = 1 for the real types, 2 for the complex ones (re, im), entry
 * (f * h + k) * nc + c is component c of the addend of ghost layer k of field f, k counted from the wall outward -- field f's part
 * is the array the single call takes.  All four arrays are read before the call returns: they may be temporaries, and the call may
 * be captured into a hipGraph (a replay applies the captured addends).  Each double is converted ONCE, on the host, by the single
 * call's rule: rounded to nearest even directly from the double, overflow to infinity.  The array of a side whose bit in `sides` is
 * clear is not looked at and may be NULL.
 *
 * All fields share dtype, halo_extents, padding, `centering` and `sides`.  One centering per call is deliberate: it changes the
 * offsets and the refusals, so a staggered solver groups its fields by centering.  One `sides` per call is deliberate too: it
 * decides which moves the plan holds and how many addends a launch carries; a solver whose walls carry different kinds of condition
 * makes one call per wall, as with the single call.  The remaining arguments are those of cudecompAmdSetWallHalos{X,Y,Z}.
 *
 * Result.  Afterwards every field f is byte for byte what cudecompAmdSetWallHalos* would have made of it alone, called with parity
 * = parities[f], field f's two addend vectors and the same remaining arguments -- with the single call's own exception: where the
 * resulting real is a NaN, any NaN of the type will do.  Flip first, add second.  Exactly the single call's cells are read and
 * written: no cells between rows, no padding, no side the rank does not own an edge of, no side whose bit is clear.  All seven
 * element types are accepted.
 *
 * Validation.  The order, result codes and CUDECOMP:ERROR messages of the existing calls, with the lists checked where the single
 * call checks `input`, as cudecompAmdReflectFieldHalos* does: inputs == NULL, n_fields < 1 or > CUDECOMP_AMD_MAX_WALL_VALUE_FIELDS,
 * a NULL entry, two equal entries and then parities == NULL are each CUDECOMP_RESULT_INVALID_USAGE.  The entries of `parities` are
 * checked where the single call checks `parity`.  Then, on every rank, in this order: `centering` other than 0 or 1
 * (INVALID_USAGE); `sides` outside 1 .. 3 (INVALID_USAGE); a NULL value array of a side named in `sides` (INVALID_USAGE);
 * halo_extents[dim] > CUDECOMP_AMD_MAX_WALL_HALO (CUDECOMP_RESULT_NOT_SUPPORTED).  Last, the reflection's refusal
 * halo_extents[dim] + centering > n - 2 * halo_extents[dim] (INVALID_USAGE) applies only to a side that would be written.  Fields
 * that overlap partly are the caller's error and are not detected.  halo_extents[dim] == 0, a periodic dim and a rank away from
 * the edges of the domain succeed, launch nothing and need no device.
 *
 * Local and asynchronous.  No exchange, no workspace, not collective.  The call is enqueued on `stream`, never blocks the host on
 * GPU work, and can be captured into a hipGraph.
 *
 * One field.  n_fields == 1 IS the single call with parities[0]: the same plan, kernels and launches.
 *
 * Two fields or more: the launch rule.  The addends travel in the kernel arguments, in a table of 2048 bytes that holds each
 * converted element once.  With S the sides this rank writes (1 or 2), h = halo_extents[dim] and es the element size in bytes, one
 * launch serves F = min(32, 2048 / (S * h * es)) consecutive fields, and the call makes ceil(n_fields / F) launches in field
 * order.  32 fp64 fields with h <= 2 at both walls are one launch; 32 complex128 fields with h = 8 at both walls are F = 8 and
 * four launches.  Parities and addends are no part of the cached plan: calls that differ only in them share it.  The performance
 * report does not sample these calls.
 *
 * Out of scope: addends that vary along the wall; an adjoint of the affine call; the performance report and the autotuner.
 */
cudecompResult_t cudecompAmdSetWallFieldHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                               int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                               int32_t centering, int32_t sides, const double values_low[],
                                               const double values_high[], const int32_t halo_extents[], const bool halo_periods[],
                                               int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdSetWallFieldHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                               int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                               int32_t centering, int32_t sides, const double values_low[],
                                               const double values_high[], const int32_t halo_extents[], const bool halo_periods[],
                                               int32_t dim, const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdSetWallFieldHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const inputs[],
                                               int32_t n_fields, cudecompDataType_t dtype, const int32_t parities[],
                                               int32_t centering, int32_t sides, const double values_low[],
                                               const double values_high[], const int32_t halo_extents[], const bool halo_periods[],
                                               int32_t dim, const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_HALO_WALL_VALUE_FIELDS_H */
