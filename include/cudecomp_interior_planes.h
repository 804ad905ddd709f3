/*
 * cudecomp_interior_planes.h -- interior plane updates: every cell a rank OWNS is updated in place with a coefficient that depends
 * on its index along one dim alone, u <- u + c or u <- u * c.  An extension of the cuDecomp API a solver may use, accepted by this
 * library only.  It is the adjoint of cudecomp_interior_profile.h: the profile gathers one pair of doubles per plane, this call
 * scatters one pair per plane back onto the pencil, with the profile's cells, dim, L and layout of the pairs.
 *
 * A channel-flow solver uses it for the fluctuations u' = u - <u>(y) before the Reynolds stresses (ADD of the all-reduced SUM
 * profile with scale = -1 / (N1 * N2)), for the constant-mass-flux correction, for the per-plane metric 1 / dy(k) of a stretched grid
 * (MUL), in spectral space for the derivative i * k along one dim (complex MUL) and for a 0/1 de-aliasing mask along one dim (MUL).
 * Ghost cells and padding are never written, not even with their own value: a halo update on another stream may be writing them.
 */
#ifndef CUDECOMP_INTERIOR_PLANES_H
#define CUDECOMP_INTERIOR_PLANES_H

#include "cudecomp_interior_profile.h"

#define CUDECOMP_AMD_PLANES_ADD 0
#define CUDECOMP_AMD_PLANES_MUL 1

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which cells.  The interior, dim and L are cudecomp_interior_profile.h's: with P what cudecompGetPencilInfo returns for this axis,
 * halo_extents and padding, the interior is P without halo_extents[d] cells at either end of every dim d and without the padding;
 * `dim` is a GLOBAL dim 0 .. 2 at any position of the pencil's memory order; L is the interior extent of P along dim.
 *
 * The update.  For field f, interior index k along dim, 0 <= k < L, and every interior cell u of that plane:
 *
 *   op                           update
 *   CUDECOMP_AMD_PLANES_ADD (0)  u <- u + c
 *   CUDECOMP_AMD_PLANES_MUL (1)  u <- u * c
 *
 * with c = scale * (coef[2 * (f * ld + k)], coef[2 * (f * ld + k) + 1]).
 *
 * Coefficients.  `coef` is DEVICE memory, 8-byte aligned, laid out as the profile's `results`: an all-reduced profile can be passed
 * as it is.  `scale` is a host double: the fluctuations are ADD with scale = -1.0 / (N1 * N2) on the SUM profile.  ld >= L gives every
 * field its own row of coefficients; ld == 0 makes all fields share row 0.  Across ranks a rank passes coef + 2 * lo[dim] of one
 * global array and ld = N_dim, as for the profile.  The contents are read when the kernel runs: a replayed hipGraph picks up new
 * coefficients without re-capture.  Real types use the first double of a pair; the second may hold anything, NaN included, and never
 * influences a result.  Complex types use the pair as (re, im): ADD is componentwise, MUL is the complex product
 * (ur * cr - ui * ci, ur * ci + ui * cr).
 *
 * Arithmetic, "in the real type of dtype".  scale * coef is one fp64 multiplication per component.  That double is converted once, on
 * the device, to the real type T of dtype, to nearest even DIRECTLY from the double -- for fp16 and bf16 never through fp32 (the wall
 * values' host rule): 1 + 2^-11 + 2^-30 becomes 1 + 2^-10 in fp16.  The update itself runs in T: fp16, fp32 and fp64 with IEEE
 * operations, bf16 as the round-to-nearest-even bf16 of the fp32 result of the widened operands.  Every product and every sum of the
 * complex MUL is rounded separately, nothing is contracted into a fused multiply-add: numpy reproduces every result bit for bit.
 *
 * Writes.  Only bytes of interior cells of fields[f] are stored.  Ghost cells and padding are not written, not even with their own
 * value.  Loads may cover ghost or padding cells of the same pencil; they never cover a byte outside
 * [fields[f], fields[f] + P.size * element size).  One launch serves up to CUDECOMP_AMD_MAX_REDUCE_FIELDS fields.  L == 0, or any
 * empty interior extent, makes no launch.  No workspace.
 *
 * Local, asynchronous, capturable.  Not collective, no communication.  Enqueued on `stream`, never blocks the host on GPU work,
 * allocates nothing and can be captured into a hipGraph.  Pointers, `scale` and `ld` are captured; the contents of `coef` and of the
 * fields are read at replay.
 *
 * Validation.  Each CUDECOMP_RESULT_INVALID_USAGE with a CUDECOMP:ERROR message, on the host, before anything is launched.  First
 * the checks of cudecompAmdProfileInterior*, in its order: handle, descriptor, data type, halo_extents (NULL or negative), padding
 * (negative), n_fields outside 1 .. CUDECOMP_AMD_MAX_REDUCE_FIELDS.  Then, in this order: op outside 0 .. 1; dim outside 0 .. 2;
 * `fields` NULL or a NULL entry; two equal entries in `fields`; `coef` NULL or not 8-byte aligned; ld neither 0 nor >= L.  Without a
 * usable device the result is CUDECOMP_RESULT_CUDA_ERROR.
 *
 * Out of scope: two coefficient arrays in one call (s * u + t); out-of-place operation; a 2-D coefficient; managed memory; the
 * performance report and the autotuner.
 */
cudecompResult_t cudecompAmdApplyPlanesInteriorX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const fields[],
                                                 int32_t n_fields, int32_t op, int32_t dim, const double* coef, int64_t ld,
                                                 double scale, cudecompDataType_t dtype, const int32_t halo_extents[],
                                                 const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdApplyPlanesInteriorY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const fields[],
                                                 int32_t n_fields, int32_t op, int32_t dim, const double* coef, int64_t ld,
                                                 double scale, cudecompDataType_t dtype, const int32_t halo_extents[],
                                                 const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdApplyPlanesInteriorZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const fields[],
                                                 int32_t n_fields, int32_t op, int32_t dim, const double* coef, int64_t ld,
                                                 double scale, cudecompDataType_t dtype, const int32_t halo_extents[],
                                                 const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_INTERIOR_PLANES_H */
