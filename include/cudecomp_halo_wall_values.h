/*
 * cudecomp_halo_wall_values.h -- wall values: ghost cells at the non-periodic edges of the domain from inhomogeneous Dirichlet or
 * Neumann data.  An extension of the cuDecomp API a solver may use, accepted by this library only (cudecomp_amd.h,
 * cudecomp_amd_fill.h, cudecomp_amd_reflect.h, cudecomp_halo_fold.h and the multi-field headers have the others).
 *
 * cudecompAmdReflectHalos{X,Y,Z} (cudecomp_amd_reflect.h) states the two HOMOGENEOUS wall conditions: parity -1 gives u = 0 at
 * the wall, parity +1 gives du/dn = 0.  A moving wall (Couette flow, a driven lid), a fixed wall temperature (Rayleigh-Benard), a
 * prescribed flux, blowing or suction are affine in the interior instead: ghost = +-mirror + a.
 *   Dirichlet value g, both centerings:  parity -1 and a_k = 2 g for every k.
 *   Neumann data q (the gradient):       parity +1 and a_k = -+ d_k q, d_k the distance between ghost cell k and its mirror image,
 *                                        which the caller computes with its own grid metric (wall-normal grids are usually
 *                                        stretched); - at the low wall, + at the high one for q = du/dx.
 * The call takes one addend per ghost layer k and per side, and a mask of the sides to write, because the two walls of a channel
 * often carry different kinds of condition (parity -1 at one wall, +1 at the other: two calls).  The library knows the memory
 * order, the halo widths, the padding and which ranks sit on the domain's edge.
 */
#ifndef CUDECOMP_HALO_WALL_VALUES_H
#define CUDECOMP_HALO_WALL_VALUES_H

#include "cudecomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CUDECOMP_AMD_MAX_WALL_HALO 8 /* the widest halo_extents[dim] the call accepts */

/*
 * Which cells.  Exactly the cells cudecompAmdReflectHalos{X,Y,Z} writes for the same grid_desc, halo_extents, halo_periods, dim
 * and padding, narrowed by `sides`: bit 0 is the low halo, bit 1 the high halo.  A side whose bit is clear is neither read nor
 * written.  A side the rank does not own an edge of -- there is a neighbour behind it, or halo_periods[dim] is true -- is not
 * touched, as in the reflection.  Each slab spans the other two dims INCLUDING their halos; padding is never touched; the kernels
 * never take a whole-line form that would rewrite the cells between rows.
 *
 * Definition.  With h = halo_extents[dim], n = the pencil's extent along `dim` without padding, c = centering, s = parity, for k
 * in [0, h):
 *   low side:   cell(h - 1 - k) = s * cell(h + k + c)         + a_low[k]
 *   high side:  cell(n - h + k) = s * cell(n - h - 1 - k - c) + a_high[k]
 * along `dim`, at every position of the other two dims.  s * x for s = -1 inverts the sign bit of every real component: the
 * reflection's rule.  Flip first, add second; nothing is ever subtracted.  `+` is the addition cudecomp_amd.h states for the
 * accumulation, in the real type of `dtype`: IEEE binary16, fp32 and fp64 addition, and for CUDECOMP_AMD_BFLOAT16 the
 * round-to-nearest-even of the fp32 sum of the widened operands.  Complex elements add componentwise.  All seven element types are
 * accepted.
 *
 * Addends.  values_low and values_high are HOST arrays of h doubles for the real types and of 2 h doubles (re, im interleaved) for
 * the complex types; entry k belongs to ghost layer k, counted from the wall outward.  Each double is converted ONCE, on the host,
 * to the real type of `dtype`, rounding to nearest even directly from the double -- also for fp16 and bf16: never through fp32 --
 * and overflow gives infinity.  The arrays are read before the call returns: they may be temporaries, and the call may be captured
 * into a hipGraph (the captured addends are the ones a replay applies).  The array of a side whose bit in `sides` is clear is not
 * looked at and may be NULL.  A NaN addend is accepted; the NaN's payload in the result is unspecified.
 *
 * Not the reflection.  With all addends zero the result still differs from cudecompAmdReflectHalos: -0 + 0 is +0, and NaNs are
 * quieted.  A caller with a homogeneous condition uses the reflection.
 *
 * Local and asynchronous.  No workspace, no communication: the call is not collective, a rank may call it alone.  It is enqueued
 * on `stream`, never blocks the host on GPU work, and can be captured into a hipGraph.
 *
 * Validation.  What cudecompAmdReflectHalos* refuses is refused here with the same result code and kind of CUDECOMP:ERROR message,
 * in the same order: what the fill refuses, then parity, then centering.  Three checks follow the centering check, in this order:
 * `sides` outside 1 .. 3 is CUDECOMP_RESULT_INVALID_USAGE; a NULL value array of a side named in `sides` is
 * CUDECOMP_RESULT_INVALID_USAGE; halo_extents[dim] > CUDECOMP_AMD_MAX_WALL_HALO is CUDECOMP_RESULT_NOT_SUPPORTED.  They are made on
 * every rank, whether or not it owns an edge, so all ranks agree on the result; also when the dim is periodic or h == 0, where
 * the arrays are checked for NULL only.  Last, the reflection's refusal h + centering > n - 2 h (INVALID_USAGE) applies only to a
 * side that would be written.  Otherwise the call succeeds; without a usable device the result is CUDECOMP_RESULT_CUDA_ERROR only
 * when there are cells to write.
 *
 * Several fields at once, each with a parity and addends of its own: cudecompAmdSetWallFieldHalos{X,Y,Z},
 * cudecomp_halo_wall_value_fields.h.
 *
 * Addends that vary along the wall (a plane of values in device memory) and halos wider than CUDECOMP_AMD_MAX_WALL_HALO:
 * cudecompAmdSetWallPlaneHalos{X,Y,Z}, cudecomp_halo_wall_planes.h.
 *
 * Out of scope: an adjoint ("fold") of the affine call; the performance report and the autotuner.
 */
cudecompResult_t cudecompAmdSetWallHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                          cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t sides,
                                          const double values_low[], const double values_high[],
                                          const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                          const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdSetWallHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                          cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t sides,
                                          const double values_low[], const double values_high[],
                                          const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                          const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdSetWallHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                          cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t sides,
                                          const double values_low[], const double values_high[],
                                          const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                          const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_HALO_WALL_VALUES_H */
