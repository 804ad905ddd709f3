/*
 * cudecomp_halo_wall_planes.h -- wall planes: ghost cells at the non-periodic edges of the domain from wall data that VARIES ALONG
 * THE WALL and lives in device memory.  An extension of the cuDecomp API a solver may use, accepted by this library only
 * (cudecomp_amd.h, cudecomp_amd_fill.h, cudecomp_amd_reflect.h, cudecomp_halo_fold.h, cudecomp_halo_wall_values.h and the
 * multi-field headers have the others).
 *
 * cudecompAmdSetWallHalos{X,Y,Z} (cudecomp_halo_wall_values.h) writes ghost = +-mirror + a with one addend per ghost layer and
 * side: host doubles, constant along the whole wall, baked into a captured graph.  That covers a moving lid or one wall
 * temperature.  An inflow plane fed from a precursor run, blowing and suction for flow control, a heated patch or a roughness
 * strip, a prescribed flux map, and any time-dependent wall data a replayed hipGraph must pick up without re-capture need an addend
 * per CELL of the ghost slab instead:
 *   ghost(k; p, q) = +-mirror(k; p, q) + plane(k; p, q)
 * with (p, q) the position on the wall.  Dirichlet data g(p, q): parity -1 and plane(k; p, q) = 2 g(p, q) for every k.  Neumann
 * data q(p, q): parity +1 and plane(k; p, q) = -+ d_k q(p, q), d_k the distance between ghost cell k and its mirror image.
 */
#ifndef CUDECOMP_HALO_WALL_PLANES_H
#define CUDECOMP_HALO_WALL_PLANES_H

#include "cudecomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which cells.  Exactly the cells cudecompAmdSetWallHalos{X,Y,Z} writes for the same grid_desc, sides, halo_extents, halo_periods,
 * dim and padding: the reflection's cells narrowed by `sides` (bit 0 the low halo, bit 1 the high halo).  A side whose bit is clear
 * is neither read nor written, and its plane is not looked at.  A side the rank does not own an edge of -- there is a neighbour
 * behind it, or halo_periods[dim] is true -- is not touched.  Each slab spans the other two dims INCLUDING their halos; padding is
 * never touched; the kernels never take a whole-line form that would rewrite the cells between rows.
 *
 * Definition.  With h = halo_extents[dim], n = the pencil's extent along `dim` without padding, c = centering, s = parity, for k
 * in [0, h) and every position (p, q) of the other two dims:
 *   low side:   cell(h - 1 - k; p, q) = s * cell(h + k + c; p, q)         + planes_low(k; p, q)
 *   high side:  cell(n - h + k; p, q) = s * cell(n - h - 1 - k - c; p, q) + planes_high(k; p, q)
 * s * x for s = -1 inverts the sign bit of every real component: the reflection's rule.  Flip first, add second; nothing is ever
 * subtracted.  `+` is the addition cudecomp_amd.h states for the accumulation, in the real type of `dtype`: IEEE binary16, fp32 and
 * fp64 addition, and for CUDECOMP_AMD_BFLOAT16 the round-to-nearest-even of the fp32 sum of the widened operands.  Complex elements
 * add componentwise.  All seven element types are accepted.
 *
 * Plane layout: a slab of the pencil.  planes_low and planes_high are DEVICE arrays of `dtype` elements.  Let P be what
 * cudecompGetPencilInfo returns for this axis, halo_extents and padding, and a the memory-order position with P.order[a] == dim.
 * The plane has P's shape with shape[a] replaced by h, stored densely in the pencil's memory order:
 *   plane[i0 + shape'[0] * (i1 + shape'[1] * i2)],   shape' = P.shape with shape'[a] = h.
 * The index along position a is the ghost layer k, counted from the wall outward, as in cudecompAmdSetWallHalos; the other two
 * indices are the pencil's own indices, halo and padding offsets included.  The size is P.size / P.shape[a] * h elements.  A solver
 * addresses the plane with the index arithmetic it already has.  When `dim` is not the fastest memory axis a plane row has the
 * pencil's row pitch, hence the same 16-byte phase as the pencil row it serves.  Plane entries at padding positions are never
 * read.  Plane entries at halo positions of the other two dims ARE read, because the slabs span them: they must be readable.  (A
 * caller that updates the periodic dims after the walls overwrites those ghost cells anyway.)  The planes are only read; the two
 * sides may name the same array; a plane must not overlap the pencil.
 *
 * No width limit.  halo_extents[dim] > CUDECOMP_AMD_MAX_WALL_HALO is accepted; the only width rule is the reflection's
 * h + c > n - 2 h, applied to a side that would be written.
 *
 * Local, asynchronous, capturable.  No workspace, no communication: the call is not collective, a rank may call it alone.  It is
 * enqueued on `stream`, never blocks the host on GPU work, and can be captured into a hipGraph.  The plane POINTERS are captured;
 * the plane CONTENTS are read when the kernel runs, so a replay applies whatever the planes hold at that moment.
 *
 * Validation.  What cudecompAmdReflectHalos* refuses is refused here with the same result code and kind of CUDECOMP:ERROR message,
 * in the same order: what the fill refuses, then parity, then centering.  Three checks follow, in this order, each
 * CUDECOMP_RESULT_INVALID_USAGE: `sides` outside 1 .. 3; a NULL plane of a side named in `sides`; a named plane whose byte range
 * overlaps the pencil's P.size elements (a host comparison of addresses).  They are made on every rank, whether or not it owns an
 * edge, so all ranks agree on the result; also when the dim is periodic or h == 0, where the planes are checked for NULL only.
 * Last, the reflection's refusal h + centering > n - 2 h (INVALID_USAGE) applies only to a side that would be written.  Otherwise
 * the call succeeds; without a usable device the result is CUDECOMP_RESULT_CUDA_ERROR only when there are cells to write.
 *
 * Out of scope: several fields in one launch; an adjoint ("fold") of the call; the performance report; the autotuner.
 */
cudecompResult_t cudecompAmdSetWallPlaneHalosX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                               cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t sides,
                                               const void* planes_low, const void* planes_high,
                                               const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                               const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdSetWallPlaneHalosY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                               cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t sides,
                                               const void* planes_low, const void* planes_high,
                                               const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                               const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdSetWallPlaneHalosZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* input,
                                               cudecompDataType_t dtype, int32_t parity, int32_t centering, int32_t sides,
                                               const void* planes_low, const void* planes_high,
                                               const int32_t halo_extents[], const bool halo_periods[], int32_t dim,
                                               const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_HALO_WALL_PLANES_H */
