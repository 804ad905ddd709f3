/*
 * cudecomp_interior_reduce.h -- interior reductions: the sum, the dot product and the largest magnitude of a pencil over the cells a
 * rank OWNS, skipping ghost cells and padding.  An extension of the cuDecomp API a solver may use, accepted by this library only
 * (cudecomp_amd.h, cudecomp_amd_fill.h, cudecomp_amd_reflect.h, cudecomp_halo_fold.h, cudecomp_halo_wall_values.h,
 * cudecomp_halo_wall_planes.h and the multi-field headers have the others).
 *
 * The halo calls do everything a solver needs TO the ghost cells of a pencil.  These calls are the arithmetic a solver does
 * BETWEEN them: r.r and p.Ap of a conjugate-gradient step, the conservation check sum(rho) of a scatter loop, max|u| for the CFL
 * number.  Each must count every grid cell exactly once.  The interior cells of all ranks partition the global grid, so the
 * per-rank results combine with one MPI_Allreduce of 2 * n_fields doubles (MPI_SUM, or MPI_MAX for MAX_ABS); the call itself is
 * local.
 */
#ifndef CUDECOMP_INTERIOR_REDUCE_H
#define CUDECOMP_INTERIOR_REDUCE_H

#include "cudecomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CUDECOMP_AMD_MAX_REDUCE_FIELDS 32
#define CUDECOMP_AMD_REDUCE_SUM 0
#define CUDECOMP_AMD_REDUCE_DOT 1
#define CUDECOMP_AMD_REDUCE_MAX_ABS 2

/*
 * Which cells.  Let P be what cudecompGetPencilInfo returns for this axis, halo_extents and padding.  The interior is P without
 * halo_extents[d] cells at either end of every dim d and without the padding: exactly the cells no other rank owns.  Ghost and
 * padding cells never influence a result, whatever they hold -- NaN, infinity or poison.
 *
 * Results.  `results` is DEVICE memory of 2 * n_fields doubles, overwritten, never accumulated into; field f owns results[2f] and
 * results[2f + 1].  Results are fp64 for all seven element types; 2-byte and fp32 reals are widened exactly.
 *
 *   op        real types           complex types
 *   SUM       (sum a, +0.0)        (sum re, sum im)
 *   DOT       (sum a * b, +0.0)    sum conj(a) * b as (re, im)
 *   MAX_ABS   (max |a|, +0.0)      (max |re|, max |im|)
 *
 * DOT: a[f] == b[f] is allowed (the squared 2-norm).  `b` is not read for the other two operations and may be NULL.  MAX_ABS of a
 * component with a NaN in any interior cell is NaN.  An empty interior gives +0.0 everywhere; the results are still written.
 * The sign of a zero: every sum starts from +0.0, so a SUM or DOT whose terms are all zeros, of either sign, is +0.0 -- also where
 * the IEEE sum of -0.0 terms alone would be -0.0; MAX_ABS is never negative.
 *
 * Arithmetic and order.  All additions are fp64.  Products of 2-byte and fp32 reals are exact in fp64; for fp64 inputs, whether
 * the product is fused into the addition is unspecified.  The order of the additions is unspecified but FIXED: there are no
 * floating-point atomics.  Results are bit-identical from run to run and between an eager call and a graph replay, for identical
 * arguments, and for any buffers whose addresses agree modulo 16.  With every field 16-byte aligned (every hipMalloc /
 * cudecompMalloc pointer is) field f of a multi-field call is bit-identical to the single-field call on it.  Error bound of SUM and
 * DOT over n cells, per component: |got - exact| <= n * 2^-53 * sum |term|.
 *
 * Workspace.  `work` is DEVICE memory of at least cudecompAmdReduceInteriorWorkspaceBytes(n_fields) bytes, 8-byte aligned.  It holds
 * the partial results of the workgroups; its contents before and after the call are unspecified.  The size depends on n_fields
 * alone and is at most 1 MiB (at 32 fields).  It is the caller's so that two streams can reduce at once, each with a workspace of
 * its own, and so that nothing is allocated inside a captured call.
 *
 * Local, asynchronous, capturable.  Not collective, no communication: a rank may call it alone.  It is enqueued on `stream`, never
 * blocks the host on GPU work, and can be captured into a hipGraph.  Pointers are captured; contents are read at replay.  The
 * fields are only read.
 *
 * Reads.  Loads may cover ghost or padding cells of the same pencil: the fast form reads aligned 16-byte vectors and masks the
 * lanes outside a row.  No byte outside [a[f], a[f] + P.size * element size) -- and the same for b[f] -- is ever read.
 *
 * Validation.  Each CUDECOMP_RESULT_INVALID_USAGE with a CUDECOMP:ERROR message, on the host, before anything is launched.  First
 * what cudecompAmdFillHalos* refuses: handle, descriptor, data type, halo_extents (NULL or negative), padding (negative).  Then, in
 * this order: n_fields outside 1 .. CUDECOMP_AMD_MAX_REDUCE_FIELDS; op outside 0 .. 2; `a` NULL or a NULL entry; DOT: `b` NULL or a
 * NULL entry; `results` NULL or not 8-byte aligned; `work` NULL or not 8-byte aligned.  Without a usable device the result is
 * CUDECOMP_RESULT_CUDA_ERROR.  cudecompAmdReduceInteriorWorkspaceBytes returns INVALID_USAGE for n_fields out of range or NULL
 * `bytes`.
 *
 * Out of scope: a cross-rank combine inside the call; weighted or masked reductions; modulus-based complex norms; a single-launch
 * combine; the performance report; the autotuner; reading managed memory.
 */
cudecompResult_t cudecompAmdReduceInteriorWorkspaceBytes(int32_t n_fields, int64_t* bytes);

cudecompResult_t cudecompAmdReduceInteriorX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, const void* const a[],
                                            const void* const b[], int32_t n_fields, int32_t op, double* results, void* work,
                                            cudecompDataType_t dtype, const int32_t halo_extents[], const int32_t padding[],
                                            hipStream_t stream);
cudecompResult_t cudecompAmdReduceInteriorY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, const void* const a[],
                                            const void* const b[], int32_t n_fields, int32_t op, double* results, void* work,
                                            cudecompDataType_t dtype, const int32_t halo_extents[], const int32_t padding[],
                                            hipStream_t stream);
cudecompResult_t cudecompAmdReduceInteriorZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, const void* const a[],
                                            const void* const b[], int32_t n_fields, int32_t op, double* results, void* work,
                                            cudecompDataType_t dtype, const int32_t halo_extents[], const int32_t padding[],
                                            hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_INTERIOR_REDUCE_H */
