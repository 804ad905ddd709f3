/*
 * cudecomp_interior_profile.h -- interior profiles: the sum, the dot product and the largest magnitude of a pencil over the cells a
 * rank OWNS, reduced over two dims and KEPT along the third.  An extension of the cuDecomp API a solver may use, accepted by this
 * library only.  It is cudecomp_interior_reduce.h one rank lower in dimension, and reuses its operations and its field limit.
 *
 * A channel or boundary-layer solver reduces over the two homogeneous directions and keeps the wall-normal one: mean profiles <u>(y),
 * Reynolds stresses <u v>(y) (a DOT of u and v), max|u| per plane for the CFL number of a stretched grid, the per-plane conservation
 * check after a scatter.  The call is local.  To combine the ranks: zero-fill n_fields x N_dim pairs of doubles (N_dim the GLOBAL
 * extent of `dim`), pass `results + 2 * lo[dim]` and `ld = N_dim` (lo from cudecompGetPencilInfo, for the pencil's position of `dim`),
 * and combine all ranks with one MPI_Allreduce of 2 * n_fields * N_dim doubles (MPI_SUM, or MPI_MAX for MAX_ABS): ranks that own
 * other planes left zeros there, ranks that share planes add up.
 */
#ifndef CUDECOMP_INTERIOR_PROFILE_H
#define CUDECOMP_INTERIOR_PROFILE_H

#include "cudecomp_interior_reduce.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which cells.  Let P be what cudecompGetPencilInfo returns for this axis, halo_extents and padding.  The interior is P without
 * halo_extents[d] cells at either end of every dim d and without the padding: exactly the cells no other rank owns.  Ghost and
 * padding cells never influence a result, whatever they hold -- NaN, infinity or poison.
 *
 * dim and L.  `dim` is a GLOBAL dim 0 .. 2, as in cudecompUpdateHalos*; it may sit at any position of the pencil's memory order.
 * L is the interior extent of P along dim: shape - 2 * halo_extents[dim] - padding[dim], floored at 0.  Entry k of field f,
 * 0 <= k < L, is the reduction of `op` (CUDECOMP_AMD_REDUCE_SUM / _DOT / _MAX_ABS) over the interior cells whose interior index along
 * dim is k.
 *
 * Results.  `results` is DEVICE memory; field f, entry k owns results[2 * (f * ld + k)] and the double after it, overwritten, never
 * accumulated into.  ld >= L; the pairs k >= L of a field are NOT touched.  The pair is the scalar call's:
 *
 *   op        real types           complex types
 *   SUM       (sum a, +0.0)        (sum re, sum im)
 *   DOT       (sum a * b, +0.0)    sum conj(a) * b as (re, im)
 *   MAX_ABS   (max |a|, +0.0)      (max |re|, max |im|)
 *
 * DOT: a[f] == b[f] is allowed.  `b` is not read for the other two operations and may be NULL.  L == 0: nothing is written.  L > 0
 * with another interior extent of 0: all L pairs are written as +0.0.  MAX_ABS of a component with a NaN in a cell of plane k is NaN
 * in entry k, and in no other.  The sign of a zero: every sum starts from +0.0, so a SUM or DOT whose terms are all zeros, of either
 * sign, is +0.0; MAX_ABS is never negative.
 *
 * Arithmetic and order.  All additions are fp64.  Products of 2-byte and fp32 reals are exact in fp64; for fp64 inputs, whether the
 * product is fused into the addition is unspecified.  The order of the additions is unspecified but FIXED: there are no
 * floating-point atomics.  Results are bit-identical from run to run and between an eager call and a graph replay, for identical
 * arguments, and for any buffers whose addresses agree modulo 16.  With every field 16-byte aligned (every hipMalloc /
 * cudecompMalloc pointer is) field f of a multi-field call is bit-identical to the single-field call on it.  Error bound of SUM and
 * DOT per entry and component: |got - exact| <= n_k * 2^-53 * sum |term|, n_k the number of cells of the plane.
 *
 * Workspace.  `work` is DEVICE memory, 8-byte aligned, of at least cudecompAmdProfileInteriorWorkspaceBytes(n_fields, L) bytes:
 *
 *   bytes(n_fields, length) = n_fields * max(length, 65536) * 16
 *
 * a function of n_fields and length alone, non-decreasing in both, so a solver sizes it once from cudecompGetPencilInfo with the
 * largest L it will pass.  It holds the partial results: the cells of an entry are cut into at most min(1024, max(1, 65536 / L))
 * parts, each of which leaves one pair.  Its contents before and after the call are unspecified.
 *
 * Local, asynchronous, capturable.  Not collective, no communication.  Enqueued on `stream`, never blocks the host on GPU work, and
 * can be captured into a hipGraph.  Pointers are captured; contents are read at replay.  The fields are only read.
 *
 * Reads.  Loads may cover ghost or padding cells of the same pencil: the fast forms read aligned 16-byte vectors.  No byte outside
 * [a[f], a[f] + P.size * element size) -- and the same for b[f] -- is ever read.
 *
 * Validation.  Each CUDECOMP_RESULT_INVALID_USAGE with a CUDECOMP:ERROR message, on the host, before anything is launched.  First
 * the checks of cudecompAmdReduceInterior*, in its order, up to and including `op`: handle, descriptor, data type, halo_extents (NULL
 * or negative), padding (negative), n_fields outside 1 .. CUDECOMP_AMD_MAX_REDUCE_FIELDS, op outside 0 .. 2.  Then, in this order:
 * dim outside 0 .. 2; `a` NULL or a NULL entry; DOT: `b` NULL or a NULL entry; `results` NULL or not 8-byte aligned; ld < L; `work`
 * NULL or not 8-byte aligned.  Without a usable device the result is CUDECOMP_RESULT_CUDA_ERROR.
 * cudecompAmdProfileInteriorWorkspaceBytes returns INVALID_USAGE for n_fields out of range, a negative length or NULL `bytes`.
 *
 * Out of scope: the cross-rank combine; weights; modulus-based complex norms; a 2-D result (the reduction over one dim only); the
 * performance report; the autotuner; reading managed memory.
 */
cudecompResult_t cudecompAmdProfileInteriorWorkspaceBytes(int32_t n_fields, int64_t length, int64_t* bytes);

cudecompResult_t cudecompAmdProfileInteriorX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, const void* const a[],
                                             const void* const b[], int32_t n_fields, int32_t op, int32_t dim, double* results,
                                             int64_t ld, void* work, cudecompDataType_t dtype, const int32_t halo_extents[],
                                             const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdProfileInteriorY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, const void* const a[],
                                             const void* const b[], int32_t n_fields, int32_t op, int32_t dim, double* results,
                                             int64_t ld, void* work, cudecompDataType_t dtype, const int32_t halo_extents[],
                                             const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdProfileInteriorZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, const void* const a[],
                                             const void* const b[], int32_t n_fields, int32_t op, int32_t dim, double* results,
                                             int64_t ld, void* work, cudecompDataType_t dtype, const int32_t halo_extents[],
                                             const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_INTERIOR_PROFILE_H */
