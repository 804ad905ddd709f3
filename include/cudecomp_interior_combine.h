/*
 * cudecomp_interior_combine.h -- interior combinations: every cell a rank OWNS of a pencil y becomes a * x + b * y, with x a second
 * pencil of the same shape and the coefficients a and b RATIOS of doubles read from device memory.  An extension of the cuDecomp API a
 * solver may use, accepted by this library only.  It is the other half of the Krylov step cudecomp_interior_reduce.h names: the
 * reduction leaves r.r and p.Ap in device memory, this call does x += alpha p, r -= alpha Ap and p = r + beta p with
 * alpha = r.r / p.Ap and beta = r.r(new) / r.r(old) taken from those results where they lie -- no copy to the host, no division on
 * the host, nothing that stalls the stream or breaks a graph capture.
 *
 * Ghost cells and padding are never written, not even with their own value: a halo update on another stream may be writing them.
 * And they never influence a result: NaN or poison there raises nothing.
 */
#ifndef CUDECOMP_INTERIOR_COMBINE_H
#define CUDECOMP_INTERIOR_COMBINE_H

#include "cudecomp_interior_reduce.h"

#define CUDECOMP_AMD_COMBINE_AXPY 0  /* y <- y + a*x        */
#define CUDECOMP_AMD_COMBINE_XPBY 1  /* y <- x + b*y        */
#define CUDECOMP_AMD_COMBINE_AXPBY 2 /* y <- a*x + b*y      */
#define CUDECOMP_AMD_COMBINE_AX 3    /* y <- a*x, y is never read */

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Which cells.  The interior is cudecomp_interior_reduce.h's: with P what cudecompGetPencilInfo returns for this axis, halo_extents
 * and padding, the interior is P without halo_extents[d] cells at either end of every dim d and without the padding.  x[f] and y[f]
 * are pencils of the same descriptor, axis, halo_extents and padding; up to CUDECOMP_AMD_MAX_REDUCE_FIELDS pairs go in one launch.
 *
 * The update.  For field f and every interior cell, with t = a * x and s = b * y:
 *
 *   op                             stored in y
 *   CUDECOMP_AMD_COMBINE_AXPY (0)  y + t
 *   CUDECOMP_AMD_COMBINE_XPBY (1)  x + s
 *   CUDECOMP_AMD_COMBINE_AXPBY (2) t + s
 *   CUDECOMP_AMD_COMBINE_AX (3)    t          (y is never read: the copy p = r with a = 1, the scaling y = a * x)
 *
 * Coefficients.  For field f let i = f * coef_stride, coef_stride 0 or 1: at 0 all fields share pair 0 (one alpha for three velocity
 * components), at 1 every field has its own pair.  Then
 *
 *   a = (a_scale * a_num[2i + c]) / a_den[2i]        c = 0 for the real types, c = 0, 1 (re, im) for the complex ones
 *
 * -- one fp64 multiplication, then one fp64 division.  a_num == NULL stands for the pair (1.0, 0.0), so that a is a host constant
 * (a_scale) or its quotient by a_den; a_den == NULL means no division.  Only the FIRST double of a den pair is used: r.r and p.Ap of a
 * Hermitian operator are real.  A zero or NaN denominator gives what IEEE gives.  Real types never read the second double of a num
 * pair.  b follows the same rules with b_num, b_den, b_scale.  The layouts are those of the reduction's `results`: two result arrays
 * are passed as they are.  All four arrays are DEVICE memory, 8-byte aligned, and read when the kernel runs: a replayed hipGraph picks
 * up new values without re-capture.  The coefficient an op does not use -- b for AXPY and AX, a for XPBY -- is ignored: its pointers
 * may be anything, all NULL included, and its scale any value.
 *
 * Arithmetic, "in the real type of dtype".  The quotient is converted once, on the device, to the real type T of dtype, to nearest even
 * DIRECTLY from the double -- for fp16 and bf16 never through fp32 (the plane updates' rule): 1 + 2^-11 + 2^-30 becomes 1 + 2^-10 in
 * fp16.  The update itself runs in T: fp16, fp32 and fp64 with IEEE operations, bf16 as the round-to-nearest-even bf16 of the fp32
 * result of the widened operands.  Real types: t = a * x.  Complex types: t = (ar * xr - ai * xi, ar * xi + ai * xr); s is formed from
 * b and y in the same way.  Every product and every sum is rounded on its own, nothing is contracted into a fused multiply-add:
 * numpy reproduces every result bit for bit.
 *
 * Reads and writes.  Only bytes of interior cells of y[f] are stored.  Ghost cells and padding are not written, not even with their
 * own value.  Loads of x[f] and y[f] may cover ghost or padding cells of the same pencil; they never cover a byte outside
 * [ptr, ptr + P.size * element size).  AX loads nothing from y.  One call makes one launch; an empty interior makes none.  No workspace.
 *
 * Local, asynchronous, capturable.  Not collective, no communication.  Enqueued on `stream`, never blocks the host on GPU work,
 * allocates nothing and can be captured into a hipGraph.  Pointers, scales and coef_stride are captured; the contents of the
 * coefficient arrays and of the fields are read at replay.
 *
 * Validation.  Each CUDECOMP_RESULT_INVALID_USAGE with a CUDECOMP:ERROR message, on the host, before anything is launched.  First
 * the checks of cudecompAmdReduceInterior*, in its order: handle, descriptor, data type, halo_extents (NULL or negative), padding
 * (negative), n_fields outside 1 .. CUDECOMP_AMD_MAX_REDUCE_FIELDS.  Then, in this order: op outside 0 .. 3; `y` NULL or a NULL entry;
 * `x` NULL or a NULL entry; two equal entries in `y`; an entry of `x` equal to an entry of `y`; coef_stride outside 0 .. 1; for each
 * coefficient the op uses, num then den: non-NULL and not 8-byte aligned.  Equal entries in `x` are allowed.  Without a usable device
 * the result is CUDECOMP_RESULT_CUDA_ERROR.
 *
 * Out of scope: x and y with different halo extents or padding; x[f] == y[f] (scaling in place); a third, output pencil; a complex
 * denominator; conjugation of a coefficient or of x; per-plane coefficients (cudecomp_interior_planes.h has them); managed memory; the
 * performance report and the autotuner.
 */
cudecompResult_t cudecompAmdCombineInteriorX(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const y[],
                                             const void* const x[], int32_t n_fields, int32_t op, const double* a_num,
                                             const double* a_den, double a_scale, const double* b_num, const double* b_den,
                                             double b_scale, int32_t coef_stride, cudecompDataType_t dtype,
                                             const int32_t halo_extents[], const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdCombineInteriorY(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const y[],
                                             const void* const x[], int32_t n_fields, int32_t op, const double* a_num,
                                             const double* a_den, double a_scale, const double* b_num, const double* b_den,
                                             double b_scale, int32_t coef_stride, cudecompDataType_t dtype,
                                             const int32_t halo_extents[], const int32_t padding[], hipStream_t stream);
cudecompResult_t cudecompAmdCombineInteriorZ(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, void* const y[],
                                             const void* const x[], int32_t n_fields, int32_t op, const double* a_num,
                                             const double* a_den, double a_scale, const double* b_num, const double* b_den,
                                             double b_scale, int32_t coef_stride, cudecompDataType_t dtype,
                                             const int32_t halo_extents[], const int32_t padding[], hipStream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* CUDECOMP_INTERIOR_COMBINE_H */
