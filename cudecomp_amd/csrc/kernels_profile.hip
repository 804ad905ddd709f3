// kernels_profile.hip -- profiles OF a box of cells along one dim (interior profiles, include/cudecomp_interior_profile.h): sum, dot
// product and largest magnitude over two dims of the box, kept along the third -- L entries per field, for several fields in one
// launch.  Hand-written gfx950 (CDNA4 / MI355X) kernels, read-only and HBM-bound like the reductions of kernels_reduce.hip, whose
// device pieces they share (kernels_reduce_dev.h).  The family is compiled in TWO parts, for the size of the code objects: the
// including unit sets CD_PROFILE_PART to 1 (kernels_window.hip: profile_rows_kernel and profile_final_kernel) or to 2
// (kernels_rows.hip: profile_columns_kernel and profile_elements_kernel).
//
// Two stages, no floating-point atomics, every order fixed.  Stage one cuts the cells of an entry into g.parts parts and writes one
// pair of fp64 partials per (field, part, entry) to work[2 * ((field * parts + part) * L + entry)]:
//   profile_rows_kernel<T, OP>       the kept dim is NOT the contiguous one: the cells of entry k are contiguous rows.  The tile walk
//                                    of reduce_rows_kernel (reduceRowTile: lanes on the 16-byte grid of memory, aligned 16-byte loads,
//                                    the reals outside a row masked by a select, a vector not wholly inside the readable range read real
//                                    by real) with (field, entry, part) decoded from the workgroup index; part p takes the tiles p,
//                                    p + parts, ... of its entry, so every tile belongs to one entry.  The workgroup combines as
//                                    storePartials does: wave butterfly, waves through LDS.
//   profile_columns_kernel<T, OP>    the kept dim IS the contiguous one: an entry is one column of every row, and the sum runs across
//                                    rows.  A lane owns one 16-byte slot of the row and walks DOWN the rows with one fp64 accumulator per
//                                    real of the slot; no cross-lane shuffle at all.  (256 >> p0) row-lanes x (1 << p0) slots per
//                                    workgroup; the workgroup index gives (field, tile column, part), part p the rows [p * rows_per_part,
//                                    ...).  The row-lanes of a workgroup combine through LDS in lane order, and the lanes of row-lane 0
//                                    store the reals that lie inside the row.  Every row of the box shares its phase on the 16-byte
//                                    grid (row and plane pitch are multiples of 16 bytes; the host takes the element-wise kernel
//                                    otherwise), so which reals of a slot lie in the row is the same for all rows: nothing is masked in
//                                    the loop, an accumulator of a real outside the row is simply never stored.
//   profile_elements_kernel<T, OP>   element by element, for all three positions of the kept dim: the cross-check of the other two and
//                                    the form for boxes off the grid (planProfile, kernels.cc).
//   profile_final_kernel<OP>         stage two: a lane, or the 64 lanes of a wave (g.final_lanes_log2), per (field, entry) combine its
//                                    parts in index order and write the pair to results[2 * (field * ld + entry)].
// T is the REAL type, OP one of kReduce*.  All arithmetic is fp64 on exactly widened reals.
#include "kernels_dispatch.h"
#include "kernels_reduce_dev.h"

#include "errors.h"

#ifndef CD_PROFILE_PART
#error "kernels_profile.hip is compiled as a part of kernels_window.hip (CD_PROFILE_PART 1) and of kernels_rows.hip (2)"
#endif

namespace cudecomp {
namespace kern {
namespace {

#if CD_PROFILE_PART == 1
// ---------------------------------------------------------------------------------------------
// profile_rows_kernel: blockIdx -> (field, entry, part) once.  Entry k starts at byte k * g.sk; its g.rows rows of g.row_bytes lie
// g.s1 bytes apart; g.t0 x g.t1 tiles of (1 << p0) slots x (256 >> p0) * kRowsUnroll rows.
// ---------------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void profile_rows_kernel(const ProfileGeom g, const ReduceFields fl, double* __restrict__ work) {
  const unsigned int L = (unsigned int)g.L;
  const unsigned int part = blockIdx.x % g.parts, rest = blockIdx.x / g.parts;
  const unsigned int entry = rest % L, field = rest / L;
  const char* __restrict__ const a = fl.a[field] + g.box_off;
  const char* __restrict__ const b = OP == kReduceDot ? fl.b[field] + g.box_off : nullptr;
  const bool cplx = g.reals == 2, stream = g.stream != 0;
  const int lg = g.p0, lpr = 1 << lg, rb = kThreads >> lg;
  const long long lane_col = threadIdx.x & (lpr - 1), lane_row = threadIdx.x >> lg;
  const long long base = (long long)entry * g.sk;
  const unsigned long long tiles = (unsigned long long)g.t0 * g.t1;
  double acc0 = 0.0, acc1 = 0.0;

  for (unsigned long long tile = part; tile < tiles; tile += g.parts) {
    const unsigned long long bc = tile % g.t0, br = tile / g.t0;
    const long long col = (long long)bc * lpr + lane_col;
    const long long r0 = (long long)br * rb * kRowsUnroll + lane_row;
    if (col >= g.slots) continue;
    reduceRowTile<T, OP>(a, b, base, r0, rb, g.rows, g.s1, g.row_bytes, g.row_bytes, col * 16, g.rd_lo, g.rd_hi, cplx, stream, acc0, acc1);
  }
  if (!cplx) acc0 = combine<OP>(acc0, acc1), acc1 = 0.0;
  storePartials<OP>(acc0, acc1, work + 2 * (((size_t)field * g.parts + part) * L + entry));
}

// ---------------------------------------------------------------------------------------------
// profile_final_kernel: lane group e = global lane >> lg serves (field e / L, entry e % L); its 1 << lg lanes (one, or a wave) take
// the runs [t * per, (t + 1) * per) of the entry's parts in index order, per = ceil(parts / lanes), and combine by the butterfly of
// stage one.  parts == 0 (an empty entry): +0.0.
// ---------------------------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(kThreads) void profile_final_kernel(double* __restrict__ results, const double* __restrict__ work, long long L,
                                                                 long long ld, unsigned int parts, unsigned long long entries, int lg) {
  const unsigned long long lane = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long e = lane >> lg;
  const unsigned int sub = (unsigned int)(lane & ((1u << lg) - 1));
  const bool live = e < entries;  // (a group of lanes is live or not as a whole: no lane leaves before the shuffles)
  const unsigned long long field = live ? e / (unsigned long long)L : 0, k = live ? e % (unsigned long long)L : 0;
  const unsigned int per = (parts + (1u << lg) - 1) >> lg;
  const unsigned int first = sub * per, end = !live ? 0 : (first + per < parts ? first + per : parts);
  double acc0 = 0.0, acc1 = 0.0;
  for (unsigned int p = first; p < end; ++p) {
    const double* const w = work + 2 * (((size_t)field * parts + p) * (size_t)L + k);
    acc0 = combine<OP>(acc0, w[0]);
    acc1 = combine<OP>(acc1, w[1]);
  }
  for (int mask = (1 << lg) >> 1; mask >= 1; mask >>= 1) {
    acc0 = combine<OP>(acc0, __shfl_xor(acc0, mask, 64));
    acc1 = combine<OP>(acc1, __shfl_xor(acc1, mask, 64));
  }
  if (live && sub == 0) {
    double* const r = results + 2 * (field * (unsigned long long)ld + k);
    r[0] = acc0;
    r[1] = acc1;
  }
}
#endif  // CD_PROFILE_PART == 1

#if CD_PROFILE_PART == 2
// ---------------------------------------------------------------------------------------------
// profile_columns_kernel: blockIdx -> (field, tile column, part) once.  Row r of the box (r = j + g.e1 * i) starts at byte
// j * g.s1 + i * g.s2 and holds the L entries; all rows share the phase `ph` of the box's first cell on the 16-byte grid.
// ---------------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void profile_columns_kernel(const ProfileGeom g, const ReduceFields fl, double* __restrict__ work) {
  constexpr int RS = (int)sizeof(T), NR = 16 / RS;
  __shared__ double lds[kThreads * NR];
  const unsigned int part = blockIdx.x % g.parts, rest = blockIdx.x / g.parts;
  const unsigned int bc = rest % g.t0, field = rest / g.t0;
  const char* __restrict__ const a = fl.a[field] + g.box_off;
  const char* __restrict__ const b = OP == kReduceDot ? fl.b[field] + g.box_off : nullptr;
  const bool cplx = g.reals == 2, stream = g.stream != 0;
  const int lg = g.p0, lpr = 1 << lg, rb = kThreads >> lg;
  const int lane_col = threadIdx.x & (lpr - 1), lane_row = threadIdx.x >> lg;
  const long long ph = (long long)(reinterpret_cast<uintptr_t>(a) & 15);  // every row is bytes [ph, ph + row_bytes) of its slots
  const long long lo16 = ((long long)bc * lpr + lane_col) * 16;
  const long long first = lo16 > ph ? lo16 : ph, end = lo16 + 16 < ph + g.row_bytes ? lo16 + 16 : ph + g.row_bytes;
  const bool live = first < end;
  const int lo = (int)(first - lo16), hi = (int)(end - lo16);
  const unsigned int e1 = (unsigned int)g.e1;
  const long long r_begin = (long long)part * g.rows_per_part;
  const long long r_end = r_begin + g.rows_per_part < g.rows ? r_begin + g.rows_per_part : g.rows;
  double acc[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) acc[j] = 0.0;

  if (live) {
    for (long long r0 = r_begin + lane_row; r0 < r_end; r0 += (long long)rb * kRowsUnroll) {
      u32x4 va[kRowsUnroll], vb[kRowsUnroll];
      bool on[kRowsUnroll];
      // phase one: all loads
#pragma unroll
      for (int u = 0; u < kRowsUnroll; ++u) {
        const long long r = r0 + (long long)u * rb;
        va[u] = u32x4{0u, 0u, 0u, 0u};
        vb[u] = u32x4{0u, 0u, 0u, 0u};
        on[u] = r < r_end;
        if (!on[u]) continue;
        const unsigned int i = (unsigned int)r / e1, j = (unsigned int)r - i * e1;  // (rows < 2^31: planProfile)
        const long long slot_off = (long long)j * g.s1 + (long long)i * g.s2 - ph + lo16;
        loadSlot<T, OP>(a, b, slot_off, lo, hi, g.rd_lo, g.rd_hi, stream, va[u], vb[u]);
      }
      // phase two: the arithmetic, real by real; a real outside the row may hold anything and is never stored
#pragma unroll
      for (int u = 0; u < kRowsUnroll; ++u) {
        if (!on[u]) continue;
        if constexpr (OP == kReduceDot) {
          if (cplx) {  // (rows on element boundaries: reals 2k, 2k + 1 are one element)
#pragma unroll
            for (int k = 0; k < NR / 2; ++k) {
              const double ar = realOf<T>(va[u], 2 * k), ai = realOf<T>(va[u], 2 * k + 1);
              const double br = realOf<T>(vb[u], 2 * k), bi = realOf<T>(vb[u], 2 * k + 1);
              acc[2 * k] += ar * br;
              acc[2 * k] += ai * bi;
              acc[2 * k + 1] += ar * bi;
              acc[2 * k + 1] -= ai * br;
            }
            continue;
          }
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          double x = realOf<T>(va[u], j);
          if constexpr (OP == kReduceDot) x *= realOf<T>(vb[u], j);
          if constexpr (OP == kReduceMaxAbs) x = __builtin_fabs(x);
          acc[j] = combine<OP>(acc[j], x);
        }
      }
    }
  }
  // the row-lanes of the workgroup, in lane order
#pragma unroll
  for (int j = 0; j < NR; ++j) lds[threadIdx.x * NR + j] = acc[j];
  __syncthreads();
  if (lane_row == 0 && live) {
    double* const out = work + 2 * ((size_t)field * g.parts + part) * (size_t)g.L;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      double tot = lds[lane_col * NR + j];
      for (int rr = 1; rr < rb; ++rr) tot = combine<OP>(tot, lds[(rr * lpr + lane_col) * NR + j]);
      const long long pos = lo16 + j * RS;
      if (pos < ph || pos >= ph + g.row_bytes) continue;
      const long long q = (pos - ph) / RS;  // the real of the row
      if (cplx) {
        out[q] = tot;  // (2 * entry + component)
      } else {
        out[2 * q] = tot;
        out[2 * q + 1] = 0.0;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// profile_elements_kernel: blockIdx -> (field, entry, part) once; the part's lanes stride over the g.e1 * g.e2 cells of the entry,
// cell (j, i) at byte entry * g.sk + j * g.s1 + i * g.s2.
// ---------------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void profile_elements_kernel(const ProfileGeom g, const ReduceFields fl, double* __restrict__ work) {
  const unsigned int L = (unsigned int)g.L;
  const unsigned int part = blockIdx.x % g.parts, rest = blockIdx.x / g.parts;
  const unsigned int entry = rest % L, field = rest / L;
  const char* __restrict__ const a = fl.a[field] + g.box_off;
  const char* __restrict__ const b = OP == kReduceDot ? fl.b[field] + g.box_off : nullptr;
  const bool cplx = g.reals == 2;
  const long long base = (long long)entry * g.sk;
  const unsigned long long cells = (unsigned long long)g.e1 * (unsigned long long)g.e2, e1 = (unsigned long long)g.e1;
  double acc0 = 0.0, acc1 = 0.0;
  for (unsigned long long c = (unsigned long long)part * kThreads + threadIdx.x; c < cells; c += (unsigned long long)g.parts * kThreads) {
    const unsigned long long i = c / e1, j = c - i * e1;
    reduceElement<T, OP>(a, b, base + (long long)j * g.s1 + (long long)i * g.s2, cplx, acc0, acc1);
  }
  storePartials<OP>(acc0, acc1, work + 2 * (((size_t)field * g.parts + part) * L + entry));
}
#endif  // CD_PROFILE_PART == 2

}  // namespace
}  // namespace kern

#if CD_PROFILE_PART == 1
void launchProfileRows(const KernelChoice& k, int op, const kern::ProfileGeom& g, const kern::ReduceFields& fields, double* work,
                       hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_ROWS_PROFILE) CD_INTERNAL_ERROR("not the row kernel of a profile");
  const dim3 grid((unsigned int)g.n_fields * (unsigned int)g.L * g.parts), block(kThreads);
  const bool ok = dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatchInt<kReduceSum, kReduceDot, kReduceMaxAbs>(op, [&](auto o) {
      profile_rows_kernel<T, decltype(o)::value><<<grid, block, 0, stream>>>(g, fields, work);
    });
  });
  if (!ok) CD_INTERNAL_ERROR("no profile kernel for this real type and operation");
  CD_CHECK_HIP(hipGetLastError());
}

void launchProfileFinal(int op, const kern::ProfileGeom& g, double* results, long long ld, const double* work, hipStream_t stream) {
  using namespace kern;
  const unsigned long long entries = (unsigned long long)g.n_fields * (unsigned long long)g.L;
  const unsigned long long lanes = entries << g.final_lanes_log2;
  const dim3 grid((unsigned int)((lanes + kThreads - 1) / kThreads)), block(kThreads);
  const bool ok = dispatchInt<kReduceSum, kReduceDot, kReduceMaxAbs>(op, [&](auto o) {
    profile_final_kernel<decltype(o)::value><<<grid, block, 0, stream>>>(results, work, g.L, ld, g.parts, entries, g.final_lanes_log2);
  });
  if (!ok) CD_INTERNAL_ERROR("no final profile kernel for this operation");
  CD_CHECK_HIP(hipGetLastError());
}
#endif

#if CD_PROFILE_PART == 2
void launchProfileColumnsOrElements(const KernelChoice& k, int op, const kern::ProfileGeom& g, const kern::ReduceFields& fields, double* work,
                                    hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_COLUMNS_PROFILE && k.kind != K_GENERIC_PROFILE) CD_INTERNAL_ERROR("not a column or element-wise kernel of a profile");
  const unsigned int per_field = k.kind == K_COLUMNS_PROFILE ? g.t0 : (unsigned int)g.L;
  const dim3 grid((unsigned int)g.n_fields * per_field * g.parts), block(kThreads);
  const bool ok = dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatchInt<kReduceSum, kReduceDot, kReduceMaxAbs>(op, [&](auto o) {
      constexpr int OP = decltype(o)::value;
      if (k.kind == K_COLUMNS_PROFILE) {
        profile_columns_kernel<T, OP><<<grid, block, 0, stream>>>(g, fields, work);
      } else {
        profile_elements_kernel<T, OP><<<grid, block, 0, stream>>>(g, fields, work);
      }
    });
  });
  if (!ok) CD_INTERNAL_ERROR("no profile kernel for this real type and operation");
  CD_CHECK_HIP(hipGetLastError());
}
#endif

}  // namespace cudecomp
