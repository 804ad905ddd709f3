// kernels_reduce_dev.h -- device pieces shared by the reductions of a box (kernels_reduce.hip), the profiles along one dim
// (kernels_profile.hip), the plane updates (kernels_planes.hip) and the combinations (kernels_combine.hip): the operations on fp64
// accumulators, exact widening of the reals of a 16-byte vector, the real-by-real read of a vector that is not wholly inside the
// readable range, one tile of the row walk on the 16-byte grid, a workgroup's pair of partials; and, for the two updating families,
// a double rounded once to the real type, the reals of a vector as that type, and the loads and stores of a 16-byte slot of which
// only a part lies inside a row.  Everything is internal to the translation unit that includes it.
#pragma once

#include <type_traits>

#include "kernels_dev.h"

namespace cudecomp {
namespace kern {
namespace {

// ---- the operations on fp64 accumulators ----------------------------------------------------------------------------------------
// MAX_ABS propagates NaN: a NaN operand wins, and an accumulator that is NaN stays
template <int OP> __device__ __forceinline__ double combine(double acc, double x) {
  if constexpr (OP == kReduceMaxAbs) return (x > acc || x != x) ? x : acc;
  else return acc + x;
}

// real j of a 16-byte vector, widened exactly
template <typename T> __device__ __forceinline__ double realOf(const u32x4& v, int j) {
  if constexpr (sizeof(T) == 8) {
    return __builtin_bit_cast(double, j == 0 ? (u32x2)v.xy : (u32x2)v.zw);
  } else if constexpr (sizeof(T) == 4) {
    return (double)__uint_as_float(v[j]);
  } else {
    const unsigned short h = (unsigned short)(v[j >> 1] >> ((j & 1) * 16));
    if constexpr (std::is_same<T, __bf16>::value) return (double)__uint_as_float((unsigned int)h << 16);
    else return (double)__builtin_bit_cast(_Float16, h);
  }
}

// one real at p, widened exactly
template <typename T> __device__ __forceinline__ double loadReal(const char* p) {
  if constexpr (sizeof(T) == 8) return *reinterpret_cast<const double*>(p);
  else if constexpr (sizeof(T) == 4) return (double)*reinterpret_cast<const float*>(p);
  else if constexpr (std::is_same<T, __bf16>::value) return (double)__uint_as_float((unsigned int)*reinterpret_cast<const unsigned short*>(p) << 16);
  else return (double)*reinterpret_cast<const _Float16*>(p);
}

// the reals [lo, hi) (bytes, multiples of RS) of the 16-byte slot at `slot`, each with a load of its own; zero elsewhere
template <int RS> __device__ __forceinline__ u32x4 loadPieces(const char* slot, int lo, int hi) {
  u32x4 v = {0u, 0u, 0u, 0u};
  if constexpr (RS == 8) {
    if (lo <= 0 && 8 <= hi) v.xy = *reinterpret_cast<const u32x2*>(slot);
    if (lo <= 8 && 16 <= hi) v.zw = *reinterpret_cast<const u32x2*>(slot + 8);
  } else if constexpr (RS == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lo <= 4 * j && 4 * j + 4 <= hi) v[j] = *reinterpret_cast<const unsigned int*>(slot + 4 * j);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (lo <= 2 * j && 2 * j + 2 <= hi)
        v[j >> 1] |= (unsigned int)*reinterpret_cast<const unsigned short*>(slot + 2 * j) << ((j & 1) * 16);
  }
  return v;
}

// the 16-byte slot at a + slot_off (and b + slot_off, DOT only) of which the bytes [lo, hi) lie inside a row: one aligned vector
// when the slot lies wholly inside the readable range [rd_lo, rd_hi), else only the reals inside the row.  `stream`: non-temporal
// loads, a uniform branch around the loads alone
template <typename T, int OP>
__device__ __forceinline__ void loadSlot(const char* a, const char* b, long long slot_off, int lo, int hi, long long rd_lo, long long rd_hi,
                                         bool stream, u32x4& va, u32x4& vb) {
  constexpr int RS = (int)sizeof(T);
  if (slot_off >= rd_lo && slot_off + 16 <= rd_hi) {
    if (stream) {
      va = loadVec<true, 16>(a + slot_off);
      if constexpr (OP == kReduceDot) vb = loadVec<true, 16>(b + slot_off);
    } else {
      va = loadVec<false, 16>(a + slot_off);
      if constexpr (OP == kReduceDot) vb = loadVec<false, 16>(b + slot_off);
    }
  } else {  // the pencil's first or last vector: only the reals inside the row
    va = loadPieces<RS>(a + slot_off, lo, hi);
    if constexpr (OP == kReduceDot) vb = loadPieces<RS>(b + slot_off, lo, hi);
  }
}

// ---------------------------------------------------------------------------------------------
// One lane's share of one tile of the row walk: the slot at bytes [lo16, lo16 + 16) of the 16-byte grid of the rows r0, r0 + rb, ...
// (kRowsUnroll of them, those below `rows`); row r starts at a + base + r * s1 and is `row_bytes` long (`last_row_bytes` for row
// rows - 1).  All loads first, then the arithmetic.  acc0 / acc1 take the even and the odd real position counted from the row's
// start (complex: real and imaginary part); the reals of the slot outside the row are masked by a select.
// ---------------------------------------------------------------------------------------------
template <typename T, int OP>
__device__ __forceinline__ void reduceRowTile(const char* __restrict__ a, const char* __restrict__ b, long long base, long long r0, long long rb,
                                              long long rows, long long s1, long long row_bytes, long long last_row_bytes, long long lo16,
                                              long long rd_lo, long long rd_hi, bool cplx, bool stream, double& acc0, double& acc1) {
  constexpr int RS = (int)sizeof(T), NR = 16 / RS;
  u32x4 va[kRowsUnroll], vb[kRowsUnroll];
  int lo[kRowsUnroll], hi[kRowsUnroll], par[kRowsUnroll];
  // phase one: all loads
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = r0 + (long long)u * rb;
    va[u] = u32x4{0u, 0u, 0u, 0u};
    vb[u] = u32x4{0u, 0u, 0u, 0u};
    lo[u] = hi[u] = par[u] = 0;
    if (r >= rows) continue;
    const long long row_off = base + r * s1;
    const long long ph = (long long)(reinterpret_cast<uintptr_t>(a + row_off) & 15);  // the row is bytes [ph, ph + n) of its slots
    const long long n = r == rows - 1 ? last_row_bytes : row_bytes;
    const long long first = lo16 > ph ? lo16 : ph, end = lo16 + 16 < ph + n ? lo16 + 16 : ph + n;
    if (first >= end) continue;
    lo[u] = (int)(first - lo16), hi[u] = (int)(end - lo16);
    par[u] = (int)((lo16 - ph) / RS) & 1;
    loadSlot<T, OP>(a, b, row_off - ph + lo16, lo[u], hi[u], rd_lo, rd_hi, stream, va[u], vb[u]);
  }
  // phase two: the arithmetic
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    if (lo[u] >= hi[u]) continue;
    if constexpr (OP == kReduceDot) {
      if (cplx) {  // (rows on element boundaries: reals 2k, 2k + 1 are one element, both inside the row or neither)
#pragma unroll
        for (int k = 0; k < NR / 2; ++k) {
          const bool in = lo[u] <= 2 * k * RS && 2 * k * RS < hi[u];
          const double ar = in ? realOf<T>(va[u], 2 * k) : 0.0, ai = in ? realOf<T>(va[u], 2 * k + 1) : 0.0;
          const double br_ = in ? realOf<T>(vb[u], 2 * k) : 0.0, bi = in ? realOf<T>(vb[u], 2 * k + 1) : 0.0;
          acc0 += ar * br_;
          acc0 += ai * bi;
          acc1 += ar * bi;
          acc1 -= ai * br_;
        }
        continue;
      }
    }
    double even = 0.0, odd = 0.0;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const bool in = lo[u] <= j * RS && j * RS < hi[u];
      double x = in ? realOf<T>(va[u], j) : 0.0;
      if constexpr (OP == kReduceDot) x *= in ? realOf<T>(vb[u], j) : 0.0;
      if constexpr (OP == kReduceMaxAbs) x = __builtin_fabs(x);
      if (j & 1) odd = combine<OP>(odd, x);
      else even = combine<OP>(even, x);
    }
    acc0 = combine<OP>(acc0, par[u] ? odd : even);
    acc1 = combine<OP>(acc1, par[u] ? even : odd);
  }
}

// one element at a + off (and b + off) into the pair of accumulators
template <typename T, int OP>
__device__ __forceinline__ void reduceElement(const char* a, const char* b, long long off, bool cplx, double& acc0, double& acc1) {
  constexpr int RS = (int)sizeof(T);
  const double ar = loadReal<T>(a + off), ai = cplx ? loadReal<T>(a + off + RS) : 0.0;
  if constexpr (OP == kReduceDot) {
    const double br = loadReal<T>(b + off), bi = cplx ? loadReal<T>(b + off + RS) : 0.0;
    acc0 += ar * br;
    if (cplx) {
      acc0 += ai * bi;
      acc1 += ar * bi;
      acc1 -= ai * br;
    }
  } else if constexpr (OP == kReduceMaxAbs) {
    acc0 = combine<OP>(acc0, __builtin_fabs(ar));
    if (cplx) acc1 = combine<OP>(acc1, __builtin_fabs(ai));
  } else {
    acc0 += ar;
    if (cplx) acc1 += ai;
  }
}

// ---- the 16-byte slots of the updating families (kernels_planes.hip, kernels_combine.hip): a double as T, the reals of a vector as
// T, and the loads and stores of a slot of which only a part lies inside a row --------------------------------------------------------
// ---- the coefficient in T -----------------------------------------------------------------------------------------------------------
// d rounded to fp32 TO ODD: the fp32 below |d| with the sticky bit in its last place.  RNE of that to a type of 11 or 8 significant
// bits is RNE of d itself (24 >= 11 + 2), overflow and subnormals of the narrow type included.
__device__ __forceinline__ float roundToOddF32(double d) {
  const float f = (float)d;  // to nearest even
  const double back = (double)f;
  if (d != d || back == d) return f;  // NaN; exact (zeros and infinities among them)
  unsigned int bits = __float_as_uint(f);
  if (__builtin_fabs(back) > __builtin_fabs(d)) bits -= 1;  // one step towards zero (from infinity: the largest finite)
  return __uint_as_float(bits | 1u);
}
template <typename T> __device__ __forceinline__ T toReal(double d) {
  if constexpr (sizeof(T) == 8) return d;
  else if constexpr (sizeof(T) == 4) return (float)d;
  else return (T)roundToOddF32(d);
}

// ---- the reals of a 16-byte vector as T ---------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ T typedReal(const u32x4& v, int j) {
  if constexpr (sizeof(T) == 8) return __builtin_bit_cast(double, j == 0 ? (u32x2)v.xy : (u32x2)v.zw);
  else if constexpr (sizeof(T) == 4) return __uint_as_float(v[j]);
  else return __builtin_bit_cast(T, (unsigned short)(v[j >> 1] >> ((j & 1) * 16)));
}
template <typename T, int NR> __device__ __forceinline__ u32x4 packReals(const T (&x)[NR]) {
  u32x4 v;
  if constexpr (sizeof(T) == 8) {
    v.xy = __builtin_bit_cast(u32x2, x[0]);
    v.zw = __builtin_bit_cast(u32x2, x[1]);
  } else if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __float_as_uint(x[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      v[j] = (unsigned int)__builtin_bit_cast(unsigned short, x[2 * j]) | ((unsigned int)__builtin_bit_cast(unsigned short, x[2 * j + 1]) << 16);
  }
  return v;
}

// the reals [lo, hi) (bytes, multiples of RS) of `v` to the 16-byte slot at `slot`, each with a store of its own; nothing else
template <int RS> __device__ __forceinline__ void storePieces(char* slot, const u32x4& v, int lo, int hi) {
  if constexpr (RS == 8) {
    if (lo <= 0 && 8 <= hi) *reinterpret_cast<u32x2*>(slot) = v.xy;
    if (lo <= 8 && 16 <= hi) *reinterpret_cast<u32x2*>(slot + 8) = v.zw;
  } else if constexpr (RS == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lo <= 4 * j && 4 * j + 4 <= hi) *reinterpret_cast<unsigned int*>(slot + 4 * j) = v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (lo <= 2 * j && 2 * j + 2 <= hi) *reinterpret_cast<unsigned short*>(slot + 2 * j) = (unsigned short)(v[j >> 1] >> ((j & 1) * 16));
  }
}

// The slots lie on the 16-byte grid.  The non-temporal accesses say so (a u32x4 of natural alignment), the cached ones go through the
// library's dword-aligned payload type.  `stream` is a uniform branch; the compiler merges two branches that differ in nothing but
// their non-temporal mark, and drops the mark.  So the stores differ in their alignment as well, and the loads of a tile sit on the
// two sides of ONE branch around all of them (loadSlots), not each in a branch of its own.
__device__ __forceinline__ void storeGrid(char* p, const u32x4& v, bool stream) {
  if (stream) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p));
  else *reinterpret_cast<u32x4_g*>(p) = v;
}

// the slot at a + slot_off, of which the bytes [lo, hi) lie inside a row: one aligned vector when the slot lies wholly inside the
// readable range [rd_lo, rd_hi), else only the reals inside the row (loadSlot's rule, kernels_reduce_dev.h); lo >= hi: nothing
template <int RS, bool NT>
__device__ __forceinline__ u32x4 loadSlotOf(const char* a, long long slot_off, int lo, int hi, long long rd_lo, long long rd_hi) {
  if (lo >= hi) return u32x4{0u, 0u, 0u, 0u};
  if (slot_off >= rd_lo && slot_off + 16 <= rd_hi) {
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a + slot_off));
    else return *reinterpret_cast<const u32x4_g*>(a + slot_off);
  }
  return loadPieces<RS>(a + slot_off, lo, hi);
}
// the kRowsUnroll slots of a lane's share of a tile, all loads issued before anything else happens to them
template <int RS>
__device__ __forceinline__ void loadSlots(const char* a, const long long (&off)[kRowsUnroll], const int (&lo)[kRowsUnroll],
                                          const int (&hi)[kRowsUnroll], long long rd_lo, long long rd_hi, bool stream,
                                          u32x4 (&va)[kRowsUnroll]) {
  if (stream) {
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) va[u] = loadSlotOf<RS, true>(a, off[u], lo[u], hi[u], rd_lo, rd_hi);
  } else {
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) va[u] = loadSlotOf<RS, false>(a, off[u], lo[u], hi[u], rd_lo, rd_hi);
  }
}

// the same slot back: one 16-byte store when all of it lies inside the row, else real by real inside the row alone
template <int RS> __device__ __forceinline__ void storeSlot(char* a, long long slot_off, const u32x4& v, int lo, int hi, bool stream) {
  if (lo == 0 && hi == 16) storeGrid(a + slot_off, v, stream);
  else storePieces<RS>(a + slot_off, v, lo, hi);
}

// ---- a workgroup's pair of partials -----------------------------------------------------------------------------------------------
// the wave's 64 lanes by a butterfly (the same tree in every lane), the waves through LDS in wave order, one 16-byte store to `pair`
template <int OP> __device__ __forceinline__ void storePartials(double acc0, double acc1, double* pair) {
  __shared__ double part[kThreads / 64][2];
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) {
    acc0 = combine<OP>(acc0, __shfl_xor(acc0, mask, 64));
    acc1 = combine<OP>(acc1, __shfl_xor(acc1, mask, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) part[wave][0] = acc0, part[wave][1] = acc1;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r0 = part[0][0], r1 = part[0][1];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) r0 = combine<OP>(r0, part[w][0]), r1 = combine<OP>(r1, part[w][1]);
    const u32x2 b0 = __builtin_bit_cast(u32x2, r0), b1 = __builtin_bit_cast(u32x2, r1);
    const u32x4 pair_bits = {b0.x, b0.y, b1.x, b1.y};
    *reinterpret_cast<u32x4_g*>(pair) = pair_bits;
  }
}

}  // namespace
}  // namespace kern
}  // namespace cudecomp
