// kernels_combine.hip -- combinations OF two boxes of cells (interior combinations, include/cudecomp_interior_combine.h):
// y <- a * x + b * y over the same box of x[f] and y[f], for several fields in one launch, the coefficients ratios of doubles in
// device memory: the vector updates of a Krylov step next to the dot products of kernels_reduce.hip, whose geometry these kernels
// take over.  Hand-written gfx950 (CDNA4 / MI355X) kernels, HBM-bound: two reads and one write of the box, one read and one write
// for AX.  The family is compiled in FOUR parts, for the size of the code objects: the including unit -- kernels_transpose.hip, once
// per element size -- sets CD_COMBINE_PART to 2, 4 or 8 (combine_rows_kernel for the real types of that many bytes) or to 16
// (combine_elements_kernel for every type).
//
// The store rule, the one of kernels_planes.hip: ONLY bytes of cells of y's box are stored.  The row form puts its lanes on the
// 16-byte grid of memory, which x[f] and y[f] share (planCombine); a slot that lies wholly inside a row is one aligned 16-byte load
// per operand and one 16-byte store, a slot that straddles a row end is stored real by real inside the row alone (storePieces).
// Loads may cover what lies beside a row where the readable range [g.rd_lo, g.rd_hi) holds the whole vector (loadSlotOf); what they
// bring along is never stored.
//   combine_rows_kernel<T, OP, CPLX>   reduce_rows_kernel's walk: blockIdx -> (field, workgroup) once, the field's two coefficients
//                                      computed and converted once per workgroup, the workgroup strides over the tiles of
//                                      (1 << p0) slots x (256 >> p0) * kRowsUnroll rows; per tile all loads of a lane -- kRowsUnroll
//                                      vectors of x and, for every op but AX, as many of y -- before its first store.  Complex
//                                      fields sit on element boundaries: the reals 2k, 2k + 1 of a slot are one element.
//   combine_elements_kernel<T>         element by element (the grid-stride walk of reduce_elements_kernel), uniform branches on op and
//                                      on complex: the cross-check of the row form and the form for boxes off the grid.
// T is the REAL type, OP one of kCombine*.  A coefficient is (scale * num[2i + c]) / den[2i] -- one fp64 multiplication, then one fp64
// division -- rounded ONCE to T, to nearest even directly from the double (toReal); the update itself runs in T (kernels_arith.h:
// arithReal), every product and every sum rounded on its own.
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_reduce_dev.h"
#include "kernels_walk.h"

#include "errors.h"

#ifndef CD_COMBINE_PART
#error "kernels_combine.hip is compiled as a part of kernels_transpose.hip (CD_COMBINE_PART 2, 4, 8: the row kernel per real size; 16: the element-wise kernel)"
#endif

namespace cudecomp {
namespace kern {
namespace {

// component c of the coefficient of pair i, in T: null num the pair (1.0, 0.0), null den no division; a zero or NaN denominator
// gives what IEEE gives
template <typename T>
__device__ __forceinline__ T combineCoef(const double* __restrict__ num, const double* __restrict__ den, double scale, size_t i, int c) {
  double v = scale * (num ? num[2 * i + c] : (c == 0 ? 1.0 : 0.0));
  if (den) v = v / den[2 * i];
  return toReal<T>(v);
}

// one element: (xr, xi) and (yr, yi) to what is stored; real types take the first component alone.  t = a * x, s = b * y, each a
// complex product for the complex types; AXPY y + t, XPBY x + s, AXPBY t + s, AX t
template <typename T, int OP, bool CPLX>
__device__ __forceinline__ void combineElement(T xr, T xi, T yr, T yi, T ar, T ai, T br, T bi, T& outr, T& outi) {
  T tr = xr, ti = xi, sr = yr, si = yi;
  if constexpr (OP != kCombineXpby) {
    if constexpr (CPLX) {
      tr = subReal<T>(mulReal<T>(ar, xr), mulReal<T>(ai, xi));
      ti = addReal<T>(mulReal<T>(ar, xi), mulReal<T>(ai, xr));
    } else {
      tr = mulReal<T>(ar, xr);
    }
  }
  if constexpr (OP == kCombineXpby || OP == kCombineAxpby) {
    if constexpr (CPLX) {
      sr = subReal<T>(mulReal<T>(br, yr), mulReal<T>(bi, yi));
      si = addReal<T>(mulReal<T>(br, yi), mulReal<T>(bi, yr));
    } else {
      sr = mulReal<T>(br, yr);
    }
  }
  if constexpr (OP == kCombineAx) {
    outr = tr;
    if constexpr (CPLX) outi = ti;
  } else {  // AXPY: y + t; XPBY: x + s; AXPBY: t + s
    outr = OP == kCombineAxpy ? addReal<T>(sr, tr) : addReal<T>(tr, sr);
    if constexpr (CPLX) outi = OP == kCombineAxpy ? addReal<T>(si, ti) : addReal<T>(ti, si);
  }
}

#if CD_COMBINE_PART != 16
// the update of one vector
template <typename T, int OP, bool CPLX>
__device__ __forceinline__ u32x4 combineVec(const u32x4& vx, const u32x4& vy, T ar, T ai, T br, T bi) {
  constexpr int NR = 16 / (int)sizeof(T);
  T out[NR];
  if constexpr (CPLX) {
#pragma unroll
    for (int k = 0; k < NR / 2; ++k)
      combineElement<T, OP, true>(typedReal<T>(vx, 2 * k), typedReal<T>(vx, 2 * k + 1), typedReal<T>(vy, 2 * k), typedReal<T>(vy, 2 * k + 1),
                                  ar, ai, br, bi, out[2 * k], out[2 * k + 1]);
  } else {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      T unused = ar;
      combineElement<T, OP, false>(typedReal<T>(vx, j), ar, typedReal<T>(vy, j), ar, ar, ai, br, bi, out[j], unused);
    }
  }
  return packReals<T, NR>(out);
}

// the kRowsUnroll slots of a lane's share of a tile in x and (Y) in y, all loads issued before anything else happens to them; ONE
// branch on `stream` around all of them (kernels_reduce_dev.h says why)
template <int RS, bool Y>
__device__ __forceinline__ void loadSlotPairs(const char* x, const char* y, const long long (&off)[kRowsUnroll], const int (&lo)[kRowsUnroll],
                                              const int (&hi)[kRowsUnroll], long long rd_lo, long long rd_hi, bool stream,
                                              u32x4 (&vx)[kRowsUnroll], u32x4 (&vy)[kRowsUnroll]) {
  if (stream) {
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      vx[u] = loadSlotOf<RS, true>(x, off[u], lo[u], hi[u], rd_lo, rd_hi);
      if constexpr (Y) vy[u] = loadSlotOf<RS, true>(y, off[u], lo[u], hi[u], rd_lo, rd_hi);
      else vy[u] = vx[u];
    }
  } else {
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      vx[u] = loadSlotOf<RS, false>(x, off[u], lo[u], hi[u], rd_lo, rd_hi);
      if constexpr (Y) vy[u] = loadSlotOf<RS, false>(y, off[u], lo[u], hi[u], rd_lo, rd_hi);
      else vy[u] = vx[u];
    }
  }
}

// ---------------------------------------------------------------------------------------------
// combine_rows_kernel: g.slots = 16-byte slots per row (the most a row can touch), g.rows, g.planes; g.s1, g.s2 in BYTES;
// g.row_bytes, and g.last_row_bytes for the last row of every plane (a long single row is cut into rows of kReduceChunkBytes).
// Row r of plane q starts at byte q * g.s2 + r * g.s1 of the box in x[f] and in y[f], at ONE phase of the 16-byte grid in both.
// ---------------------------------------------------------------------------------------------
template <typename T, int OP, bool CPLX>
__global__ __launch_bounds__(kThreads) void combine_rows_kernel(const CombineGeom g, const CombineFields fl, const CombineCoefs cf) {
  constexpr int RS = (int)sizeof(T);
  constexpr bool USES_A = OP != kCombineXpby, USES_B = OP == kCombineXpby || OP == kCombineAxpby, READS_Y = OP != kCombineAx;
  const unsigned int field = blockIdx.x / g.blocks, wg = blockIdx.x % g.blocks;
  const char* const x = fl.x[field] + g.box_off;
  char* const y = fl.y[field] + g.box_off;
  const bool stream = g.stream != 0;
  const size_t pair = (size_t)field * (size_t)g.coef_stride;
  const T zero = toReal<T>(0.0);
  const T ar = USES_A ? combineCoef<T>(cf.a_num, cf.a_den, g.a_scale, pair, 0) : zero;
  const T ai = USES_A && CPLX ? combineCoef<T>(cf.a_num, cf.a_den, g.a_scale, pair, 1) : zero;  // (real types never read the second double)
  const T br = USES_B ? combineCoef<T>(cf.b_num, cf.b_den, g.b_scale, pair, 0) : zero;
  const T bi = USES_B && CPLX ? combineCoef<T>(cf.b_num, cf.b_den, g.b_scale, pair, 1) : zero;
  const int lg = g.p0, lpr = 1 << lg;
  const long long rb = kThreads >> lg;
  const long long lane_col = threadIdx.x & (lpr - 1), lane_row = threadIdx.x >> lg;

  for (unsigned long long tile = wg; tile < g.tiles; tile += g.blocks) {
    const unsigned long long bc = tile % g.t0, rest = tile / g.t0;
    const unsigned long long brow = rest % g.t1, plane = rest / g.t1;
    const long long col = (long long)bc * lpr + lane_col;
    const long long r0 = (long long)brow * rb * kRowsUnroll + lane_row;
    if (col >= g.slots) continue;
    const long long lo16 = col * 16, base = (long long)plane * g.s2;
    u32x4 vx[kRowsUnroll], vy[kRowsUnroll];
    long long off[kRowsUnroll];
    int lo[kRowsUnroll], hi[kRowsUnroll];
    // phase one: where the lane's slots lie, then all loads
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      const long long r = r0 + (long long)u * rb;
      lo[u] = hi[u] = 0;
      off[u] = 0;
      if (r >= g.rows) continue;
      const long long row_off = base + r * g.s1;
      const long long ph = (long long)(reinterpret_cast<uintptr_t>(y + row_off) & 15);  // the row is bytes [ph, ph + n) of its slots
      const long long n = r == g.rows - 1 ? g.last_row_bytes : g.row_bytes;
      const long long first = lo16 > ph ? lo16 : ph, end = lo16 + 16 < ph + n ? lo16 + 16 : ph + n;
      if (first >= end) continue;
      lo[u] = (int)(first - lo16), hi[u] = (int)(end - lo16);
      off[u] = row_off - ph + lo16;
    }
    loadSlotPairs<RS, READS_Y>(x, y, off, lo, hi, g.rd_lo, g.rd_hi, stream, vx, vy);
    // phase two: the arithmetic and the stores, inside the row alone
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      if (lo[u] >= hi[u]) continue;
      storeSlot<RS>(y, off[u], combineVec<T, OP, CPLX>(vx[u], vy[u], ar, ai, br, bi), lo[u], hi[u], stream);
    }
  }
}
#endif  // CD_COMBINE_PART != 16

#if CD_COMBINE_PART == 16
// ---------------------------------------------------------------------------------------------
// combine_elements_kernel: the field's g.blocks workgroups stride over the g.e[0] * g.e[1] * g.e[2] elements, lanes along dim g.p0;
// extents and strides g.s[] in ELEMENTS of g.reals reals.  One load per operand and one store of sizeof(T) per real.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void combine_elements_kernel(const CombineGeom g, const CombineFields fl, const CombineCoefs cf) {
  constexpr int RS = (int)sizeof(T);
  const unsigned int field = blockIdx.x / g.blocks, wg = blockIdx.x % g.blocks;
  const char* const x = fl.x[field] + g.box_off;
  char* const y = fl.y[field] + g.box_off;
  const bool cplx = g.reals == 2;
  const int op = g.op;
  const bool uses_a = op != kCombineXpby, uses_b = op == kCombineXpby || op == kCombineAxpby;
  const size_t pair = (size_t)field * (size_t)g.coef_stride;
  const T zero = toReal<T>(0.0);
  const T ar = uses_a ? combineCoef<T>(cf.a_num, cf.a_den, g.a_scale, pair, 0) : zero;
  const T ai = uses_a && cplx ? combineCoef<T>(cf.a_num, cf.a_den, g.a_scale, pair, 1) : zero;
  const T br = uses_b ? combineCoef<T>(cf.b_num, cf.b_den, g.b_scale, pair, 0) : zero;
  const T bi = uses_b && cplx ? combineCoef<T>(cf.b_num, cf.b_den, g.b_scale, pair, 1) : zero;
  const long long es = (long long)g.reals * RS;
  const ElementWalk w = elementWalk(g.e, g.p0, wg, g.blocks);
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    const long long off = (long long)(kf * g.s[w.f] + kg * g.s[w.g] + kh * g.s[w.h]) * es;
    const T* const px = reinterpret_cast<const T*>(x + off);
    T* const py = reinterpret_cast<T*>(y + off);
    const T xr = px[0], xi = cplx ? px[1] : zero;
    T yr = zero, yi = zero, outr = zero, outi = zero;
    if (op != kCombineAx) {  // (AX loads nothing from y)
      yr = py[0];
      if (cplx) yi = py[1];
    }
    if (cplx) {
      if (op == kCombineAxpy) combineElement<T, kCombineAxpy, true>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      else if (op == kCombineXpby) combineElement<T, kCombineXpby, true>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      else if (op == kCombineAxpby) combineElement<T, kCombineAxpby, true>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      else combineElement<T, kCombineAx, true>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      py[0] = outr;
      py[1] = outi;
    } else {
      if (op == kCombineAxpy) combineElement<T, kCombineAxpy, false>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      else if (op == kCombineXpby) combineElement<T, kCombineXpby, false>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      else if (op == kCombineAxpby) combineElement<T, kCombineAxpby, false>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      else combineElement<T, kCombineAx, false>(xr, xi, yr, yi, ar, ai, br, bi, outr, outi);
      py[0] = outr;
    }
  });
}
#endif  // CD_COMBINE_PART == 16

#if CD_COMBINE_PART != 16
// the row kernel of T for the op and for real or complex elements (no complex type of bf16: no such kernel)
template <typename T>
bool launchCombineRowsOf(const CombineGeom& g, const CombineFields& fields, const CombineCoefs& coefs, hipStream_t stream) {
  const dim3 grid(g.blocks * (unsigned int)g.n_fields), block(kThreads);
  return dispatchInt<kCombineAxpy, kCombineXpby, kCombineAxpby, kCombineAx>(g.op, [&](auto o) {
    constexpr int OP = decltype(o)::value;
    if (g.reals == 1) combine_rows_kernel<T, OP, false><<<grid, block, 0, stream>>>(g, fields, coefs);
    else if constexpr (!std::is_same<T, __bf16>::value) combine_rows_kernel<T, OP, true><<<grid, block, 0, stream>>>(g, fields, coefs);
  });
}
#endif

}  // namespace
}  // namespace kern

#if CD_COMBINE_PART == 2
void launchCombineRows2(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                        hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_ROWS_COMBINE || (k.arith != ARITH_F16 && k.arith != ARITH_BF16)) CD_INTERNAL_ERROR("not the row kernel of a combination of 2-byte reals");
  if (k.arith == ARITH_BF16 && g.reals != 1) CD_INTERNAL_ERROR("bf16 has no complex type");
  const bool ok = k.arith == ARITH_F16 ? launchCombineRowsOf<_Float16>(g, fields, coefs, stream) : launchCombineRowsOf<__bf16>(g, fields, coefs, stream);
  if (!ok) CD_INTERNAL_ERROR("no combination kernel for this operation");
  CD_CHECK_HIP(hipGetLastError());
}
#elif CD_COMBINE_PART == 4
void launchCombineRows4(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                        hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_ROWS_COMBINE || k.arith != ARITH_F32) CD_INTERNAL_ERROR("not the row kernel of a combination of 4-byte reals");
  if (!launchCombineRowsOf<float>(g, fields, coefs, stream)) CD_INTERNAL_ERROR("no combination kernel for this operation");
  CD_CHECK_HIP(hipGetLastError());
}
#elif CD_COMBINE_PART == 8
void launchCombineRows8(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                        hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_ROWS_COMBINE || k.arith != ARITH_F64) CD_INTERNAL_ERROR("not the row kernel of a combination of 8-byte reals");
  if (!launchCombineRowsOf<double>(g, fields, coefs, stream)) CD_INTERNAL_ERROR("no combination kernel for this operation");
  CD_CHECK_HIP(hipGetLastError());
}
#else
void launchCombineElements(const KernelChoice& k, const kern::CombineGeom& g, const kern::CombineFields& fields, const kern::CombineCoefs& coefs,
                           hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_GENERIC_COMBINE) CD_INTERNAL_ERROR("not the element-wise kernel of a combination");
  if (g.op < kCombineAxpy || g.op > kCombineAx) CD_INTERNAL_ERROR("no combination kernel for this operation");
  const dim3 grid(g.blocks * (unsigned int)g.n_fields), block(kThreads);
  const bool ok = dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    if (g.reals == 2 && std::is_same<T, __bf16>::value) return false;
    return combine_elements_kernel<T><<<grid, block, 0, stream>>>(g, fields, coefs), true;
  });
  if (!ok) CD_INTERNAL_ERROR("no combination kernel for this real type");
  CD_CHECK_HIP(hipGetLastError());
}
#endif

}  // namespace cudecomp
