// kernels_planes.hip -- plane updates OF a box of cells along one dim (interior plane updates, include/cudecomp_interior_planes.h):
// every cell of the box is updated in place with the coefficient of its index k along the kept dim, u <- u + c or u <- u * c, for
// several fields in one launch.  The adjoint of the profiles of kernels_profile.hip, whose walks and geometry these kernels take
// over.  Hand-written gfx950 (CDNA4 / MI355X) kernels, HBM-bound: one read and one write of the box.  The family is compiled in TWO
// parts, for the size of the code objects: the including unit sets CD_PLANES_PART to 1 (kernels_lines.hip: planes_rows_kernel) or
// to 2 (kernels_rowlines.hip: planes_columns_kernel and planes_elements_kernel).
//
// The store rule, the same in all three forms: ONLY bytes of cells of the box are stored.  The fast forms put their lanes on the
// 16-byte grid of memory; a slot that lies wholly inside a row is one aligned 16-byte load and one 16-byte store, a slot that
// straddles a row end is stored real by real inside the row alone (storePieces).  Loads may cover what lies beside a row where the
// readable range [g.rd_lo, g.rd_hi) holds the whole vector (loadSlotOf: the rule of loadSlot, kernels_reduce_dev.h); what they bring
// along is never stored.
//   planes_rows_kernel<T, MODE>      the kept dim is NOT the contiguous one: the cells of entry k are contiguous rows and share one
//                                    coefficient, converted once per workgroup.  The tile walk of profile_rows_kernel: (field, entry,
//                                    part) from the workgroup index, part p the tiles p, p + parts, ... of its entry; per tile all
//                                    loads of a lane (kRowsUnroll vectors) before its first store.
//   planes_columns_kernel<T, MODE>   the kept dim IS the contiguous one: a lane owns one 16-byte slot of the row, loads and converts
//                                    its 1 to 16 / sizeof(T) coefficients once and walks DOWN the rows as profile_columns_kernel
//                                    does.  Every row of the box shares its phase on the 16-byte grid (the host takes the
//                                    element-wise kernel otherwise): which reals of a slot lie in the row is the same for all rows,
//                                    and only the first and the last slot of a row take the narrow stores.
//   planes_elements_kernel<T>        element by element, for all three positions of the kept dim and both operations (a uniform
//                                    branch): the cross-check of the other two and the form for boxes off the grid (planPlanes).
// T is the REAL type; MODE 0 adds (complex: alternating coefficients), 1 multiplies real by real, 2 is the complex product.  The
// coefficient is scale * coef[...] -- one fp64 multiplication -- rounded ONCE to T, to nearest even directly from the double
// (toReal); the update itself runs in T (kernels_arith.h: arithReal), every product and every sum rounded on its own.
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_reduce_dev.h"

#include "errors.h"

#ifndef CD_PLANES_PART
#error "kernels_planes.hip is compiled as a part of kernels_lines.hip (CD_PLANES_PART 1) and of kernels_rowlines.hip (2)"
#endif

namespace cudecomp {
namespace kern {
namespace {

// (toReal, typedReal, packReals, storePieces, storeGrid, loadSlotOf, loadSlots and storeSlot: kernels_reduce_dev.h, shared with
// kernels_combine.hip)

// the update of one vector: real j with coefficient c[j]; MODE 2: the reals 2k, 2k + 1 are one element, c[2k], c[2k + 1] its (re, im)
template <typename T, int MODE> __device__ __forceinline__ u32x4 applyVec(const u32x4& v, const T (&c)[16 / sizeof(T)]) {
  constexpr int NR = 16 / (int)sizeof(T);
  T out[NR];
  if constexpr (MODE == 2) {
#pragma unroll
    for (int k = 0; k < NR / 2; ++k) {
      const T ur = typedReal<T>(v, 2 * k), ui = typedReal<T>(v, 2 * k + 1);
      out[2 * k] = subReal<T>(mulReal<T>(ur, c[2 * k]), mulReal<T>(ui, c[2 * k + 1]));
      out[2 * k + 1] = addReal<T>(mulReal<T>(ur, c[2 * k + 1]), mulReal<T>(ui, c[2 * k]));
    }
  } else {
#pragma unroll
    for (int j = 0; j < NR; ++j) out[j] = MODE == 0 ? addReal<T>(typedReal<T>(v, j), c[j]) : mulReal<T>(typedReal<T>(v, j), c[j]);
  }
  return packReals<T, NR>(out);
}

#if CD_PLANES_PART == 1
// ---------------------------------------------------------------------------------------------
// planes_rows_kernel: blockIdx -> (field, entry, part) once.  Entry k starts at byte k * g.sk; its g.rows rows of g.row_bytes lie
// g.s1 bytes apart; g.t0 x g.t1 tiles of (1 << p0) slots x (256 >> p0) * kRowsUnroll rows.  c0 / c1: the coefficient of the even and
// of the odd real position counted from the row's start (real types: the same; complex: real and imaginary part).
// ---------------------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void planes_rows_kernel(const PlanesGeom g, const PlanesFields fl, const double* __restrict__ coef) {
  constexpr int RS = (int)sizeof(T), NR = 16 / RS;
  const unsigned int L = (unsigned int)g.L;
  const unsigned int part = blockIdx.x % g.parts, rest = blockIdx.x / g.parts;
  const unsigned int entry = rest % L, field = rest / L;
  char* const a = fl.a[field] + g.box_off;
  const bool stream = g.stream != 0;
  const double* const pair = coef + 2 * ((size_t)field * (size_t)g.ld + entry);
  const T c0 = toReal<T>(g.scale * pair[0]);
  const T c1 = g.reals == 2 ? toReal<T>(g.scale * pair[1]) : c0;  // (real types never read the second double)
  const int lg = g.p0, lpr = 1 << lg;
  const long long rb = kThreads >> lg;
  const long long lane_col = threadIdx.x & (lpr - 1), lane_row = threadIdx.x >> lg;
  const long long base = (long long)entry * g.sk;
  const unsigned long long tiles = (unsigned long long)g.t0 * g.t1;

  for (unsigned long long tile = part; tile < tiles; tile += g.parts) {
    const unsigned long long bc = tile % g.t0, br = tile / g.t0;
    const long long col = (long long)bc * lpr + lane_col;
    const long long r0 = (long long)br * rb * kRowsUnroll + lane_row;
    if (col >= g.slots) continue;
    const long long lo16 = col * 16;
    u32x4 va[kRowsUnroll];
    long long off[kRowsUnroll];
    int lo[kRowsUnroll], hi[kRowsUnroll], par[kRowsUnroll];
    // phase one: where the lane's slots lie, then all loads
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      const long long r = r0 + (long long)u * rb;
      lo[u] = hi[u] = par[u] = 0;
      off[u] = 0;
      if (r >= g.rows) continue;
      const long long row_off = base + r * g.s1;
      const long long ph = (long long)(reinterpret_cast<uintptr_t>(a + row_off) & 15);  // the row is bytes [ph, ph + n) of its slots
      const long long first = lo16 > ph ? lo16 : ph, end = lo16 + 16 < ph + g.row_bytes ? lo16 + 16 : ph + g.row_bytes;
      if (first >= end) continue;
      lo[u] = (int)(first - lo16), hi[u] = (int)(end - lo16);
      par[u] = (int)((lo16 - ph) / RS) & 1;  // parity of the slot's real 0, counted from the row's start
      off[u] = row_off - ph + lo16;
    }
    loadSlots<RS>(a, off, lo, hi, g.rd_lo, g.rd_hi, stream, va);
    // phase two: the arithmetic and the stores, inside the row alone
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      if (lo[u] >= hi[u]) continue;
      T c[NR];
#pragma unroll
      for (int j = 0; j < NR; ++j) c[j] = ((j & 1) != par[u]) ? c1 : c0;
      storeSlot<RS>(a, off[u], applyVec<T, MODE>(va[u], c), lo[u], hi[u], stream);
    }
  }
}
#endif  // CD_PLANES_PART == 1

#if CD_PLANES_PART == 2
// ---------------------------------------------------------------------------------------------
// planes_columns_kernel: blockIdx -> (field, tile column, part) once.  Row r of the box (r = j + g.e1 * i) starts at byte
// j * g.s1 + i * g.s2 and holds the L entries; all rows share the phase `ph` of the box's first cell on the 16-byte grid.  Real q of
// the row, counted from its start, takes the double at 2 * q of the field's coefficient row (complex: at q, the component q & 1 of
// element q / 2).
// ---------------------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(kThreads) void planes_columns_kernel(const PlanesGeom g, const PlanesFields fl, const double* __restrict__ coef) {
  constexpr int RS = (int)sizeof(T), NR = 16 / RS;
  const unsigned int part = blockIdx.x % g.parts, rest = blockIdx.x / g.parts;
  const unsigned int bc = rest % g.t0, field = rest / g.t0;
  char* const a = fl.a[field] + g.box_off;
  const bool cplx = g.reals == 2, stream = g.stream != 0;
  const int lg = g.p0, lpr = 1 << lg, rb = kThreads >> lg;
  const int lane_col = threadIdx.x & (lpr - 1), lane_row = threadIdx.x >> lg;
  const long long ph = (long long)(reinterpret_cast<uintptr_t>(a) & 15);  // every row is bytes [ph, ph + row_bytes) of its slots
  const long long lo16 = ((long long)bc * lpr + lane_col) * 16;
  const long long first = lo16 > ph ? lo16 : ph, end = lo16 + 16 < ph + g.row_bytes ? lo16 + 16 : ph + g.row_bytes;
  if (first >= end) return;  // (no barrier in this kernel)
  const int lo = (int)(first - lo16), hi = (int)(end - lo16);
  const double* const row = coef + 2 * (size_t)field * (size_t)g.ld;
  T c[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const long long pos = lo16 + j * RS;
    c[j] = toReal<T>(0.0);
    if (pos < ph || pos >= ph + g.row_bytes) continue;  // (a real outside the row is never stored, and has no coefficient)
    const long long q = (pos - ph) / RS;
    c[j] = toReal<T>(g.scale * row[cplx ? q : 2 * q]);
  }
  const unsigned int e1 = (unsigned int)g.e1;
  const long long r_begin = (long long)part * g.rows_per_part;
  const long long r_end = r_begin + g.rows_per_part < g.rows ? r_begin + g.rows_per_part : g.rows;

  for (long long r0 = r_begin + lane_row; r0 < r_end; r0 += (long long)rb * kRowsUnroll) {
    u32x4 va[kRowsUnroll];
    long long off[kRowsUnroll];
    int los[kRowsUnroll], his[kRowsUnroll];  // (lo, hi) of the rows that exist, (0, 0) of the others
    // phase one: where the lane's slots lie, then all loads
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      const long long r = r0 + (long long)u * rb;
      off[u] = 0;
      los[u] = his[u] = 0;
      if (r >= r_end) continue;
      const unsigned int i = (unsigned int)r / e1, j = (unsigned int)r - i * e1;  // (rows < 2^31: planPlanes)
      off[u] = (long long)j * g.s1 + (long long)i * g.s2 - ph + lo16;
      los[u] = lo, his[u] = hi;
    }
    loadSlots<RS>(a, off, los, his, g.rd_lo, g.rd_hi, stream, va);
    // phase two: the arithmetic and the stores
#pragma unroll
    for (int u = 0; u < kRowsUnroll; ++u) {
      if (los[u] >= his[u]) continue;
      storeSlot<RS>(a, off[u], applyVec<T, MODE>(va[u], c), lo, hi, stream);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// planes_elements_kernel: blockIdx -> (field, entry, part) once; the part's lanes stride over the g.e1 * g.e2 cells of the entry,
// cell (j, i) at byte entry * g.sk + j * g.s1 + i * g.s2.  One load and one store of sizeof(T) per real.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void planes_elements_kernel(const PlanesGeom g, const PlanesFields fl, const double* __restrict__ coef) {
  const unsigned int L = (unsigned int)g.L;
  const unsigned int part = blockIdx.x % g.parts, rest = blockIdx.x / g.parts;
  const unsigned int entry = rest % L, field = rest / L;
  char* const a = fl.a[field] + g.box_off;
  const bool cplx = g.reals == 2, mul = g.op == kPlanesMul;
  const double* const pair = coef + 2 * ((size_t)field * (size_t)g.ld + entry);
  const T c0 = toReal<T>(g.scale * pair[0]);
  const T c1 = cplx ? toReal<T>(g.scale * pair[1]) : c0;
  const long long base = (long long)entry * g.sk;
  const unsigned long long cells = (unsigned long long)g.e1 * (unsigned long long)g.e2, e1 = (unsigned long long)g.e1;
  for (unsigned long long cell = (unsigned long long)part * kThreads + threadIdx.x; cell < cells; cell += (unsigned long long)g.parts * kThreads) {
    const unsigned long long i = cell / e1, j = cell - i * e1;
    T* const p = reinterpret_cast<T*>(a + base + (long long)j * g.s1 + (long long)i * g.s2);
    const T ur = p[0];
    if (!cplx) {
      p[0] = mul ? mulReal<T>(ur, c0) : addReal<T>(ur, c0);
    } else {
      const T ui = p[1];
      if (mul) {
        p[0] = subReal<T>(mulReal<T>(ur, c0), mulReal<T>(ui, c1));
        p[1] = addReal<T>(mulReal<T>(ur, c1), mulReal<T>(ui, c0));
      } else {
        p[0] = addReal<T>(ur, c0);
        p[1] = addReal<T>(ui, c1);
      }
    }
  }
}
#endif  // CD_PLANES_PART == 2

// MODE of the fast forms: 0 adds, 1 multiplies real by real, 2 the complex product (no complex type of bf16: no such kernel)
template <typename T, typename F> bool dispatchPlanesMode(const PlanesGeom& g, F&& f) {
  const int mode = g.op == kPlanesAdd ? 0 : g.reals == 2 ? 2 : 1;
  if constexpr (std::is_same<T, __bf16>::value) return dispatchInt<0, 1>(mode, f);
  else return dispatchInt<0, 1, 2>(mode, f);
}

}  // namespace
}  // namespace kern

#if CD_PLANES_PART == 1
void launchPlanesRows(const KernelChoice& k, const kern::PlanesGeom& g, const kern::PlanesFields& fields, const double* coef,
                      hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_ROWS_PLANES) CD_INTERNAL_ERROR("not the row kernel of a plane update");
  const dim3 grid((unsigned int)g.n_fields * (unsigned int)g.L * g.parts), block(kThreads);
  const bool ok = dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatchPlanesMode<T>(g, [&](auto m) { planes_rows_kernel<T, decltype(m)::value><<<grid, block, 0, stream>>>(g, fields, coef); });
  });
  if (!ok) CD_INTERNAL_ERROR("no plane-update kernel for this real type and operation");
  CD_CHECK_HIP(hipGetLastError());
}
#endif

#if CD_PLANES_PART == 2
void launchPlanesColumnsOrElements(const KernelChoice& k, const kern::PlanesGeom& g, const kern::PlanesFields& fields, const double* coef,
                                   hipStream_t stream) {
  using namespace kern;
  if (k.kind != K_COLUMNS_PLANES && k.kind != K_GENERIC_PLANES) CD_INTERNAL_ERROR("not a column or element-wise kernel of a plane update");
  const unsigned int per_field = k.kind == K_COLUMNS_PLANES ? g.t0 : (unsigned int)g.L;
  const dim3 grid((unsigned int)g.n_fields * per_field * g.parts), block(kThreads);
  const bool ok = dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    if (g.reals == 2 && std::is_same<T, __bf16>::value) return false;
    if (k.kind == K_GENERIC_PLANES) return planes_elements_kernel<T><<<grid, block, 0, stream>>>(g, fields, coef), true;
    return dispatchPlanesMode<T>(g, [&](auto m) { planes_columns_kernel<T, decltype(m)::value><<<grid, block, 0, stream>>>(g, fields, coef); });
  });
  if (!ok) CD_INTERNAL_ERROR("no plane-update kernel for this real type and operation");
  CD_CHECK_HIP(hipGetLastError());
}
#endif

}  // namespace cudecomp
