// kernels_field_accumulate.hip -- lists of field-moves that ADD or TAKE: up to kMaxBatch moves, each carried out for up to
// kMaxFields pencils, in ONE launch (multi-field halo accumulation, include/cudecomp_halo_accumulate_fields.h).  Hand-written
// gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several).
//
// The phases of a multi-field halo accumulation are the single accumulation's one or two sides; their geometry is the same for
// every field, only the base pointers differ.  The descriptor is the FieldMoveBatch of the copying lists
// (kernels_field_transpose.hip), the workgroup decode is theirs (kernels_field_list.h), the arithmetic is that of the single
// accumulation (kernels_arith.h: addPayload, with its operand order -- destination first -- so sums are bit for bit the single call's).
//   rows_fields_accumulate_kernel<T, VB, STREAM, TAKE>  dst += src (TAKE: then src = 0).  Fastest dim contiguous on both sides:
//                                                       the lane layout of rows_kernel, kRowsUnroll source vectors and
//                                                       kRowsUnroll destination vectors in flight per lane.
//   rows_fields_take_kernel<VB, STREAM>                 dst = src; src = 0: the clearing pack.
//   generic_fields_accumulate_kernel<T, NC, TAKE>       element-wise (NC reals per element) with a grid-stride loop per field:
//   generic_fields_take_kernel<ES>                      faces one element thick along the fastest memory axis, degenerate shapes
//                                                       and the forced case.  Always cached.
// TAKE stores zero bytes where the lane loaded the source, at that load's width, after the load.  No pointer is __restrict__: a
// self-periodic addition reads and writes the same pencil, and the zero store follows a load of the same bytes -- the compiler
// keeps their order, the hardware keeps a wave's accesses to one address in order.  Exactly the cells of the moves are read and
// written.  Source and destination cells of a list are disjoint, so no lane clears or rewrites what another still has to read.
// Local buffers only.  Bound: HBM; 3 bytes moved per byte of an addition or a take, 4 of an add-take.
#include "kernels_arith.h"
#include "kernels_field_list.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

template <int N> __device__ __forceinline__ Bytes<N> zeroBytes() {
  Bytes<N> z = {};
  return z;
}

// ---------------------------------------------------------------------------------------------
// rows_fields_accumulate_kernel / rows_fields_take_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in
// BYTES.  p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors of one field.
// STREAM: 0 default caching; 1 non-temporal source loads and zero stores (the plain take: its destination stores too).  The
// destination of an addition is read and rewritten with the default policy, as in rows_accumulate_kernel.
// ---------------------------------------------------------------------------------------------
template <typename T, int VB, int STREAM, bool TAKE>
__global__ __launch_bounds__(kThreads) void rows_fields_accumulate_kernel(const FieldMoveBatch b) {
  using V = Bytes<VB>;
  int mi;
  unsigned int f, lb;
  locateFieldMove(b, blockIdx.x, mi, f, lb);
  if (f >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const int lg = m.p0;
  const int lpr = 1 << lg;
  const int rb = kThreads >> lg;
  const unsigned int tc = m.t0, tr = m.t1;
  const unsigned int bc = lb % tc;
  const unsigned int rest = lb / tc;
  const unsigned int br = rest % tr;
  const long long plane = rest / tr;

  const long long col = (long long)bc * lpr + (threadIdx.x & (lpr - 1));
  const long long r0 = (long long)br * rb * kRowsUnroll + (threadIdx.x >> lg);
  if (col >= m.e[0]) return;
  char* s = const_cast<char*>(sourceOf(b, m, f)) + plane * m.ss[2] + col * VB;  // (written too under TAKE: the zeroes)
  char* d = destinationOf(b, m, f) + plane * m.ds[2] + col * VB;

  V x[kRowsUnroll], y[kRowsUnroll];
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = r0 + (long long)u * rb;
    if (r < m.e[1]) {
      x[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
      y[u] = loadVec<false, VB>(d + r * m.ds[1]);
    }
  }
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = r0 + (long long)u * rb;
    if (r < m.e[1]) {
      storeVec<ST_CACHED, VB>(d + r * m.ds[1], addPayload<T, VB>(y[u], x[u]));
      if constexpr (TAKE) storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(s + r * m.ss[1], zeroBytes<VB>());
    }
  }
}

template <int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_fields_take_kernel(const FieldMoveBatch b) {
  using V = Bytes<VB>;
  constexpr int POLICY = STREAM >= 1 ? ST_STREAM : ST_CACHED;
  int mi;
  unsigned int f, lb;
  locateFieldMove(b, blockIdx.x, mi, f, lb);
  if (f >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const int lg = m.p0;
  const int lpr = 1 << lg;
  const int rb = kThreads >> lg;
  const unsigned int tc = m.t0, tr = m.t1;
  const unsigned int bc = lb % tc;
  const unsigned int rest = lb / tc;
  const unsigned int br = rest % tr;
  const long long plane = rest / tr;

  const long long col = (long long)bc * lpr + (threadIdx.x & (lpr - 1));
  const long long r0 = (long long)br * rb * kRowsUnroll + (threadIdx.x >> lg);
  if (col >= m.e[0]) return;
  char* s = const_cast<char*>(sourceOf(b, m, f)) + plane * m.ss[2] + col * VB;  // (written too: the zeroes)
  char* d = destinationOf(b, m, f) + plane * m.ds[2] + col * VB;

  V v[kRowsUnroll];
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = r0 + (long long)u * rb;
    if (r < m.e[1]) v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
  }
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = r0 + (long long)u * rb;
    if (r < m.e[1]) {
      storeVec<POLICY, VB>(d + r * m.ds[1], v[u]);
      storeVec<POLICY, VB>(s + r * m.ss[1], zeroBytes<VB>());
    }
  }
}

// ---------------------------------------------------------------------------------------------
// generic_fields_accumulate_kernel / generic_fields_take_kernel: element-wise, lanes along dim p0 (the destination-fast dim when
// there is one); extents and strides in ELEMENTS; a field's `blocks` workgroups stride over its move.  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <typename T, int NC, bool TAKE>
__global__ __launch_bounds__(kThreads) void generic_fields_accumulate_kernel(const FieldMoveBatch b) {
  constexpr int ES = (int)sizeof(T) * NC;
  using E = Bytes<ES>;
  int mi;
  unsigned int fi, lb;
  locateFieldMove(b, blockIdx.x, mi, fi, lb);
  if (fi >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const unsigned int nb = m.blocks;
  const int f = m.p0, g = (f + 1) % 3, h = (f + 2) % 3;
  const unsigned long long ef = m.e[f], eg = m.e[g];
  const unsigned long long total = ef * eg * (unsigned long long)m.e[h];
  char* src = const_cast<char*>(sourceOf(b, m, fi));
  char* dst = destinationOf(b, m, fi);
  for (unsigned long long n = (unsigned long long)lb * kThreads + threadIdx.x; n < total;
       n += (unsigned long long)nb * kThreads) {
    const unsigned long long kf = n % ef, t = n / ef;
    const unsigned long long kg = t % eg, kh = t / eg;
    char* s = src + (long long)(kf * m.ss[f] + kg * m.ss[g] + kh * m.ss[h]) * ES;
    char* d = dst + (long long)(kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]) * ES;
    const E x = loadVec<false, ES>(s);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, x));
    if constexpr (TAKE) storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  }
}

template <int ES>
__global__ __launch_bounds__(kThreads) void generic_fields_take_kernel(const FieldMoveBatch b) {
  using E = Bytes<ES>;
  int mi;
  unsigned int fi, lb;
  locateFieldMove(b, blockIdx.x, mi, fi, lb);
  if (fi >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const unsigned int nb = m.blocks;
  const int f = m.p0, g = (f + 1) % 3, h = (f + 2) % 3;
  const unsigned long long ef = m.e[f], eg = m.e[g];
  const unsigned long long total = ef * eg * (unsigned long long)m.e[h];
  char* src = const_cast<char*>(sourceOf(b, m, fi));
  char* dst = destinationOf(b, m, fi);
  for (unsigned long long n = (unsigned long long)lb * kThreads + threadIdx.x; n < total;
       n += (unsigned long long)nb * kThreads) {
    const unsigned long long kf = n % ef, t = n / ef;
    const unsigned long long kg = t % eg, kh = t / eg;
    char* s = src + (long long)(kf * m.ss[f] + kg * m.ss[g] + kh * m.ss[h]) * ES;
    const E x = loadVec<false, ES>(s);
    storeVec<ST_CACHED, ES>(dst + (long long)(kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]) * ES, x);
    storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  }
}

// only the forms a data type can reach: a lane holds whole elements, so 8-byte reals never take 4- or 2-byte lanes and 4-byte
// reals never 2-byte ones; bf16 has no complex type
template <typename T, int VB, bool TAKE>
void launchAddRowsOf(int s, const FieldMoveBatch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (s == 1) rows_fields_accumulate_kernel<T, VB, 1, TAKE><<<grid, block, 0, stream>>>(b);
  else rows_fields_accumulate_kernel<T, VB, 0, TAKE><<<grid, block, 0, stream>>>(b);
}

template <typename T, bool TAKE>
bool launchAddRowsOfType(int vb, int s, const FieldMoveBatch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (vb == 16) {
    launchAddRowsOf<T, 16, TAKE>(s, b, grid, block, stream);
    return true;
  }
  if (vb == 8) {
    launchAddRowsOf<T, 8, TAKE>(s, b, grid, block, stream);
    return true;
  }
  if constexpr (sizeof(T) <= 4) {
    if (vb == 4) {
      launchAddRowsOf<T, 4, TAKE>(s, b, grid, block, stream);
      return true;
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (vb == 2) {
      launchAddRowsOf<T, 2, TAKE>(s, b, grid, block, stream);
      return true;
    }
  }
  return false;
}

template <typename T, bool TAKE>
bool launchAddGenericOfType(int nc, bool complex_ok, const FieldMoveBatch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (nc == 1) {
    generic_fields_accumulate_kernel<T, 1, TAKE><<<grid, block, 0, stream>>>(b);
    return true;
  }
  if constexpr (!__is_same(T, __bf16)) {
    if (nc == 2 && complex_ok) {
      generic_fields_accumulate_kernel<T, 2, TAKE><<<grid, block, 0, stream>>>(b);
      return true;
    }
  }
  return false;
}

template <bool TAKE>
bool launchAdd(const KernelChoice& k, bool rows, int s, const FieldMoveBatch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  const int vb = k.vec, es = k.es;
  if (rows) {
    switch (k.arith) {
      case ARITH_F16: return launchAddRowsOfType<_Float16, TAKE>(vb, s, b, grid, block, stream);
      case ARITH_BF16: return launchAddRowsOfType<__bf16, TAKE>(vb, s, b, grid, block, stream);
      case ARITH_F32: return launchAddRowsOfType<float, TAKE>(vb, s, b, grid, block, stream);
      case ARITH_F64: return launchAddRowsOfType<double, TAKE>(vb, s, b, grid, block, stream);
      default: return false;
    }
  }
  switch (k.arith) {
    case ARITH_F16: return launchAddGenericOfType<_Float16, TAKE>(es / 2, true, b, grid, block, stream);
    case ARITH_BF16: return es == 2 && launchAddGenericOfType<__bf16, TAKE>(1, false, b, grid, block, stream);
    case ARITH_F32: return launchAddGenericOfType<float, TAKE>(es / 4, true, b, grid, block, stream);
    case ARITH_F64: return launchAddGenericOfType<double, TAKE>(es / 8, true, b, grid, block, stream);
    default: return false;
  }
}

template <int VB>
void launchTakeRowsOf(int s, const FieldMoveBatch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (s == 1) rows_fields_take_kernel<VB, 1><<<grid, block, 0, stream>>>(b);
  else rows_fields_take_kernel<VB, 0><<<grid, block, 0, stream>>>(b);
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchFieldAccumulateBatch(const KernelChoice& k, const FieldMoveBatch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int vb = k.vec, s = streamArgOf(k.kind, k.access), es = k.es;
  if (s != 0 && s != 1) CD_INTERNAL_ERROR("no accumulating field-move kernel for this access mode");
  bool ok = true;
  switch (k.kind) {
    case K_ROWS_FIELDS_ADD: ok = launchAdd<false>(k, true, s, b, grid, block, stream); break;
    case K_GENERIC_FIELDS_ADD: ok = launchAdd<false>(k, false, s, b, grid, block, stream); break;
    case K_ROWS_FIELDS_ADD_TAKE: ok = launchAdd<true>(k, true, s, b, grid, block, stream); break;
    case K_GENERIC_FIELDS_ADD_TAKE: ok = launchAdd<true>(k, false, s, b, grid, block, stream); break;
    case K_ROWS_FIELDS_TAKE:
      if (vb == 16) launchTakeRowsOf<16>(s, b, grid, block, stream);
      else if (vb == 8) launchTakeRowsOf<8>(s, b, grid, block, stream);
      else if (vb == 4) launchTakeRowsOf<4>(s, b, grid, block, stream);
      else if (vb == 2) launchTakeRowsOf<2>(s, b, grid, block, stream);
      else ok = false;
      break;
    case K_GENERIC_FIELDS_TAKE:
      if (es == 2) generic_fields_take_kernel<2><<<grid, block, 0, stream>>>(b);
      else if (es == 4) generic_fields_take_kernel<4><<<grid, block, 0, stream>>>(b);
      else if (es == 8) generic_fields_take_kernel<8><<<grid, block, 0, stream>>>(b);
      else if (es == 16) generic_fields_take_kernel<16><<<grid, block, 0, stream>>>(b);
      else ok = false;
      break;
    default: ok = false; break;
  }
  if (!ok) CD_INTERNAL_ERROR("no accumulating field-move kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
