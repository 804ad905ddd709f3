// kernels_take.hip -- take-moves (Move3D::take): the move of its kind, then zero bytes into the source cells it has read.
// Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several).
//
// The moves of the fused halo accumulate-and-clear (cudecompAmdAccumulateAndClearHalos{X,Y,Z}, plan.h
// buildHaloAccumulateClearPlan): the ghost cells an accumulation reads are the cells a fill would clear afterwards, so the lane
// that loads them clears them.  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_take_kernel<VB, STREAM>                dst = src; src = 0.  Fastest dim contiguous on both sides: lane layout, workgroup
//                                               decode and batching of rows_kernel (kernels_rows.hip).
//   generic_take_kernel<ES>                     the same, element-wise (faces one element thick along the fastest memory axis).
//   rows_accumulate_take_kernel<T, VB, STREAM>  dst += src; src = 0.  Layout of rows_accumulate_kernel (kernels_accumulate.hip),
//                                               arithmetic of kernels_arith.h.
//   generic_accumulate_take_kernel<T, NC>       the same, element-wise (NC reals per element).
// The zero goes to the address the lane loaded from, with the width of that load: it is aligned whenever the load was, and it
// covers exactly the source cells of the move -- never a gap cell between rows.  Loads and stores are the plain loadVec /
// storeVec of kernels_dev.h on pointers that are NOT __restrict__: the compiler sees a load and a later store of the same
// bytes and keeps their order; the hardware keeps a wave's accesses to one address in order.  Source and destination cells of a
// list are disjoint (the planner's and the harness's contract), so no lane clears what another still has to read.  Local
// buffers only: no remote stores.
// Bound: HBM.  Algorithmic bytes per byte of the move: 3 for a take (source read, destination written, source written), 4 for
// an add-take (the destination is read as well).
#include "kernels_arith.h"
#include "kernels_dev.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

template <int N> __device__ __forceinline__ Bytes<N> zeroBytes() {
  Bytes<N> z = {};
  return z;
}

// ---------------------------------------------------------------------------------------------
// rows_take_kernel / rows_accumulate_take_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES.
// p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors.
// STREAM: 0 default caching; 1 (moves of 32 MiB and more): non-temporal source loads, non-temporal zero stores (the fill's rule
// for its stores) and, for the plain take, non-temporal destination stores (the row copy's rule).  The destination of an
// add-take is read and rewritten with the default policy, as in rows_accumulate_kernel.
// ---------------------------------------------------------------------------------------------
template <int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_take_kernel(const Batch b) {
  using V = Bytes<VB>;
  constexpr int POLICY = STREAM >= 1 ? ST_STREAM : ST_CACHED;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const int lg = b.p0[mi];
  const int lpr = 1 << lg;
  const int rb = kThreads >> lg;
  const unsigned int tc = b.t0[mi], tr = b.t1[mi];
  const unsigned int bc = lb % tc;
  const unsigned int rest = lb / tc;
  const unsigned int br = rest % tr;
  const long long plane = rest / tr;

  const long long col = (long long)bc * lpr + (threadIdx.x & (lpr - 1));
  const long long r0 = (long long)br * rb * kRowsUnroll + (threadIdx.x >> lg);
  if (col >= m.e[0]) return;
  char* s = const_cast<char*>(m.src) + plane * m.ss[2] + col * VB;  // (written too: the zeroes)
  char* d = m.dst + plane * m.ds[2] + col * VB;

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

template <typename T, int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_accumulate_take_kernel(const Batch b) {
  using V = Bytes<VB>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const int lg = b.p0[mi];
  const int lpr = 1 << lg;
  const int rb = kThreads >> lg;
  const unsigned int tc = b.t0[mi], tr = b.t1[mi];
  const unsigned int bc = lb % tc;
  const unsigned int rest = lb / tc;
  const unsigned int br = rest % tr;
  const long long plane = rest / tr;

  const long long col = (long long)bc * lpr + (threadIdx.x & (lpr - 1));
  const long long r0 = (long long)br * rb * kRowsUnroll + (threadIdx.x >> lg);
  if (col >= m.e[0]) return;
  char* s = const_cast<char*>(m.src) + plane * m.ss[2] + col * VB;  // (a wrap onto myself: both sides are slabs of one pencil)
  char* d = m.dst + plane * m.ds[2] + col * VB;

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
      storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(s + r * m.ss[1], zeroBytes<VB>());
    }
  }
}

// ---------------------------------------------------------------------------------------------
// generic_take_kernel / generic_accumulate_take_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there
// is one); extents and strides in ELEMENTS.  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <int ES>
__global__ __launch_bounds__(kThreads) void generic_take_kernel(const Batch b) {
  using E = Bytes<ES>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const unsigned int nb = b.first_block[mi + 1] - b.first_block[mi];
  const int f = b.p0[mi], g = (f + 1) % 3, h = (f + 2) % 3;
  const unsigned long long ef = m.e[f], eg = m.e[g];
  const unsigned long long total = ef * eg * (unsigned long long)m.e[h];
  char* src = const_cast<char*>(m.src);
  char* dst = m.dst;
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

template <typename T, int NC>
__global__ __launch_bounds__(kThreads) void generic_accumulate_take_kernel(const Batch b) {
  constexpr int ES = (int)sizeof(T) * NC;
  using E = Bytes<ES>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const unsigned int nb = b.first_block[mi + 1] - b.first_block[mi];
  const int f = b.p0[mi], g = (f + 1) % 3, h = (f + 2) % 3;
  const unsigned long long ef = m.e[f], eg = m.e[g];
  const unsigned long long total = ef * eg * (unsigned long long)m.e[h];
  char* src = const_cast<char*>(m.src);
  char* dst = m.dst;
  for (unsigned long long n = (unsigned long long)lb * kThreads + threadIdx.x; n < total;
       n += (unsigned long long)nb * kThreads) {
    const unsigned long long kf = n % ef, t = n / ef;
    const unsigned long long kg = t % eg, kh = t / eg;
    char* s = src + (long long)(kf * m.ss[f] + kg * m.ss[g] + kh * m.ss[h]) * ES;
    char* d = dst + (long long)(kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]) * ES;
    const E x = loadVec<false, ES>(s);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, x));
    storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  }
}

template <int VB>
void launchTakeRowsOf(int stream_access, const Batch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (stream_access == 1) rows_take_kernel<VB, 1><<<grid, block, 0, stream>>>(b);
  else rows_take_kernel<VB, 0><<<grid, block, 0, stream>>>(b);
}

template <typename T, int VB>
void launchAddTakeRowsOf(int stream_access, const Batch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (stream_access == 1) rows_accumulate_take_kernel<T, VB, 1><<<grid, block, 0, stream>>>(b);
  else rows_accumulate_take_kernel<T, VB, 0><<<grid, block, 0, stream>>>(b);
}

template <typename T>
bool launchAddTakeRowsOfType(int vb, int stream_access, const Batch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (vb == 16) {
    launchAddTakeRowsOf<T, 16>(stream_access, b, grid, block, stream);
    return true;
  }
  if (vb == 8) {
    launchAddTakeRowsOf<T, 8>(stream_access, b, grid, block, stream);
    return true;
  }
  if constexpr (sizeof(T) <= 4) {
    if (vb == 4) {
      launchAddTakeRowsOf<T, 4>(stream_access, b, grid, block, stream);
      return true;
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (vb == 2) {
      launchAddTakeRowsOf<T, 2>(stream_access, b, grid, block, stream);
      return true;
    }
  }
  return false;
}

template <typename T>
bool launchAddTakeGenericOfType(int nc, const Batch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (nc == 1) generic_accumulate_take_kernel<T, 1><<<grid, block, 0, stream>>>(b);
  else if (nc == 2) generic_accumulate_take_kernel<T, 2><<<grid, block, 0, stream>>>(b);
  else return false;
  return true;
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchTakeBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int vb = k.vec, s = streamArgOf(k.kind, k.access), es = k.es;
  bool ok = true;
  if (k.kind == K_ROWS_TAKE) {
    if (vb == 16) launchTakeRowsOf<16>(s, b, grid, block, stream);
    else if (vb == 8) launchTakeRowsOf<8>(s, b, grid, block, stream);
    else if (vb == 4) launchTakeRowsOf<4>(s, b, grid, block, stream);
    else if (vb == 2) launchTakeRowsOf<2>(s, b, grid, block, stream);
    else ok = false;
  } else if (k.kind == K_GENERIC_TAKE) {
    if (es == 2) generic_take_kernel<2><<<grid, block, 0, stream>>>(b);
    else if (es == 4) generic_take_kernel<4><<<grid, block, 0, stream>>>(b);
    else if (es == 8) generic_take_kernel<8><<<grid, block, 0, stream>>>(b);
    else if (es == 16) generic_take_kernel<16><<<grid, block, 0, stream>>>(b);
    else ok = false;
  } else if (k.kind == K_ROWS_ADD_TAKE) {
    switch (k.arith) {
      case ARITH_F16: ok = launchAddTakeRowsOfType<_Float16>(vb, s, b, grid, block, stream); break;
      case ARITH_BF16: ok = launchAddTakeRowsOfType<__bf16>(vb, s, b, grid, block, stream); break;
      case ARITH_F32: ok = launchAddTakeRowsOfType<float>(vb, s, b, grid, block, stream); break;
      case ARITH_F64: ok = launchAddTakeRowsOfType<double>(vb, s, b, grid, block, stream); break;
      default: ok = false; break;
    }
  } else if (k.kind == K_GENERIC_ADD_TAKE) {
    switch (k.arith) {
      case ARITH_F16: ok = launchAddTakeGenericOfType<_Float16>(es / 2, b, grid, block, stream); break;
      case ARITH_BF16: ok = es == 2 && launchAddTakeGenericOfType<__bf16>(1, b, grid, block, stream); break;
      case ARITH_F32: ok = launchAddTakeGenericOfType<float>(es / 4, b, grid, block, stream); break;
      case ARITH_F64: ok = launchAddTakeGenericOfType<double>(es / 8, b, grid, block, stream); break;
      default: ok = false; break;
    }
  } else {
    ok = false;
  }
  if (!ok) CD_INTERNAL_ERROR("no take kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
