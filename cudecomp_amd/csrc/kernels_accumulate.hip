// kernels_accumulate.hip -- add-moves (Move3D::add): dst = dst + src, element by element, in the arithmetic of the call's data
// type.  Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several).
//
// The only moves of the library that are not pure copies: the face additions of halo accumulation
// (cudecompAmdAccumulateHalos{X,Y,Z}, plan.h buildHaloAccumulatePlan).  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_accumulate_kernel<T, VB, STREAM>  fastest dim contiguous on both sides: lane layout, workgroup decode and batching of
//                                          rows_kernel (kernels_rows.hip) -- one (row, plane) decode per WORKGROUP, kRowsUnroll
//                                          vectors per lane in flight on EACH side.  A lane loads VB bytes of the source and VB
//                                          bytes of the destination, adds per element of T and stores VB bytes.
//   generic_accumulate_kernel<T, NC>       element-wise (NC reals per element: 2 for the complex types), for everything else:
//                                          faces one element thick along the fastest memory axis, degenerate shapes.
// T: _Float16 (IEEE binary16 addition, packed), __bf16 (RNE-to-bf16 of the fp32 sum of the widened operands), float, double
// (kernels_arith.h: addPayload, shared with kernels_take.hip).
// Only the cells of the move are read or written: no dense / shifted / window forms (those rewrite gap cells), no remote
// destinations.  Bound: HBM, 3 bytes moved per byte of the move (source read, destination read, destination written).
#include "kernels_arith.h"
#include "kernels_dev.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// ---------------------------------------------------------------------------------------------
// rows_accumulate_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES.
// p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors.
// STREAM: 0 default caching; 1 (moves of 32 MiB and more) the source is read once -> non-temporal loads.  The destination is
// read and rewritten with the default policy in both: non-temporal stores measured the same within 1 % from 64 MiB to 256 MiB
// (DESIGN.md section 4), so there is no such variant.
// ---------------------------------------------------------------------------------------------
template <typename T, int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_accumulate_kernel(const Batch b) {
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
  const char* s = m.src + plane * m.ss[2] + col * VB;  // (no __restrict__: a wrap onto myself adds one slab of a pencil to another)
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
    if (r < m.e[1]) storeVec<ST_CACHED, VB>(d + r * m.ds[1], addPayload<T, VB>(y[u], x[u]));
  }
}

// ---------------------------------------------------------------------------------------------
// generic_accumulate_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one); extents and
// strides in ELEMENTS of NC reals.
// ---------------------------------------------------------------------------------------------
template <typename T, int NC>
__global__ __launch_bounds__(kThreads) void generic_accumulate_kernel(const Batch b) {
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
  const char* src = m.src;
  char* dst = m.dst;
  for (unsigned long long n = (unsigned long long)lb * kThreads + threadIdx.x; n < total;
       n += (unsigned long long)nb * kThreads) {
    const unsigned long long kf = n % ef, t = n / ef;
    const unsigned long long kg = t % eg, kh = t / eg;
    char* d = dst + (long long)(kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]) * ES;
    const E x = loadVec<false, ES>(src + (long long)(kf * m.ss[f] + kg * m.ss[g] + kh * m.ss[h]) * ES);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, x));
  }
}

template <typename T, int VB>
void launchRowsOf(int stream_access, const Batch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (stream_access == 1) rows_accumulate_kernel<T, VB, 1><<<grid, block, 0, stream>>>(b);
  else rows_accumulate_kernel<T, VB, 0><<<grid, block, 0, stream>>>(b);
}

template <typename T>
bool launchRowsOfType(int vb, int stream_access, const Batch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (vb == 16) {
    launchRowsOf<T, 16>(stream_access, b, grid, block, stream);
    return true;
  }
  if (vb == 8) {
    launchRowsOf<T, 8>(stream_access, b, grid, block, stream);
    return true;
  }
  if constexpr (sizeof(T) <= 4) {
    if (vb == 4) {
      launchRowsOf<T, 4>(stream_access, b, grid, block, stream);
      return true;
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (vb == 2) {
      launchRowsOf<T, 2>(stream_access, b, grid, block, stream);
      return true;
    }
  }
  return false;
}

template <typename T>
bool launchGenericOfType(int nc, const Batch& b, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (nc == 1) generic_accumulate_kernel<T, 1><<<grid, block, 0, stream>>>(b);
  else if (nc == 2) generic_accumulate_kernel<T, 2><<<grid, block, 0, stream>>>(b);
  else return false;
  return true;
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchAccumulateBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int vb = k.vec, s = streamArgOf(k.kind, k.access), es = k.es;
  bool ok = false;
  if (k.kind == K_ROWS_ADD) {
    switch (k.arith) {
      case ARITH_F16: ok = launchRowsOfType<_Float16>(vb, s, b, grid, block, stream); break;
      case ARITH_BF16: ok = launchRowsOfType<__bf16>(vb, s, b, grid, block, stream); break;
      case ARITH_F32: ok = launchRowsOfType<float>(vb, s, b, grid, block, stream); break;
      case ARITH_F64: ok = launchRowsOfType<double>(vb, s, b, grid, block, stream); break;
      default: break;
    }
  } else if (k.kind == K_GENERIC_ADD) {
    switch (k.arith) {
      case ARITH_F16: ok = launchGenericOfType<_Float16>(es / 2, b, grid, block, stream); break;
      case ARITH_BF16: ok = es == 2 && launchGenericOfType<__bf16>(1, b, grid, block, stream); break;
      case ARITH_F32: ok = launchGenericOfType<float>(es / 4, b, grid, block, stream); break;
      case ARITH_F64: ok = launchGenericOfType<double>(es / 8, b, grid, block, stream); break;
      default: break;
    }
  }
  if (!ok) CD_INTERNAL_ERROR("no accumulation kernel for this arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
