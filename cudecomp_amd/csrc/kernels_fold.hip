// kernels_fold.hip -- fold-moves (Move3D::reflect with Move3D::add): an addition whose source runs BACKWARDS along one dim,
// optionally with the sign bit of every real component of the source inverted first (Move3D::negate) and with zero bytes stored
// to the source cells afterwards (Move3D::take).  Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object
// (kernels_batch.h says why there are several).
//
// The moves of halo folding (cudecompAmdFoldHalos{X,Y,Z}, plan.h buildHaloFoldPlan), the transpose of the reflection
// (kernels_reflect.hip): what a scatter has left in the ghost cells beyond a non-periodic edge of the domain is added onto the
// interior cells those ghosts mirror -- as it is at a symmetry plane, with the sign flipped at an odd wall.  Nothing like them
// exists in NVIDIA/cuDecomp.
//   rows_fold_kernel<T, VB, STREAM, TAKE>  fastest dim contiguous on both sides and NOT the mirrored one: lane layout, workgroup
//                                          decode and batching of rows_kernel (kernels_rows.hip).  The mirror is the SIGN of the
//                                          source's row or plane stride in DevMove, as in rows_reflect_kernel: the address
//                                          arithmetic of rows_accumulate_kernel.  A lane loads VB bytes of source and of
//                                          destination, kRowsUnroll vectors of each in flight, XORs the source with the sign mask,
//                                          adds with addPayload<T, VB> (kernels_arith.h) and stores VB bytes.
//   generic_fold_kernel<T, NC, TAKE>       everything else, element by element (NC reals each) with a grid-stride loop: the
//                                          mirrored dim as the fastest memory axis (rows of h elements, reversed in themselves, a
//                                          row pitch apart) and the degenerate shapes.
// The sign mask -- bit 8 * sizeof(T) - 1 of every T in 16 bytes -- is a kernel argument of its own and all zero for parity +1:
// parity is not a template argument.  One XOR per dword on an HBM-bound kernel keeps the code object half the size.  Lanes are
// VB >= sizeof(T) bytes wide and start on a real's boundary, so the low VB bytes of the mask serve every lane.  The flip comes
// before the addition: the addend of a ghost +0 is -0, and nothing is ever subtracted.
// TAKE: the zero goes to the address the lane loaded the source from, at the width of that load, after the load -- the pointers
// are NOT __restrict__, the compiler keeps a load and a later store of the same bytes in order, the hardware keeps a wave's
// accesses to one address in order (kernels_take.hip).  Source cells are disjoint from all destination cells of the launch.
// Exactly the destination cells of the move are loaded and stored, exactly its source cells loaded (and cleared).  Local buffers only.
// Bound: HBM.  Algorithmic bytes per byte of the move: 3 (source read, destination read and written), 4 with TAKE.
#include "kernels_arith.h"
#include "kernels_dev.h"

#include <type_traits>

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

template <int N> __device__ __forceinline__ Bytes<N> signBits(const SignMask& mask) {
  if constexpr (N == 2) return (unsigned short)mask.w[0];
  else if constexpr (N == 4) return mask.w[0];
  else if constexpr (N == 8) return u32x2{mask.w[0], mask.w[1]};
  else return u32x4{mask.w[0], mask.w[1], mask.w[2], mask.w[3]};
}

template <int N> __device__ __forceinline__ Bytes<N> zeroBytes() {
  Bytes<N> z = {};
  return z;
}

// ---------------------------------------------------------------------------------------------
// rows_fold_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES, ss[1] or ss[2] negative for the
// mirrored dim.  p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors.
// STREAM: 0 default caching; 1 (moves of 32 MiB and more): non-temporal source loads and zero stores; the destination is read
// and rewritten with the default policy, as in rows_accumulate_kernel.
// ---------------------------------------------------------------------------------------------
template <typename T, int VB, int STREAM, bool TAKE>
__global__ __launch_bounds__(kThreads) void rows_fold_kernel(const Batch b, const SignMask mask) {
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
  char* s = const_cast<char*>(m.src) + plane * m.ss[2] + col * VB;  // (ghost and interior cells of one pencil; written with TAKE)
  char* d = m.dst + plane * m.ds[2] + col * VB;
  const V sign = signBits<VB>(mask);

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
      storeVec<ST_CACHED, VB>(d + r * m.ds[1], addPayload<T, VB>(y[u], (V)(x[u] ^ sign)));
      if constexpr (TAKE) storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(s + r * m.ss[1], zeroBytes<VB>());
    }
  }
}

// ---------------------------------------------------------------------------------------------
// generic_fold_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one, otherwise the longest);
// extents and strides in ELEMENTS, the source stride of the mirrored dim negative.  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <typename T, int NC, bool TAKE>
__global__ __launch_bounds__(kThreads) void generic_fold_kernel(const Batch b, const SignMask mask) {
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
  const E sign = signBits<ES>(mask);
  for (unsigned long long n = (unsigned long long)lb * kThreads + threadIdx.x; n < total;
       n += (unsigned long long)nb * kThreads) {
    const long long kf = (long long)(n % ef), t = (long long)(n / ef);
    const long long kg = t % (long long)eg, kh = t / (long long)eg;
    char* s = src + (kf * m.ss[f] + kg * m.ss[g] + kh * m.ss[h]) * ES;
    char* d = dst + (kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]) * ES;
    const E x = loadVec<false, ES>(s);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, (E)(x ^ sign)));
    if constexpr (TAKE) storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  }
}

template <typename T, int VB, bool TAKE>
void launchFoldRowsOf(int stream_access, const Batch& b, const SignMask& mask, const dim3& grid, const dim3& block,
                      hipStream_t stream) {
  if (stream_access == 1) rows_fold_kernel<T, VB, 1, TAKE><<<grid, block, 0, stream>>>(b, mask);
  else rows_fold_kernel<T, VB, 0, TAKE><<<grid, block, 0, stream>>>(b, mask);
}

// lanes never narrower than one real: 8-byte reals take 16 or 8 bytes, 4-byte reals 4 as well, 2-byte reals 2 as well
template <typename T, bool TAKE>
bool launchFoldRowsOfType(int vb, int stream_access, const Batch& b, const SignMask& mask, const dim3& grid, const dim3& block,
                          hipStream_t stream) {
  if (vb == 16) {
    launchFoldRowsOf<T, 16, TAKE>(stream_access, b, mask, grid, block, stream);
    return true;
  }
  if (vb == 8) {
    launchFoldRowsOf<T, 8, TAKE>(stream_access, b, mask, grid, block, stream);
    return true;
  }
  if constexpr (sizeof(T) <= 4) {
    if (vb == 4) {
      launchFoldRowsOf<T, 4, TAKE>(stream_access, b, mask, grid, block, stream);
      return true;
    }
  }
  if constexpr (sizeof(T) == 2) {
    if (vb == 2) {
      launchFoldRowsOf<T, 2, TAKE>(stream_access, b, mask, grid, block, stream);
      return true;
    }
  }
  return false;
}

template <typename T, bool TAKE>
bool launchFoldGenericOfType(int nc, const Batch& b, const SignMask& mask, const dim3& grid, const dim3& block, hipStream_t stream) {
  if (nc == 1) {
    generic_fold_kernel<T, 1, TAKE><<<grid, block, 0, stream>>>(b, mask);
    return true;
  }
  if constexpr (!std::is_same<T, __bf16>::value) {  // (there is no complex bf16 type: that form could never be launched)
    if (nc == 2) {
      generic_fold_kernel<T, 2, TAKE><<<grid, block, 0, stream>>>(b, mask);
      return true;
    }
  }
  return false;
}

template <typename T, bool TAKE>
bool launchFoldOfType(const KernelChoice& k, bool rows, const Batch& b, const SignMask& mask, const dim3& grid, const dim3& block,
                      hipStream_t stream) {
  if (rows) return launchFoldRowsOfType<T, TAKE>(k.vec, streamArgOf(k.kind, k.access), b, mask, grid, block, stream);
  return launchFoldGenericOfType<T, TAKE>(k.es / (int)sizeof(T), b, mask, grid, block, stream);
}

template <bool TAKE>
bool launchFoldOf(const KernelChoice& k, bool rows, const Batch& b, const SignMask& mask, const dim3& grid, const dim3& block,
                  hipStream_t stream) {
  switch (k.arith) {
    case ARITH_F16: return launchFoldOfType<_Float16, TAKE>(k, rows, b, mask, grid, block, stream);
    case ARITH_BF16: return (rows || k.es == 2) && launchFoldOfType<__bf16, TAKE>(k, rows, b, mask, grid, block, stream);
    case ARITH_F32: return launchFoldOfType<float, TAKE>(k, rows, b, mask, grid, block, stream);
    case ARITH_F64: return launchFoldOfType<double, TAKE>(k, rows, b, mask, grid, block, stream);
    default: return false;
  }
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchFoldBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  // the sign bit of every real in 16 bytes (kernels_reflect.hip); all zero when the fold adds the ghost cells as they are
  SignMask mask = {{0, 0, 0, 0}};
  if (k.neg) {
    switch (k.arith) {
      case ARITH_F16:
      case ARITH_BF16: mask = {{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u}}; break;
      case ARITH_F32: mask = {{0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u}}; break;
      case ARITH_F64: mask = {{0u, 0x80000000u, 0u, 0x80000000u}}; break;
      default: break;
    }
  }
  const bool rows = k.kind == K_ROWS_FOLD || k.kind == K_ROWS_FOLD_TAKE;
  const bool take = k.kind == K_ROWS_FOLD_TAKE || k.kind == K_GENERIC_FOLD_TAKE;
  const bool fold = rows || k.kind == K_GENERIC_FOLD || k.kind == K_GENERIC_FOLD_TAKE;
  const bool ok = fold && (take ? launchFoldOf<true>(k, rows, b, mask, grid, block, stream)
                                : launchFoldOf<false>(k, rows, b, mask, grid, block, stream));
  if (!ok) CD_INTERNAL_ERROR("no fold kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
