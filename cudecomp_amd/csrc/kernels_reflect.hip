// kernels_reflect.hip -- reflect-moves (Move3D::reflect): a copy whose source runs BACKWARDS along one dim, optionally with the
// sign bit of every real component inverted (Move3D::negate).  Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object
// (kernels_batch.h says why there are several).
//
// The moves of halo reflection (cudecompAmdReflectHalos{X,Y,Z}, plan.h buildHaloReflectPlan): the ghost cells at a non-periodic
// edge of the domain receive the mirror image of the interior -- the even mirror (zero gradient) as it is, the odd one (no-slip
// walls) with the sign flipped.  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_reflect_kernel<VB, STREAM, NEG>   fastest dim contiguous on both sides and NOT the mirrored one: lane layout, workgroup
//                                          decode and batching of rows_kernel (kernels_rows.hip).  The mirror is the SIGN of the
//                                          source's row or plane stride in DevMove (the launcher folds it in), so the kernel pays
//                                          nothing for it: the same address arithmetic as the row copy.
//   generic_reflect_kernel<ES, NEG>        everything else, element by element with a grid-stride loop: the mirrored dim as the
//                                          fastest memory axis (rows of h elements, reversed in themselves, a row pitch apart)
//                                          and the degenerate shapes.
// NEG: every loaded vector is XORed with a sign mask before the store -- bit 8 * sizeof(real) - 1 of every real.  The mask is a
// 16-byte kernel argument of its own (kern::Batch is unchanged); lanes are VB >= sizeof(real) bytes wide and start on a real's
// boundary, so the low VB bytes of the mask serve every lane: no phase.  Pure bit movement: -0 becomes +0, NaN payloads and
// infinities keep every other bit, nothing is converted or rounded.
// Source and destination are disjoint cells of ONE buffer (interior and halo of a pencil): the pointers are not __restrict__.
// Exactly the destination cells of the move are stored and exactly its source cells loaded.  Local buffers only.
// Bound: HBM.  Algorithmic bytes per byte of the move: 2, as for a copy.
#include "kernels_dev.h"

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

// ---------------------------------------------------------------------------------------------
// rows_reflect_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES, ss[1] or ss[2] negative for
// the mirrored dim.  p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors.
// STREAM: 0 default caching; 1 (moves of 32 MiB and more): non-temporal loads and stores, the row copy's rule.
// ---------------------------------------------------------------------------------------------
template <int VB, int STREAM, bool NEG>
__global__ __launch_bounds__(kThreads) void rows_reflect_kernel(const Batch b, const SignMask mask) {
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
  const char* s = m.src + plane * m.ss[2] + col * VB;
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
      if constexpr (NEG) v[u] ^= signBits<VB>(mask);
      storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], v[u]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// generic_reflect_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one, otherwise the longest);
// extents and strides in ELEMENTS, the source stride of the mirrored dim negative.  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <int ES, bool NEG>
__global__ __launch_bounds__(kThreads) void generic_reflect_kernel(const Batch b, const SignMask mask) {
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
    const long long kf = (long long)(n % ef), t = (long long)(n / ef);
    const long long kg = t % (long long)eg, kh = t / (long long)eg;
    E x = loadVec<false, ES>(src + (kf * m.ss[f] + kg * m.ss[g] + kh * m.ss[h]) * ES);
    if constexpr (NEG) x ^= signBits<ES>(mask);
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]) * ES, x);
  }
}

template <int VB, bool NEG>
void launchReflectRowsOf(int stream_access, const Batch& b, const SignMask& mask, const dim3& grid, const dim3& block,
                         hipStream_t stream) {
  if (stream_access == 1) rows_reflect_kernel<VB, 1, NEG><<<grid, block, 0, stream>>>(b, mask);
  else rows_reflect_kernel<VB, 0, NEG><<<grid, block, 0, stream>>>(b, mask);
}

template <bool NEG>
bool launchReflectOf(const KernelChoice& k, const Batch& b, const SignMask& mask, const dim3& grid, const dim3& block,
                     hipStream_t stream) {
  const int vb = k.vec, s = streamArgOf(k.kind, k.access), es = k.es;
  if (k.kind == K_ROWS_REFLECT) {
    if (vb == 16) launchReflectRowsOf<16, NEG>(s, b, mask, grid, block, stream);
    else if (vb == 8) launchReflectRowsOf<8, NEG>(s, b, mask, grid, block, stream);
    else if (vb == 4) launchReflectRowsOf<4, NEG>(s, b, mask, grid, block, stream);
    else if (vb == 2) launchReflectRowsOf<2, NEG>(s, b, mask, grid, block, stream);
    else return false;
    return true;
  }
  if (k.kind == K_GENERIC_REFLECT) {
    if (es == 2) generic_reflect_kernel<2, NEG><<<grid, block, 0, stream>>>(b, mask);
    else if (es == 4) generic_reflect_kernel<4, NEG><<<grid, block, 0, stream>>>(b, mask);
    else if (es == 8) generic_reflect_kernel<8, NEG><<<grid, block, 0, stream>>>(b, mask);
    else if (es == 16) generic_reflect_kernel<16, NEG><<<grid, block, 0, stream>>>(b, mask);
    else return false;
    return true;
  }
  return false;
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchReflectBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  // the sign bit of every real in 16 bytes: 2-byte reals 0x8000 in every half word, 4-byte reals the top bit of every word,
  // 8-byte reals the top bit of every second word (little endian)
  SignMask mask = {{0, 0, 0, 0}};
  bool ok = true;
  switch (k.arith) {
    case ARITH_NONE: break;
    case ARITH_F16:
    case ARITH_BF16: mask = {{0x80008000u, 0x80008000u, 0x80008000u, 0x80008000u}}; break;
    case ARITH_F32: mask = {{0x80000000u, 0x80000000u, 0x80000000u, 0x80000000u}}; break;
    case ARITH_F64: mask = {{0u, 0x80000000u, 0u, 0x80000000u}}; break;
    default: ok = false; break;
  }
  if (ok) ok = k.arith != ARITH_NONE ? launchReflectOf<true>(k, b, mask, grid, block, stream)
                                     : launchReflectOf<false>(k, b, mask, grid, block, stream);
  if (!ok) CD_INTERNAL_ERROR("no reflect kernel for this kind, real type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
