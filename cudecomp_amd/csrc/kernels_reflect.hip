// kernels_reflect.hip -- reflect-moves (Move3D::reflect): a copy whose source runs BACKWARDS along one dim, optionally with the
// sign bit of every real component inverted (Move3D::negate).  Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object
// (kernels_batch.h says why there are several).
//
// The moves of halo reflection (cudecompAmdReflectHalos{X,Y,Z}, plan.h buildHaloReflectPlan): the ghost cells at a non-periodic
// edge of the domain receive the mirror image of the interior -- the even mirror (zero gradient) as it is, the odd one (no-slip
// walls) with the sign flipped.  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_reflect_kernel<VB, STREAM, NEG>   fastest dim contiguous on both sides and NOT the mirrored one: lane layout, workgroup
//                                          decode and batching of rows_kernel (kernels_rows.hip): rowLane and forRows of
//                                          kernels_walk.h.  The mirror is the SIGN of the source's row or plane stride in DevMove
//                                          (the launcher folds it in), so the kernel pays nothing for it: the same address
//                                          arithmetic as the row copy.
//   generic_reflect_kernel<ES, NEG>        everything else, element by element with a grid-stride loop: the mirrored dim as the
//                                          fastest memory axis (rows of h elements, reversed in themselves, a row pitch apart)
//                                          and the degenerate shapes; the element walk of kernels_walk.h with signed indices.
// NEG: every loaded vector is XORed with a sign mask before the store -- bit 8 * sizeof(real) - 1 of every real.  The mask is a
// 16-byte kernel argument of its own (kern::Batch is unchanged); lanes are VB >= sizeof(real) bytes wide and start on a real's
// boundary, so the low VB bytes of the mask serve every lane: no phase.  Pure bit movement: -0 becomes +0, NaN payloads and
// infinities keep every other bit, nothing is converted or rounded.
// Source and destination are disjoint cells of ONE buffer (interior and halo of a pencil): the pointers are not __restrict__.
// Exactly the destination cells of the move are stored and exactly its source cells loaded.  Local buffers only.
// Bound: HBM.  Algorithmic bytes per byte of the move: 2, as for a copy.
#include "kernels_dispatch.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

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
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  const char* s = m.src + l.plane * m.ss[2] + l.col * VB;
  char* d = m.dst + l.plane * m.ds[2] + l.col * VB;

  V v[kRowsUnroll];
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED { v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]); });
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    if constexpr (NEG) v[u] ^= signBits<VB>(mask);
    storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], v[u]);
  });
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
  const ElementWalk w = elementWalk(m.e, b.p0[mi], lb, b.first_block[mi + 1] - b.first_block[mi]);
  const char* src = m.src;
  char* dst = m.dst;
  forEachElement<long long>(w, [&](long long kf, long long kg, long long kh) CD_INLINED {
    E x = loadVec<false, ES>(src + (kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES);
    if constexpr (NEG) x ^= signBits<ES>(mask);
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES, x);
  });
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchReflectBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  const SignMask mask = signMaskOf(k.arith);  // (all zero and unread when no sign is flipped)
  const bool known = k.arith >= ARITH_NONE && k.arith <= ARITH_F64;
  const bool ok = known && dispatchBool(k.arith != ARITH_NONE, [&](auto neg) {
    constexpr bool NEG = decltype(neg)::value;
    if (k.kind == K_ROWS_REFLECT)
      return dispatchLaneWidth<unsigned short>(k.vec, [&](auto w) {
        dispatchAccess(s, [&](auto a) {
          rows_reflect_kernel<decltype(w)::value, decltype(a)::value, NEG><<<grid, block, 0, stream>>>(b, mask);
        });
      });
    return k.kind == K_GENERIC_REFLECT && dispatchElementSize(k.es, [&](auto es) {
             generic_reflect_kernel<decltype(es)::value, NEG><<<grid, block, 0, stream>>>(b, mask);
           });
  });
  if (!ok) CD_INTERNAL_ERROR("no reflect kernel for this kind, real type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
