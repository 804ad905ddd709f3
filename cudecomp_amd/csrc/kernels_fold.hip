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
//                                          decode and batching of rows_kernel (kernels_rows.hip; rowLane, kernels_walk.h; the two
//                                          unrolled loops stay written out, profiles/kernel_walk_refactor.md).  The mirror is the
//                                          SIGN of the source's row or plane stride in DevMove, as in rows_reflect_kernel: the
//                                          address arithmetic of rows_accumulate_kernel.  A lane loads VB bytes of source and of
//                                          destination, kRowsUnroll vectors of each in flight, XORs the source with the sign
//                                          mask, adds with addPayload<T, VB> (kernels_arith.h) and stores VB bytes.
//   generic_fold_kernel<T, NC, TAKE>       everything else, element by element (NC reals each) with a grid-stride loop: the
//                                          mirrored dim as the fastest memory axis (rows of h elements, reversed in themselves, a
//                                          row pitch apart) and the degenerate shapes; the element walk of kernels_walk.h with
//                                          signed indices.
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
#include "kernels_dispatch.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

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
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  char* s = const_cast<char*>(m.src) + l.plane * m.ss[2] + l.col * VB;  // (ghost and interior cells of one pencil; written with TAKE)
  char* d = m.dst + l.plane * m.ds[2] + l.col * VB;
  const V sign = signBits<VB>(mask);

  V x[kRowsUnroll], y[kRowsUnroll];
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = l.r0 + (long long)u * l.rb;
    if (r < m.e[1]) {
      x[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
      y[u] = loadVec<false, VB>(d + r * m.ds[1]);
    }
  }
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = l.r0 + (long long)u * l.rb;
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
  const ElementWalk w = elementWalk(m.e, b.p0[mi], lb, b.first_block[mi + 1] - b.first_block[mi]);
  char* src = const_cast<char*>(m.src);
  char* dst = m.dst;
  const E sign = signBits<ES>(mask);
  forEachElement<long long>(w, [&](long long kf, long long kg, long long kh) CD_INLINED {
    char* s = src + (kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES;
    char* d = dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES;
    const E x = loadVec<false, ES>(s);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, (E)(x ^ sign)));
    if constexpr (TAKE) storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  });
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchFoldBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  // all zero when the fold adds the ghost cells as they are
  const SignMask mask = k.neg ? signMaskOf(k.arith) : SignMask{{0, 0, 0, 0}};
  const bool rows = k.kind == K_ROWS_FOLD || k.kind == K_ROWS_FOLD_TAKE;
  const bool take = k.kind == K_ROWS_FOLD_TAKE || k.kind == K_GENERIC_FOLD_TAKE;
  const bool fold = rows || k.kind == K_GENERIC_FOLD || k.kind == K_GENERIC_FOLD_TAKE;
  // lanes never narrower than one real; there is no complex bf16 type: that element-wise form could never be launched
  const bool ok = fold && dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatchBool(take, [&](auto tk) {
      constexpr bool TAKE = decltype(tk)::value;
      if (rows)
        return dispatchLaneWidth<T>(k.vec, [&](auto w) {
          dispatchAccess(s, [&](auto a) {
            rows_fold_kernel<T, decltype(w)::value, decltype(a)::value, TAKE><<<grid, block, 0, stream>>>(b, mask);
          });
        });
      return dispatchReals<T>(k.es, [&](auto nc) { generic_fold_kernel<T, decltype(nc)::value, TAKE><<<grid, block, 0, stream>>>(b, mask); });
    });
  });
  if (!ok) CD_INTERNAL_ERROR("no fold kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
