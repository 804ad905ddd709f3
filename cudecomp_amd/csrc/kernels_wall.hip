// kernels_wall.hip -- wall-moves (Move3D::affine): a reflect-move that ADDS one value per ghost layer on the way,
// dst = src + a[layer] or dst = -src + a[layer], the source running BACKWARDS along one dim and `layer` the destination's index
// along that dim.  Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several, and
// why these are not appended to kernels_reflect.hip).
//
// The moves of cudecompAmdSetWallHalos{X,Y,Z} (include/cudecomp_halo_wall_values.h, plan.h buildHaloWallValuesPlan): the ghost cells
// at a non-periodic edge of the domain receive the mirror image of the interior plus the wall's data -- Dirichlet values (odd
// mirror, a = 2g) or Neumann data (even mirror, a_k = -+d_k q).  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_wall_kernel<T, VB, STREAM, NEG>   fastest dim contiguous on both sides and NOT the mirrored one: lane layout, workgroup
//                                          decode and batching of rows_reflect_kernel (rowLane and forRows of kernels_walk.h); the
//                                          mirror is the SIGN of the source's row or plane stride in DevMove.  After the optional
//                                          XOR with the sign mask every lane adds the addend of its destination layer -- the row or
//                                          the plane index, Batch::p1 says which -- with addPayload<T, VB> (kernels_arith.h).
//   generic_wall_kernel<T, ES, NEG>        everything else, element by element with a grid-stride loop: the mirrored dim as the
//                                          fastest memory axis, the degenerate shapes, forced element-wise runs; the element walk
//                                          of kernels_walk.h with signed indices.
// The addends are a kernel argument of their own (kern::WallTable; kern::Batch is unchanged): per move of the launch, per
// DESTINATION layer, the converted element replicated to 16 bytes.  The host has reversed the low side, so the kernels index by
// destination layer and pay nothing for the mirror.  Lanes are VB >= sizeof(element) bytes wide and start on an element's
// boundary, so the low VB bytes of an entry serve every lane: no phase.  The flip comes before the addition; the addition is the
// one the accumulation states (IEEE for binary16, fp32 and fp64; bf16: round-to-nearest-even of the fp32 sum), so -0 + 0 is +0
// and NaNs come out quiet: with all addends zero this is still not the reflection.
// Source and destination are disjoint cells of ONE buffer (interior and halo of a pencil): the pointers are not __restrict__.
// Exactly the destination cells of the move are stored and exactly its source cells loaded.  Local buffers only.
// Bound: HBM.  Algorithmic bytes per byte of the move: 2, as for the reflection; the table is 1 KB and stays in cache.
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// the low N bytes of the addend of destination layer `layer` of move `mi`.  The index is masked: the host never asks for a layer
// beyond the table (kernels.cc classifyReflect), and a read can never leave the kernel arguments.
template <int N> __device__ __forceinline__ Bytes<N> wallAddend(const WallTable& table, int mi, long long layer) {
  const unsigned int* w = table.w[mi][(int)layer & (kMaxWallHalo - 1)];
  if constexpr (N == 2) return (unsigned short)w[0];
  else if constexpr (N == 4) return w[0];
  else if constexpr (N == 8) return u32x2{w[0], w[1]};
  else return u32x4{w[0], w[1], w[2], w[3]};
}

// ---------------------------------------------------------------------------------------------
// rows_wall_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES, ss[1] or ss[2] negative for the
// mirrored dim.  p0 = log2(lanes per row); p1 = 1: the layer is the row index, 2: the plane index, anything else: layer 0.
// STREAM: 0 default caching; 1 (moves of 32 MiB and more): non-temporal loads and stores, the reflection's rule.
// ---------------------------------------------------------------------------------------------
template <typename T, int VB, int STREAM, bool NEG>
__global__ __launch_bounds__(kThreads) void rows_wall_kernel(const Batch b, const SignMask mask, const WallTable table) {
  using V = Bytes<VB>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  const char* s = m.src + l.plane * m.ss[2] + l.col * VB;
  char* d = m.dst + l.plane * m.ds[2] + l.col * VB;
  const int along = b.p1[mi];

  // the addends are loaded in the load phase, beside the payload: a row index differs from lane to lane, so the table is read with
  // vector loads (from the kernel arguments, always cached), and all of a lane's loads are in flight together
  V v[kRowsUnroll], a[kRowsUnroll];
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
    a[u] = wallAddend<VB>(table, mi, along == 1 ? r : (along == 2 ? l.plane : 0));
  });
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    if constexpr (NEG) v[u] ^= signBits<VB>(mask);
    storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], addPayload<T, VB>(v[u], a[u]));
  });
}

// ---------------------------------------------------------------------------------------------
// generic_wall_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one, otherwise the longest);
// extents and strides in ELEMENTS, the source stride of the mirrored dim negative; p1 = the mirrored entry of e[] (-1: one
// layer).  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <typename T, int ES, bool NEG>
__global__ __launch_bounds__(kThreads) void generic_wall_kernel(const Batch b, const SignMask mask, const WallTable table) {
  static_assert(ES % (int)sizeof(T) == 0 && ES / (int)sizeof(T) <= 2, "an element is one real or two");
  using E = Bytes<ES>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const ElementWalk w = elementWalk(m.e, b.p0[mi], lb, b.first_block[mi + 1] - b.first_block[mi]);
  const char* src = m.src;
  char* dst = m.dst;
  const int along = b.p1[mi];
  forEachElement<long long>(w, [&](long long kf, long long kg, long long kh) CD_INLINED {
    E x = loadVec<false, ES>(src + (kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES);
    if constexpr (NEG) x ^= signBits<ES>(mask);
    const long long layer = along == w.f ? kf : (along == w.g ? kg : (along == w.h ? kh : 0));
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES,
                            addPayload<T, ES>(x, wallAddend<ES>(table, mi, layer)));
  });
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchWallBatch(const KernelChoice& k, const Batch& b, const WallTable& table, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  const SignMask mask = k.neg ? signMaskOf(k.arith) : SignMask{{0, 0, 0, 0}};  // (unread when no sign is flipped)
  // the table's invariant: a lane holds whole elements, so the low bytes of a replicated entry are its addend at any column
  if (k.vec < k.es || k.es < 2 || 16 % k.es != 0) CD_INTERNAL_ERROR("wall-move whose lanes are narrower than one element");
  const bool rows = k.kind == K_ROWS_WALL;
  const bool ok = (rows || k.kind == K_GENERIC_WALL) && dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatchBool(k.neg, [&](auto neg) {
      constexpr bool NEG = decltype(neg)::value;
      if (rows)
        return dispatchLaneWidth<T>(k.vec, [&](auto w) {
          dispatchAccess(s, [&](auto a) {
            rows_wall_kernel<T, decltype(w)::value, decltype(a)::value, NEG><<<grid, block, 0, stream>>>(b, mask, table);
          });
        });
      return dispatchReals<T>(k.es, [&](auto nc) {
        generic_wall_kernel<T, decltype(nc)::value * (int)sizeof(T), NEG><<<grid, block, 0, stream>>>(b, mask, table);
      });
    });
  });
  if (!ok) CD_INTERNAL_ERROR("no wall kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
