// kernels_wall_plane.hip -- wall-plane moves (Move3D::plane): a reflect-move with a THIRD operand in device memory,
// dst = src + plane or dst = -src + plane, the source running BACKWARDS along one dim and the plane entry that of the destination
// cell.  Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several, and why these
// are not appended to kernels_wall.hip).
//
// The moves of cudecompAmdSetWallPlaneHalos{X,Y,Z} (include/cudecomp_halo_wall_planes.h, plan.h buildHaloWallPlanesPlan): the ghost
// cells at a non-periodic edge of the domain receive the mirror image of the interior plus wall data that varies ALONG the wall -- an
// inflow plane, blowing and suction, a heated patch, a flux map.  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_wall_plane_kernel<T, VB, STREAM, NEG>   fastest dim contiguous on all THREE operands and NOT the mirrored one: lane layout,
//                                                workgroup decode and batching of rows_wall_kernel (locate, rowLane and forRows of
//                                                kernels_walk.h); the mirror is the SIGN of the source's row or plane stride in
//                                                DevMove, and of the plane's on a low side.  In the load phase a lane issues its
//                                                source vectors AND its plane vectors before any use: 2 x kRowsUnroll loads of VB
//                                                bytes in flight.  Then the optional XOR with the sign mask, addPayload<T, VB>
//                                                (kernels_arith.h) and the store.
//   generic_wall_plane_kernel<T, ES, NEG>        everything else, element by element with a grid-stride loop: the mirrored dim as the
//                                                fastest memory axis, the degenerate shapes, forced element-wise runs; the element
//                                                walk of kernels_walk.h with signed indices, the plane addressed by the same
//                                                (kf, kg, kh) through its own strides.
// The third operand is a kernel argument of its own (kern::PlaneOperands; kern::Batch is unchanged): per move of the launch one
// pointer and three signed strides.  The values stay in device memory and are read when the kernel runs.  The flip comes before
// the addition; the addition is the one the accumulation states (IEEE for binary16, fp32 and fp64; bf16: round-to-nearest-even of
// the fp32 sum).
// Source and destination are disjoint cells of ONE buffer (interior and halo of a pencil): the pointers are not __restrict__.
// Exactly the destination cells of the move are stored; exactly its source cells and the matching plane entries are loaded.  Local
// buffers only.  STREAM follows the reflection's rule; the plane is read once per call, so it streams with the payload.
// Bound: HBM.  Algorithmic bytes per byte of the move: 3 (mirror read, plane read, ghost write).  No rate has been measured.
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// ---------------------------------------------------------------------------------------------
// rows_wall_plane_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] and the operand's s[1], s[2] in BYTES,
// negative for the mirrored dim (source always, the plane on a low side).  p0 = log2(lanes per row); p1 is not read.
// STREAM: 0 default caching; 1 (moves of 32 MiB and more): non-temporal loads and stores, the reflection's rule.
// ---------------------------------------------------------------------------------------------
template <typename T, int VB, int STREAM, bool NEG>
__global__ __launch_bounds__(kThreads) void rows_wall_plane_kernel(const Batch b, const SignMask mask, const PlaneOperands planes) {
  using V = Bytes<VB>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const PlaneOperand& po = planes.m[mi];
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  const char* s = m.src + l.plane * m.ss[2] + l.col * VB;
  const char* p = po.p + l.plane * po.s[2] + l.col * VB;
  char* d = m.dst + l.plane * m.ds[2] + l.col * VB;

  // all of a lane's loads, of both read operands, are in flight before the first use
  V v[kRowsUnroll], a[kRowsUnroll];
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
    a[u] = loadVec<(STREAM >= 1), VB>(p + r * po.s[1]);
  });
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    if constexpr (NEG) v[u] ^= signBits<VB>(mask);
    storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], addPayload<T, VB>(v[u], a[u]));
  });
}

// ---------------------------------------------------------------------------------------------
// generic_wall_plane_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one, otherwise the longest);
// extents and strides in ELEMENTS, signed.  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <typename T, int ES, bool NEG>
__global__ __launch_bounds__(kThreads) void generic_wall_plane_kernel(const Batch b, const SignMask mask, const PlaneOperands planes) {
  static_assert(ES % (int)sizeof(T) == 0 && ES / (int)sizeof(T) <= 2, "an element is one real or two");
  using E = Bytes<ES>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const PlaneOperand& po = planes.m[mi];
  const ElementWalk w = elementWalk(m.e, b.p0[mi], lb, b.first_block[mi + 1] - b.first_block[mi]);
  const char* src = m.src;
  const char* pl = po.p;
  char* dst = m.dst;
  forEachElement<long long>(w, [&](long long kf, long long kg, long long kh) CD_INLINED {
    E x = loadVec<false, ES>(src + (kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES);
    const E a = loadVec<false, ES>(pl + (kf * po.s[w.f] + kg * po.s[w.g] + kh * po.s[w.h]) * ES);
    if constexpr (NEG) x ^= signBits<ES>(mask);
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES, addPayload<T, ES>(x, a));
  });
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchWallPlaneBatch(const KernelChoice& k, const Batch& b, const PlaneOperands& planes, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  const SignMask mask = k.neg ? signMaskOf(k.arith) : SignMask{{0, 0, 0, 0}};  // (unread when no sign is flipped)
  if (k.vec < k.es || k.es < 2 || 16 % k.es != 0) CD_INTERNAL_ERROR("wall-plane move whose lanes are narrower than one element");
  for (int i = 0; i < b.n; ++i)
    if (!planes.m[i].p) CD_INTERNAL_ERROR("wall-plane move without its plane");
  const bool rows = k.kind == K_ROWS_WALL_PLANE;
  const bool ok = (rows || k.kind == K_GENERIC_WALL_PLANE) && dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatchBool(k.neg, [&](auto neg) {
      constexpr bool NEG = decltype(neg)::value;
      if (rows)
        return dispatchLaneWidth<T>(k.vec, [&](auto w) {
          dispatchAccess(s, [&](auto a) {
            rows_wall_plane_kernel<T, decltype(w)::value, decltype(a)::value, NEG><<<grid, block, 0, stream>>>(b, mask, planes);
          });
        });
      return dispatchReals<T>(k.es, [&](auto nc) {
        generic_wall_plane_kernel<T, decltype(nc)::value * (int)sizeof(T), NEG><<<grid, block, 0, stream>>>(b, mask, planes);
      });
    });
  });
  if (!ok) CD_INTERNAL_ERROR("no wall-plane kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
