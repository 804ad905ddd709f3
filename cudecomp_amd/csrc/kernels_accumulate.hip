// kernels_accumulate.hip -- add-moves (Move3D::add): dst = dst + src, element by element, in the arithmetic of the call's data
// type.  Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several).
//
// The only moves of the library that are not pure copies: the face additions of halo accumulation
// (cudecompAmdAccumulateHalos{X,Y,Z}, plan.h buildHaloAccumulatePlan).  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_accumulate_kernel<T, VB, STREAM>  fastest dim contiguous on both sides: lane layout, workgroup decode and batching of
//                                          rows_kernel (kernels_rows.hip; rowLane, kernels_walk.h) -- one (row, plane) decode per
//                                          WORKGROUP, kRowsUnroll vectors per lane in flight on EACH side.  A lane loads VB bytes
//                                          of the source and VB bytes of the destination, adds per element of T and stores VB
//                                          bytes.
//   generic_accumulate_kernel<T, NC>       element-wise (NC reals per element: 2 for the complex types), for everything else:
//                                          faces one element thick along the fastest memory axis, degenerate shapes.
// T: _Float16 (IEEE binary16 addition, packed), __bf16 (RNE-to-bf16 of the fp32 sum of the widened operands), float, double
// (kernels_arith.h: addPayload, shared with kernels_take.hip).
// The row kernel keeps its two unrolled loops written out (all loads, then all stores): through forRows its 8-byte-lane forms
// compile to other waits than these loops do (profiles/kernel_walk_refactor.md).  The element walk is forEachElement's.
// Only the cells of the move are read or written: no dense / shifted / window forms (those rewrite gap cells), no remote
// destinations.  Bound: HBM, 3 bytes moved per byte of the move (source read, destination read, destination written).
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_walk.h"

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
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  const char* s = m.src + l.plane * m.ss[2] + l.col * VB;  // (no __restrict__: a wrap onto myself adds one slab of a pencil to another)
  char* d = m.dst + l.plane * m.ds[2] + l.col * VB;

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
  const ElementWalk w = elementWalk(m.e, b.p0[mi], lb, b.first_block[mi + 1] - b.first_block[mi]);
  const char* src = m.src;
  char* dst = m.dst;
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    char* d = dst + (long long)(kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES;
    const E x = loadVec<false, ES>(src + (long long)(kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, x));
  });
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchAccumulateBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  const bool ok = dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    if (k.kind == K_ROWS_ADD)
      return dispatchLaneWidth<T>(k.vec, [&](auto w) {
        dispatchAccess(s, [&](auto a) { rows_accumulate_kernel<T, decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b); });
      });
    // (there is no complex bf16 type: the two-real form of bf16 is compiled here and never launched)
    return k.kind == K_GENERIC_ADD && (!std::is_same<T, __bf16>::value || k.es == 2) &&
           dispatchInt<1, 2>(k.es / (int)sizeof(T), [&](auto nc) { generic_accumulate_kernel<T, decltype(nc)::value><<<grid, block, 0, stream>>>(b); });
  });
  if (!ok) CD_INTERNAL_ERROR("no accumulation kernel for this arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
