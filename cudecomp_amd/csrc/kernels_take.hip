// kernels_take.hip -- take-moves (Move3D::take): the move of its kind, then zero bytes into the source cells it has read.
// Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several).
//
// The moves of the fused halo accumulate-and-clear (cudecompAmdAccumulateAndClearHalos{X,Y,Z}, plan.h
// buildHaloAccumulateClearPlan): the ghost cells an accumulation reads are the cells a fill would clear afterwards, so the lane
// that loads them clears them.  Nothing like them exists in NVIDIA/cuDecomp.
//   rows_take_kernel<VB, STREAM>                dst = src; src = 0.  Fastest dim contiguous on both sides: lane layout, workgroup
//                                               decode and batching of rows_kernel (kernels_rows.hip) -- rowLane of kernels_walk.h,
//                                               shared in code by every family.
//   generic_take_kernel<ES>                     the same, element-wise (faces one element thick along the fastest memory axis):
//                                               the element walk of kernels_walk.h.
//   rows_accumulate_take_kernel<T, VB, STREAM>  dst += src; src = 0.  Layout of rows_accumulate_kernel (kernels_accumulate.hip),
//                                               arithmetic of kernels_arith.h.
//   generic_accumulate_take_kernel<T, NC>       the same, element-wise (NC reals per element).
// The zero goes to the address the lane loaded from, with the width of that load: it is aligned whenever the load was, and it
// covers exactly the source cells of the move -- never a gap cell between rows.  Loads and stores are the plain loadVec /
// storeVec of kernels_dev.h on pointers that are NOT __restrict__: the compiler sees a load and a later store of the same
// bytes and keeps their order; the hardware keeps a wave's accesses to one address in order.  Source and destination cells of a
// list are disjoint (the planner's and the harness's contract), so no lane clears what another still has to read.  Local
// buffers only: no remote stores.
// The two row kernels keep their two unrolled loops written out (all loads, then all stores, into arrays of the kernel's own):
// through forRows some of their instantiations compile to other register counts and waits than these loops do
// (profiles/kernel_walk_refactor.md).
// Bound: HBM.  Algorithmic bytes per byte of the move: 3 for a take (source read, destination written, source written), 4 for
// an add-take (the destination is read as well).
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

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
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  char* s = const_cast<char*>(m.src) + l.plane * m.ss[2] + l.col * VB;  // (written too: the zeroes)
  char* d = m.dst + l.plane * m.ds[2] + l.col * VB;

  V v[kRowsUnroll];
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = l.r0 + (long long)u * l.rb;
    if (r < m.e[1]) v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
  }
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = l.r0 + (long long)u * l.rb;
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
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  char* s = const_cast<char*>(m.src) + l.plane * m.ss[2] + l.col * VB;  // (a wrap onto myself: both sides are slabs of one pencil)
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
  const ElementWalk w = elementWalk(m.e, b.p0[mi], lb, b.first_block[mi + 1] - b.first_block[mi]);
  char* src = const_cast<char*>(m.src);
  char* dst = m.dst;
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    char* s = src + (long long)(kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES;
    const E x = loadVec<false, ES>(s);
    storeVec<ST_CACHED, ES>(dst + (long long)(kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES, x);
    storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  });
}

template <typename T, int NC>
__global__ __launch_bounds__(kThreads) void generic_accumulate_take_kernel(const Batch b) {
  constexpr int ES = (int)sizeof(T) * NC;
  using E = Bytes<ES>;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const ElementWalk w = elementWalk(m.e, b.p0[mi], lb, b.first_block[mi + 1] - b.first_block[mi]);
  char* src = const_cast<char*>(m.src);
  char* dst = m.dst;
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    char* s = src + (long long)(kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES;
    char* d = dst + (long long)(kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES;
    const E x = loadVec<false, ES>(s);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, x));
    storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  });
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchTakeBatch(const KernelChoice& k, const Batch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  bool ok = false;
  if (k.kind == K_ROWS_TAKE) {
    ok = dispatchLaneWidth<unsigned short>(k.vec, [&](auto w) {
      dispatchAccess(s, [&](auto a) { rows_take_kernel<decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b); });
    });
  } else if (k.kind == K_GENERIC_TAKE) {
    ok = dispatchElementSize(k.es, [&](auto es) { generic_take_kernel<decltype(es)::value><<<grid, block, 0, stream>>>(b); });
  } else if (k.kind == K_ROWS_ADD_TAKE || k.kind == K_GENERIC_ADD_TAKE) {
    ok = dispatchArith(k.arith, [&](auto t) {
      using T = typename decltype(t)::type;
      if (k.kind == K_ROWS_ADD_TAKE)
        return dispatchLaneWidth<T>(k.vec, [&](auto w) {
          dispatchAccess(s, [&](auto a) {
            rows_accumulate_take_kernel<T, decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b);
          });
        });
      // (there is no complex bf16 type: the two-real form of bf16 is compiled here and never launched)
      return (!std::is_same<T, __bf16>::value || k.es == 2) && dispatchInt<1, 2>(k.es / (int)sizeof(T), [&](auto nc) {
               generic_accumulate_take_kernel<T, decltype(nc)::value><<<grid, block, 0, stream>>>(b);
             });
    });
  }
  if (!ok) CD_INTERNAL_ERROR("no take kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
