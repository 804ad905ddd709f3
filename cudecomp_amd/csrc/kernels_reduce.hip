// kernels_reduce.hip -- reductions OF a box of cells (interior reductions, include/cudecomp_interior_reduce.h): sum, dot product
// and largest magnitude over exactly the cells of the box, for several fields in one launch.  Hand-written gfx950 (CDNA4 / MI355X)
// kernels; the first family here that moves no data: read-only and HBM-bound.  Compiled into the unit kernels_edge.hip.
//
// Two stages, no floating-point atomics, every order fixed:
//   reduce_rows_kernel<T, OP>           stage one, fastest dim contiguous.  Lanes lie on the 16-BYTE GRID of memory, from the boundary
//                                       below each row's start: every load is one naturally aligned 16-byte vector, and the reals of a
//                                       row's first and last vector that lie outside the row are masked (a select, so NaN or poison
//                                       there never reaches an accumulator).  A vector that is not wholly inside the readable range
//                                       the host names (the pencil) is read real by real instead, inside the row only.  Workgroup
//                                       decode and batching of rows_kernel (kernels_rows.hip): (256 >> p0) * kRowsUnroll rows x
//                                       (1 << p0) vectors per tile, all of a lane's loads before their first use.  The field's
//                                       workgroups stride over the tiles.  g.stream: non-temporal loads (boxes of kStreamBytes and more), a
//                                       uniform branch around the loads alone -- no second instantiation, for the size of the code object.
//   reduce_elements_kernel<T, OP>       stage one, element by element (grid-stride walk, forEachElement): the cross-check of the row
//                                       kernel and the form for boxes without a contiguous dim or with operands off each other's grid.
//   reduce_final_kernel<OP>             stage two: one workgroup per field combines that field's partials and writes its two results.
// T is the REAL type (complex elements are two of them), OP one of kReduce*.  Every lane keeps two fp64 accumulators: for the even
// and the odd real position counted from the row's start.  Complex elements: real and imaginary part.  Real elements: the two are
// combined when the lane is done.  All arithmetic is fp64 on exactly widened reals.  Per workgroup: the wave's 64 lanes combine by
// __shfl_xor (a butterfly: the same tree in every lane), the four waves through LDS in wave order, and ONE pair of partials goes to
// the workspace at (field * kReduceMaxBlocks + workgroup) with a plain 16-byte vector store.
//
// Complex DOT pairs the two reals of an element inside one vector: the host takes the row kernel for it only when every row starts
// on an element's boundary of the 16-byte grid, and for any DOT only when a and b share their phase on that grid (kernels.cc
// planReduce).
#include "kernels_dispatch.h"
#include "kernels_reduce_dev.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// (combine, realOf, loadReal, loadPieces, reduceRowTile, reduceElement and storePartials: kernels_reduce_dev.h, shared with
// kernels_profile.hip)

// ---------------------------------------------------------------------------------------------
// reduce_rows_kernel: g.slots = 16-byte slots per row (the most a row can touch), g.rows, g.planes; g.s1, g.s2 in BYTES;
// g.row_bytes, and g.last_row_bytes for the last row of every plane (a long single row is cut into rows of kReduceChunkBytes).
// blockIdx -> (field, workgroup of the field) once; the workgroup strides over the g.tiles tiles.
// ---------------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void reduce_rows_kernel(const ReduceGeom g, const ReduceFields fl, double* __restrict__ work) {
  const unsigned int field = blockIdx.x / g.blocks, wg = blockIdx.x % g.blocks;
  const char* __restrict__ const a = fl.a[field] + g.box_off;
  const char* __restrict__ const b = OP == kReduceDot ? fl.b[field] + g.box_off : nullptr;
  const bool cplx = g.reals == 2, stream = g.stream != 0;
  const int lg = g.p0, lpr = 1 << lg, rb = kThreads >> lg;
  const long long lane_col = threadIdx.x & (lpr - 1), lane_row = threadIdx.x >> lg;
  double acc0 = 0.0, acc1 = 0.0;

  for (unsigned long long tile = wg; tile < g.tiles; tile += g.blocks) {
    const unsigned long long bc = tile % g.t0, rest = tile / g.t0;
    const unsigned long long br = rest % g.t1, plane = rest / g.t1;
    const long long col = (long long)bc * lpr + lane_col;
    const long long r0 = (long long)br * rb * kRowsUnroll + lane_row;
    if (col >= g.slots) continue;
    const long long lo16 = col * 16;

    reduceRowTile<T, OP>(a, b, (long long)plane * g.s2, r0, rb, g.rows, g.s1, g.row_bytes, g.last_row_bytes, lo16, g.rd_lo, g.rd_hi, cplx,
                         stream, acc0, acc1);
  }
  if (!cplx) acc0 = combine<OP>(acc0, acc1), acc1 = 0.0;
  storePartials<OP>(acc0, acc1, work + 2 * ((size_t)field * kReduceMaxBlocks + wg));
}

// ---------------------------------------------------------------------------------------------
// reduce_elements_kernel: the field's g.blocks workgroups stride over the g.e[0] * g.e[1] * g.e[2] elements, lanes along dim g.p0;
// extents and strides g.s[] in ELEMENTS of g.reals reals.
// ---------------------------------------------------------------------------------------------
template <typename T, int OP>
__global__ __launch_bounds__(kThreads) void reduce_elements_kernel(const ReduceGeom g, const ReduceFields fl, double* __restrict__ work) {
  constexpr int RS = (int)sizeof(T);
  const unsigned int field = blockIdx.x / g.blocks, wg = blockIdx.x % g.blocks;
  const char* __restrict__ const a = fl.a[field] + g.box_off;
  const char* __restrict__ const b = OP == kReduceDot ? fl.b[field] + g.box_off : nullptr;
  const bool cplx = g.reals == 2;
  const long long es = (long long)g.reals * RS;
  const ElementWalk w = elementWalk(g.e, g.p0, wg, g.blocks);
  double acc0 = 0.0, acc1 = 0.0;
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    const long long off = (long long)(kf * g.s[w.f] + kg * g.s[w.g] + kh * g.s[w.h]) * es;
    reduceElement<T, OP>(a, b, off, cplx, acc0, acc1);
  });
  storePartials<OP>(acc0, acc1, work + 2 * ((size_t)field * kReduceMaxBlocks + wg));
}

// ---------------------------------------------------------------------------------------------
// reduce_final_kernel: workgroup f combines the nb pairs of partials of field f -- lane t the run [t * per, (t + 1) * per) in index
// order, per = ceil(nb / 256), so any number of partials is served; then the lanes as in stage one -- and writes results[2f],
// results[2f + 1].  nb == 0 (an empty box): +0.0.
// ---------------------------------------------------------------------------------------------
template <int OP>
__global__ __launch_bounds__(kThreads) void reduce_final_kernel(double* __restrict__ results, const double* __restrict__ work, unsigned int nb) {
  __shared__ double part[kThreads / 64][2];
  const unsigned int field = blockIdx.x;
  const double* const w = work + 2 * (size_t)field * kReduceMaxBlocks;
  const unsigned int per = (nb + kThreads - 1) / kThreads;
  const unsigned int first = threadIdx.x * per, end = first + per < nb ? first + per : nb;
  double acc0 = 0.0, acc1 = 0.0;
  for (unsigned int i = first; i < end; ++i) {
    acc0 = combine<OP>(acc0, w[2 * i]);
    acc1 = combine<OP>(acc1, w[2 * i + 1]);
  }
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) {
    acc0 = combine<OP>(acc0, __shfl_xor(acc0, mask, 64));
    acc1 = combine<OP>(acc1, __shfl_xor(acc1, mask, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) part[wave][0] = acc0, part[wave][1] = acc1;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r0 = part[0][0], r1 = part[0][1];
#pragma unroll
    for (int v = 1; v < kThreads / 64; ++v) r0 = combine<OP>(r0, part[v][0]), r1 = combine<OP>(r1, part[v][1]);
    results[2 * field] = r0;
    results[2 * field + 1] = r1;
  }
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchReduceStageOne(const KernelChoice& k, int op, const ReduceGeom& g, const ReduceFields& fields, double* work, hipStream_t stream) {
  if (k.kind != K_ROWS_REDUCE && k.kind != K_GENERIC_REDUCE) CD_INTERNAL_ERROR("not a reduction kernel");
  const dim3 grid(g.blocks * (unsigned int)g.n_fields), block(kThreads);
  const bool ok = dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    return dispatchInt<kReduceSum, kReduceDot, kReduceMaxAbs>(op, [&](auto o) {
      constexpr int OP = decltype(o)::value;
      if (k.kind == K_ROWS_REDUCE) {
        reduce_rows_kernel<T, OP><<<grid, block, 0, stream>>>(g, fields, work);
      } else {
        reduce_elements_kernel<T, OP><<<grid, block, 0, stream>>>(g, fields, work);
      }
    });
  });
  if (!ok) CD_INTERNAL_ERROR("no reduction kernel for this real type and operation");
  CD_CHECK_HIP(hipGetLastError());
}

void launchReduceFinal(int op, int n_fields, unsigned int partials, double* results, const double* work, hipStream_t stream) {
  const dim3 grid((unsigned int)n_fields), block(kThreads);
  const bool ok = dispatchInt<kReduceSum, kReduceDot, kReduceMaxAbs>(op, [&](auto o) {
    reduce_final_kernel<decltype(o)::value><<<grid, block, 0, stream>>>(results, work, partials);
  });
  if (!ok) CD_INTERNAL_ERROR("no final reduction kernel for this operation");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
