// kernels_fill.hip -- fill-moves (Move3D::fill): dst = one value, over exactly the cells of the move.  Hand-written gfx950
// (CDNA4 / MI355X) kernels, one small code object (kernels_batch.h says why there are several).
//
// The moves of halo fill (cudecompAmdFillHalos{X,Y,Z}, plan.h buildHaloFillPlan).  Nothing like them exists in NVIDIA/cuDecomp.
// A pure store stream: the kernels issue NO loads from the destination, so a solver may write the neighbouring cells from
// another stream meanwhile -- no dense / shifted / window forms (those read and rewrite gap cells), no remote destinations.
//   rows_fill_kernel<VB, STREAM>  fastest dim contiguous in the destination.  Workgroup decode and batching of rows_kernel
//                                 (kernels_rows.hip; rowLane, kernels_walk.h): one (row, plane) decode per WORKGROUP, kRowsUnroll
//                                 stores per lane in flight.  A fill has no source alignment to respect, so the lanes lie on the
//                                 destination's VB = 16-byte grid, from the boundary below each row's start: the body of every
//                                 row is stored as whole, naturally aligned 16-byte vectors whatever the row's base (2-byte
//                                 elements at 2 mod 4 included), only a row's head and tail take narrower, naturally aligned
//                                 pieces.  What costs a store stream is the partly written 128-byte line (profiles/r05_tuning.md
//                                 section 3); whole aligned vectors leave one at each row end at most, and none inside a slab
//                                 that is contiguous in memory (normalizeMove has fused it into one long row: a plain streaming
//                                 fill).
//   generic_fill_kernel<ES>       element-wise, for everything else: faces one element thick along the fastest memory axis (cells
//                                 a row pitch apart), degenerate shapes.
// The value arrives as FillPattern, a kernel argument of its own: the 16 bytes of ANY 16-byte-aligned slot of the destination
// (the element replicated, at the phase the destination's address gives it; kernels.cc fillPatternOf).  Every store takes its
// bytes from the pattern at the offset of its address inside the slot, so no store ever depends on which row it belongs to.
// No store of 4 bytes or more is issued at an address that is not a multiple of its size.
#include "kernels_dispatch.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// bytes [lo, hi) of the 16-byte-aligned slot at `slot`, 0 <= lo < hi <= 16, lo and hi even: the widest naturally aligned
// pieces that lie inside
template <int POLICY>
__device__ __forceinline__ void storeSlot(char* slot, int lo, int hi, const u32x4& pat) {
  if (lo == 0 && hi == 16) {
    storeVec<POLICY, 16>(slot, pat);
    return;
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int o8 = 8 * h;
    if (lo <= o8 && o8 + 8 <= hi) {
      const u32x2 v = {pat[2 * h], pat[2 * h + 1]};
      storeVec<POLICY, 8>(slot + o8, v);
      continue;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int o4 = o8 + 4 * q;
      const unsigned int w = pat[2 * h + q];
      if (lo <= o4 && o4 + 4 <= hi) {
        storeVec<POLICY, 4>(slot + o4, w);
      } else {
        if (lo <= o4 && o4 + 2 <= hi) storeVec<POLICY, 2>(slot + o4, (unsigned short)w);
        if (lo <= o4 + 2 && o4 + 4 <= hi) storeVec<POLICY, 2>(slot + o4 + 2, (unsigned short)(w >> 16));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// rows_fill_kernel: e[0] = 16-byte slots per row (the most a row can touch), e[1] = rows, e[2] = planes; ss[0] = row length
// in BYTES; ds[1], ds[2] in BYTES.  p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0)
// slots; lane `col` of a row serves the slot `col` slots above the 16-byte boundary below the row's first byte.
// STREAM: 0 default caching (the kernel that deposits next finds the lines in L2); 1 (moves of 32 MiB and more) non-temporal.
// ---------------------------------------------------------------------------------------------
template <int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_fill_kernel(const Batch b, const FillPattern pattern) {
  static_assert(VB == 16, "the lanes lie on the 16-byte grid");
  constexpr int POLICY = STREAM ? ST_STREAM : ST_CACHED;
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  const RowLane l = rowLane(b.p0[mi], b.t0[mi], b.t1[mi], lb);
  if (l.col >= m.e[0]) return;
  const u32x4 pat = {pattern.w[0], pattern.w[1], pattern.w[2], pattern.w[3]};
  char* const d = m.dst + l.plane * m.ds[2];
  const long long row_bytes = m.ss[0], lo = l.col * VB;
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = l.r0 + (long long)u * l.rb;
    if (r >= m.e[1]) continue;
    char* const row = d + r * m.ds[1];
    const long long ph = (long long)(reinterpret_cast<uintptr_t>(row) & (VB - 1));  // the row is bytes [ph, ph + row_bytes) of its slots
    const long long first = lo > ph ? lo : ph, end = ph + row_bytes;
    const long long last = lo + VB < end ? lo + VB : end;
    if (first < last) storeSlot<POLICY>(row - ph + lo, (int)(first - lo), (int)(last - lo), pat);
  }
}

// ---------------------------------------------------------------------------------------------
// generic_fill_kernel: element-wise with a grid-stride loop, lanes along dim p0 (the destination-fast dim when there is one);
// extents and strides in ELEMENTS of ES bytes.  An element lies in one slot of the grid, or -- 16-byte elements at 4- or
// 8-byte-aligned addresses -- in two.
// ---------------------------------------------------------------------------------------------
template <int ES>
__global__ __launch_bounds__(kThreads) void generic_fill_kernel(const Batch b, const FillPattern pattern) {
  int mi;
  unsigned int lb;
  if (!locate(b, blockIdx.x, mi, lb)) return;
  const DevMove& m = b.m[mi];
  // (the element walk of kernels_walk.h, written out: through forEachElement the 2-byte form compiles to 52 instructions more
  // than this loop -- other branches around storeSlot -- profiles/kernel_walk_refactor.md)
  const unsigned int nb = b.first_block[mi + 1] - b.first_block[mi];
  const int f = b.p0[mi], g = (f + 1) % 3, h = (f + 2) % 3;
  const unsigned long long ef = m.e[f], eg = m.e[g];
  const unsigned long long total = ef * eg * (unsigned long long)m.e[h];
  const u32x4 pat = {pattern.w[0], pattern.w[1], pattern.w[2], pattern.w[3]};
  char* dst = m.dst;
  for (unsigned long long n = (unsigned long long)lb * kThreads + threadIdx.x; n < total;
       n += (unsigned long long)nb * kThreads) {
    const unsigned long long kf = n % ef, t = n / ef;
    const unsigned long long kg = t % eg, kh = t / eg;
    char* const d = dst + (long long)(kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]) * ES;
    const int ph = (int)(reinterpret_cast<uintptr_t>(d) & 15);
    storeSlot<ST_CACHED>(d - ph, ph, ph + ES < 16 ? ph + ES : 16, pat);
    if (ph + ES > 16) storeSlot<ST_CACHED>(d - ph + 16, 0, ph + ES - 16, pat);
  }
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchFillBatch(const KernelChoice& k, const Batch& b, const FillPattern& pattern, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  bool ok = false;
  if (k.kind == K_ROWS_FILL) {
    ok = dispatchInt<16>(k.vec, [&](auto w) {
      dispatchAccess(streamArgOf(k.kind, k.access), [&](auto a) {
        rows_fill_kernel<decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b, pattern);
      });
    });
  } else if (k.kind == K_GENERIC_FILL) {
    ok = dispatchElementSize(k.es, [&](auto es) { generic_fill_kernel<decltype(es)::value><<<grid, block, 0, stream>>>(b, pattern); });
  }
  if (!ok) CD_INTERNAL_ERROR("no fill kernel for this lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
