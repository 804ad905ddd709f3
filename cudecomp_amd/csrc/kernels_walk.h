// kernels_walk.h -- how the row and element-wise kernels of every family walk a move: the workgroup -> lane decode of the row
// kernels, the unrolled loop over a lane's rows, the grid-stride element walk, and the two small payload helpers (zero bytes, sign
// bits) the taking, reflecting and folding families share.  Device code, included by the kernel code objects only; one
// definition each, so a change to the decode reaches every family (kernels_rows.hip, kernels_accumulate.hip, kernels_take.hip,
// kernels_reflect.hip, kernels_fold.hip, kernels_fill.hip, kernels_field_transpose.hip, kernels_field_accumulate.hip,
// kernels_field_mirror.hip).
//
// What is NOT here, on purpose: the payload arrays and the two phases of a row kernel (all loads, then all stores).  They stay in
// each kernel's body, as do its pointer qualifiers.  Moved into a shared function together with the loops, the compiler treats a
// lane's vectors as one wide tuple, copies them and waits between the loads (a prototype of that form: 90 VGPRs for
// rows_accumulate_kernel<double,16,*>, which takes 42 here, and a vmcnt wait between a lane's loads) -- the hazard kernels_dev.h
// names for payloads.  forRows serves the row kernels that compile through it to the code of the written-out loops (the copies,
// the reflection, the field copy and the field take); the adding kernels and rows_take_kernel keep their two loops written out,
// and generic_fill_kernel its element loop: there the helpers change register counts, waits or instruction counts of some
// instantiations (profiles/kernel_walk_refactor.md has every kernel).
#pragma once
#include "kernels_dev.h"

// On the lambdas handed to forRows / forEachElement: inlined before any optimisation, like the __forceinline__ helpers, so that a
// kernel compiles as if its loops were written out in its body.
#define CD_INLINED __attribute__((always_inline))

namespace cudecomp {
namespace kern {

// ---------------------------------------------------------------------------------------------
// Row kernels: e[0] = vectors per row, e[1] = rows, e[2] = planes; p0 = log2(lanes per row).  A workgroup covers
// (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors: workgroup lb of a move is tile column lb % t0 of row tile (lb / t0) % t1
// of plane lb / t0 / t1.  No per-element index math: one (row, plane) decode per WORKGROUP.
// A lane serves vector `col` of rows r0, r0 + rb, ... (kRowsUnroll of them) of `plane`; col may lie beyond the row (the last
// tile column), rows beyond the last one (the last row tile): the kernel tests col once, forRows tests every row.
// ---------------------------------------------------------------------------------------------
struct RowLane {
  long long col;    // vector along the row
  long long r0;     // first row
  int rb;           // rows between a lane's rows
  long long plane;
};

__device__ __forceinline__ RowLane rowLane(int p0, unsigned int t0, unsigned int t1, unsigned int lb) {
  const int lg = p0;
  const int lpr = 1 << lg;
  const int rb = kThreads >> lg;
  const unsigned int tc = t0, tr = t1;
  const unsigned int bc = lb % tc;
  const unsigned int rest = lb / tc;
  const unsigned int br = rest % tr;
  RowLane l;
  l.plane = rest / tr;
  l.col = (long long)bc * lpr + (threadIdx.x & (lpr - 1));
  l.r0 = (long long)br * rb * kRowsUnroll + (threadIdx.x >> lg);
  l.rb = rb;
  return l;
}

// fn(u, r) for the lane's rows r = r0 + u * rb that exist, u = 0 .. kRowsUnroll - 1.  A kernel calls it once per phase -- all
// loads into ITS arrays, then all stores -- so that kRowsUnroll vectors per side are in flight.
template <typename F>
__device__ __forceinline__ void forRows(const RowLane& l, long long rows, F fn) {
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = l.r0 + (long long)u * l.rb;
    if (r < rows) fn(u, r);
  }
}

// ---------------------------------------------------------------------------------------------
// Element-wise kernels: the move's nb workgroups stride over its e[0] * e[1] * e[2] elements, lanes along dim f = p0, then g, then
// h.  elementWalk is the decode (a kernel takes it where the row kernels take rowLane: before it forms its pointers);
// forEachElement calls fn(kf, kg, kh) with the element's indices along f, g, h.  Index: unsigned long long, or long long for the
// reflecting and folding kernels, whose source stride along the mirrored dim is negative (index times stride must be a signed
// product).
// ---------------------------------------------------------------------------------------------
struct ElementWalk {
  int f, g, h;
  unsigned long long ef, eg, total;
  unsigned int lb, nb;  // this workgroup of the move's nb
};

__device__ __forceinline__ ElementWalk elementWalk(const long long (&e)[3], int p0, unsigned int lb, unsigned int nb) {
  ElementWalk w;
  w.nb = nb, w.lb = lb;
  w.f = p0, w.g = (w.f + 1) % 3, w.h = (w.f + 2) % 3;
  w.ef = e[w.f], w.eg = e[w.g];
  w.total = w.ef * w.eg * (unsigned long long)e[w.h];
  return w;
}

template <typename Index = unsigned long long, typename F>
__device__ __forceinline__ void forEachElement(const ElementWalk& w, F fn) {
  for (unsigned long long n = (unsigned long long)w.lb * kThreads + threadIdx.x; n < w.total;
       n += (unsigned long long)w.nb * kThreads) {
    const Index kf = (Index)(n % w.ef), t = (Index)(n / w.ef);
    const Index kg = t % (Index)w.eg, kh = t / (Index)w.eg;
    fn(kf, kg, kh);
  }
}

// the zero a TAKE stores where its lane loaded the source, at that load's width
template <int N> __device__ __forceinline__ Bytes<N> zeroBytes() {
  Bytes<N> z = {};
  return z;
}

// the low N bytes of the sign mask (kernels_batch.h signMaskOf): lanes are at least one real wide and start on a real's boundary
template <int N> __device__ __forceinline__ Bytes<N> signBits(const SignMask& mask) {
  if constexpr (N == 2) return (unsigned short)mask.w[0];
  else if constexpr (N == 4) return mask.w[0];
  else if constexpr (N == 8) return u32x2{mask.w[0], mask.w[1]};
  else return u32x4{mask.w[0], mask.w[1], mask.w[2], mask.w[3]};
}

}  // namespace kern
}  // namespace cudecomp
