// kernels_field_transpose.hip -- lists of field-moves: up to kMaxBatch moves, each carried out for up to kMaxFields (input,
// output) pairs of pencils, in ONE launch (multi-field transposes, include/cudecomp_transpose_fields.h, and multi-field halo
// updates, include/cudecomp_halo_fields.h).  Hand-written gfx950 (CDNA4 / MI355X) data-movement kernels, one code object (see
// kernels_batch.h for why there are several).
//
// The pack (or unpack) phase of a multi-field transpose is the single transpose's list of moves -- one per peer -- and a phase of
// a multi-field halo update the update's one or two sides; their geometry is the same for every field: only the base pointers
// differ.  The descriptor (kern::FieldMoveBatch, kernels_batch.h) holds the geometry once per move, with byte offsets in the
// place of pointers, two tables of the fields' pencils (inputs, outputs; a halo update names the same pencils in both) and the
// workspace; each end of a move is "field f's input", "field f's output" or "the workspace at f * a per-move byte step".
//   transpose_fields_kernel<ES,VW,TI,TJ,STREAM,GUARD>
//                                    fastest source dim != fastest destination dim: the LDS-tiled transposition of
//                                    kernels_tile.h (transposeTile: XOR-swizzled LDS rows, 16-byte lanes when the tile edges
//                                    hold whole vectors; transposeTilePadded for 16-byte elements).  Workgroup -> (move, field,
//                                    plane, tile): one decode per WORKGROUP; tiles are walked along i first, with no XCD or run
//                                    walk.  GUARD = false when every move of the launch consists of whole tiles.
//   rows_fields_kernel<VB,STREAM>    fastest dim contiguous on both sides: the lane layout of rows_kernel (kernels_rows.hip) --
//                                    each lane moves VB = 16 (8, 4, 2) bytes, kRowsUnroll vectors per lane in flight, lanes along
//                                    the row; one decode per WORKGROUP (rowLane and forRows, kernels_walk.h), no per-element
//                                    index math.
//   generic_fields_kernel<ES>        element-wise with a grid-stride loop per field, lanes along the destination-fast dim: faces
//                                    one element thick along the fastest memory axis, everything else, and the forced case
//                                    (forEachElement, kernels_walk.h).
// Exactly the cells of the moves are read and written: no window, lines, shifted or dense form (the cells between rows belong
// to the fields' pencils and are not the move's to rewrite), no remote destination.
// Pure data movement: no MFMA; the bound is HBM (8 TB/s spec, ~6.3 TB/s achievable copy rate).
#include "kernels_dispatch.h"
#include "kernels_field_list.h"
#include "kernels_tile.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// ---------------------------------------------------------------------------------------------
// transpose_fields_kernel: dims (i, j, k) as transpose_kernel (kernels_tile.h): i unit-stride in the source, j unit-stride in the
// destination, k the batch dim; e = {ei, ej, ek}, ss = {1, sj, sk}, ds = {di, 1, dk} in elements.  t0 x t1 tiles per plane.
// STREAM: 0 default caching, 2 non-temporal loads and stores.
// ---------------------------------------------------------------------------------------------
template <int ES, int VW, int TI, int TJ, int STREAM, bool GUARD>
__global__ __launch_bounds__(kThreads) void transpose_fields_kernel(const FieldMoveBatch b) {
  using E = Bytes<ES>;
  constexpr bool SWZ = ES != 16;
  static_assert(TI % VW == 0 && TJ % VW == 0, "tile must hold whole vectors");
  static_assert(kThreads % (TI / VW) == 0 && TJ % (kThreads / (TI / VW)) == 0, "load mapping");
  static_assert(kThreads % (TJ / VW) == 0 && TI % (kThreads / (TJ / VW) * VW) == 0, "store mapping");
  __shared__ __attribute__((aligned(16))) E tile[SWZ ? TJ * TI : TJ * (TI + 1)];

  int mi;
  unsigned int f, lb;
  locateFieldMove(b, blockIdx.x, mi, f, lb);
  if (f >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const unsigned int bi = lb % m.t0;
  unsigned int rest = lb / m.t0;
  const unsigned int bj = rest % m.t1;
  const long long k = rest / m.t1;

  const long long i0 = (long long)bi * TI, j0 = (long long)bj * TJ;
  const long long ei = m.e[0], ej = m.e[1];
  const E* __restrict__ src = reinterpret_cast<const E*>(sourceOf(b, m, f)) + k * m.ss[2];
  E* __restrict__ dst = reinterpret_cast<E*>(destinationOf(b, m, f)) + k * m.ds[2];
  if constexpr (SWZ) transposeTile<ES, VW, TI, TJ, STREAM, GUARD>(tile, src, dst, i0, j0, ei, ej, m.ss[1], m.ds[0], threadIdx.x);
  else transposeTilePadded<ES, VW, TI, TJ, STREAM, GUARD>(tile, src, dst, i0, j0, ei, ej, m.ss[1], m.ds[0], threadIdx.x);
}

// ---------------------------------------------------------------------------------------------
// rows_fields_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES.
// p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors of one field.
// STREAM: 0 default caching, 1 non-temporal loads and stores.
// ---------------------------------------------------------------------------------------------
template <int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_fields_kernel(const FieldMoveBatch b) {
  using V = Bytes<VB>;
  int mi;
  unsigned int f, lb;
  locateFieldMove(b, blockIdx.x, mi, f, lb);
  if (f >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const RowLane l = rowLane(m.p0, m.t0, m.t1, lb);
  if (l.col >= m.e[0]) return;
  const char* __restrict__ s = sourceOf(b, m, f) + l.plane * m.ss[2] + l.col * VB;
  char* __restrict__ d = destinationOf(b, m, f) + l.plane * m.ds[2] + l.col * VB;

  V v[kRowsUnroll];
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED { v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]); });
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED { storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], v[u]); });
}

// ---------------------------------------------------------------------------------------------
// generic_fields_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one); extents and strides
// in elements; a field's `blocks` workgroups stride over its move.
// ---------------------------------------------------------------------------------------------
template <int ES>
__global__ __launch_bounds__(kThreads) void generic_fields_kernel(const FieldMoveBatch b) {
  using E = Bytes<ES>;
  int mi;
  unsigned int fi, lb;
  locateFieldMove(b, blockIdx.x, mi, fi, lb);
  if (fi >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const ElementWalk w = elementWalk(m.e, m.p0, lb, m.blocks);
  const E* __restrict__ src = reinterpret_cast<const E*>(sourceOf(b, m, fi));
  E* __restrict__ dst = reinterpret_cast<E*>(destinationOf(b, m, fi));
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]), src[kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]]);
  });
}

// one tile per element size and lane width (the shapes of kernels_transpose.hip without the longer tiles).  The unguarded form
// exists only where a move can reach it: element-wise lanes of 4- and 8-byte elements mean an odd extent, hence a tile that ends
// inside the move (2-byte elements also take them on whole tiles, when a field sits at 2 mod 4; 16-byte elements always)
template <int STREAM, bool GUARD>
bool launchTransposing(const KernelChoice& k, const FieldMoveBatch& b, unsigned int blocks, hipStream_t stream) {
  CD_TILED_SHAPE(transpose_fields_kernel, 2, 8, 128, 128, STREAM, GUARD)
  CD_TILED_SHAPE(transpose_fields_kernel, 2, 1, 64, 64, STREAM, GUARD)
  CD_TILED_SHAPE(transpose_fields_kernel, 4, 4, 64, 128, STREAM, GUARD)
  CD_TILED_SHAPE(transpose_fields_kernel, 8, 2, 64, 64, STREAM, GUARD)
  CD_TILED_SHAPE(transpose_fields_kernel, 16, 1, 32, 32, STREAM, GUARD)
  if constexpr (GUARD) {
    CD_TILED_SHAPE(transpose_fields_kernel, 4, 1, 64, 64, STREAM, true)
    CD_TILED_SHAPE(transpose_fields_kernel, 8, 1, 64, 64, STREAM, true)
  }
  return false;
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchFieldMoveBatch(const KernelChoice& k, const FieldMoveBatch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access), vb = k.vec;
  if (k.kind == K_TRANSPOSE_FIELDS) {
    if (s != 0 && s != 2) CD_INTERNAL_ERROR("no field transpose kernel for this access mode");
    const bool ok = s == 2 ? (k.guard ? launchTransposing<2, true>(k, b, blocks, stream) : launchTransposing<2, false>(k, b, blocks, stream))
                           : (k.guard ? launchTransposing<0, true>(k, b, blocks, stream) : launchTransposing<0, false>(k, b, blocks, stream));
    if (!ok) CD_INTERNAL_ERROR("no field transpose kernel for this element size, lane width and tile");
    CD_CHECK_HIP(hipGetLastError());
    return;
  }
  const bool rows = k.kind == K_ROWS_FIELDS, generic = k.kind == K_GENERIC_FIELDS;
  if (rows && s != 0 && s != 1) CD_INTERNAL_ERROR("no field-move row kernel for this access mode");
  bool ok = false;
  if (rows)
    ok = dispatchLaneWidth<unsigned short>(vb, [&](auto w) {
      dispatchAccess(s, [&](auto a) { rows_fields_kernel<decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b); });
    });
  else if (generic)
    ok = dispatchElementSize(k.es, [&](auto es) { generic_fields_kernel<decltype(es)::value><<<grid, block, 0, stream>>>(b); });
  if (!ok) CD_INTERNAL_ERROR("no field-move kernel for this lane width");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
