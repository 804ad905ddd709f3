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
//                                    the row; one decode per WORKGROUP, no per-element index math.
//   generic_fields_kernel<ES>        element-wise with a grid-stride loop per field, lanes along the destination-fast dim: faces
//                                    one element thick along the fastest memory axis, everything else, and the forced case.
// Exactly the cells of the moves are read and written: no window, lines, shifted or dense form (the cells between rows belong
// to the fields' pencils and are not the move's to rewrite), no remote destination.
// Pure data movement: no MFMA; the bound is HBM (8 TB/s spec, ~6.3 TB/s achievable copy rate).
#include "kernels_field_list.h"
#include "kernels_tile.h"

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
  const int lg = m.p0;
  const int lpr = 1 << lg;
  const int rb = kThreads >> lg;
  const unsigned int tc = m.t0, tr = m.t1;
  const unsigned int bc = lb % tc;
  const unsigned int rest = lb / tc;
  const unsigned int br = rest % tr;
  const long long plane = rest / tr;

  const long long col = (long long)bc * lpr + (threadIdx.x & (lpr - 1));
  const long long r0 = (long long)br * rb * kRowsUnroll + (threadIdx.x >> lg);
  if (col >= m.e[0]) return;
  const char* __restrict__ s = sourceOf(b, m, f) + plane * m.ss[2] + col * VB;
  char* __restrict__ d = destinationOf(b, m, f) + plane * m.ds[2] + col * VB;

  V v[kRowsUnroll];
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = r0 + (long long)u * rb;
    if (r < m.e[1]) v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
  }
#pragma unroll
  for (int u = 0; u < kRowsUnroll; ++u) {
    const long long r = r0 + (long long)u * rb;
    if (r < m.e[1]) storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], v[u]);
  }
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
  const unsigned int nb = m.blocks;
  const int f = m.p0, g = (f + 1) % 3, h = (f + 2) % 3;
  const unsigned long long ef = m.e[f], eg = m.e[g];
  const unsigned long long total = ef * eg * (unsigned long long)m.e[h];
  const E* __restrict__ src = reinterpret_cast<const E*>(sourceOf(b, m, fi));
  E* __restrict__ dst = reinterpret_cast<E*>(destinationOf(b, m, fi));
  for (unsigned long long n = (unsigned long long)lb * kThreads + threadIdx.x; n < total;
       n += (unsigned long long)nb * kThreads) {
    const unsigned long long kf = n % ef, t = n / ef;
    const unsigned long long kg = t % eg, kh = t / eg;
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[f] + kg * m.ds[g] + kh * m.ds[h]), src[kf * m.ss[f] + kg * m.ss[g] + kh * m.ss[h]]);
  }
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
#define CD_ROWS_FIELDS(VB)                                                \
  do {                                                                    \
    if (s == 1) rows_fields_kernel<VB, 1><<<grid, block, 0, stream>>>(b); \
    else rows_fields_kernel<VB, 0><<<grid, block, 0, stream>>>(b);        \
  } while (0)
  if (rows && s != 0 && s != 1) CD_INTERNAL_ERROR("no field-move row kernel for this access mode");
  if (rows && vb == 16) CD_ROWS_FIELDS(16);
  else if (rows && vb == 8) CD_ROWS_FIELDS(8);
  else if (rows && vb == 4) CD_ROWS_FIELDS(4);
  else if (rows && vb == 2) CD_ROWS_FIELDS(2);
  else if (generic && k.es == 2) generic_fields_kernel<2><<<grid, block, 0, stream>>>(b);
  else if (generic && k.es == 4) generic_fields_kernel<4><<<grid, block, 0, stream>>>(b);
  else if (generic && k.es == 8) generic_fields_kernel<8><<<grid, block, 0, stream>>>(b);
  else if (generic && k.es == 16) generic_fields_kernel<16><<<grid, block, 0, stream>>>(b);
  else CD_INTERNAL_ERROR("no field-move kernel for this lane width");
#undef CD_ROWS_FIELDS
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
