// kernels_fields.hip -- field-moves: the one or two moves of a halo phase carried out for up to kMaxFields pencils in ONE launch
// (multi-field halo updates, include/cudecomp_halo_fields.h).  Hand-written gfx950 (CDNA4 / MI355X) data-movement kernels, one
// code object (see kernels_batch.h for why there are several).
//
// A phase of a halo update has at most two sides, low and high, and their geometry is the same for every field: only the base
// pointers differ.  The descriptor (kern::FieldBatch, kernels_batch.h) therefore holds the geometry once per side, with byte
// offsets in the place of pointers, a table of the fields' pencils and the workspace; each end of a side is "field f's pencil"
// or "the workspace at f * a byte step".
//   rows_fields_kernel<VB,STREAM>  fastest dim contiguous on both sides: the lane layout of rows_kernel (kernels_rows.hip) -- each
//                                  lane moves VB = 16 (8, 4, 2) bytes, kRowsUnroll vectors per lane in flight, lanes along the row.
//                                  Workgroup -> side -> (field, workgroup of that field) -> (row block, plane): one decode per
//                                  WORKGROUP, no per-element index math.
//   generic_fields_kernel<ES>      element-wise with a grid-stride loop per field, lanes along the destination-fast dim: faces one
//                                  element thick along the fastest memory axis, degenerate shapes, forced.
// Exactly the cells of the moves are read and written: no shifted or dense form (the cells between rows belong to the fields'
// pencils and are not the move's to rewrite), no remote destination.
// Pure data movement: no MFMA; the bound is HBM (8 TB/s spec, ~6.3 TB/s achievable copy rate).
#include "kernels_dev.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// workgroup -> (side, field, workgroup index inside that field's move); false beyond the last field (never launched)
__device__ __forceinline__ bool locateField(const FieldBatch& b, unsigned int block, int& si, unsigned int& f, unsigned int& lb) {
  si = (b.n_sides > 1 && block >= b.side1_first) ? 1 : 0;
  const unsigned int rel = block - (si ? b.side1_first : 0u);
  const unsigned int per = b.side[si].blocks;
  f = rel / per;
  lb = rel - f * per;
  return f < (unsigned int)b.n_fields;
}

__device__ __forceinline__ const char* sourceOf(const FieldBatch& b, const FieldSide& s, unsigned int f) {
  return (s.src_work ? b.work + (long long)f * s.src_step : b.field[f]) + s.src_off;
}
__device__ __forceinline__ char* destinationOf(const FieldBatch& b, const FieldSide& s, unsigned int f) {
  return (s.dst_work ? b.work + (long long)f * s.dst_step : b.field[f]) + s.dst_off;
}

// ---------------------------------------------------------------------------------------------
// rows_fields_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES.
// p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors of one field.
// STREAM: 0 default caching, 1 non-temporal loads and stores.
// ---------------------------------------------------------------------------------------------
template <int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_fields_kernel(const FieldBatch b) {
  using V = Bytes<VB>;
  int si;
  unsigned int f, lb;
  if (!locateField(b, blockIdx.x, si, f, lb)) return;
  const FieldSide& m = b.side[si];
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
// generic_fields_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one); extents and strides in
// elements; a field's `blocks` workgroups stride over its move.
// ---------------------------------------------------------------------------------------------
template <int ES>
__global__ __launch_bounds__(kThreads) void generic_fields_kernel(const FieldBatch b) {
  using E = Bytes<ES>;
  int si;
  unsigned int fi, lb;
  if (!locateField(b, blockIdx.x, si, fi, lb)) return;
  const FieldSide& m = b.side[si];
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

}  // namespace
}  // namespace kern

using namespace kern;

void launchFieldsBatch(const KernelChoice& k, const FieldBatch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int rs = streamArgOf(k.kind, k.access), vb = k.vec;
  const bool rows = k.kind == K_ROWS_FIELDS, generic = k.kind == K_GENERIC_FIELDS;
#define CD_ROWS_FIELDS(VB)                                                 \
  do {                                                                     \
    if (rs == 1) rows_fields_kernel<VB, 1><<<grid, block, 0, stream>>>(b); \
    else rows_fields_kernel<VB, 0><<<grid, block, 0, stream>>>(b);         \
  } while (0)
  if (rows && rs != 0 && rs != 1) CD_INTERNAL_ERROR("no field-move row kernel for this access mode");
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
