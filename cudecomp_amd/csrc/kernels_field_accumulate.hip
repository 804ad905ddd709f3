// kernels_field_accumulate.hip -- lists of field-moves that ADD or TAKE: up to kMaxBatch moves, each carried out for up to
// kMaxFields pencils, in ONE launch (multi-field halo accumulation, include/cudecomp_halo_accumulate_fields.h).  Hand-written
// gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several).
//
// The phases of a multi-field halo accumulation are the single accumulation's one or two sides; their geometry is the same for
// every field, only the base pointers differ.  The descriptor is the FieldMoveBatch of the copying lists
// (kernels_field_transpose.hip), the workgroup decode is theirs (kernels_field_list.h, then rowLane / forEachElement of
// kernels_walk.h; the adding row kernel keeps its two unrolled loops written out, profiles/kernel_walk_refactor.md), the
// arithmetic is that of the single accumulation (kernels_arith.h: addPayload, with its operand order -- destination first -- so
// sums are bit for bit the single call's).
//   rows_fields_accumulate_kernel<T, VB, STREAM, TAKE>  dst += src (TAKE: then src = 0).  Fastest dim contiguous on both sides:
//                                                       the lane layout of rows_kernel, kRowsUnroll source vectors and
//                                                       kRowsUnroll destination vectors in flight per lane.
//   rows_fields_take_kernel<VB, STREAM>                 dst = src; src = 0: the clearing pack.
//   generic_fields_accumulate_kernel<T, NC, TAKE>       element-wise (NC reals per element) with a grid-stride loop per field:
//   generic_fields_take_kernel<ES>                      faces one element thick along the fastest memory axis, degenerate shapes
//                                                       and the forced case.  Always cached.
// TAKE stores zero bytes where the lane loaded the source, at that load's width, after the load.  No pointer is __restrict__: a
// self-periodic addition reads and writes the same pencil, and the zero store follows a load of the same bytes -- the compiler
// keeps their order, the hardware keeps a wave's accesses to one address in order.  Exactly the cells of the moves are read and
// written.  Source and destination cells of a list are disjoint, so no lane clears or rewrites what another still has to read.
// Local buffers only.  Bound: HBM; 3 bytes moved per byte of an addition or a take, 4 of an add-take.
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_field_list.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {
namespace {

// ---------------------------------------------------------------------------------------------
// rows_fields_accumulate_kernel / rows_fields_take_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in
// BYTES.  p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors of one field.
// STREAM: 0 default caching; 1 non-temporal source loads and zero stores (the plain take: its destination stores too).  The
// destination of an addition is read and rewritten with the default policy, as in rows_accumulate_kernel.
// ---------------------------------------------------------------------------------------------
template <typename T, int VB, int STREAM, bool TAKE>
__global__ __launch_bounds__(kThreads) void rows_fields_accumulate_kernel(const FieldMoveBatch b) {
  using V = Bytes<VB>;
  int mi;
  unsigned int f, lb;
  locateFieldMove(b, blockIdx.x, mi, f, lb);
  if (f >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const RowLane l = rowLane(m.p0, m.t0, m.t1, lb);
  if (l.col >= m.e[0]) return;
  char* s = const_cast<char*>(sourceOf(b, m, f)) + l.plane * m.ss[2] + l.col * VB;  // (written too under TAKE: the zeroes)
  char* d = destinationOf(b, m, f) + l.plane * m.ds[2] + l.col * VB;

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
      if constexpr (TAKE) storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(s + r * m.ss[1], zeroBytes<VB>());
    }
  }
}

template <int VB, int STREAM>
__global__ __launch_bounds__(kThreads) void rows_fields_take_kernel(const FieldMoveBatch b) {
  using V = Bytes<VB>;
  constexpr int POLICY = STREAM >= 1 ? ST_STREAM : ST_CACHED;
  int mi;
  unsigned int f, lb;
  locateFieldMove(b, blockIdx.x, mi, f, lb);
  if (f >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const RowLane l = rowLane(m.p0, m.t0, m.t1, lb);
  if (l.col >= m.e[0]) return;
  char* s = const_cast<char*>(sourceOf(b, m, f)) + l.plane * m.ss[2] + l.col * VB;  // (written too: the zeroes)
  char* d = destinationOf(b, m, f) + l.plane * m.ds[2] + l.col * VB;

  V v[kRowsUnroll];
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED { v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]); });
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    storeVec<POLICY, VB>(d + r * m.ds[1], v[u]);
    storeVec<POLICY, VB>(s + r * m.ss[1], zeroBytes<VB>());
  });
}

// ---------------------------------------------------------------------------------------------
// generic_fields_accumulate_kernel / generic_fields_take_kernel: element-wise, lanes along dim p0 (the destination-fast dim when
// there is one); extents and strides in ELEMENTS; a field's `blocks` workgroups stride over its move.  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <typename T, int NC, bool TAKE>
__global__ __launch_bounds__(kThreads) void generic_fields_accumulate_kernel(const FieldMoveBatch b) {
  constexpr int ES = (int)sizeof(T) * NC;
  using E = Bytes<ES>;
  int mi;
  unsigned int fi, lb;
  locateFieldMove(b, blockIdx.x, mi, fi, lb);
  if (fi >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const ElementWalk w = elementWalk(m.e, m.p0, lb, m.blocks);
  char* src = const_cast<char*>(sourceOf(b, m, fi));
  char* dst = destinationOf(b, m, fi);
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    char* s = src + (long long)(kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES;
    char* d = dst + (long long)(kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES;
    const E x = loadVec<false, ES>(s);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, x));
    if constexpr (TAKE) storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  });
}

template <int ES>
__global__ __launch_bounds__(kThreads) void generic_fields_take_kernel(const FieldMoveBatch b) {
  using E = Bytes<ES>;
  int mi;
  unsigned int fi, lb;
  locateFieldMove(b, blockIdx.x, mi, fi, lb);
  if (fi >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const ElementWalk w = elementWalk(m.e, m.p0, lb, m.blocks);
  char* src = const_cast<char*>(sourceOf(b, m, fi));
  char* dst = destinationOf(b, m, fi);
  forEachElement(w, [&](unsigned long long kf, unsigned long long kg, unsigned long long kh) CD_INLINED {
    char* s = src + (long long)(kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES;
    const E x = loadVec<false, ES>(s);
    storeVec<ST_CACHED, ES>(dst + (long long)(kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES, x);
    storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  });
}

}  // namespace
}  // namespace kern

using namespace kern;

void launchFieldAccumulateBatch(const KernelChoice& k, const FieldMoveBatch& b, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  if (s != 0 && s != 1) CD_INTERNAL_ERROR("no accumulating field-move kernel for this access mode");
  const bool rows = k.kind == K_ROWS_FIELDS_ADD || k.kind == K_ROWS_FIELDS_ADD_TAKE;
  const bool take = k.kind == K_ROWS_FIELDS_ADD_TAKE || k.kind == K_GENERIC_FIELDS_ADD_TAKE;
  const bool adds = rows || k.kind == K_GENERIC_FIELDS_ADD || k.kind == K_GENERIC_FIELDS_ADD_TAKE;  // the four adding kinds
  bool ok = false;
  if (k.kind == K_ROWS_FIELDS_TAKE) {
    ok = dispatchLaneWidth<unsigned short>(k.vec, [&](auto w) {
      dispatchAccess(s, [&](auto a) { rows_fields_take_kernel<decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b); });
    });
  } else if (k.kind == K_GENERIC_FIELDS_TAKE) {
    ok = dispatchElementSize(k.es, [&](auto es) { generic_fields_take_kernel<decltype(es)::value><<<grid, block, 0, stream>>>(b); });
  } else if (adds) {
    // only the forms a data type can reach: a lane holds whole elements, so 8-byte reals never take 4- or 2-byte lanes and 4-byte
    // reals never 2-byte ones; bf16 has no complex type
    ok = dispatchArith(k.arith, [&](auto t) {
      using T = typename decltype(t)::type;
      return dispatchBool(take, [&](auto tk) {
        constexpr bool TAKE = decltype(tk)::value;
        if (rows)
          return dispatchLaneWidth<T>(k.vec, [&](auto w) {
            dispatchAccess(s, [&](auto a) {
              rows_fields_accumulate_kernel<T, decltype(w)::value, decltype(a)::value, TAKE><<<grid, block, 0, stream>>>(b);
            });
          });
        return dispatchReals<T>(k.es, [&](auto nc) {
          generic_fields_accumulate_kernel<T, decltype(nc)::value, TAKE><<<grid, block, 0, stream>>>(b);
        });
      });
    });
  }
  if (!ok) CD_INTERNAL_ERROR("no accumulating field-move kernel for this kind, arithmetic type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
