// kernels_field_wall.hip -- lists of WALL field-moves: up to kMaxBatch wall-moves (Move3D::affine: dst = +-src + a[layer], the source
// running backwards along one dim), each carried out for up to kMaxFields pencils with a sign PER FIELD and addends PER FIELD, in
// ONE launch (multi-field wall values, include/cudecomp_halo_wall_value_fields.h).  Hand-written gfx950 (CDNA4 / MI355X) kernels;
// compiled into the unit kernels_executor.hip (kernels_batch.h says why there are several code objects and why this file joins
// the smallest of them: neither kernels_wall.hip nor kernels_field_mirror.hip has room).
//
// The phases of a multi-field wall-value call are the single call's one or two sides; their geometry is the same for every field,
// only the base pointers, the parities and the addends differ.  Everything is built from parts that exist: the FieldMoveBatch of
// the copying lists, unchanged, and its workgroup decode (kernels_field_list.h, then rowLane / forEachElement of kernels_walk.h);
// the lane layout and unroll of rows_fields_reflect_kernel; its per-field sign -- bit f of `fields_neg`, chosen once per workgroup,
// XORed into every loaded vector, no template over the sign; the addition of the single wall-moves (kernels_arith.h addPayload:
// flip first, add second), so every field is bit for bit what cudecompAmdSetWallHalos* makes of it alone.
//   rows_fields_wall_kernel<T, VB, STREAM>   fastest dim contiguous on both sides and NOT the mirrored one; the destination layer is
//                                            the row or the plane index (FieldWallWalk::along, Batch::p1's meaning for wall-moves).
//   generic_fields_wall_kernel<T, ES>        element-wise with a grid-stride loop per field: the mirrored dim as the fastest memory
//                                            axis, degenerate shapes and the forced case.  Always cached.
// The addends are a kernel argument of their own (kern::FieldWallTable, kernels_batch.h): 2048 bytes of `es`-byte entries, the entry
// of (move i, field f, destination layer j) at byte ((i * n_fields + f) * layers + j) * es.  The host has reversed the low side, so
// the kernels index by destination layer.  A lane is VB >= es bytes wide and starts on an element's boundary: it replicates the
// entry to its width in registers, no phase.  The entry index is masked, so a read can never leave the kernel arguments.
// Source and destination are disjoint cells of ONE buffer per field: no pointer is __restrict__.  Exactly the destination cells of
// the moves are stored and exactly their source cells loaded.  Local buffers only.  Bound: HBM, 2 bytes moved per byte of a move.
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_field_list.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {

// The kernels are `static` members of kern, as in kernels_field_mirror.hip and for its reason: every character of a mangled name
// costs the code object about thirteen bytes per kernel.

// the first entry of (move mi, field f) of the table, in elements
__device__ __forceinline__ unsigned int fieldWallRow(const FieldMoveBatch& b, const FieldWallWalk& walk, int mi, unsigned int f) {
  return ((unsigned int)mi * (unsigned int)b.n_fields + f) * (unsigned int)walk.layers;
}

// entry `index` (in elements of walk.es bytes) replicated to N bytes.  The byte offset is masked into the table and kept on the
// entry's boundary; the host never asks for an entry beyond it (kernels.cc planFieldWallLaunches).
template <int N> __device__ __forceinline__ Bytes<N> fieldWallAddend(const FieldWallTable& table, int es, unsigned int index) {
  const unsigned int at = (index * (unsigned int)es) & (unsigned int)(kFieldWallTableBytes - 1);  // (es divides the table)
  const unsigned int* w = table.w + (at >> 2);
  if constexpr (N == 2) {
    return (unsigned short)(w[0] >> ((at & 2u) * 8));
  } else {
    if (es == 2) {
      const unsigned int half = (w[0] >> ((at & 2u) * 8)) & 0xffffu, both = half | (half << 16);
      if constexpr (N == 4) return both;
      else if constexpr (N == 8) return u32x2{both, both};
      else return u32x4{both, both, both, both};
    }
    // es is 4, 8 or 16 and at most N: word k of the lane is word k mod (es / 4) of the entry, which ends inside the table
    if constexpr (N == 4) return w[0];
    else if constexpr (N == 8) return es == 4 ? u32x2{w[0], w[0]} : u32x2{w[0], w[1]};
    else return es == 4 ? u32x4{w[0], w[0], w[0], w[0]} : (es == 8 ? u32x4{w[0], w[1], w[0], w[1]} : u32x4{w[0], w[1], w[2], w[3]});
  }
}

template <int N> __device__ __forceinline__ Bytes<N> fieldWallSign(const SignMask& mask, unsigned int fields_neg, unsigned int f) {
  return ((fields_neg >> f) & 1u) ? signBits<N>(mask) : zeroBytes<N>();
}

// ---------------------------------------------------------------------------------------------
// rows_fields_wall_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in BYTES, ss[1] or ss[2] negative for
// the mirrored dim.  p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll rows x (1 << p0) vectors of one field.
// walk.along[move] = 1: the layer is the row index, 2: the plane index, anything else: layer 0.  STREAM: 0 default caching; 1
// non-temporal loads and stores (the reflection's rule by the size of one field's move; unmeasured for this kernel).
// ---------------------------------------------------------------------------------------------
template <typename T, int VB, int STREAM>
static __global__ __launch_bounds__(kThreads) void rows_fields_wall_kernel(const FieldMoveBatch b, const SignMask mask,
                                                                           const unsigned int fields_neg, const FieldWallTable table,
                                                                           const FieldWallWalk walk) {
  using V = Bytes<VB>;
  int mi;
  unsigned int f, lb;
  locateFieldMove(b, blockIdx.x, mi, f, lb);
  if (f >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const RowLane l = rowLane(m.p0, m.t0, m.t1, lb);
  if (l.col >= m.e[0]) return;
  const char* s = sourceOf(b, m, f) + l.plane * m.ss[2] + l.col * VB;
  char* d = destinationOf(b, m, f) + l.plane * m.ds[2] + l.col * VB;
  const V sign = fieldWallSign<VB>(mask, fields_neg, f);
  const int along = walk.along[mi];
  const unsigned int row0 = fieldWallRow(b, walk, mi, f);

  // the addends are loaded in the load phase, beside the payload, as in rows_wall_kernel: a row index differs from lane to lane
  V v[kRowsUnroll], a[kRowsUnroll];
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]);
    a[u] = fieldWallAddend<VB>(table, walk.es, row0 + (unsigned int)(along == 1 ? r : (along == 2 ? l.plane : 0)));
  });
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    v[u] ^= sign;
    storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], addPayload<T, VB>(v[u], a[u]));
  });
}

// ---------------------------------------------------------------------------------------------
// generic_fields_wall_kernel: element-wise, lanes along dim p0 (the destination-fast dim when there is one, otherwise the longest);
// extents and strides in ELEMENTS, the source stride of the mirrored dim negative (signed indices); a field's `blocks` workgroups
// stride over its move.  walk.along[move] = the mirrored entry of e[] (-1: one layer).  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <typename T, int ES>
static __global__ __launch_bounds__(kThreads) void generic_fields_wall_kernel(const FieldMoveBatch b, const SignMask mask,
                                                                              const unsigned int fields_neg, const FieldWallTable table,
                                                                              const FieldWallWalk walk) {
  static_assert(ES % (int)sizeof(T) == 0 && ES / (int)sizeof(T) <= 2, "an element is one real or two");
  using E = Bytes<ES>;
  int mi;
  unsigned int fi, lb;
  locateFieldMove(b, blockIdx.x, mi, fi, lb);
  if (fi >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const ElementWalk w = elementWalk(m.e, m.p0, lb, m.blocks);
  const char* src = sourceOf(b, m, fi);
  char* dst = destinationOf(b, m, fi);
  const E sign = fieldWallSign<ES>(mask, fields_neg, fi);
  const int along = walk.along[mi];
  const unsigned int row0 = fieldWallRow(b, walk, mi, fi);
  forEachElement<long long>(w, [&](long long kf, long long kg, long long kh) CD_INLINED {
    E x = loadVec<false, ES>(src + (kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES);
    x ^= sign;
    const long long layer = along == w.f ? kf : (along == w.g ? kg : (along == w.h ? kh : 0));
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES,
                            addPayload<T, ES>(x, fieldWallAddend<ES>(table, ES, row0 + (unsigned int)layer)));
  });
}

}  // namespace kern

using namespace kern;

void launchFieldWallBatch(const KernelChoice& k, const FieldMoveBatch& b, unsigned int fields_neg, const FieldWallTable& table,
                          const FieldWallWalk& walk, unsigned int blocks, hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  if (s != 0 && s != 1) CD_INTERNAL_ERROR("no wall field-move kernel for this access mode");
  if (b.n_fields < kMaxFields && (fields_neg >> b.n_fields) != 0) CD_INTERNAL_ERROR("sign bit of a field the list does not have");
  // the table's invariants: a lane holds whole elements, and every entry the launch can ask for lies inside the table
  if (k.vec < k.es || k.es < 2 || 16 % k.es != 0 || walk.es != k.es) CD_INTERNAL_ERROR("wall field-move whose lanes are narrower than one element");
  if (walk.layers < 1 || walk.layers > kMaxWallHalo || b.n < 1 || b.n_fields < 1 ||
      (long long)b.n * b.n_fields * walk.layers * k.es > kFieldWallTableBytes)
    CD_INTERNAL_ERROR("wall field-moves whose addends do not fit the table");
  const SignMask mask = signMaskOf(k.arith);
  const bool rows = k.kind == K_ROWS_FIELDS_WALL;
  const bool ok = (rows || k.kind == K_GENERIC_FIELDS_WALL) && dispatchArith(k.arith, [&](auto t) {
    using T = typename decltype(t)::type;
    if (rows)
      return dispatchLaneWidth<T>(k.vec, [&](auto w) {
        dispatchAccess(s, [&](auto a) {
          rows_fields_wall_kernel<T, decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b, mask, fields_neg, table, walk);
        });
      });
    return dispatchReals<T>(k.es, [&](auto nc) {
      generic_fields_wall_kernel<T, decltype(nc)::value * (int)sizeof(T)><<<grid, block, 0, stream>>>(b, mask, fields_neg, table, walk);
    });
  });
  if (!ok) CD_INTERNAL_ERROR("no wall field-move kernel for this kind, real type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
