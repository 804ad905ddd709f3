// kernels_field_mirror.hip -- lists of MIRRORED field-moves: up to kMaxBatch reflect- or fold-moves, each carried out for up to
// kMaxFields pencils with a sign PER FIELD, in ONE launch (multi-field wall halos, include/cudecomp_halo_wall_fields.h).
// Hand-written gfx950 (CDNA4 / MI355X) kernels, one code object (kernels_batch.h says why there are several).
//
// The phases of a multi-field reflection or fold are the single call's one or two sides; their geometry is the same for every
// field, only the base pointers and the parities differ.  The descriptor is the FieldMoveBatch of the copying lists
// (kernels_field_transpose.hip), unchanged; the workgroup decode is theirs (kernels_field_list.h, then rowLane / forEachElement of
// kernels_walk.h); the mirror is what it is in kernels_reflect.hip and kernels_fold.hip: the SIGN of the source's row or plane
// stride (FieldMove::ss is signed; only the mirrored dim is negative and src_off names the source cell of index 0); the
// arithmetic is the single fold's (kernels_arith.h: addPayload, destination first, the sign bits of the source flipped before
// the addition), so every field is bit for bit what its single call makes of it.
//   rows_fields_reflect_kernel<VB, STREAM>          dst = +-src.  Fastest dim contiguous on both sides and NOT the mirrored one:
//                                                   the lane layout of rows_kernel, kRowsUnroll vectors in flight per lane.
//   generic_fields_reflect_kernel<ES>               element-wise with a grid-stride loop per field: the mirrored dim as the
//                                                   fastest memory axis, degenerate shapes and the forced case.  Always cached.
//   rows_fields_fold_kernel<T, VB, STREAM, TAKE>    dst += +-src (TAKE: then src = 0); kRowsUnroll source and kRowsUnroll
//                                                   destination vectors in flight per lane, the two loops written out as in
//                                                   rows_fold_kernel (profiles/kernel_walk_refactor.md).
//   generic_fields_fold_kernel<T, NC, TAKE>         element-wise (NC reals per element).  Always cached.
// The sign: bit f of `fields_neg` says that field f has parity -1.  f comes out of the workgroup decode and is uniform over the
// workgroup, so the lane's mask -- signBits<VB>(mask) or zero -- is chosen once per workgroup by a scalar select; every loaded
// vector is XORed with it (XOR with zero is the identity): no divergent branch, no template over the sign, and one kernel serves
// every combination of parities.  `fields_neg` and the 16-byte SignMask are kernel arguments beside the batch.
// TAKE stores zero bytes where the lane loaded the source, at that load's width, after the load.  No pointer is __restrict__:
// source and destination are disjoint cells of ONE buffer per field, and the zero store follows a load of the same bytes -- the
// compiler keeps their order, the hardware keeps a wave's accesses to one address in order.  Exactly the cells of the moves are
// read and written.  Local buffers only.  Bound: HBM; 2 bytes moved per byte of a reflection, 3 of a fold, 4 of a fold with TAKE.
#include "kernels_arith.h"
#include "kernels_dispatch.h"
#include "kernels_field_list.h"
#include "kernels_walk.h"

#include "errors.h"

namespace cudecomp {
namespace kern {

// The kernels are `static` members of kern, not of an anonymous namespace as in the other code objects: a code object carries about
// thirteen symbols per kernel, so with the 78 instantiations here every character of a mangled name costs it 1 KB, and the
// anonymous namespace's fourteen would take it past the size tests/test_abi.py guards (kernels_batch.h says why there is one).

// the sign bits field f's vectors are XORed with: those of the real type where bit f of fields_neg is set, none otherwise
template <int N> __device__ __forceinline__ Bytes<N> fieldSignBits(const SignMask& mask, unsigned int fields_neg, unsigned int f) {
  return ((fields_neg >> f) & 1u) ? signBits<N>(mask) : zeroBytes<N>();
}

// ---------------------------------------------------------------------------------------------
// rows_fields_reflect_kernel / rows_fields_fold_kernel: e[0] = vectors per row, e[1] = rows, e[2] = planes; ss/ds[1], [2] in
// BYTES, ss[1] or ss[2] negative for the mirrored dim.  p0 = log2(lanes per row).  A workgroup covers (256 >> p0) * kRowsUnroll
// rows x (1 << p0) vectors of one field.  STREAM: 0 default caching; 1 non-temporal: the reflection's loads and stores, the fold's
// source loads and zero stores (its destination is read and rewritten with the default policy, as in rows_fold_kernel).
// ---------------------------------------------------------------------------------------------
template <int VB, int STREAM>
static __global__ __launch_bounds__(kThreads) void rows_fields_reflect_kernel(const FieldMoveBatch b, const SignMask mask,
                                                                              const unsigned int fields_neg) {
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
  const V sign = fieldSignBits<VB>(mask, fields_neg, f);

  V v[kRowsUnroll];
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED { v[u] = loadVec<(STREAM >= 1), VB>(s + r * m.ss[1]); });
  forRows(l, m.e[1], [&](int u, long long r) CD_INLINED {
    v[u] ^= sign;
    storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(d + r * m.ds[1], v[u]);
  });
}

template <typename T, int VB, int STREAM, bool TAKE>
static __global__ __launch_bounds__(kThreads) void rows_fields_fold_kernel(const FieldMoveBatch b, const SignMask mask,
                                                                           const unsigned int fields_neg) {
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
  const V sign = fieldSignBits<VB>(mask, fields_neg, f);

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
      storeVec<ST_CACHED, VB>(d + r * m.ds[1], addPayload<T, VB>(y[u], (V)(x[u] ^ sign)));
      if constexpr (TAKE) storeVec<(STREAM >= 1 ? ST_STREAM : ST_CACHED), VB>(s + r * m.ss[1], zeroBytes<VB>());
    }
  }
}

// ---------------------------------------------------------------------------------------------
// generic_fields_reflect_kernel / generic_fields_fold_kernel: element-wise, lanes along dim p0 (the destination-fast dim when
// there is one, otherwise the longest); extents and strides in ELEMENTS, the source stride of the mirrored dim negative (signed
// indices); a field's `blocks` workgroups stride over its move.  Default caching throughout.
// ---------------------------------------------------------------------------------------------
template <int ES>
static __global__ __launch_bounds__(kThreads) void generic_fields_reflect_kernel(const FieldMoveBatch b, const SignMask mask,
                                                                                 const unsigned int fields_neg) {
  using E = Bytes<ES>;
  int mi;
  unsigned int fi, lb;
  locateFieldMove(b, blockIdx.x, mi, fi, lb);
  if (fi >= (unsigned int)b.n_fields) return;
  const FieldMove& m = b.m[mi];
  const ElementWalk w = elementWalk(m.e, m.p0, lb, m.blocks);
  const char* src = sourceOf(b, m, fi);
  char* dst = destinationOf(b, m, fi);
  const E sign = fieldSignBits<ES>(mask, fields_neg, fi);
  forEachElement<long long>(w, [&](long long kf, long long kg, long long kh) CD_INLINED {
    E x = loadVec<false, ES>(src + (kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES);
    x ^= sign;
    storeVec<ST_CACHED, ES>(dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES, x);
  });
}

template <typename T, int NC, bool TAKE>
static __global__ __launch_bounds__(kThreads) void generic_fields_fold_kernel(const FieldMoveBatch b, const SignMask mask,
                                                                              const unsigned int fields_neg) {
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
  const E sign = fieldSignBits<ES>(mask, fields_neg, fi);
  forEachElement<long long>(w, [&](long long kf, long long kg, long long kh) CD_INLINED {
    char* s = src + (kf * m.ss[w.f] + kg * m.ss[w.g] + kh * m.ss[w.h]) * ES;
    char* d = dst + (kf * m.ds[w.f] + kg * m.ds[w.g] + kh * m.ds[w.h]) * ES;
    const E x = loadVec<false, ES>(s);
    const E y = loadVec<false, ES>(d);
    storeVec<ST_CACHED, ES>(d, addPayload<T, ES>(y, (E)(x ^ sign)));
    if constexpr (TAKE) storeVec<ST_CACHED, ES>(s, zeroBytes<ES>());
  });
}

}  // namespace kern

using namespace kern;

void launchFieldMirrorBatch(const KernelChoice& k, const FieldMoveBatch& b, unsigned int fields_neg, unsigned int blocks,
                            hipStream_t stream) {
  const dim3 grid(blocks), block(kThreads);
  const int s = streamArgOf(k.kind, k.access);
  if (s != 0 && s != 1) CD_INTERNAL_ERROR("no mirrored field-move kernel for this access mode");
  if (b.n_fields < kMaxFields && (fields_neg >> b.n_fields) != 0) CD_INTERNAL_ERROR("sign bit of a field the list does not have");
  const SignMask mask = signMaskOf(k.arith);  // (the real type of the elements: always known, whatever the parities)
  const bool known = k.arith > ARITH_NONE && k.arith <= ARITH_F64;
  const bool rows = k.kind == K_ROWS_FIELDS_FOLD || k.kind == K_ROWS_FIELDS_FOLD_TAKE;
  const bool take = k.kind == K_ROWS_FIELDS_FOLD_TAKE || k.kind == K_GENERIC_FIELDS_FOLD_TAKE;
  const bool fold = rows || k.kind == K_GENERIC_FIELDS_FOLD || k.kind == K_GENERIC_FIELDS_FOLD_TAKE;
  bool ok = false;
  if (!known) {
  } else if (k.kind == K_ROWS_FIELDS_REFLECT) {
    ok = dispatchLaneWidth<unsigned short>(k.vec, [&](auto w) {
      dispatchAccess(s, [&](auto a) {
        rows_fields_reflect_kernel<decltype(w)::value, decltype(a)::value><<<grid, block, 0, stream>>>(b, mask, fields_neg);
      });
    });
  } else if (k.kind == K_GENERIC_FIELDS_REFLECT) {
    ok = dispatchElementSize(k.es, [&](auto es) {
      generic_fields_reflect_kernel<decltype(es)::value><<<grid, block, 0, stream>>>(b, mask, fields_neg);
    });
  } else if (fold) {
    // lanes never narrower than one real; there is no complex bf16 type: that element-wise form could never be launched
    ok = dispatchArith(k.arith, [&](auto t) {
      using T = typename decltype(t)::type;
      return dispatchBool(take, [&](auto tk) {
        constexpr bool TAKE = decltype(tk)::value;
        if (rows)
          return dispatchLaneWidth<T>(k.vec, [&](auto w) {
            dispatchAccess(s, [&](auto a) {
              rows_fields_fold_kernel<T, decltype(w)::value, decltype(a)::value, TAKE><<<grid, block, 0, stream>>>(b, mask, fields_neg);
            });
          });
        return dispatchReals<T>(k.es, [&](auto nc) {
          generic_fields_fold_kernel<T, decltype(nc)::value, TAKE><<<grid, block, 0, stream>>>(b, mask, fields_neg);
        });
      });
    });
  }
  if (!ok) CD_INTERNAL_ERROR("no mirrored field-move kernel for this kind, real type, lane width and element size");
  CD_CHECK_HIP(hipGetLastError());
}

}  // namespace cudecomp
