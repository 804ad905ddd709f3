// plan.cc -- see plan.h.
#include "plan.h"

#include <algorithm>
#include <utility>

#include "errors.h"

namespace cudecomp {

namespace {

struct OpAxes {
  int a, b, c;
};

OpAxes axesOf(TransposeOp op) {
  // X->Y, Y->Z step "forward" through the axes, Z->Y, Y->X step back
  switch (op) {
    case OP_X_TO_Y: return {0, 1, 2};
    case OP_Y_TO_Z: return {1, 2, 0};
    case OP_Z_TO_Y: return {2, 1, 0};
    default: return {1, 0, 2};
  }
}

bool anySet(const int32_t* v) { return v && (v[0] != 0 || v[1] != 0 || v[2] != 0); }

// strides (indexed by GLOBAL axis) of a dense block with extents E (by global axis) stored in `order`
void denseStrides(const Int3& order, const i64 E[3], i64 st[3]) {
  st[order[0]] = 1;
  st[order[1]] = E[order[0]];
  st[order[2]] = E[order[0]] * E[order[1]];
}

Move3D blockMove(BufId sb, i64 soff, const i64 sst[3], BufId db, i64 doff, const i64 dst[3], const i64 E[3],
                 int peer) {
  Move3D m;
  m.src_buf = sb;
  m.dst_buf = db;
  m.src_off = soff;
  m.dst_off = doff;
  for (int g = 0; g < 3; ++g) {
    m.extent[g] = E[g];
    m.ss[g] = sst[g];
    m.ds[g] = dst[g];
  }
  m.peer = peer;
  return m;
}

// only nearest-neighbour halos (updates and accumulations alike): a halo of `he` cells along the split dim `dim` may not be
// wider than my slab or a neighbour's slab
void requireNearestNeighbourHalo(const GridShape& g, const std::array<int32_t, 2>& pidx, CommAxis comm_axis, int dim, i64 he,
                                 bool periodic) {
  const int np = g.pdims[comm_axis];
  const auto splits = splitExtent(g.gdims_dist[dim], np, g.gdims[dim] - g.gdims_dist[dim]);
  const int me = pidx[comm_axis == COMM_COL ? 0 : 1];
  int l = me - 1, r = me + 1;
  if (periodic) {
    l = (l + np) % np;
    r = (r + np) % np;
  }
  if ((l >= 0 && (he > splits[l] || he > splits[me])) || (r < np && (he > splits[r] || he > splits[me])))
    CD_INVALID_USAGE("halo includes ranks other than nearest neighbor processes, this is not currently supported.");
}

}  // namespace

TransposePlan buildTransposePlan(const GridShape& g, int rank, TransposeOp op, const int32_t* in_halo,
                                 const int32_t* out_halo, const int32_t* in_pad, const int32_t* out_pad, bool inplace,
                                 const TransportTraits& traits, int npergroup) {
  TransposePlan p;
  const OpAxes ax = axesOf(op);
  p.ax_a = ax.a;
  p.ax_b = ax.b;
  p.ax_c = ax.c;
  // whichever of the two pencils involves Z is exchanged inside a row of the process grid
  p.comm_axis = (ax.a == 2 || ax.b == 2) ? COMM_ROW : COMM_COL;
  const int P = g.pdims[p.comm_axis == COMM_COL ? 0 : 1];
  const auto pidx = gridIndexOfRank(g, rank);
  const int me = pidx[p.comm_axis == COMM_COL ? 0 : 1];
  p.nranks = P;
  p.comm_rank = me;

  const Pencil a = makePencil(g, pidx, ax.a, nullptr, nullptr);
  const Pencil ah = makePencil(g, pidx, ax.a, in_halo, in_pad);
  const Pencil b = makePencil(g, pidx, ax.b, nullptr, nullptr);
  const Pencil bh = makePencil(g, pidx, ax.b, out_halo, out_pad);
  if (anyEmptyPencil(g, ax.a) || anyEmptyPencil(g, ax.b))
    CD_NOT_SUPPORTED("transposes on configurations with empty pencils not supported");

  const bool orders_equal = (a.order == b.order);
  const bool in_hp = anySet(in_halo) || anySet(in_pad);
  const bool out_hp = anySet(out_halo) || anySet(out_pad);
  bool hp_equal = true;
  for (int i = 0; i < 3; ++i) {
    if ((in_halo ? in_halo[i] : 0) != (out_halo ? out_halo[i] : 0)) hp_equal = false;
    if ((in_pad ? in_pad[i] : 0) != (out_pad ? out_pad[i] : 0)) hp_equal = false;
  }

  i64 Sa[3], Sb[3], ast[3], bst[3];
  for (int ga = 0; ga < 3; ++ga) {
    Sa[ga] = a.extentG(ga);
    Sb[ga] = b.extentG(ga);
    ast[ga] = ah.strideG(ga);
    bst[ga] = bh.strideG(ga);
  }
  p.pencil_elements_a = a.size;

  if (P == 1 && !traits.self_exchange) {
    // The whole transpose is local.  Out of place: one move straight from the input interior to the
    // output interior (a copy when the layouts agree, a permutation otherwise).  In place: nothing to
    // do if the layouts agree, else stage the interior through the workspace.
    if (!inplace) {
      p.pack.push_back(blockMove(BUF_IN, ah.interiorOffset(), ast, BUF_OUT, bh.interiorOffset(), bst, Sa, 0));
      p.pack.back().dst_row_pitch = Sb[b.order[0]] > 1 ? bst[b.order[1]] : 0;  // the whole interior of the output pencil
    } else if (orders_equal && hp_equal) {
      p.noop = true;
    } else {
      i64 wst[3];
      denseStrides(b.order, Sb, wst);
      p.pack.push_back(blockMove(BUF_IN, ah.interiorOffset(), ast, BUF_WORK, 0, wst, Sa, 0));
      p.unpack.push_back(blockMove(BUF_WORK, 0, wst, BUF_OUT, bh.interiorOffset(), bst, Sb, 0));
      p.unpack.back().dst_row_pitch = Sb[b.order[0]] > 1 ? bst[b.order[1]] : 0;
      // cubic and halo-free: memory position i of the input holds axis a.order[i]; the output wants b.order[i] there
      if (!in_hp && !out_hp && Sa[0] == Sa[1] && Sa[1] == Sa[2] && Sa[0] > 1) {
        if (a.order[0] == b.order[2] && a.order[1] == b.order[0] && a.order[2] == b.order[1]) p.rotate = 1;    // new[p] = old[p2,p0,p1]
        if (a.order[0] == b.order[1] && a.order[1] == b.order[2] && a.order[2] == b.order[0]) p.rotate = -1;   // new[p] = old[p1,p2,p0]
        if (p.rotate) p.rotate_n = Sa[0];
      }
    }
    p.schedule_dst = {0};
    p.schedule_src = {0};
    return p;
  }

  const auto splits_a = splitExtent(g.gdims_dist[ax.a], P, g.gdims[ax.a] - g.gdims_dist[ax.a]);
  const auto splits_b = splitExtent(g.gdims_dist[ax.b], P, g.gdims[ax.b] - g.gdims_dist[ax.b]);
  const auto off_a = prefixOffsets(splits_a);
  const auto off_b = prefixOffsets(splits_b);

  // What travels: member d gets the slab off_a[d] .. +splits_a[d] of my pencil along ax_a; from member s I
  // get the slab off_b[s] .. +splits_b[s] of my output pencil along ax_b.  Chunks are dense blocks stored
  // in a "wire order" W.  If ax_a is the slowest axis of the input (and it carries no halos/padding) the
  // chunks already sit in the input: send from there (W = input order).  If ax_b is the slowest axis of a
  // halo-free output the chunks can land in place: receive there (W = output order).  Per-peer overlapped
  // in-place operation keeps both stagings so a chunk never lands on data still to be sent.
  const bool elide_ok = !(traits.pipelined && inplace) && !traits.no_elide;
  const bool skip_pack = elide_ok && a.order[2] == ax.a && !in_hp;
  const bool skip_unpack = !skip_pack && elide_ok && !traits.symmetric_recv && b.order[2] == ax.b && !out_hp;
  Int3 W = a.order;
  if (!skip_pack && (skip_unpack || (b.order[2] == ax.a && !orders_equal))) W = b.order;

  p.exchange = true;
  // staging: all chunks are cut along their slowest wire dim.  Its extent is splits_a[d] (chunk for d) when that dim is
  // ax_a, the sender's slab splits_b[s] when it is ax_b, and the common extent along ax_c otherwise.
  p.stage_axis = W[2];
  if (W[2] == ax.a) p.stage_limit = *std::min_element(splits_a.begin(), splits_a.end());
  else if (W[2] == ax.b) p.stage_limit = *std::min_element(splits_b.begin(), splits_b.end());
  else p.stage_limit = Sa[ax.c];
  p.stage_elements = maxPencilElements(g, ax.a);
  p.send_buf = skip_pack ? BUF_IN : BUF_WORK;
  p.send_base = 0;
  p.recv_buf = skip_unpack ? BUF_OUT : BUF_WORK;
  if (skip_pack || skip_unpack) {
    p.recv_base = 0;
  } else {
    p.recv_base = alignElements(traits.symmetric_recv ? maxPencilElements(g, ax.a) : a.size);
  }

  p.send_cnt.resize(P);
  p.send_off.resize(P);
  p.recv_cnt.resize(P);
  p.recv_off.resize(P);
  p.remote_recv_off.resize(P);
  for (int i = 0; i < P; ++i) {
    p.send_cnt[i] = splits_a[i] * Sa[ax.b] * Sa[ax.c];
    p.send_off[i] = off_a[i] * Sa[ax.b] * Sa[ax.c];
    p.recv_cnt[i] = splits_b[i] * Sb[ax.a] * Sb[ax.c];
    p.recv_off[i] = off_b[i] * Sb[ax.a] * Sb[ax.c];
    p.remote_recv_off[i] = off_b[me] * splits_a[i] * Sa[ax.c];  // = member i's recv_off[me]
  }
  p.send_n.resize(P);
  p.recv_n.resize(P);
  for (int i = 0; i < P; ++i) {
    p.send_n[i] = (p.stage_axis == ax.a) ? splits_a[i] : Sa[p.stage_axis];
    p.recv_n[i] = (p.stage_axis == ax.b) ? splits_b[i] : Sb[p.stage_axis];
  }

  p.schedule_dst.resize(P);
  p.schedule_src.resize(P);
  for (int j = 0; j < P; ++j) alltoallPeers(P, npergroup, me, j, &p.schedule_src[j], &p.schedule_dst[j]);

  if (!skip_pack) {
    for (int j = 1; j <= P; ++j) {  // peers in schedule order, my own chunk last
      const int d = (j == P) ? me : p.schedule_dst[j];
      i64 E[3] = {Sa[0], Sa[1], Sa[2]}, wst[3];
      E[ax.a] = splits_a[d];
      denseStrides(W, E, wst);
      p.pack.push_back(blockMove(BUF_IN, ah.interiorOffset() + off_a[d] * ast[ax.a], ast, BUF_WORK,
                                 p.send_base + p.send_off[d], wst, E, d));
    }
  }
  if (traits.symmetric_recv && !inplace) {
    // the same slabs, written straight into the owners' output pencils (their geometry, their halos / padding)
    for (int j = 1; j <= P; ++j) {
      const int d = (j == P) ? me : p.schedule_dst[j];
      auto pidx_d = pidx;
      pidx_d[p.comm_axis == COMM_COL ? 0 : 1] = d;
      const Pencil bd = makePencil(g, pidx_d, ax.b, out_halo, out_pad);
      i64 E[3] = {Sa[0], Sa[1], Sa[2]}, dst[3];
      E[ax.a] = splits_a[d];
      for (int ga = 0; ga < 3; ++ga) dst[ga] = bd.strideG(ga);
      p.direct.push_back(blockMove(BUF_IN, ah.interiorOffset() + off_a[d] * ast[ax.a], ast, BUF_OUT,
                                   bd.interiorOffset() + off_b[me] * dst[ax.b], dst, E, d));
    }
  }
  if (!skip_unpack) {
    for (int j = 0; j < P; ++j) {  // my own chunk first, then peers in schedule order
      const int s = (j == 0) ? me : p.schedule_src[j];
      i64 E[3] = {Sb[0], Sb[1], Sb[2]}, wst[3];
      E[ax.b] = splits_b[s];
      denseStrides(W, E, wst);
      p.unpack.push_back(blockMove(BUF_WORK, p.recv_base + p.recv_off[s], wst, BUF_OUT,
                                   bh.interiorOffset() + off_b[s] * bst[ax.b], bst, E, s));
      // the chunks are slabs along ax_b: unless that is the output's fastest memory axis every chunk holds whole rows
      // (one-element rows excepted: the next axis is then the contiguous one, and it may be the split one)
      p.unpack.back().dst_row_pitch = ((b.order[0] != ax.b) && Sb[b.order[0]] > 1) ? bst[b.order[1]] : 0;
    }
  }
  return p;
}

TransposeFieldsPlan buildTransposeFieldsPlan(const GridShape& g, int rank, TransposeOp op, const int32_t* in_halo,
                                             const int32_t* out_halo, const int32_t* in_pad, const int32_t* out_pad, bool inplace,
                                             const TransportTraits& traits, int npergroup, int n_fields) {
  if (n_fields < 1) CD_INVALID_USAGE("n_fields argument out of range");
  TransposeFieldsPlan fp;
  fp.n_fields = n_fields;
  TransportTraits t = traits;
  if (n_fields >= 2) {
    t.no_elide = true;
    t.pipelined = false;
  }
  fp.base = buildTransposePlan(g, rank, op, in_halo, out_halo, in_pad, out_pad, inplace, t, npergroup);
  TransposePlan& p = fp.base;
  fp.pack_step.assign(p.pack.size(), 0);
  fp.unpack_step.assign(p.unpack.size(), 0);
  if (n_fields == 1) return fp;
  const i64 n = n_fields;
  p.direct.clear();
  p.rotate = 0;
  p.rotate_n = 0;
  for (Move3D& m : p.pack) m.dst_row_pitch = 0;
  for (Move3D& m : p.unpack) m.dst_row_pitch = 0;
  if (p.noop) return fp;
  if (!p.exchange) {
    // out of place: pencil -> pencil.  In place: the interior of every field staged through its own piece of the workspace
    for (size_t i = 0; i < p.pack.size(); ++i) {
      const Move3D& m = p.pack[i];
      if (m.src_buf != BUF_IN || (m.dst_buf == BUF_WORK && (m.dst_off != 0 || p.pack.size() != 1 || p.unpack.size() != 1)))
        CD_INTERNAL_ERROR("a local transpose plan of unexpected shape");
      if (m.dst_buf == BUF_WORK) fp.pack_step[i] = p.pencil_elements_a;
    }
    for (size_t i = 0; i < p.unpack.size(); ++i) {
      const Move3D& m = p.unpack[i];
      if (m.src_buf != BUF_WORK || m.src_off != 0 || m.dst_buf != BUF_OUT) CD_INTERNAL_ERROR("a local transpose plan of unexpected shape");
      fp.unpack_step[i] = p.pencil_elements_a;
    }
    return fp;
  }
  if (p.send_buf != BUF_WORK || p.recv_buf != BUF_WORK || p.send_base != 0 || (int)p.pack.size() != p.nranks ||
      (int)p.unpack.size() != p.nranks)
    CD_INTERNAL_ERROR("a multi-field transpose plan came out with an elided pack or unpack");
  const i64 unaligned = t.symmetric_recv ? p.stage_elements : p.pencil_elements_a;
  if (alignElements(unaligned) != p.recv_base) CD_INTERNAL_ERROR("a transpose plan with an unexpected receive base");
  const i64 single_recv_base = p.recv_base;
  p.recv_base = alignElements(n * unaligned);
  for (size_t i = 0; i < p.pack.size(); ++i) {
    Move3D& m = p.pack[i];
    const int d = m.peer;
    if (m.src_buf != BUF_IN || m.dst_buf != BUF_WORK || d < 0 || d >= p.nranks || m.dst_off != p.send_off[d] ||
        m.elements() != p.send_cnt[d])
      CD_INTERNAL_ERROR("a transpose pack that does not fill its peer's chunk");
    m.dst_off = n * p.send_off[d];
    fp.pack_step[i] = p.send_cnt[d];
  }
  for (size_t i = 0; i < p.unpack.size(); ++i) {
    Move3D& m = p.unpack[i];
    const int s = m.peer;
    if (m.src_buf != BUF_WORK || m.dst_buf != BUF_OUT || s < 0 || s >= p.nranks || m.src_off != single_recv_base + p.recv_off[s] ||
        m.elements() != p.recv_cnt[s])
      CD_INTERNAL_ERROR("a transpose unpack that does not drain its peer's chunk");
    m.src_off = p.recv_base + n * p.recv_off[s];
    fp.unpack_step[i] = p.recv_cnt[s];
  }
  for (int i = 0; i < p.nranks; ++i) {
    p.send_cnt[i] *= n;
    p.send_off[i] *= n;
    p.recv_cnt[i] *= n;
    p.recv_off[i] *= n;
    p.remote_recv_off[i] *= n;
  }
  return fp;
}

int stageCount(const TransposePlan& p, int wanted, int es, i64 min_stage_bytes) {
  const i64 by_size = min_stage_bytes > 0 ? std::max<i64>(1, p.stage_elements * es / min_stage_bytes) : (i64)wanted;
  return (int)std::max<i64>(1, std::min<i64>({(i64)wanted, p.stage_limit, (i64)14, by_size}));
}

Move3D stageOfMove(const Move3D& m, int axis, int k, int K) {
  Move3D r = m;
  const i64 n = m.extent[axis], lo = n * k / K, hi = n * (k + 1) / K;
  r.extent[axis] = hi - lo;
  r.src_off += lo * m.ss[axis];
  r.dst_off += lo * m.ds[axis];
  if (K > 1 && m.ds[axis] == 1) r.dst_row_pitch = 0;  // (a stage that cuts the rows themselves)
  return r;
}

HaloPlan buildHaloPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                       const int32_t* pad, bool force_packed, bool self_exchange) {
  HaloPlan p;
  p.axis = axis;
  p.dim = dim;
  const auto pidx = gridIndexOfRank(g, rank);
  const Pencil h = makePencil(g, pidx, axis, halo, nullptr);  // extents of what is exchanged
  const Pencil hp = makePencil(g, pidx, axis, halo, pad);     // strides of the user's buffer
  if (anyEmptyPencil(g, axis)) CD_NOT_SUPPORTED("halo operations on configurations with empty pencils not supported");

  const bool periodic = periods && periods[dim];
  p.neighbor[0] = shiftedRank(g, rank, axis, dim, -1, periodic);
  p.neighbor[1] = shiftedRank(g, rank, axis, dim, +1, periodic);
  const i64 he = halo[dim];
  if (he == 0) return p;

  p.comm_axis = commAxisOfDim(axis, dim);
  if (p.neighbor[0] == rank && p.neighbor[1] == rank && !self_exchange) {
    p.kind = HaloPlan::SELF_PERIODIC;
  } else if (p.neighbor[0] == -1 && p.neighbor[1] == -1) {
    return p;  // one rank along a non-periodic dimension
  } else {
    // only nearest-neighbour halos: the halo may not be wider than my slab or a neighbour's slab
    if (p.neighbor[0] == rank && p.neighbor[1] == rank) {  // self_exchange: periodic wrap onto myself, through the transport
      if (he > h.extentG(dim) - 2 * he) CD_INVALID_USAGE("halo wider than the pencil it wraps around");
    } else {
      requireNearestNeighbourHalo(g, pidx, p.comm_axis, dim, he, periodic);
    }
    const bool faces_contiguous = (dim == h.order[2]);
    p.kind = (faces_contiguous && !anySet(pad) && !force_packed) ? HaloPlan::DIRECT : HaloPlan::PACKED;
  }

  // A face is the slab of thickness he along `dim`, spanning the other two dims INCLUDING their halos
  // (so that updating dims 0,1,2 in turn also fills edges and corners) but not their padding.
  i64 E[3], st[3], fst[3];
  for (int ga = 0; ga < 3; ++ga) {
    E[ga] = (ga == dim) ? he : h.extentG(ga);
    st[ga] = hp.strideG(ga);
  }
  denseStrides(h.order, E, fst);
  p.face_elements = E[0] * E[1] * E[2];
  const i64 sd = st[dim];
  const i64 n = hp.extentG(dim) - (pad ? pad[dim] : 0);  // extent along dim without padding
  const i64 lo_halo = 0, lo_face = he * sd, hi_face = (n - 2 * he) * sd, hi_halo = (n - he) * sd;

  switch (p.kind) {
    case HaloPlan::SELF_PERIODIC:
      p.pre.push_back(blockMove(BUF_IN, hi_face, st, BUF_IN, lo_halo, st, E, -1));
      p.pre.push_back(blockMove(BUF_IN, lo_face, st, BUF_IN, hi_halo, st, E, -1));
      break;
    case HaloPlan::PACKED: {
      const i64 A = alignElements(p.face_elements);
      p.xbuf = BUF_WORK;
      p.send_off[0] = 0;
      p.send_off[1] = A;
      p.recv_off[0] = 2 * A;
      p.recv_off[1] = 3 * A;
      if (p.neighbor[0] != -1) {
        p.pre.push_back(blockMove(BUF_IN, lo_face, st, BUF_WORK, p.send_off[0], fst, E, 0));
        p.post.push_back(blockMove(BUF_WORK, p.recv_off[0], fst, BUF_IN, lo_halo, st, E, 0));
      }
      if (p.neighbor[1] != -1) {
        p.pre.push_back(blockMove(BUF_IN, hi_face, st, BUF_WORK, p.send_off[1], fst, E, 1));
        p.post.push_back(blockMove(BUF_WORK, p.recv_off[1], fst, BUF_IN, hi_halo, st, E, 1));
      }
    } break;
    case HaloPlan::DIRECT:
      p.xbuf = BUF_IN;
      p.send_off[0] = lo_face;
      p.send_off[1] = hi_face;
      p.recv_off[0] = lo_halo;
      p.recv_off[1] = hi_halo;
      break;
    default: break;
  }
  return p;
}

HaloPlan buildHaloAccumulatePlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, bool /*force_packed*/, bool self_exchange) {
  HaloPlan p;
  p.axis = axis;
  p.dim = dim;
  p.op.kind = HaloOp::ACCUMULATE;
  const auto pidx = gridIndexOfRank(g, rank);
  const Pencil h = makePencil(g, pidx, axis, halo, nullptr);  // extents of what is exchanged
  const Pencil hp = makePencil(g, pidx, axis, halo, pad);     // strides of the user's buffer
  if (anyEmptyPencil(g, axis)) CD_NOT_SUPPORTED("halo operations on configurations with empty pencils not supported");

  const bool periodic = periods && periods[dim];
  p.neighbor[0] = shiftedRank(g, rank, axis, dim, -1, periodic);
  p.neighbor[1] = shiftedRank(g, rank, axis, dim, +1, periodic);
  const i64 he = halo[dim];
  if (he == 0) return p;
  if (p.neighbor[0] == -1 && p.neighbor[1] == -1) return p;  // one rank along a non-periodic dimension

  p.comm_axis = commAxisOfDim(axis, dim);
  const i64 interior = h.extentG(dim) - 2 * he;
  if (p.neighbor[0] == rank && p.neighbor[1] == rank) {  // periodic wrap onto myself
    if (he > interior) CD_INVALID_USAGE("halo wider than the pencil it wraps around");
    p.kind = self_exchange ? HaloPlan::PACKED : HaloPlan::SELF_PERIODIC;
  } else {
    // only nearest-neighbour halos: the halo may not be wider than my slab or a neighbour's slab
    requireNearestNeighbourHalo(g, pidx, p.comm_axis, dim, he, periodic);
    p.kind = HaloPlan::PACKED;
  }
  p.ordered = interior < 2 * he;

  // the slabs of buildHaloPlan: thickness he along `dim`, the other two dims INCLUDING their halos, not their padding
  i64 E[3], st[3], fst[3];
  for (int ga = 0; ga < 3; ++ga) {
    E[ga] = (ga == dim) ? he : h.extentG(ga);
    st[ga] = hp.strideG(ga);
  }
  denseStrides(h.order, E, fst);
  p.face_elements = E[0] * E[1] * E[2];
  const i64 sd = st[dim];
  const i64 n = hp.extentG(dim) - (pad ? pad[dim] : 0);  // extent along dim without padding
  const i64 lo_halo = 0, lo_face = he * sd, hi_face = (n - 2 * he) * sd, hi_halo = (n - he) * sd;
  auto adding = [](Move3D m) {
    m.add = true;
    return m;
  };

  if (p.kind == HaloPlan::SELF_PERIODIC) {
    p.pre.push_back(adding(blockMove(BUF_IN, hi_halo, st, BUF_IN, lo_face, st, E, -1)));
    p.pre.push_back(adding(blockMove(BUF_IN, lo_halo, st, BUF_IN, hi_face, st, E, -1)));
    return p;
  }
  const i64 A = alignElements(p.face_elements);
  p.xbuf = BUF_WORK;
  p.send_off[0] = 0;
  p.send_off[1] = A;
  p.recv_off[0] = 2 * A;
  p.recv_off[1] = 3 * A;
  if (p.neighbor[0] != -1) {
    p.pre.push_back(blockMove(BUF_IN, lo_halo, st, BUF_WORK, p.send_off[0], fst, E, 0));
    p.post.push_back(adding(blockMove(BUF_WORK, p.recv_off[0], fst, BUF_IN, lo_face, st, E, 0)));
  }
  if (p.neighbor[1] != -1) {
    p.pre.push_back(blockMove(BUF_IN, hi_halo, st, BUF_WORK, p.send_off[1], fst, E, 1));
    p.post.push_back(adding(blockMove(BUF_WORK, p.recv_off[1], fst, BUF_IN, hi_face, st, E, 1)));
  }
  return p;
}

HaloPlan buildHaloAccumulateClearPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                      const int32_t* pad, bool force_packed, bool self_exchange) {
  HaloPlan p = buildHaloAccumulatePlan(g, rank, axis, dim, halo, periods, pad, force_packed, self_exchange);
  p.op.clear = true;
  for (Move3D& m : p.pre) {  // (SELF_PERIODIC: the wrap additions; PACKED: the packs -- the moves that read the pencil)
    if (m.src_buf != BUF_IN) CD_INTERNAL_ERROR("the first phase of a halo accumulation reads something other than the pencil");
    m.take = true;
  }
  for (const Move3D& m : p.post)
    if (m.src_buf != BUF_WORK) CD_INTERNAL_ERROR("the last phase of a halo accumulation reads something other than the workspace");
  return p;
}

HaloPlan buildHaloFillPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                           const int32_t* pad, bool force_packed, bool self_exchange) {
  const HaloPlan u = buildHaloPlan(g, rank, axis, dim, halo, periods, pad, force_packed, self_exchange);  // (its refusals)
  HaloPlan p;
  p.axis = axis;
  p.dim = dim;
  p.op.kind = HaloOp::FILL;
  p.comm_axis = u.comm_axis;
  p.neighbor[0] = u.neighbor[0];
  p.neighbor[1] = u.neighbor[1];
  p.face_elements = u.face_elements;
  if (u.kind == HaloPlan::NONE) return p;
  auto filling = [](const Move3D& w) {  // the destination of `w`, nothing else
    Move3D m;
    m.src_buf = BUF_IN;
    m.dst_buf = BUF_IN;
    m.dst_off = w.dst_off;
    for (int i = 0; i < 3; ++i) {
      m.extent[i] = w.extent[i];
      m.ds[i] = w.ds[i];
    }
    m.peer = w.peer;
    m.fill = true;
    return m;
  };
  if (u.kind == HaloPlan::DIRECT) {  // what arrives lands in the pencil itself: whole contiguous faces
    for (int i = 0; i < 2; ++i) {
      if (u.neighbor[i] == -1) continue;
      Move3D w;
      w.dst_off = u.recv_off[i];
      w.extent[0] = u.face_elements;
      w.ds[0] = 1;
      w.peer = i;
      p.pre.push_back(filling(w));
    }
  } else {
    for (const Move3D& w : (u.kind == HaloPlan::SELF_PERIODIC ? u.pre : u.post)) {
      if (w.dst_buf != BUF_IN) CD_INTERNAL_ERROR("a halo update writes its pencil from outside the plan's last phase");
      p.pre.push_back(filling(w));
    }
  }
  p.kind = HaloPlan::SELF_PERIODIC;
  return p;
}

// the reflection's plan for the sides of `sides` (bit 0 low, bit 1 high): the reflection itself takes both, the wall values those
// the caller names.  A side left out is neither written nor checked.
static HaloPlan reflectSides(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                             const int32_t* pad, int centering, bool negate, int sides, bool self_exchange) {
  const HaloPlan u = buildHaloPlan(g, rank, axis, dim, halo, periods, pad, false, self_exchange);  // (its refusals, its neighbours)
  if (centering != 0 && centering != 1) CD_INVALID_USAGE("centering argument must be 0 or 1");
  HaloPlan p;
  p.axis = axis;
  p.dim = dim;
  p.op.kind = HaloOp::REFLECT;
  p.op.centering = centering;
  p.op.negate = negate;
  p.comm_axis = commAxisOfDim(axis, dim);
  p.neighbor[0] = u.neighbor[0];
  p.neighbor[1] = u.neighbor[1];
  const i64 he = halo[dim];
  const bool writes[2] = {p.neighbor[0] == -1 && (sides & 1) != 0, p.neighbor[1] == -1 && (sides & 2) != 0};
  if (he == 0 || (!writes[0] && !writes[1])) return p;

  const auto pidx = gridIndexOfRank(g, rank);
  const Pencil h = makePencil(g, pidx, axis, halo, nullptr);
  const Pencil hp = makePencil(g, pidx, axis, halo, pad);
  const i64 c = centering;
  if (he + c > h.extentG(dim) - 2 * he) CD_INVALID_USAGE("halo reflection reaches beyond the interior of the pencil");
  // the slabs of buildHaloPlan: thickness he along `dim`, the other two dims INCLUDING their halos, not their padding
  i64 E[3], st[3], sst[3];
  for (int ga = 0; ga < 3; ++ga) {
    E[ga] = (ga == dim) ? he : h.extentG(ga);
    st[ga] = hp.strideG(ga);
    sst[ga] = (ga == dim) ? -st[ga] : st[ga];
  }
  p.face_elements = E[0] * E[1] * E[2];
  const i64 sd = st[dim];
  const i64 n = hp.extentG(dim) - (pad ? pad[dim] : 0);  // extent along dim without padding
  auto mirroring = [&](i64 src_cell, i64 dst_cell, int side) {  // destination cell dst_cell + j takes source cell src_cell - j
    Move3D m = blockMove(BUF_IN, src_cell * sd, sst, BUF_IN, dst_cell * sd, st, E, side);
    m.reflect = true;
    m.negate = negate;
    return m;
  };
  if (writes[0]) p.pre.push_back(mirroring(2 * he - 1 + c, 0, 0));
  if (writes[1]) p.pre.push_back(mirroring(n - he - 1 - c, n - he, 1));
  p.kind = HaloPlan::SELF_PERIODIC;
  return p;
}

HaloPlan buildHaloReflectPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                              const int32_t* pad, int centering, bool negate, bool self_exchange) {
  return reflectSides(g, rank, axis, dim, halo, periods, pad, centering, negate, 3, self_exchange);
}

int wallValueRefusal(int sides, bool has_low, bool has_high, i64 halo_dim) {
  if (sides < 1 || sides > 3) return 1;
  if (((sides & 1) && !has_low) || ((sides & 2) && !has_high)) return 2;
  return halo_dim > kMaxWallLayers ? 3 : 0;
}

void refuseWallValues(int refusal) {
  if (refusal == 1) CD_INVALID_USAGE("sides argument must be 1, 2 or 3: the low halo, the high halo or both");
  if (refusal == 2) CD_INVALID_USAGE("the value array of a side named in sides cannot be null");
  if (refusal == 3) CD_NOT_SUPPORTED("halo_extents[dim] is wider than CUDECOMP_AMD_MAX_WALL_HALO");
  CD_INTERNAL_ERROR("no wall-value refusal to make");
}

HaloPlan buildHaloWallValuesPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, int centering, bool negate, int sides, bool self_exchange) {
  if (sides < 1 || sides > 3) {  // (callers check first, in the contract's place; here after the reflection's own argument checks)
    reflectSides(g, rank, axis, dim, halo, periods, pad, centering, negate, 0, self_exchange);
    refuseWallValues(1);
  }
  if (halo[dim] > kMaxWallLayers) {
    reflectSides(g, rank, axis, dim, halo, periods, pad, centering, negate, 0, self_exchange);
    refuseWallValues(3);
  }
  HaloPlan p = reflectSides(g, rank, axis, dim, halo, periods, pad, centering, negate, sides, self_exchange);
  p.op.kind = HaloOp::WALL_VALUES;
  p.op.sides = sides;
  for (Move3D& m : p.pre) {
    if (!m.reflect || (m.peer != 0 && m.peer != 1)) CD_INTERNAL_ERROR("a wall-value plan whose moves are not the reflection's");
    m.affine = m.peer + 1;  // (blockMove's `peer` of a reflect-move is its side)
  }
  return p;
}

int wallPlaneRefusal(int sides, const void* plane_low, const void* plane_high, const void* pencil, i64 pencil_bytes, i64 plane_bytes) {
  if (sides < 1 || sides > 3) return 1;
  if (((sides & 1) && !plane_low) || ((sides & 2) && !plane_high)) return 2;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(pencil), p1 = p0 + (uintptr_t)pencil_bytes;
  for (int side = 0; side < 2 && plane_bytes > 0 && pencil_bytes > 0; ++side) {
    if (!(sides & (1 << side))) continue;
    const uintptr_t q0 = reinterpret_cast<uintptr_t>(side == 0 ? plane_low : plane_high), q1 = q0 + (uintptr_t)plane_bytes;
    if (q0 < p1 && p0 < q1) return 3;
  }
  return 0;
}

void refuseWallPlanes(int refusal) {
  if (refusal == 1) CD_INVALID_USAGE("sides argument must be 1, 2 or 3: the low halo, the high halo or both");
  if (refusal == 2) CD_INVALID_USAGE("the plane of a side named in sides cannot be null");
  if (refusal == 3) CD_INVALID_USAGE("a plane named in sides cannot overlap the pencil");
  CD_INTERNAL_ERROR("no wall-plane refusal to make");
}

HaloPlan buildHaloWallPlanesPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, int centering, bool negate, int sides, bool self_exchange) {
  if (sides < 1 || sides > 3) {  // (callers check first, in the contract's place; here after the reflection's own argument checks)
    reflectSides(g, rank, axis, dim, halo, periods, pad, centering, negate, 0, self_exchange);
    refuseWallPlanes(1);
  }
  HaloPlan p = reflectSides(g, rank, axis, dim, halo, periods, pad, centering, negate, sides, self_exchange);
  p.op.kind = HaloOp::WALL_PLANES;
  p.op.sides = sides;
  // the plane: the pencil's shape with the extent along `dim` replaced by h, dense in the pencil's memory order
  const Pencil hp = makePencil(g, gridIndexOfRank(g, rank), axis, halo, pad);
  const i64 he = halo[dim];
  if (he > 0 && !(periods && periods[dim]) && hp.extentG(dim) > 0) {
    p.pencil_elements = hp.size;
    p.plane_elements = hp.size / hp.extentG(dim) * he;
  }
  if (p.pre.empty()) return p;
  i64 pst[3], run = 1;
  for (int i = 0; i < 3; ++i) {
    pst[hp.order[i]] = run;
    run *= hp.order[i] == dim ? he : (i64)hp.shape[i];
  }
  for (Move3D& m : p.pre) {
    if (!m.reflect || (m.peer != 0 && m.peer != 1)) CD_INTERNAL_ERROR("a wall-plane plan whose moves are not the reflection's");
    const bool low = m.peer == 0;  // (blockMove's `peer` of a reflect-move is its side)
    m.plane = m.peer + 1;
    for (int ga = 0; ga < 3; ++ga) m.ps[ga] = pst[ga];
    // destination index j along `dim` is ghost layer h - 1 - j on the low side, layer j on the high side; the other two dims start
    // at the pencil's index 0, as the slab does
    m.plane_off = low ? (he - 1) * pst[dim] : 0;
    if (low) m.ps[dim] = -pst[dim];
  }
  return p;
}

HaloPlan buildHaloFoldPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                           const int32_t* pad, int centering, bool negate, bool clear, bool self_exchange) {
  // (its refusals, its neighbours, its sides: one fold-move per reflect-move, the same cells with source and destination swapped)
  const HaloPlan r = buildHaloReflectPlan(g, rank, axis, dim, halo, periods, pad, centering, negate, self_exchange);
  HaloPlan p;
  p.axis = axis;
  p.dim = dim;
  p.op.kind = HaloOp::FOLD;
  p.op.centering = centering;
  p.op.negate = negate;
  p.op.clear = clear;
  p.comm_axis = r.comm_axis;
  p.neighbor[0] = r.neighbor[0];
  p.neighbor[1] = r.neighbor[1];
  p.face_elements = r.face_elements;
  if (r.kind == HaloPlan::NONE) return p;

  const i64 he = halo[dim], c = centering;
  const i64 sd = -r.pre[0].ss[dim];                                                // (the pencil's stride along dim)
  const Pencil hp = makePencil(g, gridIndexOfRank(g, rank), axis, halo, pad);
  const i64 n = hp.extentG(dim) - (pad ? pad[dim] : 0);  // extent along dim without padding
  for (const Move3D& rm : r.pre) {  // destination cell dst_cell + j takes source cell src_cell - j
    const bool low = rm.peer == 0;  // (the side)
    const i64 src_cell = low ? he - 1 : n - 1, dst_cell = low ? he + c : n - 2 * he - c;
    Move3D m = rm;
    m.src_off = src_cell * sd;
    m.dst_off = dst_cell * sd;
    m.add = true;
    m.take = clear;
    p.pre.push_back(m);
  }
  p.ordered = p.pre.size() == 2 && n < 4 * he + 2 * c;
  p.kind = HaloPlan::SELF_PERIODIC;
  return p;
}

// the slots of a packed single plan are alignElements(face) apart: move them alignElements(n_fields * face) apart
static void relayFieldSlots(HaloPlan& p) {
  const int n_fields = p.op.n_fields;
  const i64 single = alignElements(p.face_elements);
  p.slot_elements = n_fields == 1 ? single : alignElements((i64)n_fields * p.face_elements);
  if (n_fields == 1) return;
  auto moved = [&](i64 off) {
    if (off % single != 0 || off / single > 3) CD_INTERNAL_ERROR("a packed halo plan with an unexpected workspace layout");
    return off / single * p.slot_elements;
  };
  for (int i = 0; i < 2; ++i) {
    p.send_off[i] = moved(p.send_off[i]);
    p.recv_off[i] = moved(p.recv_off[i]);
  }
  for (Move3D& m : p.pre) {
    if (m.src_buf != BUF_IN || m.dst_buf != BUF_WORK) CD_INTERNAL_ERROR("a halo pack that does not run pencil -> workspace");
    m.dst_off = moved(m.dst_off);
  }
  for (Move3D& m : p.post) {
    if (m.src_buf != BUF_WORK || m.dst_buf != BUF_IN) CD_INTERNAL_ERROR("a halo unpack that does not run workspace -> pencil");
    m.src_off = moved(m.src_off);
  }
}

HaloPlan buildHaloFieldsPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                             const int32_t* pad, int n_fields, bool force_packed, bool self_exchange) {
  if (n_fields < 1) CD_INVALID_USAGE("n_fields argument out of range");
  HaloPlan p = buildHaloPlan(g, rank, axis, dim, halo, periods, pad, force_packed || n_fields >= 2, self_exchange);
  p.op.n_fields = n_fields;
  if (p.kind == HaloPlan::DIRECT && n_fields >= 2) CD_INTERNAL_ERROR("a multi-field halo plan came out direct");
  if (p.kind == HaloPlan::PACKED) relayFieldSlots(p);
  return p;
}

HaloPlan buildHaloAccumulateFieldsPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                       const int32_t* pad, int n_fields, bool clear, bool self_exchange) {
  if (n_fields < 1) CD_INVALID_USAGE("n_fields argument out of range");
  HaloPlan p = (clear ? buildHaloAccumulateClearPlan : buildHaloAccumulatePlan)(g, rank, axis, dim, halo, periods, pad, true, self_exchange);
  p.op.n_fields = n_fields;
  if (p.kind == HaloPlan::DIRECT) CD_INTERNAL_ERROR("a halo accumulation plan came out direct");
  if (p.kind == HaloPlan::PACKED) relayFieldSlots(p);
  return p;
}

HaloPlan buildHaloWallFieldsPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, bool fold, int centering, bool clear, int n_fields, bool self_exchange) {
  if (n_fields < 2) CD_INTERNAL_ERROR("a multi-field wall plan for fewer than two fields");
  HaloPlan p = fold ? buildHaloFoldPlan(g, rank, axis, dim, halo, periods, pad, centering, false, clear, self_exchange)
                    : buildHaloReflectPlan(g, rank, axis, dim, halo, periods, pad, centering, false, self_exchange);
  p.op.n_fields = n_fields;
  for (const Move3D& m : p.pre)
    if (!m.reflect || m.negate || m.src_buf != BUF_IN || m.dst_buf != BUF_IN) CD_INTERNAL_ERROR("a wall plan whose moves are not unsigned mirrors of the pencil");
  return p;
}

HaloPlan buildHaloOpPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods, const int32_t* pad,
                         const HaloOp& op, bool force_packed, bool self_exchange) {
  if ((op.kind == HaloOp::REFLECT || op.kind == HaloOp::FOLD) && op.n_fields != 1) {
    if (op.negate) CD_INTERNAL_ERROR("the parities of a multi-field wall call are no part of its plan");
    return buildHaloWallFieldsPlan(g, rank, axis, dim, halo, periods, pad, op.kind == HaloOp::FOLD, op.centering, op.clear, op.n_fields,
                                   self_exchange);
  }
  switch (op.kind) {
    case HaloOp::UPDATE: return buildHaloFieldsPlan(g, rank, axis, dim, halo, periods, pad, op.n_fields, force_packed, self_exchange);
    case HaloOp::ACCUMULATE: return buildHaloAccumulateFieldsPlan(g, rank, axis, dim, halo, periods, pad, op.n_fields, op.clear, self_exchange);
    case HaloOp::FILL: return buildHaloFillPlan(g, rank, axis, dim, halo, periods, pad, force_packed, self_exchange);
    case HaloOp::REFLECT: return buildHaloReflectPlan(g, rank, axis, dim, halo, periods, pad, op.centering, op.negate, self_exchange);
    case HaloOp::FOLD: return buildHaloFoldPlan(g, rank, axis, dim, halo, periods, pad, op.centering, op.negate, op.clear, self_exchange);
    case HaloOp::WALL_VALUES: {
      // several fields (cudecomp_halo_wall_value_fields.h): the single call's moves, one per side kept, unsigned -- parities and
      // addends travel with the call and are no part of the plan
      if (op.n_fields < 1) CD_INTERNAL_ERROR("a wall-value plan without a field");
      if (op.n_fields != 1 && op.negate) CD_INTERNAL_ERROR("the parities of a multi-field wall call are no part of its plan");
      HaloPlan p = buildHaloWallValuesPlan(g, rank, axis, dim, halo, periods, pad, op.centering, op.negate, op.sides, self_exchange);
      p.op.n_fields = op.n_fields;
      return p;
    }
    case HaloOp::WALL_PLANES:
      if (op.n_fields != 1) CD_INTERNAL_ERROR("wall planes serve one field per call");
      return buildHaloWallPlanesPlan(g, rank, axis, dim, halo, periods, pad, op.centering, op.negate, op.sides, self_exchange);
  }
  CD_INTERNAL_ERROR("unknown halo operation");
}

int normalizeMove(Move3D& m) {
  struct D {
    i64 e, s, d;
  };
  D dims[3];
  int n = 0;
  for (int i = 0; i < 3; ++i)
    if (m.extent[i] != 1) dims[n++] = {m.extent[i], m.ss[i], m.ds[i]};
  std::sort(dims, dims + n, [](const D& x, const D& y) { return x.s != y.s ? x.s < y.s : x.d < y.d; });
  // fuse dims that are contiguous continuations of one another on BOTH sides
  bool fused = true;
  while (fused && n > 1) {
    fused = false;
    for (int i = 0; i < n && !fused; ++i)
      for (int j = 0; j < n && !fused; ++j) {
        if (i == j) continue;
        if (dims[j].s == dims[i].s * dims[i].e && dims[j].d == dims[i].d * dims[i].e) {
          dims[i].e *= dims[j].e;
          for (int k = j; k + 1 < n; ++k) dims[k] = dims[k + 1];
          --n;
          fused = true;
        }
      }
  }
  std::sort(dims, dims + n, [](const D& x, const D& y) { return x.s != y.s ? x.s < y.s : x.d < y.d; });
  for (int i = 0; i < 3; ++i) {
    if (i < n) {
      m.extent[i] = dims[i].e;
      m.ss[i] = dims[i].s;
      m.ds[i] = dims[i].d;
    } else {
      m.extent[i] = 1;
      m.ss[i] = 0;
      m.ds[i] = 0;
    }
  }
  return n;
}

// ---------------------------------------------------------------------------------------------------------------
// two-hop relay (plan.h)
// ---------------------------------------------------------------------------------------------------------------
RelayPlan buildRelayPlan(const GridShape& g, int nranks, int rank, TransposeOp op, const int32_t* in_halo,
                         const int32_t* out_halo, const int32_t* in_pad, const int32_t* out_pad, bool inplace,
                         const TransportTraits& traits, int npergroup) {
  RelayPlan rp;
  rp.nranks = nranks;
  if (nranks != g.pdims[0] * g.pdims[1]) return rp;
  // the plans of all ranks (cheap: index math only)
  std::vector<TransposePlan> plans;
  plans.reserve(nranks);
  for (int s = 0; s < nranks; ++s) plans.push_back(buildTransposePlan(g, s, op, in_halo, out_halo, in_pad, out_pad, inplace, traits, npergroup));
  const TransposePlan& mine = plans[rank];
  if (!mine.exchange || !relayWorthwhile(mine.nranks, nranks)) return rp;
  const int P = mine.nranks;
  rp.slots_per_source = P - 1;
  for (const TransposePlan& p : plans)
    for (int i = 0; i < P; ++i)
      if (i != p.comm_rank) rp.slot_elements = std::max(rp.slot_elements, (p.send_cnt[i] + nranks - 1) / nranks);
  rp.slot_elements = alignElements(rp.slot_elements);  // slots start on 256-byte boundaries
  for (int s = 0; s < nranks; ++s) {
    const TransposePlan& p = plans[s];
    const auto pidx = gridIndexOfRank(g, s);
    int j = 0;  // index among the chunks s sends
    for (int i = 0; i < P; ++i) {
      if (i == p.comm_rank) continue;
      const int d = globalRankOf(g, pidx, p.comm_axis, i);
      const i64 cnt = p.send_cnt[i];
      for (int q = 0; q < nranks; ++q) {
        const i64 lo = cnt * q / nranks, hi = cnt * (q + 1) / nranks;
        if (hi == lo) continue;
        const i64 slot = ((i64)s * (P - 1) + j) * rp.slot_elements;
        if (q == s || q == d) {  // straight to the destination
          if (s == rank) rp.scatter.push_back({d, false, p.send_off[i] + lo, p.remote_recv_off[i] + lo, hi - lo});
        } else {
          if (s == rank) rp.scatter.push_back({q, true, p.send_off[i] + lo, slot, hi - lo});
          if (q == rank) rp.forward.push_back({d, false, slot, p.remote_recv_off[i] + lo, hi - lo});
        }
      }
      ++j;
    }
  }
  rp.applies = true;
  return rp;
}

}  // namespace cudecomp
