// ext.cc -- cudecomp_ext.h: plan introspection and a single-move kernel entry for test harnesses.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "cudecomp_ext.h"
#include "cudecomp_halo_fields.h"
#include "cudecomp_halo_accumulate_fields.h"
#include "cudecomp_halo_wall_fields.h"
#include "cudecomp_halo_wall_values.h"
#include "cudecomp_transpose_fields.h"
#include "errors.h"
#include "internal.h"
#include "rotate_walk.h"
#include "transport.h"

using namespace cudecomp;

namespace {

cudecompResult_t fail(const Error& e) {
  std::cerr << e.what();
  return e.code();
}

// every entry point's body runs in here (api.cc: CD_API_CATCH): an Error is reported and becomes its result code
template <typename Body>
cudecompResult_t guarded(Body&& body) {
  try {
    body();
  } catch (const Error& e) {
    return fail(e);
  } catch (...) {
    return CUDECOMP_RESULT_INTERNAL_ERROR;
  }
  return CUDECOMP_RESULT_SUCCESS;
}

// tests: "the cells between consecutive destination rows are the move's to rewrite" -- the pitch of consecutive rows is the
// smallest destination stride among the dims that are not the unit-stride one
i64 wholeRowsPitchOf(const Move3D& m) {
  i64 pitch = 0;
  for (int i = 0; i < 3; ++i)
    if (m.extent[i] > 1 && m.ds[i] > 1 && (pitch == 0 || m.ds[i] < pitch)) pitch = m.ds[i];
  return pitch;
}

void exportMove(const Move3D& m, cudecompExtMove_t* o) {
  o->src_buf = m.src_buf;
  o->dst_buf = m.dst_buf;
  o->src_off = m.src_off;
  o->dst_off = m.dst_off;
  for (int i = 0; i < 3; ++i) {
    o->extent[i] = m.extent[i];
    o->ss[i] = m.ss[i];
    o->ds[i] = m.ds[i];
  }
  o->peer = m.peer;
  o->row_pitch = (int32_t)std::min<i64>(m.dst_row_pitch, 0x7fffffff);
}

void exportTransposePlan(const TransposePlan& p, const std::vector<int>& global_ranks, cudecompExtTransposePlan_t* out) {
    if (p.nranks > CUDECOMP_EXT_MAX_MEMBERS) CD_NOT_SUPPORTED("communicator too large for cudecompExtTransposePlan_t");
    std::memset(out, 0, sizeof(*out));
    out->noop = p.noop;
    out->exchange = p.exchange;
    out->comm_axis = p.comm_axis;
    out->nranks = p.nranks;
    out->comm_rank = p.comm_rank;
    out->send_buf = p.send_buf;
    out->recv_buf = p.recv_buf;
    out->send_base = p.send_base;
    out->recv_base = p.recv_base;
    out->n_pack = (int32_t)p.pack.size();
    out->n_unpack = (int32_t)p.unpack.size();
    out->rotate = p.rotate;
    for (int i = 0; i < p.nranks; ++i) {
      out->member_global_rank[i] = global_ranks[i];
      if (p.exchange) {
        out->send_cnt[i] = p.send_cnt[i];
        out->send_off[i] = p.send_off[i];
        out->recv_cnt[i] = p.recv_cnt[i];
        out->recv_off[i] = p.recv_off[i];
        out->remote_recv_off[i] = p.remote_recv_off[i];
      }
      out->schedule_dst[i] = p.schedule_dst[i];
    }
    for (size_t i = 0; i < p.pack.size(); ++i) exportMove(p.pack[i], &out->pack[i]);
    for (size_t i = 0; i < p.unpack.size(); ++i) exportMove(p.unpack[i], &out->unpack[i]);
    out->n_direct = (int32_t)p.direct.size();
    for (size_t i = 0; i < p.direct.size(); ++i) exportMove(p.direct[i], &out->direct[i]);
    out->stage_axis = p.stage_axis;
    out->stage_limit = p.stage_limit;
    for (int i = 0; i < p.nranks && p.exchange; ++i) {
      out->send_n[i] = p.send_n[i];
      out->recv_n[i] = p.recv_n[i];
    }
}

void exportHaloPlan(const HaloPlan& p, cudecompExtHaloPlan_t* out) {
    std::memset(out, 0, sizeof(*out));
    out->kind = (int32_t)p.kind;
    out->comm_axis = p.comm_axis;
    out->xbuf = p.xbuf;
    out->face_elements = p.face_elements;
    for (int i = 0; i < 2; ++i) {
      out->neighbor[i] = p.neighbor[i];
      out->send_off[i] = p.send_off[i];
      out->recv_off[i] = p.recv_off[i];
    }
    out->n_pre = (int32_t)p.pre.size();
    out->n_post = (int32_t)p.post.size();
    for (size_t i = 0; i < p.pre.size(); ++i) exportMove(p.pre[i], &out->pre[i]);
    for (size_t i = 0; i < p.post.size(); ++i) exportMove(p.post[i], &out->post[i]);
    const HaloOp& op = p.op;  // (cudecomp_ext.h: cudecompExtHaloPlan_t::reserved)
    if (op.kind == HaloOp::ACCUMULATE) {
      out->reserved = 1 | (p.ordered ? 2 : 0);
      for (size_t i = 0; i < p.pre.size(); ++i)
        if (p.pre[i].add) out->reserved |= 16 << i;
      for (size_t i = 0; i < p.post.size(); ++i)
        if (p.post[i].add) out->reserved |= 64 << i;
    }
    if (op.kind == HaloOp::FILL) out->reserved = 256;
    if (op.kind == HaloOp::REFLECT) out->reserved = 4096 | (op.negate ? 8192 : 0);
    if (op.kind == HaloOp::FOLD) out->reserved = 16384 | (op.negate ? 8192 : 0) | (p.ordered ? 2 : 0);
    if (op.kind == HaloOp::WALL_VALUES) out->reserved = 32768 | (op.negate ? 8192 : 0) | (op.sides << 16);
    if (op.kind == HaloOp::WALL_PLANES) out->reserved = 262144 | (op.negate ? 8192 : 0) | (op.sides << 16);
    if (op.clear) {
      out->reserved |= 512;
      for (size_t i = 0; i < p.pre.size(); ++i)
        if (p.pre[i].take) out->reserved |= 1024 << i;
      for (size_t i = 0; i < p.post.size(); ++i)
        if (p.post[i].take) CD_INTERNAL_ERROR("a move after the exchange clears its source");
    }
}

// the multi-field form: the single plan's fields (its flags included: 0 for an update), the number of fields and the slot length
void exportHaloPlan(const HaloPlan& p, cudecompExtHaloFieldsPlan_t* out) {
  cudecompExtHaloPlan_t single;
  exportHaloPlan(p, &single);
  std::memset(out, 0, sizeof(*out));
  out->kind = single.kind;
  out->comm_axis = single.comm_axis;
  out->n_fields = p.op.n_fields;
  out->reserved = single.reserved;
  out->face_elements = single.face_elements;
  out->slot_elements = p.slot_elements;
  for (int i = 0; i < 2; ++i) {
    out->neighbor[i] = single.neighbor[i];
    out->send_off[i] = single.send_off[i];
    out->recv_off[i] = single.recv_off[i];
    out->pre[i] = single.pre[i];
    out->post[i] = single.post[i];
  }
  out->n_pre = single.n_pre;
  out->n_post = single.n_post;
}

GridShape shapeFromSpec(const cudecompExtGridSpec_t* spec) {
  if (!spec) CD_INVALID_USAGE("grid spec cannot be null");
  GridShape g;
  for (int i = 0; i < 3; ++i) {
    g.gdims[i] = spec->gdims[i];
    g.gdims_dist[i] = spec->gdims_dist[i] > 0 ? spec->gdims_dist[i] : spec->gdims[i];
    if (g.gdims[i] < 1 || g.gdims_dist[i] > g.gdims[i]) CD_INVALID_USAGE("bad gdims / gdims_dist in grid spec");
    bool seen[3] = {false, false, false};
    for (int j = 0; j < 3; ++j) {
      const int v = spec->mem_order[i][j];
      if (v < 0 || v > 2 || seen[v]) CD_INVALID_USAGE("mem_order rows of a grid spec must be permutations of 0,1,2");
      seen[v] = true;
      g.mem_order[i][j] = v;
    }
  }
  g.pdims = {spec->pdims[0], spec->pdims[1]};
  if (g.pdims[0] < 1 || g.pdims[1] < 1) CD_INVALID_USAGE("bad pdims in grid spec");
  g.col_major = spec->col_major != 0;
  return g;
}

// cudecompExtRunMoves / cudecompExtDescribeMoves: the list, the tuning and the arithmetic as the kernel layer takes them
KernelTuning tuningOfFlags(int32_t flags) {  // the bits of cudecompExtMove3D
  KernelTuning t;
  if (flags & 1) t.force_class = MOVE_GENERIC;
  if (flags & 2) t.force_streaming = true;
  if (flags & 4) t.window_mode = 1;
  if (flags & 8) t.window_mode = 0;
  if (flags & 64) t.walk_order = 0;
  if (flags & 128) t.walk_order = 1;
  return t;
}

KernelTuning tuningOfForce(int32_t force) {  // the `force` bits of the entries that take nothing else: 1, 2, 4
  KernelTuning t;
  if (force & 1) t.force_class = MOVE_GENERIC;
  if (force & 2) t.force_streaming = true;
  if (force & 4) t.no_streaming = true;
  return t;
}

std::vector<void*> pointersOf(const uint64_t* addresses, int32_t n) {
  std::vector<void*> p(n);
  for (int32_t i = 0; i < n; ++i) p[i] = reinterpret_cast<void*>(addresses[i]);
  return p;
}

int launchesOf(const KernelStats& st) {
  int total = 0;
  for (int c = 0; c < MOVE_CLASS_COUNT; ++c) total += st.launches[c];
  return total;
}

// the cudecompExt*3D entries: the geometry of their one move from BUF_IN to BUF_OUT (a fill has no source strides) ...
Move3D move3DOf(const int64_t extent[3], const int64_t ss[3], const int64_t ds[3]) {
  Move3D m;
  m.src_buf = BUF_IN;
  m.dst_buf = BUF_OUT;
  for (int i = 0; i < 3; ++i) {
    m.extent[i] = extent[i];
    if (ss) m.ss[i] = ss[i];
    m.ds[i] = ds[i];
  }
  return m;
}

// ... and its launch with what the entry honours of its `force` bits; *kernel_class: the class that ran, -1 when nothing did
void launchMove3D(const Move3D& m, const void* src, void* dst, int es, const KernelTuning& t, int32_t* kernel_class, hipStream_t stream,
                  ArithType arith = ARITH_NONE, const void* fill_value = nullptr, const WallAddends* addends = nullptr) {
  void* bufs[3] = {const_cast<void*>(src), dst, nullptr};
  KernelStats st;
  launchMoves(&m, 1, bufs, es, stream, &t, &st, nullptr, arith, fill_value, addends);
  if (kernel_class) {
    *kernel_class = -1;
    for (int c = 0; c < MOVE_CLASS_COUNT; ++c)
      if (st.launches[c]) *kernel_class = c;
  }
}

std::vector<Move3D> importMoves(const cudecompExtMove_t* moves, int32_t n, int32_t es, int32_t mode, cudecompDataType_t dtype,
                                ArithType* arith) {
  if (n < 0 || (n > 0 && !moves)) CD_INVALID_USAGE("bad move list");
  if (es != 2 && es != 4 && es != 8 && es != 16) CD_INVALID_USAGE("element size must be 2, 4, 8 or 16");
  if (mode < 0 || mode > 14)
    CD_INVALID_USAGE("mode must be 0 (copy), 1 (add), 2 (fill), 3 (take), 4 (add and take), 5 (mirror copy), 6 (mirror copy with sign flip), "
                     "7 ... 10 (fold: plain, with sign flip, with take, with both), 11 / 12 (wall values: plain, with sign flip) or "
                     "13 / 14 (wall planes: plain, with sign flip)");
  *arith = ARITH_NONE;
  if (mode == 1 || mode == 4 || mode >= 6) {
    if (elementSize(dtype) != es) CD_INVALID_USAGE("element size does not match the data type of the arithmetic");
    *arith = arithOf(dtype);
  }
  std::vector<Move3D> out(n);
  for (int32_t i = 0; i < n; ++i) {
    const cudecompExtMove_t& e = moves[i];
    Move3D& m = out[i];
    if (e.src_buf < 0 || e.src_buf > 2 || e.dst_buf < 0 || e.dst_buf > 2) CD_INVALID_USAGE("buffer index out of range");
    m.src_buf = (BufId)e.src_buf;
    m.dst_buf = (BufId)e.dst_buf;
    m.src_off = e.src_off;
    m.dst_off = e.dst_off;
    for (int d = 0; d < 3; ++d) {
      if (e.extent[d] < 0) CD_INVALID_USAGE("negative extent");
      m.extent[d] = e.extent[d];
      m.ss[d] = e.ss[d];
      m.ds[d] = e.ds[d];
    }
    m.dst_row_pitch = e.row_pitch;
    const bool wall = mode == 11 || mode == 12, wall_plane = mode == 13 || mode == 14;
    m.add = mode == 1 || mode == 4 || (mode >= 7 && !wall && !wall_plane);
    m.fill = mode == 2;
    m.take = mode == 3 || mode == 4 || mode == 9 || mode == 10;
    m.reflect = mode >= 5;
    m.negate = mode == 6 || mode == 8 || mode == 10 || mode == 12 || mode == 14;
    if (wall_plane) {  // the move's `peer` names the plane it reads; entry n + i of the list describes the operand
      if (e.peer != 0 && e.peer != 1) CD_INVALID_USAGE("a wall-plane move (mode 13 / 14) names its plane in `peer`: 0 low, 1 high");
      if (e.src_buf != 0 || e.dst_buf != 0) CD_INVALID_USAGE("a wall-plane move (mode 13 / 14) runs between cells of buffer 0: buffers 1 and 2 are the planes");
      const cudecompExtMove_t& o = moves[n + i];
      m.plane = e.peer + 1;
      m.plane_off = o.dst_off;
      for (int d = 0; d < 3; ++d) m.ps[d] = o.ds[d];
    }
    if (wall) {  // the move's `peer` names the side whose addends it takes
      if (e.peer != 0 && e.peer != 1) CD_INVALID_USAGE("a wall-value move (mode 11 / 12) names its side in `peer`: 0 low, 1 high");
      m.affine = e.peer + 1;
    }
    // a mirror copy says which dim it mirrors: without a negative source stride the entry is a plain copy in the wrong mode
    if (m.reflect && e.ss[0] >= 0 && e.ss[1] >= 0 && e.ss[2] >= 0) {
      if (wall) CD_INVALID_USAGE("a wall-value move (mode 11 / 12) names its mirrored dim with a negative source stride");
      if (wall_plane) CD_INVALID_USAGE("a wall-plane move (mode 13 / 14) names its mirrored dim with a negative source stride");
      if (mode >= 7) CD_INVALID_USAGE("a fold (mode 7 ... 10) names its mirrored dim with a negative source stride");
      CD_INVALID_USAGE("a mirror copy (mode 5 / 6) names its mirrored dim with a negative source stride");
    }
  }
  return out;
}

// Every cudecompExtPlanHalo* function: the grid given by value, the common checks, the defaults for periods and padding, the plan
// of `op`, its export.  `clear` is the caller's number behind op.clear: refused before the plan is built (clear_first) or after
// the plan's own refusals.
template <typename Out>
cudecompResult_t planHaloOp(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[], const bool periods[],
                                   int32_t dim, const int32_t pad[], const HaloOp& op, bool force_packed, Out* out, int32_t clear = 0,
                                   bool clear_first = false, bool self_exchange = false) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!out || !halo) CD_INVALID_USAGE("null argument");
    if (axis < 0 || axis > 2 || dim < 0 || dim > 2) CD_INVALID_USAGE("axis/dim out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    if (clear_first && clear != 0 && clear != 1) CD_INVALID_USAGE("clear argument must be 0 or 1");
    const int32_t zero[3] = {0, 0, 0};
    const bool none[3] = {false, false, false};
    const HaloPlan p = buildHaloOpPlan(g, rank, axis, dim, halo, periods ? periods : none, pad ? pad : zero, op, force_packed, self_exchange);
    if (clear != 0 && clear != 1) CD_INVALID_USAGE("clear argument must be 0 or 1");
    exportHaloPlan(p, out);
  });
}

HaloOp haloOp(HaloOp::Kind kind, bool clear = false, int centering = 0, bool negate = false, int n_fields = 1) {
  HaloOp op;
  op.kind = kind;
  op.clear = clear;
  op.centering = centering;
  op.negate = negate;
  op.n_fields = n_fields;
  return op;
}

// cudecompExtSync*: the list of n flag pointers as the kernels take it; n in 0 .. kMaxFlags, every one of the n pointers set
FlagList flagListOf(uint64_t* const* flags, int32_t n) {
  if (n < 0 || n > kMaxFlags) CD_INVALID_USAGE("n must lie in 0 .. " + std::to_string(kMaxFlags));
  if (n > 0 && !flags) CD_INVALID_USAGE("null flag list");
  FlagList l;
  l.n = n;
  for (int i = 0; i < kMaxFlags; ++i) {
    if (i < n && !flags[i]) CD_INVALID_USAGE("null flag");
    l.f[i] = i < n ? reinterpret_cast<unsigned long long*>(flags[i]) : nullptr;
  }
  return l;
}

void checkFlagStep(int32_t step) {
  if (step < 0 || step >= (int32_t)kFlagScale) CD_INVALID_USAGE("step must lie in 0 .. " + std::to_string(kFlagScale - 1));
}

}  // namespace

extern "C" {

cudecompResult_t cudecompExtGetTransposePlan(cudecompHandle_t handle, cudecompGridDesc_t gd, int32_t op,
                                             const int32_t in_halo[], const int32_t out_halo[], const int32_t in_pad[],
                                             const int32_t out_pad[], bool inplace, int32_t backend_override,
                                             cudecompExtTransposePlan_t* out) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!gd || !gd->initialized || gd->handle != handle) CD_INVALID_USAGE("invalid grid descriptor");
    if (!out) CD_INVALID_USAGE("plan argument cannot be null");
    if (op < 0 || op > 3) CD_INVALID_USAGE("op out of range");
    const auto backend =
        backend_override ? (cudecompTransposeCommBackend_t)backend_override : gd->config.transpose_comm_backend;
    TransportTraits traits;
    traits.pipelined = transposeBackendIsPipelined(backend);
    traits.symmetric_recv = usesPeerTransport(handle, backend);
    traits.self_exchange = handle->self_exchange;
    const CommAxis ca = (op == OP_X_TO_Y || op == OP_Y_TO_X) ? COMM_COL : COMM_ROW;
    const cudecompCommInfo& ci = gd->comm(ca);
    const TransposePlan p = buildTransposePlan(gd->shape, handle->rank, (TransposeOp)op, in_halo, out_halo, in_pad,
                                               out_pad, inplace, traits, ci.npergroup);
    exportTransposePlan(p, ci.global_ranks, out);
  });
}

cudecompResult_t cudecompExtGetHaloPlan(cudecompHandle_t handle, cudecompGridDesc_t gd, int32_t axis,
                                        const int32_t halo[], const bool periods[], int32_t dim, const int32_t pad[],
                                        int32_t backend_override, cudecompExtHaloPlan_t* out) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!gd || !gd->initialized || gd->handle != handle) CD_INVALID_USAGE("invalid grid descriptor");
    if (!out || !halo) CD_INVALID_USAGE("null argument");
    if (axis < 0 || axis > 2 || dim < 0 || dim > 2) CD_INVALID_USAGE("axis/dim out of range");
    const auto backend = backend_override ? (cudecompHaloCommBackend_t)backend_override : gd->config.halo_comm_backend;
    const int32_t zero[3] = {0, 0, 0};
    const HaloPlan p = buildHaloPlan(gd->shape, handle->rank, axis, dim, halo, periods, pad ? pad : zero,
                                     usesPeerTransport(handle, backend), handle->self_exchange);
    exportHaloPlan(p, out);
  });
}

cudecompResult_t cudecompExtGetTransposeTimings(cudecompHandle_t handle, cudecompGridDesc_t gd, int32_t op,
                                                cudecompExtTransposeTimings_t* out) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!gd || !gd->initialized || gd->handle != handle) CD_INVALID_USAGE("invalid grid descriptor");
    if (!out || op < 0 || op > 3) CD_INVALID_USAGE("bad argument");
    const TransposeTimings t = perfCollect(gd, op);
    out->calls = t.calls;
    out->samples = t.samples;
    out->total_ms = t.total_ms;
    out->pack_ms = t.pack_ms;
    out->exchange_ms = t.exchange_ms;
    out->unpack_ms = t.unpack_ms;
    out->pencil_bytes = t.pencil_bytes;
  });
}

cudecompResult_t cudecompExtGetHaloTimings(cudecompHandle_t handle, cudecompGridDesc_t gd, int32_t axis, int32_t dim,
                                           cudecompExtTransposeTimings_t* out) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!gd || !gd->initialized || gd->handle != handle) CD_INVALID_USAGE("invalid grid descriptor");
    if (!out || axis < 0 || axis > 2 || dim < 0 || dim > 2) CD_INVALID_USAGE("bad argument");
    const TransposeTimings t = perfCollectHalo(gd, axis, dim);
    out->calls = t.calls;
    out->samples = t.samples;
    out->total_ms = t.total_ms;
    out->pack_ms = t.pack_ms;
    out->exchange_ms = t.exchange_ms;
    out->unpack_ms = t.unpack_ms;
    out->pencil_bytes = t.pencil_bytes;
  });
}

cudecompResult_t cudecompExtPlanTranspose(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t op,
                                          const int32_t in_halo[], const int32_t out_halo[], const int32_t in_pad[],
                                          const int32_t out_pad[], bool inplace, int32_t pipelined,
                                          int32_t symmetric_recv, int32_t npergroup, cudecompExtTransposePlan_t* out) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!out) CD_INVALID_USAGE("plan argument cannot be null");
    if (op < 0 || op > 3) CD_INVALID_USAGE("op out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    TransportTraits traits;
    traits.pipelined = pipelined != 0;
    traits.symmetric_recv = symmetric_recv != 0;
    const CommAxis ca = (op == OP_X_TO_Y || op == OP_Y_TO_X) ? COMM_COL : COMM_ROW;
    const int P = g.pdims[ca == COMM_COL ? 0 : 1];
    const TransposePlan p = buildTransposePlan(g, rank, (TransposeOp)op, in_halo, out_halo, in_pad, out_pad, inplace,
                                               traits, npergroup > 0 ? npergroup : P);
    std::vector<int> members(P);
    const auto pidx = gridIndexOfRank(g, rank);
    for (int i = 0; i < P; ++i) members[i] = globalRankOf(g, pidx, ca, i);
    exportTransposePlan(p, members, out);
  });
}

cudecompResult_t cudecompExtPlanRelay(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t op, const int32_t in_halo[],
                                      const int32_t out_halo[], const int32_t in_pad[], const int32_t out_pad[], bool inplace,
                                      cudecompExtRelayPlan_t* out) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!out) CD_INVALID_USAGE("plan argument cannot be null");
    if (op < 0 || op > 3) CD_INVALID_USAGE("op out of range");
    const int n = g.pdims[0] * g.pdims[1];
    if (rank < 0 || rank >= n) CD_INVALID_USAGE("rank out of range");
    TransportTraits traits;
    traits.symmetric_recv = true;
    const CommAxis ca = (op == OP_X_TO_Y || op == OP_Y_TO_X) ? COMM_COL : COMM_ROW;
    const RelayPlan rp = buildRelayPlan(g, n, rank, (TransposeOp)op, in_halo, out_halo, in_pad, out_pad, inplace, traits,
                                        g.pdims[ca == COMM_COL ? 0 : 1]);
    std::memset(out, 0, sizeof(*out));
    out->applies = rp.applies ? 1 : 0;
    out->nranks = rp.nranks;
    out->slots_per_source = rp.slots_per_source;
    out->slot_elements = rp.slot_elements;
    out->relay_elements = rp.relayElements();
    if ((int)rp.scatter.size() > CUDECOMP_EXT_MAX_RELAY_MOVES || (int)rp.forward.size() > CUDECOMP_EXT_MAX_RELAY_MOVES)
      CD_NOT_SUPPORTED("relay plan too large for the export structure");
    auto put = [](const std::vector<RelayMove>& v, cudecompExtRelayMove_t* o) {
      for (size_t k = 0; k < v.size(); ++k) o[k] = {v[k].dst_rank, v[k].to_relay ? 1 : 0, v[k].src_off, v[k].dst_off, v[k].count};
    };
    out->n_scatter = (int32_t)rp.scatter.size();
    out->n_forward = (int32_t)rp.forward.size();
    put(rp.scatter, out->scatter);
    put(rp.forward, out->forward);
  });
}

cudecompResult_t cudecompExtPlanHalo(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                     const bool periods[], int32_t dim, const int32_t pad[], int32_t force_packed,
                                     cudecompExtHaloPlan_t* out) {
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::UPDATE), force_packed != 0, out);
}

cudecompResult_t cudecompExtPlanHaloAccumulate(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis,
                                               const int32_t halo[], const bool periods[], int32_t dim, const int32_t pad[],
                                               int32_t force_packed, cudecompExtHaloPlan_t* out) {
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::ACCUMULATE), force_packed != 0, out);
}

cudecompResult_t cudecompExtPlanHaloAccumulateClear(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis,
                                                    const int32_t halo[], const bool periods[], int32_t dim, const int32_t pad[],
                                                    int32_t force_packed, cudecompExtHaloPlan_t* out) {
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::ACCUMULATE, true), force_packed != 0, out);
}

cudecompResult_t cudecompExtPlanHaloFill(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                         const bool periods[], int32_t dim, const int32_t pad[], int32_t force_packed,
                                         cudecompExtHaloPlan_t* out) {
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::FILL), force_packed != 0, out);
}

cudecompResult_t cudecompExtPlanHaloReflect(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                            const bool periods[], int32_t dim, const int32_t pad[], int32_t centering,
                                            int32_t negate, cudecompExtHaloPlan_t* out) {
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::REFLECT, false, centering, negate != 0), false, out);
}

cudecompResult_t cudecompExtPlanHaloFold(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                         const bool periods[], int32_t dim, const int32_t pad[], int32_t centering, int32_t negate,
                                         int32_t clear, cudecompExtHaloPlan_t* out) {
  // (a bad `clear` is refused after the reflection's refusals)
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::FOLD, clear == 1, centering, negate != 0), false, out, clear);
}

cudecompResult_t cudecompExtPencilInfo(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                       const int32_t pad[], cudecompPencilInfo_t* out) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!out) CD_INVALID_USAGE("pencil_info argument cannot be null");
    if (axis < 0 || axis > 2) CD_INVALID_USAGE("axis argument out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    const Pencil p = makePencil(g, gridIndexOfRank(g, rank), axis, halo, pad);
    std::memset(out, 0, sizeof(*out));
    for (int i = 0; i < 3; ++i) {
      out->shape[i] = p.shape[i];
      out->lo[i] = p.lo[i];
      out->hi[i] = p.hi[i];
      out->order[i] = p.order[i];
      out->halo_extents[i] = p.halo[i];
      out->padding[i] = p.pad[i];
    }
    out->size = p.size;
  });
}

cudecompResult_t cudecompExtShiftedRank(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, int32_t dim,
                                        int32_t displacement, bool periodic, int32_t* shifted_rank) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!shifted_rank) CD_INVALID_USAGE("shifted_rank argument cannot be null");
    if (axis < 0 || axis > 2 || dim < 0 || dim > 2) CD_INVALID_USAGE("axis/dim out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    *shifted_rank = shiftedRank(g, rank, axis, dim, displacement, periodic);
  });
}

cudecompResult_t cudecompExtWorkspaceSizes(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis,
                                           const int32_t halo[], int64_t* transpose_ws, int64_t* halo_ws) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (axis < 0 || axis > 2) CD_INVALID_USAGE("axis argument out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    if (transpose_ws) *transpose_ws = transposeWorkspaceElements(g);
    if (halo_ws) {
      if (!halo) CD_INVALID_USAGE("halo_extents argument cannot be null");
      *halo_ws = haloWorkspaceElements(g, gridIndexOfRank(g, rank), axis, halo);
    }
  });
}

cudecompResult_t cudecompExtGetCounters(cudecompHandle_t handle, cudecompGridDesc_t gd, cudecompExtCounters_t* out) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!gd || !gd->initialized || gd->handle != handle) CD_INVALID_USAGE("invalid grid descriptor");
    if (!out) CD_INVALID_USAGE("null argument");
    out->graphs_captured = (int64_t)(gd->pack_graphs.size() + gd->op_graphs.size());
    out->graph_launches = gd->graph_launches;
    out->local = gd->path_count[PATH_LOCAL];
    out->rccl = gd->path_count[PATH_RCCL];
    out->mpi = gd->path_count[PATH_MPI];
    out->peer_barrier = gd->path_count[PATH_PEER_BARRIER];
    out->peer_fused = gd->path_count[PATH_PEER_FUSED];
    out->peer_pipelined = gd->path_count[PATH_PEER_PIPELINED];
    out->direct_puts = gd->direct_puts;
    peerPoolCounters(handle, &out->workspace_pool_hits, &out->stale_ipc_mappings, &out->workspace_pool_bytes, &out->retired_imports);
    // (the LAST census -- taken when the transport came up or by cudecompExtQueueCensus -- not a fresh one: reading the
    // driver's tables per call slows ranks that share a device)
    out->compute_queues_on_device = handle->census_compute_queues;
    out->hardware_queue_slots = handle->census_queue_slots;
    out->relayed = gd->relayed;
    out->rotations = gd->rotations;
  });
}

cudecompResult_t cudecompExtQueueCensus(cudecompHandle_t handle, int32_t* compute_queues, int32_t* slots) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    int s = 0;
    const int c = peerQueueCensus(handle, false, &s);
    if (compute_queues) *compute_queues = c;
    if (slots) *slots = s;
  });
}

cudecompResult_t cudecompExtTrimWorkspacePool(cudecompHandle_t handle) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    workspaceTrimPool(handle);
  });
}

const char* cudecompExtLastKernelName(void) { return lastKernelName(); }

cudecompResult_t cudecompExtEstimateCycleMs(cudecompHandle_t handle, const cudecompExtGridSpec_t* grid, int32_t es,
                                            int32_t backend, int32_t library_buffers, int32_t inplace, double* ms) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!grid || !ms) CD_INVALID_USAGE("null argument");
    if (es != 4 && es != 8 && es != 16) CD_INVALID_USAGE("element size must be 4, 8 or 16");
    if (backend < 1 || backend > 8) CD_INVALID_USAGE("backend out of range");
    const GridShape g = shapeFromSpec(grid);
    const bool ip[4] = {inplace != 0, inplace != 0, inplace != 0, inplace != 0};
    *ms = estimateTransposeCycleMs(handle, g, es, (cudecompTransposeCommBackend_t)backend, library_buffers != 0, ip);
  });
}

cudecompResult_t cudecompExtGetLinkInfo(cudecompHandle_t handle, cudecompExtLinkInfo_t* out) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!out) CD_INVALID_USAGE("null argument");
    out->gbps_sdma = handle->link_gbps_sdma;
    out->gbps_cu = handle->link_gbps_cu;
    out->measured = (handle->link_gbps_sdma > 0 || handle->link_gbps_cu > 0) ? 1 : 0;
    out->crosses_devices = handle->link_crosses_devices ? 1 : 0;
    out->copy_engine = handle->peer_copy_engine;
    out->reserved = 0;
  });
}

cudecompResult_t cudecompExtPeerProbe(cudecompHandle_t handle, void* buffer, size_t bytes, int32_t* mismatches) {
  return guarded([&] {
    if (!handle || !handle->initialized) CD_INVALID_USAGE("invalid handle");
    if (!buffer || !mismatches) CD_INVALID_USAGE("null argument");
    *mismatches = peerProbe(handle, buffer, bytes);
  });
}

cudecompResult_t cudecompExtRunLocalPhases(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t op, int32_t pipelined,
                                           int32_t symmetric_recv, int32_t phases, void* input, void* output, void* work,
                                           int32_t es, hipStream_t stream) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (op < 0 || op > 3) CD_INVALID_USAGE("op out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    if (es != 4 && es != 8 && es != 16) CD_INVALID_USAGE("element size must be 4, 8 or 16");
    if (!input || !output || !work) CD_INVALID_USAGE("null buffer");
    TransportTraits traits;
    traits.pipelined = pipelined != 0;
    traits.symmetric_recv = symmetric_recv != 0;
    const CommAxis ca = (op == OP_X_TO_Y || op == OP_Y_TO_X) ? COMM_COL : COMM_ROW;
    const int P = g.pdims[ca == COMM_COL ? 0 : 1];
    const int32_t zero[3] = {0, 0, 0};
    const TransposePlan p = buildTransposePlan(g, rank, (TransposeOp)op, zero, zero, zero, zero, input == output, traits, P);
    void* bufs[3] = {input, output, work};
    // the launches of the executor: one batched launch per phase; pipelined: one launch per STAGE with all peers in it
    // for the one-sided transport (peer_exchange.cc: peerStagedExchange), one launch per PEER for RCCL / MPI (the reference's
    // pipeline, transpose.h:470-513, 683-744)
    int stages = 4;
    if (const char* v = std::getenv("CUDECOMP_PIPELINE_STAGES")) stages = (int)std::strtol(v, nullptr, 10);
    i64 min_stage = (i64)8 << 20;
    if (const char* v = std::getenv("CUDECOMP_PIPELINE_MIN_STAGE_MIB")) min_stage = std::strtoll(v, nullptr, 10) << 20;
    const int K = stageCount(p, stages, es, min_stage);
    auto run = [&](const std::vector<Move3D>& moves) {
      if (moves.empty()) return;
      if (traits.pipelined && traits.symmetric_recv && p.exchange) {
        std::vector<Move3D> part;
        for (int k = 0; k < K; ++k) {
          part.clear();
          for (const Move3D& m : moves) part.push_back(stageOfMove(m, p.stage_axis, k, K));
          launchMoves(part.data(), (int)part.size(), bufs, es, stream);
        }
      } else if (traits.pipelined) {
        for (const Move3D& m : moves) launchMoves(&m, 1, bufs, es, stream);
      } else {
        launchMoves(moves.data(), (int)moves.size(), bufs, es, stream);
      }
    };
    if (phases & 1) run(p.pack);
    if (phases & 2) run(p.unpack);
  });
}

cudecompResult_t cudecompExtRotateWalk(int32_t nb, int32_t walk, int64_t first, int64_t count, int32_t* blocks, int64_t* grid) {
  return guarded([&] {
    if (nb < 1 || nb > 1024 || !grid || first < 0 || count < 0 || (count > 0 && !blocks)) CD_INVALID_USAGE("bad argument");
    const int w = rotateWalkFor(walk, nb);
    *grid = rotateWalkGrid(nb, w);
    if (first + count > *grid) CD_INVALID_USAGE("workgroups beyond the grid");
    for (int64_t i = 0; i < count; ++i) {
      int b0 = -1, b1 = -1, b2 = -1;
      if (!rotateWalkBlock((unsigned int)(first + i), (unsigned int)nb, w, &b0, &b1, &b2)) b0 = b1 = b2 = -1;
      blocks[3 * i] = b0, blocks[3 * i + 1] = b1, blocks[3 * i + 2] = b2;
    }
  });
}

cudecompResult_t cudecompExtDescribeMove(uint64_t src_address, uint64_t dst_address, int32_t es, const int64_t extent[3],
                                        const int64_t ss[3], const int64_t ds[3], int32_t flags, int64_t out[10]) {
  return guarded([&] {
    if (!extent || !ss || !ds || !out) CD_INVALID_USAGE("null argument");
    if (es != 2 && es != 4 && es != 8 && es != 16) CD_INVALID_USAGE("element size must be 2, 4, 8 or 16");
    Move3D m;
    for (int i = 0; i < 3; ++i) {
      m.extent[i] = extent[i];
      m.ss[i] = ss[i];
      m.ds[i] = ds[i];
    }
    if (flags & 256) m.dst_row_pitch = wholeRowsPitchOf(m);
    if (flags >> 12) m.dst_row_pitch = flags >> 12;  // the planner's own word (cudecompExtMove_t::row_pitch)
    KernelTuning t;
    if (flags & 2) t.force_streaming = true;
    if (flags & 4) t.window_mode = 1;
    if (flags & 8) t.dense_rows = 0;  // as CUDECOMP_PRESERVE_OUTPUT_HALOS=1
    if (flags & 64) t.walk_order = 0;
    if (flags & 128) t.walk_order = 1;
    long long o[10];
    describeMove(m, reinterpret_cast<const void*>(src_address), reinterpret_cast<void*>(dst_address), es, &t, o);
    for (int i = 0; i < 10; ++i) out[i] = o[i];
  });
}

cudecompResult_t cudecompExtMove3D(const void* src, void* dst, int32_t es, const int64_t extent[3],
                                   const int64_t ss[3], const int64_t ds[3], int32_t force_generic,
                                   int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!src || !dst || !extent || !ss || !ds) CD_INVALID_USAGE("null argument");
    if (es != 2 && es != 4 && es != 8 && es != 16) CD_INVALID_USAGE("element size must be 2, 4, 8 or 16");
    Move3D m = move3DOf(extent, ss, ds);
    if (force_generic & 256) m.dst_row_pitch = wholeRowsPitchOf(m);  // the cells between consecutive destination rows are the move's to rewrite
    // bits 1, 2, and its own way with 4 / 8 (the window kernel always / never) and 64 / 128 (transposes: i first / j first)
    launchMove3D(m, src, dst, es, tuningOfFlags(force_generic), kernel_class, stream);
  });
}

cudecompResult_t cudecompExtAccumulate3D(const void* src, void* dst, cudecompDataType_t dtype, const int64_t extent[3],
                                         const int64_t ss[3], const int64_t ds[3], int32_t force_generic,
                                         int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!src || !dst || !extent || !ss || !ds) CD_INVALID_USAGE("null argument");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    Move3D m = move3DOf(extent, ss, ds);
    m.add = true;
    launchMove3D(m, src, dst, es, tuningOfForce(force_generic & 3), kernel_class, stream, arithOf(dtype));  // (bit 2 is not read)
  });
}

cudecompResult_t cudecompExtFill3D(void* dst, int32_t es, const void* value, const int64_t extent[3], const int64_t ds[3],
                                   int32_t force, int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!dst || !extent || !ds) CD_INVALID_USAGE("null argument");
    if (es != 2 && es != 4 && es != 8 && es != 16) CD_INVALID_USAGE("element size must be 2, 4, 8 or 16");
    Move3D m = move3DOf(extent, nullptr, ds);
    m.fill = true;
    launchMove3D(m, nullptr, dst, es, tuningOfForce(force), kernel_class, stream, ARITH_NONE, value);
  });
}

cudecompResult_t cudecompExtReflect3D(const void* src, void* dst, cudecompDataType_t dtype, int32_t negate, const int64_t extent[3],
                                      const int64_t ss[3], const int64_t ds[3], int32_t force, int32_t* kernel_class,
                                      hipStream_t stream) {
  return guarded([&] {
    if (!src || !dst || !extent || !ss || !ds) CD_INVALID_USAGE("null argument");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    Move3D m = move3DOf(extent, ss, ds);
    m.reflect = true;
    m.negate = negate != 0;
    launchMove3D(m, src, dst, es, tuningOfForce(force), kernel_class, stream, m.negate ? arithOf(dtype) : ARITH_NONE);
  });
}

cudecompResult_t cudecompExtFold3D(const void* src, void* dst, cudecompDataType_t dtype, int32_t negate, int32_t take,
                                   const int64_t extent[3], const int64_t ss[3], const int64_t ds[3], int32_t force,
                                   int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!src || !dst || !extent || !ss || !ds) CD_INVALID_USAGE("null argument");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    Move3D m = move3DOf(extent, ss, ds);
    m.reflect = true;
    m.add = true;
    m.negate = negate != 0;
    m.take = take != 0;
    launchMove3D(m, src, dst, es, tuningOfForce(force), kernel_class, stream, arithOf(dtype));
  });
}

cudecompResult_t cudecompExtWall3D(const void* src, void* dst, cudecompDataType_t dtype, int32_t negate, int32_t side,
                                   const void* addends, const int64_t extent[3], const int64_t ss[3], const int64_t ds[3],
                                   int32_t force, int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!src || !dst || !addends || !extent || !ss || !ds) CD_INVALID_USAGE("null argument");
    if (side != 0 && side != 1) CD_INVALID_USAGE("side must be 0 (low) or 1 (high)");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    Move3D m = move3DOf(extent, ss, ds);
    m.reflect = true;
    m.negate = negate != 0;
    m.affine = side + 1;
    int layers = -1;
    for (int i = 0; i < 3; ++i)
      if (ss[i] < 0) layers = layers < 0 ? (int)std::min<int64_t>(extent[i], CUDECOMP_AMD_MAX_WALL_HALO + 1) : CUDECOMP_AMD_MAX_WALL_HALO + 1;
    if (layers < 0) CD_INVALID_USAGE("a wall-value move names its mirrored dim with a negative source stride");
    if (layers > CUDECOMP_AMD_MAX_WALL_HALO) CD_INVALID_USAGE("one mirrored dim of at most CUDECOMP_AMD_MAX_WALL_HALO layers");
    WallAddends a;
    std::memset(&a, 0, sizeof(a));
    for (int k = 0; k < layers; ++k) std::memcpy(a.v[side][k], static_cast<const char*>(addends) + (size_t)k * es, es);
    launchMove3D(m, src, dst, es, tuningOfForce(force), kernel_class, stream, arithOf(dtype), nullptr, &a);
  });
}

cudecompResult_t cudecompExtWallPlane3D(const void* src, void* dst, const void* plane, cudecompDataType_t dtype, int32_t negate,
                                        const int64_t extent[3], const int64_t ss[3], const int64_t ds[3], const int64_t ps[3],
                                        int32_t force, int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!src || !dst || !plane || !extent || !ss || !ds || !ps) CD_INVALID_USAGE("null argument");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    Move3D m = move3DOf(extent, ss, ds);
    m.reflect = true;
    m.negate = negate != 0;
    m.plane = 1;
    bool mirrored = false;
    for (int i = 0; i < 3; ++i) {
      m.ps[i] = ps[i];
      mirrored = mirrored || ss[i] < 0;
    }
    if (!mirrored) CD_INVALID_USAGE("a wall-plane move names its mirrored dim with a negative source stride");
    const WallPlanes planes{{plane, nullptr}};
    void* bufs[3] = {const_cast<void*>(src), dst, nullptr};
    KernelStats st;
    const KernelTuning t = tuningOfForce(force);
    launchMoves(&m, 1, bufs, es, stream, &t, &st, nullptr, arithOf(dtype), nullptr, nullptr, &planes);
    if (kernel_class) {
      *kernel_class = -1;
      for (int c = 0; c < MOVE_CLASS_COUNT; ++c)
        if (st.launches[c]) *kernel_class = c;
    }
  });
}

// one box of one field through the reduction kernels (kernels.h launchReduce) / how it would run (planReduce)
static ReduceRequest reduceRequestOf(const void* const* a, const void* const* b, cudecompDataType_t dtype, int32_t op,
                                     const int64_t extent[3], const int64_t strides[3], int64_t readable_before,
                                     int64_t readable_after, const KernelTuning* tuning) {
  if (!extent || !strides) CD_INVALID_USAGE("null argument");
  if (op < 0 || op > 2) CD_INVALID_USAGE("op must be 0 (sum), 1 (dot) or 2 (max-abs)");
  if (readable_before < 0 || readable_after < 0) CD_INVALID_USAGE("readable_before and readable_after cannot be negative");
  ReduceRequest r;
  r.a = a;
  r.b = b;
  r.n_fields = 1;
  r.op = op;
  r.es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
  r.arith = arithOf(dtype);
  for (int i = 0; i < 3; ++i) {
    if (extent[i] < 0 || strides[i] < 0) CD_INVALID_USAGE("extents and strides of a reduction cannot be negative");
    r.extent[i] = extent[i];
    r.strides[i] = strides[i];
  }
  r.readable_before = readable_before;
  r.readable_after = readable_after;
  r.tuning = tuning;
  return r;
}

cudecompResult_t cudecompExtReduce3D(const void* a, const void* b, cudecompDataType_t dtype, int32_t op, const int64_t extent[3],
                                     const int64_t strides[3], int64_t readable_before, int64_t readable_after, void* work,
                                     double* results, int32_t force, int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!a || !work || !results || (op == 1 && !b)) CD_INVALID_USAGE("null argument");
    const KernelTuning t = tuningOfForce(force);
    const ReduceRequest r = reduceRequestOf(&a, &b, dtype, op, extent, strides, readable_before, readable_after, &t);
    KernelStats st;
    launchReduce(r, results, work, stream, &st);
    if (kernel_class) {
      *kernel_class = -1;
      for (int c = 0; c < MOVE_CLASS_COUNT; ++c)
        if (st.launches[c]) *kernel_class = c;
    }
  });
}

cudecompResult_t cudecompExtDescribeReduce3D(uint64_t a_address, uint64_t b_address, cudecompDataType_t dtype, int32_t op,
                                             const int64_t extent[3], const int64_t strides[3], int64_t readable_before,
                                             int64_t readable_after, int32_t force, int64_t out[5]) {
  return guarded([&] {
    if (!out) CD_INVALID_USAGE("null argument");
    const void* const a = reinterpret_cast<const void*>(a_address);
    const void* const b = reinterpret_cast<const void*>(b_address);
    const KernelTuning t = tuningOfForce(force);
    const ReducePlan p = planReduce(reduceRequestOf(&a, &b, dtype, op, extent, strides, readable_before, readable_after, &t));
    out[0] = p.k.kind;
    out[1] = p.k.vec;
    out[2] = p.g.blocks;
    out[3] = p.read_lo;
    out[4] = p.read_hi;
  });
}

// one box of one field through the profile kernels (kernels.h launchProfile) / how it would run (planProfile)
static ProfileRequest profileRequestOf(const void* const* a, const void* const* b, cudecompDataType_t dtype, int32_t op, int32_t keep,
                                       const int64_t extent[3], const int64_t strides[3], int64_t readable_before,
                                       int64_t readable_after, const KernelTuning* tuning) {
  if (!extent || !strides) CD_INVALID_USAGE("null argument");
  if (op < 0 || op > 2) CD_INVALID_USAGE("op must be 0 (sum), 1 (dot) or 2 (max-abs)");
  if (keep < 0 || keep > 2) CD_INVALID_USAGE("keep must be 0, 1 or 2");
  if (readable_before < 0 || readable_after < 0) CD_INVALID_USAGE("readable_before and readable_after cannot be negative");
  ProfileRequest r;
  r.a = a;
  r.b = b;
  r.n_fields = 1;
  r.op = op;
  r.keep = keep;
  r.es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
  r.arith = arithOf(dtype);
  for (int i = 0; i < 3; ++i) {
    if (extent[i] < 0 || strides[i] < 0) CD_INVALID_USAGE("extents and strides of a profile cannot be negative");
    r.extent[i] = extent[i];
    r.strides[i] = strides[i];
  }
  r.readable_before = readable_before;
  r.readable_after = readable_after;
  r.tuning = tuning;
  return r;
}

cudecompResult_t cudecompExtProfile3D(const void* a, const void* b, cudecompDataType_t dtype, int32_t op, int32_t keep,
                                      const int64_t extent[3], const int64_t strides[3], int64_t readable_before,
                                      int64_t readable_after, void* work, double* results, int64_t ld, int32_t force,
                                      int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!a || !work || !results || (op == 1 && !b)) CD_INVALID_USAGE("null argument");
    const KernelTuning t = tuningOfForce(force);
    const ProfileRequest r = profileRequestOf(&a, &b, dtype, op, keep, extent, strides, readable_before, readable_after, &t);
    if (ld < r.extent[keep]) CD_INVALID_USAGE("ld is smaller than the kept extent");
    KernelStats st;
    launchProfile(r, results, ld, work, stream, &st);
    if (kernel_class) {
      *kernel_class = -1;
      for (int c = 0; c < MOVE_CLASS_COUNT; ++c)
        if (st.launches[c]) *kernel_class = c;
    }
  });
}

cudecompResult_t cudecompExtDescribeProfile3D(uint64_t a_address, uint64_t b_address, cudecompDataType_t dtype, int32_t op,
                                              int32_t keep, const int64_t extent[3], const int64_t strides[3],
                                              int64_t readable_before, int64_t readable_after, int32_t force, int64_t out[8]) {
  return guarded([&] {
    if (!out) CD_INVALID_USAGE("null argument");
    const void* const a = reinterpret_cast<const void*>(a_address);
    const void* const b = reinterpret_cast<const void*>(b_address);
    const KernelTuning t = tuningOfForce(force);
    const ProfilePlan p = planProfile(profileRequestOf(&a, &b, dtype, op, keep, extent, strides, readable_before, readable_after, &t));
    out[0] = p.k.kind;
    out[1] = p.k.vec;
    out[2] = p.blocks;
    out[3] = p.read_lo;
    out[4] = p.read_hi;
    out[5] = p.g.parts;
    out[6] = p.g.L;
    out[7] = p.g.parts ? 1LL << p.g.final_lanes_log2 : 0;
  });
}

// one box of one field through the plane-update kernels (kernels.h launchPlanes) / how it would run (planPlanes)
static PlanesRequest planesRequestOf(void* const* a, cudecompDataType_t dtype, int32_t op, int32_t keep, const int64_t extent[3],
                                     const int64_t strides[3], int64_t readable_before, int64_t readable_after, double scale,
                                     const KernelTuning* tuning) {
  if (!extent || !strides) CD_INVALID_USAGE("null argument");
  if (op < 0 || op > 1) CD_INVALID_USAGE("op must be 0 (add) or 1 (multiply)");
  if (keep < 0 || keep > 2) CD_INVALID_USAGE("keep must be 0, 1 or 2");
  if (readable_before < 0 || readable_after < 0) CD_INVALID_USAGE("readable_before and readable_after cannot be negative");
  PlanesRequest r;
  r.a = a;
  r.n_fields = 1;
  r.op = op;
  r.keep = keep;
  r.es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
  r.arith = arithOf(dtype);
  for (int i = 0; i < 3; ++i) {
    if (extent[i] < 0 || strides[i] < 0) CD_INVALID_USAGE("extents and strides of a plane update cannot be negative");
    r.extent[i] = extent[i];
    r.strides[i] = strides[i];
  }
  r.readable_before = readable_before;
  r.readable_after = readable_after;
  r.ld = 0;
  r.scale = scale;
  r.tuning = tuning;
  return r;
}

cudecompResult_t cudecompExtPlanes3D(void* a, cudecompDataType_t dtype, int32_t op, int32_t keep, const int64_t extent[3],
                                     const int64_t strides[3], int64_t readable_before, int64_t readable_after, const double* coef,
                                     double scale, int32_t force, int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!a || !coef) CD_INVALID_USAGE("null argument");
    const KernelTuning t = tuningOfForce(force);
    const PlanesRequest r = planesRequestOf(&a, dtype, op, keep, extent, strides, readable_before, readable_after, scale, &t);
    KernelStats st;
    launchPlanes(r, coef, stream, &st);
    if (kernel_class) {
      *kernel_class = -1;
      for (int c = 0; c < MOVE_CLASS_COUNT; ++c)
        if (st.launches[c]) *kernel_class = c;
    }
  });
}

cudecompResult_t cudecompExtDescribePlanes3D(uint64_t a_address, cudecompDataType_t dtype, int32_t op, int32_t keep,
                                             const int64_t extent[3], const int64_t strides[3], int64_t readable_before,
                                             int64_t readable_after, int32_t force, int64_t out[7]) {
  return guarded([&] {
    if (!out) CD_INVALID_USAGE("null argument");
    void* const a = reinterpret_cast<void*>(a_address);
    const KernelTuning t = tuningOfForce(force);
    const PlanesPlan p = planPlanes(planesRequestOf(&a, dtype, op, keep, extent, strides, readable_before, readable_after, 1.0, &t));
    out[0] = p.k.kind;
    out[1] = p.k.vec;
    out[2] = p.blocks;
    out[3] = p.read_lo;
    out[4] = p.read_hi;
    out[5] = p.write_lo;
    out[6] = p.write_hi;
  });
}

// one box of one field through the combination kernels (kernels.h launchCombine) / how it would run (planCombine)
static CombineRequest combineRequestOf(void* const* y, const void* const* x, cudecompDataType_t dtype, int32_t op, const int64_t extent[3],
                                       const int64_t strides[3], int64_t readable_before, int64_t readable_after, double a_scale,
                                       double b_scale, const KernelTuning* tuning) {
  if (!extent || !strides) CD_INVALID_USAGE("null argument");
  if (op < 0 || op > 3) CD_INVALID_USAGE("op must be 0 (axpy), 1 (xpby), 2 (axpby) or 3 (ax)");
  if (readable_before < 0 || readable_after < 0) CD_INVALID_USAGE("readable_before and readable_after cannot be negative");
  CombineRequest r;
  r.y = y;
  r.x = x;
  r.n_fields = 1;
  r.op = op;
  r.es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
  r.arith = arithOf(dtype);
  for (int i = 0; i < 3; ++i) {
    if (extent[i] < 0 || strides[i] < 0) CD_INVALID_USAGE("extents and strides of a combination cannot be negative");
    r.extent[i] = extent[i];
    r.strides[i] = strides[i];
  }
  r.readable_before = readable_before;
  r.readable_after = readable_after;
  r.a_scale = a_scale, r.b_scale = b_scale;
  r.coef_stride = 0;
  r.tuning = tuning;
  return r;
}

cudecompResult_t cudecompExtCombine3D(void* y, const void* x, cudecompDataType_t dtype, int32_t op, const int64_t extent[3],
                                      const int64_t strides[3], int64_t readable_before, int64_t readable_after, const double* a_num,
                                      const double* a_den, double a_scale, const double* b_num, const double* b_den, double b_scale,
                                      int32_t force, int32_t* kernel_class, hipStream_t stream) {
  return guarded([&] {
    if (!y || !x) CD_INVALID_USAGE("null argument");
    if (x == y) CD_INVALID_USAGE("x and y cannot be the same field");
    const KernelTuning t = tuningOfForce(force);
    const CombineRequest r = combineRequestOf(&y, &x, dtype, op, extent, strides, readable_before, readable_after, a_scale, b_scale, &t);
    KernelStats st;
    launchCombine(r, a_num, a_den, b_num, b_den, stream, &st);
    if (kernel_class) {
      *kernel_class = -1;
      for (int c = 0; c < MOVE_CLASS_COUNT; ++c)
        if (st.launches[c]) *kernel_class = c;
    }
  });
}

cudecompResult_t cudecompExtDescribeCombine3D(uint64_t y_address, uint64_t x_address, cudecompDataType_t dtype, int32_t op,
                                              const int64_t extent[3], const int64_t strides[3], int64_t readable_before,
                                              int64_t readable_after, int32_t force, int64_t out[12]) {
  return guarded([&] {
    if (!out) CD_INVALID_USAGE("null argument");
    void* const y = reinterpret_cast<void*>(y_address);
    const void* const x = reinterpret_cast<const void*>(x_address);
    const KernelTuning t = tuningOfForce(force);
    const CombinePlan p = planCombine(combineRequestOf(&y, &x, dtype, op, extent, strides, readable_before, readable_after, 1.0, 1.0, &t));
    out[0] = p.k.kind;
    out[1] = p.k.vec;
    out[2] = p.blocks;
    out[3] = p.read_x_lo;
    out[4] = p.read_x_hi;
    out[5] = p.read_y_lo;
    out[6] = p.read_y_hi;
    out[7] = p.write_lo;
    out[8] = p.write_hi;
    out[9] = p.g.blocks ? (p.k.kind == K_ROWS_COMBINE ? p.g.row_bytes : 0) : 0;
    out[10] = p.g.blocks ? (p.k.kind == K_ROWS_COMBINE ? p.g.rows * p.g.planes : 0) : 0;
    out[11] = p.g.blocks ? (p.k.kind == K_ROWS_COMBINE ? p.g.last_row_bytes : 0) : 0;
  });
}

cudecompResult_t cudecompExtPlanHaloWallPlanes(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                               const bool periods[], int32_t dim, const int32_t pad[], cudecompDataType_t dtype,
                                               int32_t parity, int32_t centering, int32_t sides, uint64_t pencil_address,
                                               uint64_t plane_low_address, uint64_t plane_high_address, cudecompExtHaloPlan_t* out,
                                               cudecompExtPlaneOperand_t operands[2]) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!out || !halo || !operands) CD_INVALID_USAGE("null argument");
    if (axis < 0 || axis > 2 || dim < 0 || dim > 2) CD_INVALID_USAGE("axis/dim out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    const int32_t zero[3] = {0, 0, 0};
    const bool none[3] = {false, false, false};
    const bool* per = periods ? periods : none;
    const int32_t* pp = pad ? pad : zero;
    // the call's checks in the call's order: what the fill refuses, parity, centering, sides, NULL planes, overlap, then the plan's
    buildHaloPlan(g, rank, axis, dim, halo, per, pp, false, false);
    if (parity != 1 && parity != -1) CD_INVALID_USAGE("parity argument must be +1 or -1");
    if (centering != 0 && centering != 1) CD_INVALID_USAGE("centering argument must be 0 or 1");
    const void* low = reinterpret_cast<const void*>(plane_low_address);
    const void* high = reinterpret_cast<const void*>(plane_high_address);
    i64 pencil_bytes = 0, plane_bytes = 0;
    if (halo[dim] > 0 && !per[dim]) {
      const Pencil pencil = makePencil(g, gridIndexOfRank(g, rank), axis, halo, pp);
      const i64 along = pencil.extentG(dim);
      pencil_bytes = pencil.size * es;
      plane_bytes = along > 0 ? pencil.size / along * halo[dim] * es : 0;
    }
    const int refusal = wallPlaneRefusal(sides, low, high, reinterpret_cast<const void*>(pencil_address), pencil_bytes, plane_bytes);
    if (refusal != 0) refuseWallPlanes(refusal);
    HaloOp op = haloOp(HaloOp::WALL_PLANES, false, centering, parity == -1);
    op.sides = sides;
    const HaloPlan p = buildHaloOpPlan(g, rank, axis, dim, halo, per, pp, op, false, false);
    exportHaloPlan(p, out);
    std::memset(operands, 0, 2 * sizeof(operands[0]));
    for (size_t i = 0; i < p.pre.size() && i < 2; ++i) {
      operands[i].plane = p.pre[i].plane;
      operands[i].off = p.pre[i].plane_off;
      for (int d = 0; d < 3; ++d) operands[i].ps[d] = p.pre[i].ps[d];
    }
  });
}

cudecompResult_t cudecompExtPlanHaloWallValues(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                               const bool periods[], int32_t dim, const int32_t pad[], cudecompDataType_t dtype,
                                               int32_t parity, int32_t centering, int32_t sides, const double values_low[],
                                               const double values_high[], cudecompExtHaloPlan_t* out, uint8_t* table) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!out || !halo || !table) CD_INVALID_USAGE("null argument");
    if (axis < 0 || axis > 2 || dim < 0 || dim > 2) CD_INVALID_USAGE("axis/dim out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    const int32_t zero[3] = {0, 0, 0};
    const bool none[3] = {false, false, false};
    const bool* per = periods ? periods : none;
    const int32_t* pp = pad ? pad : zero;
    // the call's checks in the call's order: what the fill refuses, parity, centering, sides, value arrays, width, then the plan's
    buildHaloPlan(g, rank, axis, dim, halo, per, pp, false, false);
    if (parity != 1 && parity != -1) CD_INVALID_USAGE("parity argument must be +1 or -1");
    if (centering != 0 && centering != 1) CD_INVALID_USAGE("centering argument must be 0 or 1");
    const int refusal = wallValueRefusal(sides, values_low != nullptr, values_high != nullptr, halo[dim]);
    if (refusal != 0) refuseWallValues(refusal);
    HaloOp op = haloOp(HaloOp::WALL_VALUES, false, centering, parity == -1);
    op.sides = sides;
    const HaloPlan p = buildHaloOpPlan(g, rank, axis, dim, halo, per, pp, op, false, false);
    exportHaloPlan(p, out);
    const WallAddends a = wallAddendsOf(dtype, halo[dim], sides, values_low, values_high);
    for (int side = 0; side < 2; ++side)
      wallTableRow(a, side, (sides & (1 << side)) ? halo[dim] : 0, es, table + side * CUDECOMP_AMD_MAX_WALL_HALO * 16);
  });
}

// the moves of a field launch (at most 2, CUDECOMP_AMD_MAX_HALO_FIELDS fields) or of a field-move list (at most
// CUDECOMP_EXT_MAX_MEMBERS, CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS fields)
static std::vector<Move3D> importFieldMoves(const cudecompExtMove_t* moves, int32_t n, int32_t max_moves, int32_t n_fields,
                                            int32_t max_fields, int32_t es) {
  if (n < 0 || n > max_moves || (n > 0 && !moves)) CD_INVALID_USAGE("number of moves out of range");
  if (n_fields < 1 || n_fields > max_fields) CD_INVALID_USAGE("n_fields out of range");
  if (es != 2 && es != 4 && es != 8 && es != 16) CD_INVALID_USAGE("element size must be 2, 4, 8 or 16");
  std::vector<Move3D> list(n);
  for (int32_t i = 0; i < n; ++i) {
    const cudecompExtMove_t& e = moves[i];
    if (e.src_buf < 0 || e.src_buf > 2 || e.dst_buf < 0 || e.dst_buf > 2) CD_INVALID_USAGE("buffer number out of range");
    Move3D& m = list[i];
    m.src_buf = (BufId)e.src_buf;
    m.dst_buf = (BufId)e.dst_buf;
    m.src_off = e.src_off;
    m.dst_off = e.dst_off;
    for (int d = 0; d < 3; ++d) {
      m.extent[d] = e.extent[d];
      m.ss[d] = e.ss[d];
      m.ds[d] = e.ds[d];
    }
    m.dst_row_pitch = e.row_pitch;
  }
  return list;
}

cudecompResult_t cudecompExtPlanHaloFields(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                           const bool periods[], int32_t dim, const int32_t pad[], int32_t n_fields,
                                           int32_t force_packed, cudecompExtHaloFieldsPlan_t* out) {
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::UPDATE, false, 0, false, n_fields), force_packed != 0, out);
}

cudecompResult_t cudecompExtPlanHaloAccumulateFields(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                                     const bool periods[], int32_t dim, const int32_t pad[], int32_t n_fields,
                                                     int32_t clear, int32_t self_exchange, cudecompExtHaloFieldsPlan_t* out) {
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, haloOp(HaloOp::ACCUMULATE, clear != 0, 0, false, n_fields), true, out, clear,
                    true, self_exchange != 0);
}

// What a Run / Describe pair of the field-move entries shares: the imported list, what it points to and the request over them.  The
// request points into this record, which is therefore never copied.
struct ImportedFieldMoves {
  std::vector<Move3D> moves;
  std::vector<i64> steps;
  std::vector<void*> inputs, outputs;  // Describe: the fields given as addresses
  std::vector<WallAddends> addends;
  KernelTuning tuning;
  FieldMoveList list;
  ImportedFieldMoves() = default;
  ImportedFieldMoves(const ImportedFieldMoves&) = delete;
};

// the request over q.moves in the one-choice mode of the halo phases: the fields as device pointers (Run) or as addresses (Describe),
// inputs and outputs alike; of `force` the bits 1, 2 and 4
static void requestOver(ImportedFieldMoves& q, void* const* fields, const uint64_t* addresses, int32_t n_fields, int32_t es, int32_t force) {
  if (!fields) {
    q.inputs = pointersOf(addresses, n_fields);
    fields = q.inputs.data();
  }
  q.tuning = tuningOfForce(force);
  q.list.moves = q.moves.data();
  q.list.n = (int)q.moves.size();
  q.list.inputs = q.list.outputs = fields;
  q.list.n_fields = n_fields;
  q.list.es = es;
  q.list.one_choice = true;
  q.list.tuning = &q.tuning;
}

static void runFieldMoveList(const FieldMoveList& list, hipStream_t stream, int32_t* n_launches) {
  KernelStats st;
  launchFieldMoveList(list, stream, &st);
  if (n_launches) *n_launches = launchesOf(st);
}

// out[5] of the Describe entries whose lists make one launch at most (one choice, at most two moves)
static void exportFirstLaunch(const std::vector<FieldMoveLaunch>& ls, int64_t out[5]) {
  const FieldMoveLaunch none{};  // (every move is empty: nothing is launched)
  const FieldMoveLaunch& l = ls.empty() ? none : ls[0];
  out[0] = ls.empty() ? -1 : (int64_t)l.k.kind;
  out[1] = l.k.vec;
  out[2] = l.k.access;
  out[3] = l.blocks_per_field;
  out[4] = l.blocks;
}

// the operation of cudecompExtRunFieldMovesOp / cudecompExtDescribeFieldMovesOp onto an imported list; *arith as importMoves sets it
static void applyFieldMoveMode(std::vector<Move3D>& list, int32_t mode, cudecompDataType_t dtype, int32_t es, ArithType* arith) {
  if (mode != 0 && mode != 1 && mode != 3 && mode != 4) CD_INVALID_USAGE("mode must be 0 (copy), 1 (add), 3 (take) or 4 (add and take)");
  *arith = ARITH_NONE;
  if (mode == 1 || mode == 4) {
    if (elementSize(dtype) != es) CD_INVALID_USAGE("element size does not match the data type of the arithmetic");
    *arith = arithOf(dtype);
  }
  for (Move3D& m : list) {
    m.add = mode == 1 || mode == 4;
    m.take = mode == 3 || mode == 4;
  }
}

// cudecompExt{Run,Describe}FieldMoves (mode 0: plain copies) and cudecompExt{Run,Describe}FieldMovesOp
static void importFieldMovesOp(ImportedFieldMoves& q, const cudecompExtMove_t* moves, int32_t n, void* const* fields, const uint64_t* addresses,
                               int32_t n_fields, int32_t max_fields, void* work, int64_t work_field_stride, int32_t es, int32_t force,
                               int32_t mode, cudecompDataType_t dtype) {
  q.moves = importFieldMoves(moves, n, 2, n_fields, max_fields, es);
  applyFieldMoveMode(q.moves, mode, dtype, es, &q.list.arith);
  q.steps.assign(q.moves.size(), work_field_stride);
  requestOver(q, fields, addresses, n_fields, es, force);
  q.list.work_steps = q.steps.data();
  q.list.work = work;
}

cudecompResult_t cudecompExtRunFieldMoves(const cudecompExtMove_t* moves, int32_t n, void* const* fields, int32_t n_fields,
                                         void* work, int64_t work_field_stride, int32_t es, int32_t force, hipStream_t stream,
                                         int32_t* n_launches) {
  return guarded([&] {
    if (!fields) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importFieldMovesOp(q, moves, n, fields, nullptr, n_fields, CUDECOMP_AMD_MAX_HALO_FIELDS, work, work_field_stride, es, force, 0, (cudecompDataType_t)0);
    runFieldMoveList(q.list, stream, n_launches);
  });
}

cudecompResult_t cudecompExtDescribeFieldMoves(const cudecompExtMove_t* moves, int32_t n, const uint64_t* field_addresses,
                                              int32_t n_fields, uint64_t work_address, int64_t work_field_stride, int32_t es,
                                              int32_t force, int64_t out[5]) {
  return guarded([&] {
    if (!field_addresses || !out) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importFieldMovesOp(q, moves, n, nullptr, field_addresses, n_fields, CUDECOMP_AMD_MAX_HALO_FIELDS, reinterpret_cast<void*>(work_address),
                       work_field_stride, es, force, 0, (cudecompDataType_t)0);
    exportFirstLaunch(planFieldMoveLaunches(q.list), out);
  });
}

cudecompResult_t cudecompExtRunFieldMovesOp(const cudecompExtMove_t* moves, int32_t n, void* const* fields, int32_t n_fields,
                                           void* work, int64_t work_field_stride, int32_t es, int32_t force, int32_t mode,
                                           cudecompDataType_t dtype, hipStream_t stream, int32_t* n_launches) {
  return guarded([&] {
    if (!fields) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importFieldMovesOp(q, moves, n, fields, nullptr, n_fields, CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS, work, work_field_stride, es, force, mode, dtype);
    runFieldMoveList(q.list, stream, n_launches);
  });
}

cudecompResult_t cudecompExtDescribeFieldMovesOp(const cudecompExtMove_t* moves, int32_t n, const uint64_t* field_addresses,
                                                int32_t n_fields, uint64_t work_address, int64_t work_field_stride, int32_t es,
                                                int32_t force, int32_t mode, cudecompDataType_t dtype, int64_t out[5]) {
  return guarded([&] {
    if (!field_addresses || !out) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importFieldMovesOp(q, moves, n, nullptr, field_addresses, n_fields, CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS,
                       reinterpret_cast<void*>(work_address), work_field_stride, es, force, mode, dtype);
    exportFirstLaunch(planFieldMoveLaunches(q.list), out);
  });
}

// cudecompExt{Run,Describe}MirroredFieldMoves: every move a reflect-move, with add (and take) as the mode says
static void importMirroredFieldMoves(ImportedFieldMoves& q, const cudecompExtMove_t* moves, int32_t n, void* const* fields,
                                     const uint64_t* addresses, int32_t n_fields, int32_t es, int32_t force, int32_t mode,
                                     cudecompDataType_t dtype, uint32_t fields_neg) {
  q.moves = importFieldMoves(moves, n, 2, n_fields, CUDECOMP_AMD_MAX_HALO_WALL_FIELDS, es);
  if (mode != 0 && mode != 1 && mode != 4) CD_INVALID_USAGE("mode must be 0 (reflect), 1 (fold) or 4 (fold and take)");
  if (elementSize(dtype) != es) CD_INVALID_USAGE("element size does not match the data type");
  for (Move3D& m : q.moves) {
    m.reflect = true;
    m.add = mode != 0;
    m.take = mode == 4;
  }
  if (n_fields < 32 && (fields_neg >> n_fields) != 0) CD_INVALID_USAGE("sign bit of a field the list does not have");
  requestOver(q, fields, addresses, n_fields, es, force);
  q.list.arith = arithOf(dtype);
  q.list.mirrored = true;
  q.list.fields_neg = fields_neg;
}

cudecompResult_t cudecompExtRunMirroredFieldMoves(const cudecompExtMove_t* moves, int32_t n, void* const* fields, int32_t n_fields,
                                                 int32_t es, int32_t force, int32_t mode, cudecompDataType_t dtype,
                                                 uint32_t fields_neg, hipStream_t stream, int32_t* n_launches) {
  return guarded([&] {
    if (!fields) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importMirroredFieldMoves(q, moves, n, fields, nullptr, n_fields, es, force, mode, dtype, fields_neg);
    runFieldMoveList(q.list, stream, n_launches);
  });
}

cudecompResult_t cudecompExtDescribeMirroredFieldMoves(const cudecompExtMove_t* moves, int32_t n, const uint64_t* field_addresses,
                                                      int32_t n_fields, int32_t es, int32_t force, int32_t mode,
                                                      cudecompDataType_t dtype, uint32_t fields_neg, int64_t out[5]) {
  return guarded([&] {
    if (!field_addresses || !out) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importMirroredFieldMoves(q, moves, n, nullptr, field_addresses, n_fields, es, force, mode, dtype, fields_neg);
    exportFirstLaunch(planFieldMoveLaunches(q.list), out);
  });
}

cudecompResult_t cudecompExtPlanHaloWallValueFields(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t axis, const int32_t halo[],
                                                    const bool periods[], int32_t dim, const int32_t pad[], int32_t centering,
                                                    int32_t sides, int32_t n_fields, cudecompExtHaloPlan_t* out) {
  try {
    if (n_fields < 1 || n_fields > CUDECOMP_AMD_MAX_WALL_VALUE_FIELDS) CD_INVALID_USAGE("n_fields argument out of range");
  } catch (const Error& e) {
    return fail(e);
  }
  HaloOp op = haloOp(HaloOp::WALL_VALUES, false, centering, false, n_fields);
  op.sides = sides;
  return planHaloOp(grid, rank, axis, halo, periods, dim, pad, op, false, out);
}

// cudecompExt{Run,Describe}WallFieldMoves: the imported list as wall-moves (every move a reflect-move that names its side in `peer`),
// the raw addends ((f * 2 + side) * CUDECOMP_AMD_MAX_WALL_HALO + k elements) as the kernel layer takes them, and the wall list over
// both.  One field is the single call: *single_bufs then holds its buffers, the moves carry its sign, and launchMoves / planLaunches
// take q.moves, q.tuning and q.addends.
static void importWallFieldMoves(ImportedFieldMoves& q, const cudecompExtMove_t* moves, int32_t n, void* const* fields,
                                 const uint64_t* addresses, int32_t n_fields, int32_t es, int32_t force, cudecompDataType_t dtype,
                                 uint32_t fields_neg, const void* addends, void* single_bufs[3]) {
  if (!addends) CD_INVALID_USAGE("null argument");
  q.moves = importFieldMoves(moves, n, 2, n_fields, CUDECOMP_AMD_MAX_WALL_VALUE_FIELDS, es);
  if (n_fields < 32 && (fields_neg >> n_fields) != 0) CD_INVALID_USAGE("sign bit of a field the list does not have");
  for (int32_t i = 0; i < n; ++i) {
    Move3D& m = q.moves[i];
    if (moves[i].peer != 0 && moves[i].peer != 1) CD_INVALID_USAGE("a wall-value move names its side in `peer`: 0 low, 1 high");
    if (m.src_buf == BUF_WORK || m.dst_buf == BUF_WORK || m.dst_row_pitch != 0) CD_INVALID_USAGE("wall-value moves lie in the fields' own buffers");
    int mirrored = 0;
    for (int d = 0; d < 3; ++d) {
      if (m.extent[d] < 0) CD_INVALID_USAGE("negative extent");
      if (m.ss[d] < 0) {
        ++mirrored;
        if (m.extent[d] > CUDECOMP_AMD_MAX_WALL_HALO) CD_INVALID_USAGE("one mirrored dim of at most CUDECOMP_AMD_MAX_WALL_HALO layers");
      }
    }
    if (mirrored != 1) CD_INVALID_USAGE("a wall-value move names its one mirrored dim with a negative source stride");
    m.reflect = true;
    m.affine = moves[i].peer + 1;
    if (n_fields == 1) m.negate = (fields_neg & 1u) != 0;
  }
  q.addends.assign(n_fields, WallAddends());
  for (int32_t f = 0; f < n_fields; ++f) {
    std::memset(&q.addends[f], 0, sizeof(WallAddends));
    for (int side = 0; side < 2; ++side)
      for (int k = 0; k < CUDECOMP_AMD_MAX_WALL_HALO; ++k)
        std::memcpy(q.addends[f].v[side][k], static_cast<const char*>(addends) + ((size_t)(f * 2 + side) * CUDECOMP_AMD_MAX_WALL_HALO + k) * es, es);
  }
  requestOver(q, fields, addresses, n_fields, es, force);
  for (int32_t f = 0; fields && f < n_fields; ++f)
    if (!fields[f]) CD_INVALID_USAGE("null field buffer");
  q.list.arith = arithOf(dtype);
  q.list.mirrored = true;
  q.list.fields_neg = fields_neg;
  q.list.addends = q.addends.data();
  single_bufs[0] = single_bufs[1] = q.list.inputs[0];
  single_bufs[2] = nullptr;
}

cudecompResult_t cudecompExtRunWallFieldMoves(const cudecompExtMove_t* moves, int32_t n, void* const* fields, int32_t n_fields,
                                             int32_t force, cudecompDataType_t dtype, uint32_t fields_neg, const void* addends,
                                             hipStream_t stream, int32_t* n_launches) {
  return guarded([&] {
    if (!fields) CD_INVALID_USAGE("null argument");
    const int es = elementSize(dtype);  // (INVALID_USAGE for an unknown type)
    ImportedFieldMoves q;
    void* bufs[3];
    importWallFieldMoves(q, moves, n, fields, nullptr, n_fields, es, force, dtype, fields_neg, addends, bufs);
    if (n_fields == 1) {  // the single call's path
      KernelStats st;
      launchMoves(q.moves.data(), n, bufs, es, stream, &q.tuning, &st, nullptr, arithOf(dtype), nullptr, q.addends.data());
      if (n_launches) *n_launches = launchesOf(st);
    } else {
      runFieldMoveList(q.list, stream, n_launches);
    }
  });
}

cudecompResult_t cudecompExtDescribeWallFieldMoves(const cudecompExtMove_t* moves, int32_t n, const uint64_t* field_addresses,
                                                  int32_t n_fields, int32_t force, cudecompDataType_t dtype, uint32_t fields_neg,
                                                  const void* addends, int32_t max_launches, int64_t* out, uint8_t* tables,
                                                  int32_t* n_launches) {
  return guarded([&] {
    if (!field_addresses || !n_launches || max_launches < 0 || (max_launches > 0 && (!out || !tables))) CD_INVALID_USAGE("null argument");
    const int es = elementSize(dtype);
    ImportedFieldMoves q;
    void* bufs[3];
    importWallFieldMoves(q, moves, n, nullptr, field_addresses, n_fields, es, force, dtype, fields_neg, addends, bufs);
    int made = 0;
    auto record = [&](const KernelChoice& k, int64_t blocks, int64_t per_field, int first, int count, const unsigned char* table) {
      if (made < max_launches) {
        const int64_t v[7] = {(int64_t)k.kind, k.vec, k.access, blocks, per_field, first, count};
        std::memcpy(out + 7 * made, v, sizeof(v));
        std::memcpy(tables + (size_t)CUDECOMP_EXT_WALL_FIELD_TABLE_BYTES * made, table, CUDECOMP_EXT_WALL_FIELD_TABLE_BYTES);
      }
      ++made;
    };
    if (n_fields == 1) {  // the single call's launches; their addends in the compact layout, h the most layers of the list
      auto layersOf = [](const Move3D& m) {
        for (int d = 0; d < 3; ++d)
          if (m.ss[d] < 0) return (int)m.extent[d];
        return 0;
      };
      int layers = 0;
      for (const Move3D& m : q.moves)
        if (m.elements() != 0) layers = std::max(layers, layersOf(m));
      for (const Launch& l : planLaunches(q.moves.data(), n, bufs, es, &q.tuning, nullptr, arithOf(dtype))) {
        unsigned char table[CUDECOMP_EXT_WALL_FIELD_TABLE_BYTES] = {0};
        for (int i = 0; i < l.b.n; ++i) {
          const Move3D& m = q.moves[l.index[i]];
          const int mine = layersOf(m), side = m.affine - 1;
          for (int j = 0; j < mine; ++j) std::memcpy(table + ((size_t)i * layers + j) * es, q.addends[0].v[side][side == 0 ? mine - 1 - j : j], es);
        }
        record(l.k, l.blocks, l.blocks, 0, 1, table);
      }
    } else {
      for (const FieldWallLaunch& w : planFieldWallLaunches(q.list))
        record(w.l.k, w.l.blocks, w.l.blocks_per_field, w.first_field, w.l.b.n_fields, reinterpret_cast<const unsigned char*>(w.table.w));
    }
    *n_launches = made;
  });
}

cudecompResult_t cudecompExtPlanTransposeFields(const cudecompExtGridSpec_t* grid, int32_t rank, int32_t op, const int32_t in_halo[],
                                                const int32_t out_halo[], const int32_t in_pad[], const int32_t out_pad[],
                                                bool inplace, int32_t pipelined, int32_t symmetric_recv, int32_t npergroup,
                                                int32_t n_fields, cudecompExtTransposePlan_t* out, int64_t* pack_step,
                                                int64_t* unpack_step) {
  return guarded([&] {
    const GridShape g = shapeFromSpec(grid);
    if (!out || !pack_step || !unpack_step) CD_INVALID_USAGE("plan argument cannot be null");
    if (op < 0 || op > 3) CD_INVALID_USAGE("op out of range");
    if (rank < 0 || rank >= g.pdims[0] * g.pdims[1]) CD_INVALID_USAGE("rank out of range");
    TransportTraits traits;
    traits.pipelined = (pipelined & 1) != 0;
    traits.no_elide = (pipelined & 2) != 0;  // (n_fields == 1: the single plan with both elisions off, what n_fields >= 2 derive from)
    traits.symmetric_recv = symmetric_recv != 0;
    const CommAxis ca = (op == OP_X_TO_Y || op == OP_Y_TO_X) ? COMM_COL : COMM_ROW;
    const int P = g.pdims[ca == COMM_COL ? 0 : 1];
    const TransposeFieldsPlan fp = buildTransposeFieldsPlan(g, rank, (TransposeOp)op, in_halo, out_halo, in_pad, out_pad, inplace,
                                                            traits, npergroup > 0 ? npergroup : P, n_fields);
    std::vector<int> members(P);
    const auto pidx = gridIndexOfRank(g, rank);
    for (int i = 0; i < P; ++i) members[i] = globalRankOf(g, pidx, ca, i);
    exportTransposePlan(fp.base, members, out);
    for (int i = 0; i < CUDECOMP_EXT_MAX_MEMBERS; ++i) {
      pack_step[i] = i < (int)fp.pack_step.size() ? fp.pack_step[i] : 0;
      unpack_step[i] = i < (int)fp.unpack_step.size() ? fp.unpack_step[i] : 0;
    }
  });
}

// cudecompExt{Run,Describe}FieldMoveList: the phases of a multi-field transpose -- inputs and outputs apart, the caller's workspace
// steps, a kernel choice per move
static void importFieldMoveList(ImportedFieldMoves& q, const cudecompExtMove_t* moves, const int64_t* work_steps, int32_t n,
                                void* const* inputs, void* const* outputs, const uint64_t* input_addresses, const uint64_t* output_addresses,
                                int32_t n_fields, void* work, int32_t es, int32_t force) {
  q.moves = importFieldMoves(moves, n, CUDECOMP_EXT_MAX_MEMBERS, n_fields, CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS, es);
  requestOver(q, inputs, input_addresses, n_fields, es, force);
  if (output_addresses) {
    q.outputs = pointersOf(output_addresses, n_fields);
    outputs = q.outputs.data();
  }
  q.list.outputs = outputs;
  q.list.work_steps = work_steps;
  q.list.work = work;
  q.list.one_choice = false;
}

cudecompResult_t cudecompExtRunFieldMoveList(const cudecompExtMove_t* moves, const int64_t* work_steps, int32_t n,
                                             void* const* inputs, void* const* outputs, int32_t n_fields, void* work, int32_t es,
                                             int32_t force, hipStream_t stream, int32_t* n_launches) {
  return guarded([&] {
    if (!inputs) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importFieldMoveList(q, moves, work_steps, n, inputs, outputs, nullptr, nullptr, n_fields, work, es, force);
    runFieldMoveList(q.list, stream, n_launches);
  });
}

cudecompResult_t cudecompExtDescribeFieldMoveList(const cudecompExtMove_t* moves, const int64_t* work_steps, int32_t n,
                                                  const uint64_t* input_addresses, const uint64_t* output_addresses,
                                                  int32_t n_fields, uint64_t work_address, int32_t es, int32_t force,
                                                  cudecompExtFieldMoveLaunch_t* launches, int32_t max_launches,
                                                  int32_t* n_launches) {
  return guarded([&] {
    if (!input_addresses || !n_launches || (max_launches > 0 && !launches)) CD_INVALID_USAGE("null argument");
    ImportedFieldMoves q;
    importFieldMoveList(q, moves, work_steps, n, nullptr, nullptr, input_addresses, output_addresses, n_fields,
                        reinterpret_cast<void*>(work_address), es, force);
    const std::vector<FieldMoveLaunch> ls = planFieldMoveLaunches(q.list);
    *n_launches = (int32_t)ls.size();
    for (int32_t i = 0; i < (int32_t)ls.size() && i < max_launches; ++i) {
      const FieldMoveLaunch& l = ls[i];
      cudecompExtFieldMoveLaunch_t& o = launches[i];
      std::memset(&o, 0, sizeof(o));
      o.kind = (int32_t)l.k.kind;
      o.es = l.k.es;
      o.vec = l.k.vec;
      o.ti = l.k.ti;
      o.tj = l.k.tj;
      o.access = l.k.access;
      o.guard = l.k.guard ? 1 : 0;
      o.n_moves = l.b.n;
      o.blocks = l.blocks;
      o.blocks_per_field = l.blocks_per_field;
      for (int j = 0; j < l.b.n; ++j) o.index[j] = l.index[j];
    }
  });
}

cudecompResult_t cudecompExtDataLaunchCount(int64_t* launches) {
  if (!launches) return CUDECOMP_RESULT_INVALID_USAGE;
  *launches = dataLaunchCount();
  return CUDECOMP_RESULT_SUCCESS;
}

cudecompResult_t cudecompExtHaloPlanCount(cudecompHandle_t handle, cudecompGridDesc_t grid_desc, int64_t* plans) {
  if (!handle || !grid_desc || !plans) return CUDECOMP_RESULT_INVALID_USAGE;
  *plans = (int64_t)grid_desc->halo_plans.size();
  return CUDECOMP_RESULT_SUCCESS;
}

cudecompResult_t cudecompExtDescribeMoves(const cudecompExtMove_t* moves, int32_t n, const uint64_t buf_addresses[3], int32_t es,
                                         int32_t mode, cudecompDataType_t dtype, int32_t flags, const uint64_t* dst_base_addresses,
                                         cudecompExtLaunch_t* launches, int32_t max_launches, int32_t* n_launches) {
  return guarded([&] {
    if (!buf_addresses || !n_launches || max_launches < 0 || (max_launches > 0 && !launches)) CD_INVALID_USAGE("bad argument");
    ArithType arith;
    const std::vector<Move3D> list = importMoves(moves, n, es, mode, dtype, &arith);
    const KernelTuning t = tuningOfFlags(flags);
    void* bufs[3];
    for (int i = 0; i < 3; ++i) bufs[i] = reinterpret_cast<void*>(buf_addresses[i]);
    std::vector<void*> bases;
    if (dst_base_addresses) bases = pointersOf(dst_base_addresses, n);
    if (dst_base_addresses && bases.empty()) bases.push_back(nullptr);  // (an empty list with bases is still a remote one)
    // wall planes (mode 13 / 14): source and destination are buffer 0's cells, buffers 1 and 2 the low and the high plane
    const bool wall_plane = mode == 13 || mode == 14;
    const WallPlanes planes{{bufs[1], bufs[2]}};
    const std::vector<Launch> ls = planLaunches(list.data(), n, bufs, es, &t, dst_base_addresses ? bases.data() : nullptr, arith,
                                                wall_plane ? &planes : nullptr);
    *n_launches = (int32_t)ls.size();
    if ((int32_t)ls.size() > max_launches) CD_INVALID_USAGE("more launches than the output array holds");
    for (size_t i = 0; i < ls.size(); ++i) {
      const Launch& l = ls[i];
      cudecompExtLaunch_t& o = launches[i];
      std::memset(&o, 0, sizeof(o));
      o.cls = l.cls;
      o.kind = l.k.kind;
      o.es = l.k.es;
      o.vec = l.k.vec;
      o.tile_i = l.k.ti;
      o.tile_j = l.k.tj;
      o.access = l.k.access;
      o.arith = l.k.arith;
      o.n = l.b.n;
      o.interleave = l.b.interleave;
      o.blocks = l.blocks;
      o.elements = l.elements;
      for (int k = 0; k <= l.b.n; ++k) o.first_block[k] = l.b.first_block[k];
      for (int k = 0; k < 8; ++k) o.index[k] = k < l.b.n ? l.index[k] : -1;
    }
  });
}

cudecompResult_t cudecompExtDescribeResidency(const cudecompExtMove_t* moves, int32_t n, const uint64_t buf_addresses[3], int32_t es,
                                             int32_t flags, int32_t* pad_bytes, int32_t max_launches, int32_t* n_launches) {
  return guarded([&] {
    if (!buf_addresses || !n_launches || max_launches < 0 || (max_launches > 0 && !pad_bytes)) CD_INVALID_USAGE("bad argument");
    ArithType arith;
    const std::vector<Move3D> list = importMoves(moves, n, es, 0, (cudecompDataType_t)0, &arith);
    const KernelTuning t = tuningOfFlags(flags);
    void* bufs[3];
    for (int i = 0; i < 3; ++i) bufs[i] = reinterpret_cast<void*>(buf_addresses[i]);
    const std::vector<Launch> ls = planLaunches(list.data(), n, bufs, es, &t, nullptr, arith);
    *n_launches = (int32_t)ls.size();
    if ((int32_t)ls.size() > max_launches) CD_INVALID_USAGE("more launches than the output array holds");
    for (size_t i = 0; i < ls.size(); ++i) pad_bytes[i] = residencyPadBytes(ls[i].k, ls[i].b);
  });
}

cudecompResult_t cudecompExtRunMoves(const cudecompExtMove_t* moves, int32_t n, void* const bufs[3], int32_t es, int32_t mode,
                                    cudecompDataType_t dtype, const void* fill_value, int32_t flags, void* const* dst_bases,
                                    hipStream_t stream, int32_t launches[3], int64_t elements[3], int32_t* n_launches) {
  return guarded([&] {
    if (!bufs) CD_INVALID_USAGE("null argument");
    ArithType arith;
    const std::vector<Move3D> list = importMoves(moves, n, es, mode, dtype, &arith);
    const KernelTuning t = tuningOfFlags(flags);
    KernelStats st;
    WallAddends addends;
    const bool wall = mode == 11 || mode == 12;
    if (wall) {  // fill_value: 2 x CUDECOMP_AMD_MAX_WALL_HALO elements of `es` bytes, the low side's layers then the high side's
      if (!fill_value) CD_INVALID_USAGE("wall-value moves (mode 11 / 12) take their addends through fill_value");
      std::memset(&addends, 0, sizeof(addends));
      for (int side = 0; side < 2; ++side)
        for (int k = 0; k < CUDECOMP_AMD_MAX_WALL_HALO; ++k)
          std::memcpy(addends.v[side][k], static_cast<const char*>(fill_value) + (size_t)(side * CUDECOMP_AMD_MAX_WALL_HALO + k) * es, es);
    }
    // wall planes (mode 13 / 14): source and destination are buffer 0's cells, buffers 1 and 2 the low and the high plane
    const bool wall_plane = mode == 13 || mode == 14;
    const WallPlanes planes{{bufs[1], bufs[2]}};
    launchMoves(list.data(), n, bufs, es, stream, &t, &st, dst_bases, arith, mode == 2 ? fill_value : nullptr, wall ? &addends : nullptr,
                wall_plane ? &planes : nullptr);
    int total = 0;
    for (int c = 0; c < MOVE_CLASS_COUNT; ++c) {
      if (launches) launches[c] = st.launches[c];
      if (elements) elements[c] = st.elements[c];
      total += st.launches[c];
    }
    if (n_launches) *n_launches = total;
  });
}

// ---- the flag, page-tag and checksum kernels of sync.hip, one launch each (tests/test_gpu_sync_kernels.py) ----------------------
cudecompResult_t cudecompExtSyncEpochBegin(uint64_t* epoch, uint64_t* const* flags, int32_t n, hipStream_t stream) {
  return guarded([&] {
    const FlagList l = flagListOf(flags, n);
    if (!epoch) CD_INVALID_USAGE("null epoch");
    launchEpochBegin(reinterpret_cast<unsigned long long*>(epoch), l, stream);
  });
}

cudecompResult_t cudecompExtSyncSignal(const uint64_t* epoch, uint64_t* const* flags, int32_t n, int32_t step, hipStream_t stream) {
  return guarded([&] {
    const FlagList l = flagListOf(flags, n);
    checkFlagStep(step);
    if (n > 0 && !epoch) CD_INVALID_USAGE("null epoch");
    launchSignal(reinterpret_cast<const unsigned long long*>(epoch), l, stream, step);
  });
}

cudecompResult_t cudecompExtSyncWait(const uint64_t* epoch, uint64_t* const* flags, int32_t n, int32_t step, uint64_t* status,
                                     double timeout_s, hipStream_t stream) {
  return guarded([&] {
    const FlagList l = flagListOf(flags, n);
    checkFlagStep(step);
    // (the harness never parks a wave for longer than a second, whatever a test asks for; NaN fails both comparisons)
    if (!(timeout_s > 0.0 && timeout_s <= 1.0)) CD_INVALID_USAGE("timeout_s must lie in (0, 1]");
    if (n > 0 && (!epoch || !status)) CD_INVALID_USAGE("null epoch or status");
    launchWait(reinterpret_cast<const unsigned long long*>(epoch), l, reinterpret_cast<unsigned long long*>(status), timeout_s, stream,
               step);
  });
}

cudecompResult_t cudecompExtTagPages(void* base, size_t bytes, uint64_t seed, hipStream_t stream) {
  return guarded([&] {
    if (bytes >= 4096 && !base) CD_INVALID_USAGE("null buffer");
    launchTagPages(base, bytes, seed, stream);
  });
}

cudecompResult_t cudecompExtCheckPages(const void* base, size_t bytes, uint64_t seed, uint64_t* bad, hipStream_t stream) {
  return guarded([&] {
    if (bytes >= 4096 && (!base || !bad)) CD_INVALID_USAGE("null argument");
    launchCheckPages(base, bytes, seed, reinterpret_cast<unsigned long long*>(bad), stream);
  });
}

cudecompResult_t cudecompExtChecksum(const void* ptr, size_t bytes, uint64_t* out2, hipStream_t stream) {
  return guarded([&] {
    if (bytes > 0 && (!ptr || !out2)) CD_INVALID_USAGE("null argument");
    launchChecksum(ptr, bytes, reinterpret_cast<unsigned long long*>(out2), stream);
  });
}

}  // extern "C"
