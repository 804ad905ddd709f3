// halo.cc -- executes halo plans: every halo family (update, accumulation with or without clearing, fill, reflection, folding, one
// pencil or several) is ONE sequence -- find or build the plan, launch `pre`, exchange, launch `post` -- and what differs between
// them is in the HaloOp of the call.  The algorithmic content lives in plan.cc (what moves where) and kernels.cc (how).
#include "errors.h"
#include "internal.h"
#include "transport.h"
#include "kernels_batch.h"

namespace cudecomp {

// the exchange of a halo plan (update or accumulation): send slot / face i travels to neighbour i and lands in ITS receive slot
// 1 - i (update: my low face fills the low neighbour's HIGH halo; accumulation: my low halo is the addend of its HIGH face)
static HaloExchange haloExchangeOf(const HaloPlan& plan, void* const bufs[3], int es) {
  HaloExchange x;
  x.send = x.recv = static_cast<char*>(bufs[plan.xbuf]);
  for (int i = 0; i < 2; ++i) {
    x.send_off[i] = plan.send_off[i] * es;
    x.recv_off[i] = plan.recv_off[i] * es;
    x.remote_off[i] = plan.recv_off[1 - i] * es;
    x.neighbor[i] = plan.neighbor[i];
  }
  x.bytes = (i64)plan.op.n_fields * plan.face_elements * es;
  x.comm_axis = plan.comm_axis;
  return x;
}

// The sequence of every halo call.  Local kinds (fill, reflection, folding) and self-periodic plans end after `pre`; the others pack
// (`pre`), exchange op.n_fields faces per direction with the exchange of the updates (haloExchange: same routing, transports and
// stream ordering for all of them) and unpack or add what arrived (`post`).  Only the update of ONE pencil is sampled by the
// performance report and overlaps pack, exchange and unpack face by face; a one-field call of the multi-field entry points IS the
// single call: same key, same plan, same path.
void runHaloOp(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloCall& c) {
  const HaloOp& op = c.op;
  const int es = elementSize(c.dtype);
  const auto backend = gd->config.halo_comm_backend;
  const bool mirrored = op.kind == HaloOp::REFLECT || op.kind == HaloOp::FOLD;
  // The key carries force_packed also where the plan never takes the direct form (accumulation) or only takes its destinations
  // from the update's plan (fill): a descriptor whose backend changes between peer and non-peer transports caches such a plan
  // twice -- harmless.  Two fields or more are always packed: one message per direction.
  const bool force_packed = !mirrored && (op.n_fields >= 2 || usesPeerTransport(h, backend));

  std::array<int32_t, 3> hh{0, 0, 0}, pp{0, 0, 0};
  std::array<bool, 3> per{false, false, false};
  for (int i = 0; i < 3; ++i) {
    if (c.halo) hh[i] = c.halo[i];
    if (c.pad) pp[i] = c.pad[i];
    if (c.periods) per[i] = c.periods[i];
  }
  // reflection and folding check their own arguments here, in the contract's order: what the fill refuses, then parity,
  // centering and `clear`, then (the plan's) a mirror that reaches beyond the interior
  const bool bad_parity = c.parity != 1 && c.parity != -1, bad_centering = op.centering != 0 && op.centering != 1,
             bad_clear = c.clear != 0 && c.clear != 1;
  if (mirrored && (bad_parity || bad_centering || bad_clear)) {
    buildHaloPlan(gd->shape, h->rank, c.axis, c.dim, hh.data(), per.data(), pp.data(), false, h->self_exchange);  // (the fill's refusals)
    if (bad_parity) CD_INVALID_USAGE("parity argument must be +1 or -1");
    if (bad_centering) CD_INVALID_USAGE("centering argument must be 0 or 1");
    CD_INVALID_USAGE("clear argument must be 0 or 1");
  }

  const cudecompGridDesc::HaloKey hkey{c.axis, c.dim, {hh[0], hh[1], hh[2], pp[0], pp[1], pp[2]}, per, force_packed};
  const std::pair<cudecompGridDesc::HaloKey, HaloOp> key{hkey, op};
  auto it = gd->halo_plans.find(key);
  if (it == gd->halo_plans.end()) {
    HaloPlan p = buildHaloOpPlan(gd->shape, h->rank, c.axis, c.dim, hh.data(), per.data(), pp.data(), op, force_packed, h->self_exchange);
    it = gd->halo_plans.emplace(key, std::move(p)).first;
  }
  const HaloPlan& plan = it->second;
  if (plan.kind == HaloPlan::NONE) return;

  ensureDevice(h);
  void* bufs[3] = {c.fields[0], c.fields[0], c.work};
  // the arithmetic of the moves that add (accumulation, folding) or flip sign bits (reflection with parity -1; the reflection of
  // several fields always names its real type: its signs are a mask of fields, one kernel whatever they are)
  const bool computes = op.kind == HaloOp::ACCUMULATE || op.kind == HaloOp::FOLD ||
                        (op.kind == HaloOp::REFLECT && (op.negate || op.n_fields >= 2));
  const ArithType arith = computes ? arithOf(c.dtype) : ARITH_NONE;
  const int force = (h->tuning.force_class == MOVE_GENERIC ? 1 : 0) | (h->tuning.force_streaming ? 2 : 0) | (h->tuning.no_streaming ? 4 : 0);
  // The one or two sides of a phase go into ONE launch, unless they add onto overlapping cells (`ordered`): then one launch per
  // side, low side first.  Several fields: the list kernels (one_choice); either end of a move in a pencil is field f's, the fields'
  // pieces of the workspace lie one face apart; reflection and folding go as mirrored lists with the call's mask of signs.
  auto launch = [&](const std::vector<Move3D>& moves) {
    if (moves.empty()) return;
    const int n = (int)moves.size(), each = plan.ordered && moves[0].add ? 1 : n;
    if (op.n_fields == 1) {
      for (int i = 0; i < n; i += each)
        launchMoves(moves.data() + i, each, bufs, es, c.stream, &h->tuning, nullptr, nullptr, arith, c.value);
    } else {
      const std::vector<i64> steps(n, plan.face_elements);
      for (int i = 0; i < n; i += each)
        launchFieldMoveList(moves.data() + i, steps.data() + i, each, c.fields, c.fields, op.n_fields, c.work, es, c.stream, force, nullptr,
                            true, arith, mirrored, c.fields_neg);
    }
  };

  const bool exchanges = plan.kind == HaloPlan::PACKED || plan.kind == HaloPlan::DIRECT;
  hipEvent_t* pev = nullptr;  // performance-sample events: the single update only
  if (op.kind == HaloOp::UPDATE && op.n_fields == 1) {
    int64_t wire_bytes = 0;
    for (int i = 0; i < 2 && exchanges; ++i)
      if (plan.neighbor[i] >= 0) wire_bytes += plan.face_elements * es;
    pev = perfBeginHalo(h, gd, c.axis, c.dim, c.dtype, hh, per, pp, wire_bytes, c.stream);
  }
  if (!exchanges) {
    launch(plan.pre);
    perfMark(pev, 1, c.stream);
    perfMark(pev, 2, c.stream);
    perfMark(pev, 3, c.stream);
    return;
  }
  const HaloExchange x = haloExchangeOf(plan, bufs, es);
  // the single update, packed faces: pack, exchange and unpack overlap face by face (env CUDECOMP_DISABLE_HALO_OVERLAP=1 restores
  // the plain pack -> exchange -> unpack sequence of the reference, halo.h:200-260).  The overlapped path runs the plan's moves
  // itself through bufs[3]: not for several fields, and no other family has it.
  if (op.kind == HaloOp::UPDATE && op.n_fields == 1 && plan.kind == HaloPlan::PACKED && !h->halo_overlap_disable) {
    perfMark(pev, 1, c.stream);
    if (haloExchangePackedOverlapped(h, gd, x, plan, bufs, es, backend, c.stream)) {
      perfMark(pev, 2, c.stream);
      perfMark(pev, 3, c.stream);
      return;
    }
  }
  launch(plan.pre);  // (nothing for a direct plan)
  perfMark(pev, 1, c.stream);
  haloExchange(h, gd, x, backend, c.stream);
  perfMark(pev, 2, c.stream);
  launch(plan.post);
  perfMark(pev, 3, c.stream);
}

}  // namespace cudecomp
