// halo.cc -- executes halo plans: every halo family (update, accumulation with or without clearing, fill, reflection, folding, one
// pencil or several) is ONE sequence -- find or build the plan, launch `pre`, exchange, launch `post` -- and what differs between
// them is in the HaloOp of the call.  The algorithmic content lives in plan.cc (what moves where) and kernels.cc (how).
#include "errors.h"
#include "internal.h"
#include "transport.h"
#include "kernels_batch.h"

#include <cstring>
#include <vector>

namespace cudecomp {

static_assert(CUDECOMP_AMD_MAX_WALL_HALO == kern::kMaxWallHalo && kMaxWallLayers == kern::kMaxWallHalo,
              "the header's limit, the planner's and the addend table's length are one number");

// a double rounded to nearest even, in one step, to a 16-bit format of 1 sign, `ebits` exponent and `mbits` mantissa bits (binary16:
// 5, 10; bfloat16: 8, 7); overflow gives infinity, what lies below half the smallest subnormal gives zero, a NaN stays one (quiet)
static uint16_t narrowFromDouble(double x, int ebits, int mbits) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  const uint16_t sign = (uint16_t)((u >> 63) << 15);
  const int exp = (int)((u >> 52) & 0x7ff);
  const uint64_t man = u & ((1ull << 52) - 1);
  const int emax = (1 << ebits) - 1, bias = (1 << (ebits - 1)) - 1;
  const uint16_t inf = (uint16_t)(emax << mbits);
  if (exp == 0x7ff) return man ? (uint16_t)(sign | inf | (1u << (mbits - 1)) | (uint16_t)(man >> (52 - mbits))) : (uint16_t)(sign | inf);
  if (exp == 0) return sign;  // (zero, or a double subnormal: far below either format's smallest subnormal)
  int e = exp - 1023 + bias;  // the biased exponent of a normal result
  if (e >= emax) return (uint16_t)(sign | inf);
  const uint64_t sig = man | (1ull << 52);
  int shift = 52 - mbits;
  if (e <= 0) {  // subnormal result: the significand moves further down, the exponent field is 0
    shift += 1 - e;
    e = 0;
  }
  if (shift > 60) return sign;
  uint64_t q = sig >> shift;
  const uint64_t rem = sig & ((1ull << shift) - 1), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (q & 1))) ++q;
  // normal: q holds the implicit bit, and a carry out of the mantissa lands in the exponent; subnormal: q is the field
  const uint64_t bits = e > 0 ? ((uint64_t)(e - 1) << mbits) + q : q;
  return bits >= inf ? (uint16_t)(sign | inf) : (uint16_t)(sign | bits);
}

WallAddends wallAddendsOf(cudecompDataType_t dtype, int layers, int sides, const double* values_low, const double* values_high) {
  if (layers < 0 || layers > kern::kMaxWallHalo) CD_INTERNAL_ERROR("more ghost layers than the addend table holds");
  const ArithType arith = arithOf(dtype);
  const int rs = arith == ARITH_F64 ? 8 : (arith == ARITH_F32 ? 4 : 2), nc = elementSize(dtype) / rs;
  WallAddends a;
  std::memset(&a, 0, sizeof(a));
  for (int side = 0; side < 2; ++side) {
    const double* in = side == 0 ? values_low : values_high;
    if (!(sides & (1 << side))) continue;
    if (!in && layers > 0) CD_INTERNAL_ERROR("the value array of a side to write is missing");
    for (int k = 0; k < layers; ++k)
      for (int c = 0; c < nc; ++c) {
        const double x = in[k * nc + c];
        unsigned char* out = a.v[side][k] + c * rs;
        if (arith == ARITH_F64) {
          std::memcpy(out, &x, 8);
        } else if (arith == ARITH_F32) {
          const float f = (float)x;  // (IEEE: one rounding to nearest even, overflow to infinity)
          std::memcpy(out, &f, 4);
        } else {
          const uint16_t v = arith == ARITH_F16 ? narrowFromDouble(x, 5, 10) : narrowFromDouble(x, 8, 7);
          std::memcpy(out, &v, 2);
        }
      }
  }
  return a;
}

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

// The sequence of every halo call.  Local kinds (fill, reflection, folding, wall values, wall planes) and self-periodic plans end after `pre`; the others pack
// (`pre`), exchange op.n_fields faces per direction with the exchange of the updates (haloExchange: same routing, transports and
// stream ordering for all of them) and unpack or add what arrived (`post`).  Only the update of ONE pencil is sampled by the
// performance report and overlaps pack, exchange and unpack face by face; a one-field call of the multi-field entry points IS the
// single call: same key, same plan, same path.
void runHaloOp(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloCall& c) {
  const HaloOp& op = c.op;
  const int es = elementSize(c.dtype);
  const auto backend = gd->config.halo_comm_backend;
  const bool wall = op.kind == HaloOp::WALL_VALUES;
  const bool wall_planes = op.kind == HaloOp::WALL_PLANES;
  const bool mirrored = op.kind == HaloOp::REFLECT || op.kind == HaloOp::FOLD || wall || wall_planes;
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
  // centering and `clear`, then (wall values: sides, value arrays, width -- on every rank, whatever its place and the periods) then
  // (the plan's) a mirror that reaches beyond the interior
  const bool bad_parity = c.parity != 1 && c.parity != -1, bad_centering = op.centering != 0 && op.centering != 1,
             bad_clear = c.clear != 0 && c.clear != 1;
  const int bad_wall = wall ? wallValueRefusal(op.sides, c.values_low != nullptr, c.values_high != nullptr, hh[c.dim]) : 0;
  const cudecompGridDesc::HaloKey hkey{c.axis, c.dim, {hh[0], hh[1], hh[2], pp[0], pp[1], pp[2]}, per, force_packed};
  const std::pair<cudecompGridDesc::HaloKey, HaloOp> key{hkey, op};
  // wall planes: sides, NULL, then the overlap of a named plane with the pencil -- addresses only; a periodic dim or h == 0 has no
  // plane to overlap with.  The sizes depend on the key alone: a call that finds its plan cached reads them there.  Only a call
  // without a cached plan (the first, or one whose plan the builder refuses every time) works them out here -- from the pencil,
  // which only valid halos and padding give: what the fill refuses comes first -- because the overlap is reported before the
  // plan's own last refusal.
  int bad_planes = 0;
  if (wall_planes && !bad_parity && !bad_centering) {
    bad_planes = wallPlaneRefusal(op.sides, c.planes_low, c.planes_high, nullptr, 0, 0);
    if (bad_planes == 0 && hh[c.dim] > 0 && !per[c.dim]) {
      i64 pencil_elements = 0, plane_elements = 0;
      const auto cached = gd->halo_plans.find(key);
      if (cached != gd->halo_plans.end()) {
        pencil_elements = cached->second.pencil_elements;
        plane_elements = cached->second.plane_elements;
      } else {
        buildHaloPlan(gd->shape, h->rank, c.axis, c.dim, hh.data(), per.data(), pp.data(), false, h->self_exchange);  // (the fill's refusals)
        const Pencil pencil = makePencil(gd->shape, gridIndexOfRank(gd->shape, h->rank), c.axis, hh.data(), pp.data());
        const i64 along = pencil.extentG(c.dim);
        pencil_elements = pencil.size;
        plane_elements = along > 0 ? pencil.size / along * hh[c.dim] : 0;
      }
      bad_planes = wallPlaneRefusal(op.sides, c.planes_low, c.planes_high, c.fields[0], pencil_elements * es, plane_elements * es);
    }
  }
  if (mirrored && (bad_parity || bad_centering || bad_clear || bad_wall != 0 || bad_planes != 0)) {
    buildHaloPlan(gd->shape, h->rank, c.axis, c.dim, hh.data(), per.data(), pp.data(), false, h->self_exchange);  // (the fill's refusals)
    if (bad_parity) CD_INVALID_USAGE("parity argument must be +1 or -1");
    if (bad_centering) CD_INVALID_USAGE("centering argument must be 0 or 1");
    if (bad_clear) CD_INVALID_USAGE("clear argument must be 0 or 1");
    if (bad_planes != 0) refuseWallPlanes(bad_planes);
    refuseWallValues(bad_wall);
  }

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
  const bool computes = op.kind == HaloOp::ACCUMULATE || op.kind == HaloOp::FOLD || wall || wall_planes ||
                        (op.kind == HaloOp::REFLECT && (op.negate || op.n_fields >= 2));
  const ArithType arith = computes ? arithOf(c.dtype) : ARITH_NONE;
  // wall values: the addends are converted here, once per call, and travel to the launch by value -- read before the call returns
  // (several fields: values_low / values_high are field-major, hh[dim] * nc doubles per field; each field's part by the single rule)
  std::vector<WallAddends> addends(wall ? op.n_fields : 0);
  if (wall) {
    const size_t per_field = (size_t)hh[c.dim] * (size_t)(es / (arith == ARITH_F64 ? 8 : (arith == ARITH_F32 ? 4 : 2)));
    for (int f = 0; f < op.n_fields; ++f)
      addends[f] = wallAddendsOf(c.dtype, hh[c.dim], op.sides, c.values_low ? c.values_low + f * per_field : nullptr,
                                 c.values_high ? c.values_high + f * per_field : nullptr);
  }
  // The one or two sides of a phase go into ONE launch, unless they add onto overlapping cells (`ordered`): then one launch per
  // side, low side first.  Several fields: the list kernels (one_choice); either end of a move in a pencil is field f's, the fields'
  // pieces of the workspace lie one face apart; reflection and folding go as mirrored lists with the call's mask of signs, wall
  // values as wall lists with every field's addends (one launch per run of fields whose addends fit the table).
  FieldMoveList list;
  list.inputs = list.outputs = c.fields;
  list.n_fields = op.n_fields;
  list.work = c.work;
  list.es = es;
  list.arith = arith;
  list.one_choice = true;
  list.mirrored = mirrored;
  list.fields_neg = c.fields_neg;
  list.addends = wall ? addends.data() : nullptr;
  list.tuning = &h->tuning;
  // wall planes: the two device pointers travel to the launch with the call, the route of the addends; their contents are read by
  // the kernel, so a captured call applies what the planes hold at replay
  const WallPlanes planes{{c.planes_low, c.planes_high}};
  auto launch = [&](const std::vector<Move3D>& moves) {
    if (moves.empty()) return;
    const int n = (int)moves.size(), each = plan.ordered && moves[0].add ? 1 : n;
    if (op.n_fields == 1) {
      for (int i = 0; i < n; i += each)
        launchMoves(moves.data() + i, each, bufs, es, c.stream, &h->tuning, nullptr, nullptr, arith, c.value, list.addends,
                    wall_planes ? &planes : nullptr);
      return;
    }
    const std::vector<i64> steps(n, plan.face_elements);
    for (int i = 0; i < n; i += each) {
      list.moves = moves.data() + i;
      list.work_steps = steps.data() + i;
      list.n = each;
      launchFieldMoveList(list, c.stream);
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
