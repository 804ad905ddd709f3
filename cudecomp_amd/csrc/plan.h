// plan.h -- transposes and halo updates as DATA: a short list of strided block moves plus the
// exchange counts, built once per (operation, halos, padding, in-place, transport traits) and cached
// on the grid descriptor.  The executors (transpose.cc, halo.cc) only bind pointers and launch.
//
// Everything a transpose does locally is a Move3D:
//     dst[dst_off + k0*ds[0] + k1*ds[1] + k2*ds[2]] = src[src_off + k0*ss[0] + k1*ss[1] + k2*ss[2]]
// for 0 <= k_i < extent[i], all in ELEMENTS.  A pack, an unpack, a halo face copy and a full 3-D
// permutation are the same object; the kernel layer (kernels.cc + kernels_*.hip) picks the access pattern.
//
// What the plan must reproduce (bit-exact interior of the output pencil) is defined by
// NVIDIA/cuDecomp's cudecompTranspose_ / cudecompUpdateHalos_ (reference
// include/internal/transpose.h:196-905, include/internal/halo.h:41-315).  The plan is derived from
// the decomposition itself rather than transcribed from that code: see DESIGN.md "Plan".
#pragma once
#include <tuple>
#include <vector>

#include "decomp.h"

namespace cudecomp {

enum BufId : uint8_t { BUF_IN = 0, BUF_OUT = 1, BUF_WORK = 2 };

struct Move3D {
  BufId src_buf = BUF_IN, dst_buf = BUF_OUT;
  i64 src_off = 0, dst_off = 0;
  i64 extent[3] = {1, 1, 1};
  i64 ss[3] = {0, 0, 0};
  i64 ds[3] = {0, 0, 0};
  int peer = -1;  // communicator rank this move feeds / drains (-1: not tied to one peer)
  // > 0: the move writes WHOLE interior rows of the destination pencil (its unit-stride dim spans the pencil's interior
  // along the fastest memory axis) and this is the pencil's row pitch in elements.  The cells between the end of one row and
  // the start of the row one pitch further are then halo / padding cells of that pencil, written by nobody during the
  // operation, and the kernel layer may write whole cache lines across the row ends, putting back into those cells what it
  // read from them (rows_dense_kernel, kernels_rows.hip; transpose_lines_kernel, kernels_lines.hip; transpose_rowlines_kernel, kernels_rowlines.hip).  Only ever set for
  // local destinations (never for puts into a peer's pencil).  THE RULE this rests on: during a transpose nobody writes the
  // halo / padding cells of its output pencil -- no move of the plan (checked over random decompositions, tests/test_plan_sim.py),
  // no one-sided write of a peer (direct puts address interior cells, halo plans never target a peer's pencil: they exchange
  // through workspaces or whole contiguous faces, buildHaloPlan), and no kernel of the caller on another stream (the
  // documented contract; CUDECOMP_PRESERVE_OUTPUT_HALOS=1 for callers who cannot promise that).
  i64 dst_row_pitch = 0;
  // false: dst = src (every move of a transpose or a halo update).  true: dst = dst + src in the arithmetic of the call's data
  // type (halo accumulation, buildHaloAccumulatePlan): the kernel layer reads and rewrites exactly the destination cells of
  // the move -- never the gap cells between rows, never a peer's memory.
  bool add = false;
  // true: dst = the call's fill value (halo fill, buildHaloFillPlan).  The move has a destination only -- the source fields stay
  // zero and nothing is loaded -- and the kernel layer stores exactly the destination cells of the move: never the gap cells
  // between rows (dst_row_pitch is never set), never a peer's memory.
  bool fill = false;
  // true: after the move has read its source cells it stores zero bytes to them (the pack moves and wrap additions of the fused
  // halo accumulate-and-clear, buildHaloAccumulateClearPlan; with or without `add`).  The source is a local buffer whose cells
  // are disjoint from every destination and every other source of the phase; exactly the source cells of the move are written,
  // never the gap cells between rows (dst_row_pitch is never set), never a peer's memory.
  bool take = false;
  // true: the source runs BACKWARDS along one dim (halo reflection, buildHaloReflectPlan): that dim has a negative source stride
  // and src_off names the source cell of its index 0.  Only reflect-moves may have a negative stride.  Source and destination are
  // disjoint cells of one local buffer; exactly the destination cells of the move are written and exactly its source cells read.
  // A reflect-move never carries dst_row_pitch, fill or a remote destination (an internal error before any launch).
  // `reflect` together with `add` is the FOLD-MOVE (halo folding, buildHaloFoldPlan): dst = dst + src, or dst + (-src) with
  // `negate`, the source running backwards; it may carry `take` as well (zero bytes into the source cells it has read, under the
  // rule of take-moves: sources disjoint from every destination and every other source of the phase).  `reflect` with `take` but
  // without `add`, and a fold-move with dst_row_pitch, fill or a remote destination, are internal errors before any launch.
  bool reflect = false;
  // reflect- and fold-moves only: the sign bit of every real component is inverted on the way (one bit per real, two per complex
  // element); nothing else about the bytes changes.  A fold-move flips the bits first and adds then.
  bool negate = false;
  // reflect-moves of cudecompAmdSetWallHalos* only (buildHaloWallValuesPlan): the move adds the call's per-layer addend,
  // dst = +-src + a[layer], `layer` the destination's index along the mirrored dim.  1: the addends of the call's low side (ghost
  // layer k, counted from the wall outward, is destination index extent - 1 - k), 2: those of the high side (destination index k);
  // 0: none.  The addends travel with the call, not with the move (kernels.h launchMoves).  Such a move is a reflect-move with or
  // without `negate` and nothing else: with dst_row_pitch, fill, take, add or a remote destination it is an internal error before
  // any launch, and so is a mirrored dim thicker than the addend table (kern::kMaxWallHalo).
  int affine = 0;
  // reflect-moves of cudecompAmdSetWallPlaneHalos* only (buildHaloWallPlanesPlan): the move has a THIRD operand in device memory,
  // dst = +-src + plane[plane_off + k0*ps[0] + k1*ps[1] + k2*ps[2]], in elements.  1: it reads the call's low plane, 2: its high
  // plane; 0: none.  The strides are SIGNED: along the mirrored dim ps is negative on the low side (destination index j is ghost
  // layer h - 1 - j, and plane_off names the entry of index 0), so the kernels index the plane by destination, as they index the
  // source.  The plane POINTERS travel with the call, not with the move (kernels.h launchMoves).  Such a move is a reflect-move with
  // or without `negate` and nothing else: with dst_row_pitch, fill, take, add, affine or a remote destination it is an internal error
  // before any launch.  It carries no layer limit.
  int plane = 0;
  i64 plane_off = 0;
  i64 ps[3] = {0, 0, 0};

  i64 elements() const { return extent[0] * extent[1] * extent[2]; }
};

// Traits of the transport that change the plan (not the result).
struct TransportTraits {
  bool pipelined = false;        // per-peer overlap of pack / exchange / unpack
  bool symmetric_recv = false;   // one-sided peer writes: receive area must sit at the same workspace offset on
                                 // every rank and inside the workspace (never in the user's output buffer)
  bool self_exchange = false;    // test aid (CUDECOMP_TEST_SELF_EXCHANGE=1): a one-member communicator still runs
                                 // pack -> exchange (with itself) -> unpack, so that a single GPU drives the real
                                 // transports end to end
  bool no_elide = false;         // multi-field transposes (buildTransposeFieldsPlan): never send from the input or receive
                                 // into the output -- the plan always has `pack` and `unpack` and send_buf == recv_buf ==
                                 // BUF_WORK, because one message per peer must hold the chunks of ALL fields
};

struct TransposePlan {
  // identification
  int ax_a = 0, ax_b = 0, ax_c = 0;
  CommAxis comm_axis = COMM_COL;
  int nranks = 1, comm_rank = 0;  // size of / my rank in the exchanging communicator
  bool noop = false;              // nothing to do at all (single rank, in place, identical layout)

  std::vector<Move3D> pack;    // before the exchange (schedule order: peers first, self last)
  std::vector<Move3D> unpack;  // after the exchange (self first)

  // exchange: chunk for member d starts at send_off[d] of (send_buf + send_base); the chunk from
  // member s lands at recv_off[s] of (recv_buf + recv_base); all in elements
  bool exchange = false;
  BufId send_buf = BUF_WORK, recv_buf = BUF_WORK;
  i64 send_base = 0, recv_base = 0;
  std::vector<i64> send_cnt, send_off, recv_cnt, recv_off;
  std::vector<i64> remote_recv_off;  // where MY chunk lands in member d's receive area (one-sided transports)
  std::vector<int> schedule_dst, schedule_src;  // pairwise peer order, entry 0 = self
  // Staged exchange (one-sided pipelined transports): every chunk is a dense block whose SLOWEST wire dim is the global
  // axis `stage_axis`; cutting all chunks into the same number of ranges along it gives sub-chunks that are contiguous
  // in the send and receive areas.  stage_limit = the smallest extent any chunk of the communicator has along that axis
  // (the same number on every member: an upper bound for the number of stages everybody can agree on without talking).
  int stage_axis = 2;
  i64 stage_limit = 1;
  i64 stage_elements = 0;  // largest pencil of the decomposition (the same number on every rank): staging is sized by it
  std::vector<i64> send_n, recv_n;  // extent along stage_axis of the chunk for member d / from member s

  // Direct-to-destination put (one-sided transports, out of place): move `direct[j]` takes the slab of my input that
  // belongs to member direct[j].peer and writes it straight into THAT member's output pencil, in its final layout
  // (dst_off / ds are relative to the peer's output buffer) -- one HBM pass per element, no receive area, no unpack.
  // Same order as `pack` (peers in schedule order, self last).  Empty when the plan has no such form (in place).
  std::vector<Move3D> direct;

  // Single-rank, in place, cubic, no halos / padding, and the two memory orders a rotation of each other: the whole
  // operation is the in-place rotation new[p0,p1,p2] = old[p2,p0,p1] (+1) or its inverse (-1) of an n^3 array -- one read
  // and one write per element where pack + unpack through the workspace (which stay in the plan: the kernel layer says
  // whether it has the rotation for the element size, kernels_rotate.hip) need two of each.  0: no such form.
  int rotate = 0;
  i64 rotate_n = 0;

  i64 pencil_elements_a = 0;  // interior elements moved (for bandwidth accounting)
};

enum TransposeOp { OP_X_TO_Y = 0, OP_Y_TO_Z = 1, OP_Z_TO_Y = 2, OP_Y_TO_X = 3 };

TransposePlan buildTransposePlan(const GridShape& g, int rank, TransposeOp op, const int32_t* in_halo,
                                 const int32_t* out_halo, const int32_t* in_pad, const int32_t* out_pad, bool inplace,
                                 const TransportTraits& traits, int npergroup);

// Multi-field TRANSPOSE (include/cudecomp_transpose_fields.h has the contract): `n_fields` pencils of one descriptor, op, halos
// and padding transposed by one exchange.  Derived from buildTransposePlan with TransportTraits::no_elide (and never
// pipelined): its refusals, peers, schedule and "which cells" hold by construction.  The moves in `base` are those of FIELD 0:
// an end in BUF_IN / BUF_OUT is field f's input / output pencil at the same offset; an end in BUF_WORK lies at its offset +
// f * step, step = pack_step[i] for base.pack[i] and unpack_step[i] for base.unpack[i] (elements).  With an exchange the chunk
// for member d is n_fields pieces of the single plan's send_cnt[d], one behind the other, at n_fields * (the single plan's
// send_off[d]); the receive side likewise behind recv_base = alignElements(n_fields * the single plan's unaligned base): the
// same number on every rank, as the one-sided transport needs.  base.send_cnt, send_off, recv_cnt, recv_off and
// remote_recv_off are the single plan's multiplied by n_fields: the exchange reads nothing else.  The total stays within
// n_fields x transposeWorkspaceElements: alignElements(n * x) + n * y <= n * (alignElements(x) + y).  Without an exchange:
// out of place one move pencil -> pencil (steps 0), in place with differing layouts pack and unpack through n_fields pieces
// of one pencil each, in place with identical layouts a no-op.  No move carries dst_row_pitch (the field kernels write exactly
// the cells of their moves); `direct` is empty and `rotate` 0.  n_fields == 1: the plan of buildTransposePlan with the caller's
// traits, unchanged (steps 0).
struct TransposeFieldsPlan {
  TransposePlan base;
  int n_fields = 1;
  std::vector<i64> pack_step, unpack_step;
};
TransposeFieldsPlan buildTransposeFieldsPlan(const GridShape& g, int rank, TransposeOp op, const int32_t* in_halo,
                                             const int32_t* out_halo, const int32_t* in_pad, const int32_t* out_pad, bool inplace,
                                             const TransportTraits& traits, int npergroup, int n_fields);

// ---- two-hop relay of a low-fan-out exchange over the whole node (peer_exchange.cc: peerRelayAlltoall) ----------------------
// On a full xGMI mesh an exchange among P members drives P - 1 of a GPU's links.  On a pencil grid P is small -- the
// X<->Y exchange of a 2 x 4 grid has P = 2: half a pencil through ONE link while six links idle.  Here every outgoing chunk
// is cut into `nranks` equal slices (nranks = all ranks of the node); slice q travels source -> rank q -> destination, the
// slices q = source and q = destination go straight to the destination.  Every link then carries two slices per direction
// instead of one link carrying the whole chunk: wire time / (nranks / 2), paid with one extra HBM round trip of the relayed
// bytes at the relays.  (The grouping idea of the reference's schedule, include/internal/common.h:533-577, taken one step
// further; nothing like it exists there.)
//   step 1 "scatter": my slices -> relay regions of the ranks q (relay slot of (source, chunk index)) / receive area of the
//                     destination for the two direct slices;
//   step 2 "forward": what arrived in MY relay region -> the receive areas of its destinations.
// Every rank derives the moves of every other rank from the decomposition alone (the planner is stateless), so the
// forwarder knows where a slice must go without any metadata travelling with it.
struct RelayMove {
  int dst_rank = 0;      // GLOBAL rank whose memory is written
  bool to_relay = false; // destination is that rank's relay region (else its receive area)
  i64 src_off = 0;       // scatter: elements from the start of my send area; forward: elements into MY relay region
  i64 dst_off = 0;       // elements into the destination's relay region / receive area
  i64 count = 0;
};
struct RelayPlan {
  bool applies = false;
  int nranks = 0;            // ranks of the node (= of the handle)
  int slots_per_source = 0;  // chunks a rank sends = P - 1
  i64 slot_elements = 0;     // size of one relay slot = the largest slice of the decomposition
  std::vector<RelayMove> scatter, forward;
  i64 relayElements() const { return (i64)nranks * slots_per_source * slot_elements; }
};
// worth it when the exchange uses at most a third of the links a rank has
inline bool relayWorthwhile(int P, int nranks) { return P >= 2 && nranks >= 4 && 3 * (P - 1) <= nranks - 1; }
RelayPlan buildRelayPlan(const GridShape& g, int nranks, int rank, TransposeOp op, const int32_t* in_halo,
                         const int32_t* out_halo, const int32_t* in_pad, const int32_t* out_pad, bool inplace,
                         const TransportTraits& traits, int npergroup);

// What a halo call is: the operation and the arguments that change its plan.  Every builder below writes the record of its plan;
// buildHaloOpPlan goes the other way.  Ordered, so that it can be part of the key of the plan cache (internal.h).
struct HaloOp {
  enum Kind { UPDATE, ACCUMULATE, FILL, REFLECT, FOLD, WALL_VALUES, WALL_PLANES } kind = UPDATE;
  bool clear = false;  // ACCUMULATE, FOLD: the ghost cells read are cleared
  int centering = 0;   // REFLECT, FOLD, WALL_VALUES, WALL_PLANES
  bool negate = false; // REFLECT, FOLD, WALL_VALUES, WALL_PLANES of ONE field: parity -1 (several fields: false; their parities travel with the call)
  int n_fields = 1;    // UPDATE, ACCUMULATE, REFLECT, FOLD, WALL_VALUES (1 for FILL)
  int sides = 3;       // WALL_VALUES, WALL_PLANES: bit 0 the low halo, bit 1 the high halo (it changes the moves; the addends and the
                       // plane pointers do not and are no part of the record: calls that differ only in them share a plan)
  bool operator<(const HaloOp& o) const {
    return std::tie(kind, clear, centering, negate, n_fields, sides) < std::tie(o.kind, o.clear, o.centering, o.negate, o.n_fields, o.sides);
  }
};

struct HaloPlan {
  int axis = 0, dim = 0;
  enum Kind { NONE, SELF_PERIODIC, PACKED, DIRECT } kind = NONE;
  CommAxis comm_axis = COMM_COL;
  int neighbor[2] = {-1, -1};  // global ranks of the -1 / +1 neighbours (-1: none)
  std::vector<Move3D> pre;     // SELF_PERIODIC: the two wrap copies; PACKED: face -> workspace
  std::vector<Move3D> post;    // PACKED: workspace -> halo
  // exchange in elements.  Face i (0 = low side, 1 = high side) is SENT to neighbour i and halo slot i is
  // FILLED by neighbour i.  Offsets are relative to the pencil (DIRECT) or the workspace (PACKED).
  i64 face_elements = 0;
  BufId xbuf = BUF_WORK;
  i64 send_off[2] = {0, 0}, recv_off[2] = {0, 0};
  HaloOp op;             // the operation the plan was built for
  bool ordered = false;  // accumulation and fold plans: the destinations of the two add-moves overlap (interior narrower than two
                         // halos; fold: n < 4h + 2c): one launch each, in order
  i64 slot_elements = 0; // multi-field builders, PACKED: the length of one workspace slot (buildHaloFieldsPlan)
  // WALL_PLANES: the elements of the pencil and of one plane, for the runner's overlap check of a call that finds its plan cached;
  // both 0 where the dim is periodic or has no halo (no plane to overlap with).  Set on every rank, whether or not it has moves.
  i64 pencil_elements = 0, plane_elements = 0;
};

HaloPlan buildHaloPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                       const int32_t* pad, bool force_packed, bool self_exchange = false);

// Halo ACCUMULATION along `dim` -- the transpose of the update: what the neighbours hold in the halo cells they keep of MY
// cells is added to my face cells (low face += the low neighbour's high halo, then high face += the high neighbour's low
// halo; include/cudecomp_amd.h has the contract).  Same arguments and refusals as buildHaloPlan, plus: a halo wider than my
// own interior along `dim` is INVALID_USAGE.  Kinds: NONE, SELF_PERIODIC (two add-moves pencil -> pencil in `pre`), PACKED
// (`pre`: my halos -> send slots 0 / 1, plain copies; the exchange of HaloExchange: slot i travels to neighbour i and lands in
// its receive slot 1 - i; `post`: add-moves receive slot 0 -> low face, receive slot 1 -> high face).  Never DIRECT: what
// arrives must be added, not stored.  The workspace layout is buildHaloPlan's (haloWorkspaceElements covers it).
HaloPlan buildHaloAccumulatePlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, bool force_packed, bool self_exchange = false);

// Halo accumulation along `dim` that CLEARS the ghost cells it has read (include/cudecomp_amd_fill.h has the contract): the plan
// of buildHaloAccumulatePlan -- same kinds, neighbours, offsets, moves, refusals and `ordered` rule -- with Move3D::take set on
// exactly the moves whose SOURCE is the pencil: the two add-moves of SELF_PERIODIC, the two pack moves of PACKED's `pre`.  The
// add-moves of PACKED's `post` read the workspace and stay plain.  The sources are the low / high halo slabs, the cells
// buildHaloFillPlan names for the same arguments.
HaloPlan buildHaloAccumulateClearPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                      const int32_t* pad, bool force_packed, bool self_exchange = false);

// Halo FILL along `dim`: the cells the update along `dim` writes (low halo where there is a low neighbour, high halo where there
// is a high one; include/cudecomp_amd_fill.h has the contract) receive one value.  Same arguments and refusals as buildHaloPlan,
// from which the destinations are taken -- the pencil destinations of its wrap copies (SELF_PERIODIC) or unpacks (PACKED), its
// receive ranges (DIRECT: whole contiguous faces) -- so "the cells the update writes" holds by construction.  Kinds: NONE or
// SELF_PERIODIC (the word for "local": nothing is exchanged whatever the update's kind).  `pre` holds at most two fill-moves
// (Move3D::fill), the low side then the high side, destination only, in BUF_IN; their cells never overlap.
HaloPlan buildHaloFillPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                           const int32_t* pad, bool force_packed, bool self_exchange = false);

// Halo REFLECTION along `dim` (include/cudecomp_amd_reflect.h has the contract): the ghost cells the update along `dim` does NOT
// write -- the low halo where there is no low neighbour, the high halo where there is no high one -- receive the mirror image of
// the interior: low side cell(h-1-k) = cell(h+k+c), high side cell(n-h+k) = cell(n-h-1-k-c), k in [0, h), c = centering.  The
// refusals of buildHaloPlan first; then a side that would be written with h + c > n - 2h (the sources would leave the rank's
// interior) is INVALID_USAGE.  Kinds: NONE or SELF_PERIODIC ("local", as for fill plans).  `pre` holds at most two reflect-moves
// (Move3D::reflect, Move3D::negate = `negate`) pencil -> pencil in BUF_IN, the low side then the high side: the destination runs
// forwards over the halo slab (the other two dims INCLUDING their halos, not their padding), the source backwards along `dim`.
HaloPlan buildHaloReflectPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                              const int32_t* pad, int centering, bool negate, bool self_exchange = false);

// Wall VALUES along `dim` (include/cudecomp_halo_wall_values.h has the contract): the reflection with one addend per ghost layer and
// side, cell = s * mirror + a.  The moves are buildHaloReflectPlan's for the sides kept (`sides`: bit 0 low, bit 1 high, 1 .. 3) --
// same cells, same `reflect` and `negate` -- and carry Move3D::affine = 1 (low) / 2 (high).  The refusals of buildHaloPlan first, then
// the centering, then (wallValueRefusal below, for callers that hold the arguments) sides, value arrays and width; the reflection's
// refusal h + c > n - 2h only for a side that would be written.  Kinds: NONE or SELF_PERIODIC ("local").
HaloPlan buildHaloWallValuesPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, int centering, bool negate, int sides, bool self_exchange = false);
// The three checks of the wall values that follow the centering check, in the contract's order: 0 fine, 1 `sides` outside 1 .. 3,
// 2 a NULL value array of a side named in `sides`, 3 halo_extents[dim] beyond the addend table.  refuseWallValues throws what the
// contract states for 1 .. 3 (INVALID_USAGE, INVALID_USAGE, NOT_SUPPORTED).
constexpr int kMaxWallLayers = 8;  // CUDECOMP_AMD_MAX_WALL_HALO and kern::kMaxWallHalo (halo.cc asserts that the three are one number)
int wallValueRefusal(int sides, bool has_low, bool has_high, i64 halo_dim);
[[noreturn]] void refuseWallValues(int refusal);

// Wall PLANES along `dim` (include/cudecomp_halo_wall_planes.h has the contract): the reflection with an addend per CELL of the
// ghost slab, read from a device array that is a slab of the pencil, cell = s * mirror + plane(k; p, q).  The moves are
// buildHaloWallValuesPlan's for the sides kept -- same cells, same `reflect` and `negate`, no `affine` -- and each describes its third
// operand (Move3D::plane, plane_off, ps): the plane has the pencil's shape (halos and padding included) with the extent along `dim`
// replaced by h = halo[dim], dense in the pencil's memory order; the index along `dim` is the ghost layer k, counted from the wall
// outward, so ps[dim] is negative on the low side; the other two indices are the pencil's own.  No layer limit.  The refusals of
// buildHaloPlan first, then the centering, then `sides` outside 1 .. 3 (callers that hold the plane pointers check them in the
// contract's place, wallPlaneRefusal below); the reflection's refusal h + c > n - 2h only for a side that would be written.  Kinds:
// NONE or SELF_PERIODIC ("local").
HaloPlan buildHaloWallPlanesPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, int centering, bool negate, int sides, bool self_exchange = false);
// The three checks of the wall planes that follow the centering check, in the contract's order: 0 fine, 1 `sides` outside 1 .. 3, 2 a
// NULL plane of a side named in `sides`, 3 a named plane whose byte range [plane, plane + plane_bytes) overlaps the pencil's
// [pencil, pencil + pencil_bytes) -- a comparison of addresses (plane_bytes == 0: periodic dim or h == 0, NULL check only).
// refuseWallPlanes throws INVALID_USAGE for 1 .. 3.
int wallPlaneRefusal(int sides, const void* plane_low, const void* plane_high, const void* pencil, i64 pencil_bytes, i64 plane_bytes);
[[noreturn]] void refuseWallPlanes(int refusal);

// Halo FOLDING along `dim` (include/cudecomp_halo_fold.h has the contract) -- the transpose of the reflection: the ghost cells the
// reflection along `dim` writes are ADDED to the interior cells it reads them from: low side cell(h+k+c) += s * cell(h-1-k), then
// high side cell(n-h-1-k-c) += s * cell(n-h+k), k in [0, h).  Refusals, neighbours and sides are buildHaloReflectPlan's, which is
// called first, so "the sides the reflection writes" holds by construction.  Kinds: NONE or SELF_PERIODIC ("local").  `pre`
// holds at most two fold-moves (Move3D::reflect and Move3D::add, Move3D::negate = `negate`, Move3D::take = `clear`) pencil ->
// pencil in BUF_IN, the low side then the high side.  As in a reflect-move only the SOURCE stride is negative: the low
// destinations run forwards over [h+c, 2h+c) with src_off at ghost cell h-1, the high ones over [n-2h-c, n-h-c) with src_off at
// ghost cell n-1.  `ordered`: both sides present and their destination ranges overlap (n < 4h + 2c): one launch per side, in order.
HaloPlan buildHaloFoldPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                           const int32_t* pad, int centering, bool negate, bool clear, bool self_exchange = false);

// Multi-field halo UPDATE along `dim` (include/cudecomp_halo_fields.h has the contract): `n_fields` pencils of one descriptor, axis,
// halos and padding updated by one exchange.  Derived from buildHaloPlan(..., force_packed = true for n_fields >= 2): its refusals,
// neighbours, faces and "which cells" hold by construction.  Kinds: NONE, SELF_PERIODIC (the two wrap copies, pencil -> pencil,
// carried out for every field) or PACKED -- never DIRECT for n_fields >= 2: one message per direction is the point, and the
// exchange describes one contiguous piece per direction.  The moves are those of field 0 (HaloOp::n_fields says of how many): an end
// in BUF_IN is "field f's pencil" at the same offset, an end in BUF_WORK lies at its offset + f * face_elements.  Workspace: [send low | send high |
// recv low | recv high], each slot slot_elements = alignElements(n_fields * face_elements) long -- never more than n_fields times
// haloWorkspaceElements.  Neighbours along `dim` share the extents of the other two dims, so the slot size and the offsets are the
// same on both ends of every exchange (the one-sided transport needs that).  The exchange moves n_fields * face_elements elements
// per direction, from send_off[i] to the neighbour's recv_off[1 - i].  n_fields == 1: the plan of buildHaloPlan with the caller's
// force_packed, unchanged.
HaloPlan buildHaloFieldsPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                             const int32_t* pad, int n_fields, bool force_packed, bool self_exchange = false);

// Multi-field halo ACCUMULATION along `dim` (include/cudecomp_halo_accumulate_fields.h has the contract): `n_fields` pencils of one
// descriptor, axis, halos and padding accumulated by one exchange, with (`clear`) or without the clearing of the ghost cells read.
// Derived from buildHaloAccumulatePlan / buildHaloAccumulateClearPlan: refusals, neighbours, slabs, `ordered` and the add / take
// flags of the moves are the single call's by construction.  Kinds: NONE, SELF_PERIODIC (the two wrap additions, pencil -> pencil,
// carried out for every field) or PACKED.  The moves are those of field 0 under the slot layout of buildHaloFieldsPlan:
// an end in BUF_IN is "field f's pencil" at the same offset, an end in BUF_WORK lies at its offset + f * face_elements; workspace
// [send low | send high | recv low | recv high], each slot slot_elements = alignElements(n_fields * face_elements) long; the
// exchange moves n_fields * face_elements elements per direction, from send_off[i] to the neighbour's recv_off[1 - i].
// n_fields == 1: the single plan, unchanged.
HaloPlan buildHaloAccumulateFieldsPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                       const int32_t* pad, int n_fields, bool clear, bool self_exchange = false);

// Multi-field wall halos along `dim` (include/cudecomp_halo_wall_fields.h has the contract): the REFLECTION (`fold` false) or the
// FOLD of `n_fields` pencils of one descriptor, axis, halos, padding and centering, each with a parity of its own.  Derived from
// buildHaloReflectPlan / buildHaloFoldPlan: refusals, sides, "which cells" and `ordered` are the single call's by construction.
// Kinds: NONE or SELF_PERIODIC ("local").  The moves in `pre` are those of FIELD 0 -- an end in BUF_IN is "field f's pencil" at the
// same offset -- and carry NO sign (Move3D::negate false, HaloOp::negate false): the parities are no part of the plan, they reach
// the launcher with the call as a mask of the fields with parity -1 (HaloCall::fields_neg), so that one plan serves every
// combination of them.  n_fields == 1: not this builder -- the single plans, which carry their sign.
HaloPlan buildHaloWallFieldsPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods,
                                 const int32_t* pad, bool fold, int centering, bool clear, int n_fields, bool self_exchange = false);

// The plan of the halo call `op`, by the builder of its family: UPDATE buildHaloFieldsPlan, ACCUMULATE buildHaloAccumulateFieldsPlan
// (one field: the single plans, unchanged), REFLECT and FOLD their own for one field and buildHaloWallFieldsPlan for several, FILL,
// WALL_VALUES and WALL_PLANES their own.  `force_packed` reaches the builders that take it.
HaloPlan buildHaloOpPlan(const GridShape& g, int rank, int axis, int dim, const int32_t* halo, const bool* periods, const int32_t* pad,
                         const HaloOp& op, bool force_packed, bool self_exchange = false);

// Number of stages every member of the communicator arrives at without talking: at most `wanted`, at most the smallest
// chunk extent, at most 14 (flag steps), and no stage smaller than `min_stage_bytes` of the largest pencil (below that the extra
// launches cost more than the overlap gains).
int stageCount(const TransposePlan& p, int wanted, int es, i64 min_stage_bytes = (i64)8 << 20);

// range k of K (equal parts, the remainder spread over the first ranges) of the extent of `m` along global axis `axis`
Move3D stageOfMove(const Move3D& m, int axis, int k, int K);

// canonical form used by the kernel layer: unit-extent dims dropped, mergeable dims fused, dims
// ordered by source stride.  Returns the number of remaining dims (0..3).
int normalizeMove(Move3D& m);

}  // namespace cudecomp
