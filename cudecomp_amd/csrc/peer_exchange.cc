// peer_exchange.cc -- the stream-ordered one-sided exchanges of the PEER transport (transport.h): transposes all at once, fused
// put, two-hop relay and staged pipeline; the halo faces
#include "peer_context.h"

namespace cudecomp {

PeerContext& peerOf(cudecompHandle_t h, const cudecompCommInfo& ci) {
  if (!h->peer) CD_INTERNAL_ERROR("peer transport was not created for this grid descriptor");
  if (!h->peer->usable(ci)) CD_PEER_ERROR("the one-sided transport needs all members of the communicator on one node");
  h->peer->ensureDeviceView();
  return *h->peer;
}

Move3D linearMove(BufId src_buf, i64 src_off, i64 dst_off, i64 count, int peer) {
  Move3D m;
  m.src_buf = src_buf;
  m.src_off = src_off;
  m.dst_off = dst_off;
  m.extent[0] = count;
  m.ss[0] = m.ds[0] = 1;
  m.peer = peer;
  return m;
}

void peerCopy(cudecompHandle_t h, char* dst, const char* src, size_t bytes, hipStream_t stream, int engine) {
  if (bytes == 0) return;
  if (engine < 0) engine = h->peer_copy_engine;
  // (the kernel path moves 4 bytes or more per access: dword-aligned ends only, which 2-byte elements do not guarantee)
  if (engine == 1 && bytes % 4 == 0 && ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 3) == 0) {
    const int es = (bytes % 16 == 0) ? 16 : (bytes % 8 == 0 ? 8 : 4);
    const Move3D m = linearMove(BUF_IN, 0, 0, (i64)(bytes / es), -1);  // (no peer: launchMoves may classify on it)
    void* bufs[3] = {const_cast<char*>(src), nullptr, nullptr};
    void* dst_base[1] = {dst};
    launchMoves(&m, 1, bufs, es, stream, &h->tuning, nullptr, dst_base);
    return;
  }
  CD_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, stream));
}

// ------------------------------------------------------------------------------------------------
// stream-ordered one-sided exchanges
// ------------------------------------------------------------------------------------------------
// Every call on a communicator has a number (epoch), kept in device memory and advanced by the first kernel of the
// call.  Flags in the shared board carry epochs:
//   ready[r]        last call for which r's stream has reached the exchange: everything r enqueued earlier is done,
//                   so r's receive area (or output pencil) may be overwritten
//   landed[d][s]    last call whose data from s has completely arrived at d
// A sender waits for ready[d] -- once per call, on the caller's stream (peerReadyGate) or in front of its put kernel --
// moves the data, then raises landed[d][me]; a receiver waits for landed[me][s] in front of its unpack.  The step values
// (k + 1 for stage k, kFlagDone for the last) and the event indices ([0, P) copies, 2P go, 2P+1 halo ready, 2P+2+k packed)
// are fixed; peerBegin comes before the packs.  Nothing blocks the host, and because the
// epoch lives on the device the whole sequence can be captured into a hipGraph and replayed.
// Reference counterpart: the NVSHMEM signal / wait choreography, include/internal/comm_routines.h:122-258 and
// include/internal/cudecomp_kernels.cuh:51-122.

PeerCall peerBegin(cudecompHandle_t h, cudecompCommInfo& ci, bool rendezvous, const void* recv_area, const void* output,
                   bool want_direct, hipStream_t stream) {
  PeerContext& pc = peerOf(h, ci);
  pc.checkStatus();
  PeerCall call;
  call.nranks = ci.nranks;
  if (rendezvous) {
    // (host code only: under stream capture it runs once, at capture time, like every pointer in the graph)
    // Direct put: only into output pencils that come from cudecompMalloc.  Those were mapped into every rank when
    // they were allocated, collectively and once; mapping arbitrary user allocations on the fly proved fragile on
    // this platform (an allocation that is freed and re-created at the same address cannot always be re-imported by
    // a peer that still remembers its predecessor), and a transpose must not depend on that.
    const bool out_ok = want_direct && pc.find(output) != nullptr;
    const void* ptrs[2] = {recv_area, out_ok ? output : nullptr};
    const uint32_t flags[2] = {0, out_ok ? 1u : 0u};
    auto res = pc.rendezvous(ci, ptrs, flags, want_direct ? 2 : 1);
    call.remote_recv = res.remote[0];
    // every member wants it and every member's output is a library region -- all ranks read the same mailboxes, so
    // all of them reach the same verdict
    call.direct = want_direct;
    if (want_direct) {
      call.remote_out = res.remote[1];
      for (int m = 0; m < ci.nranks; ++m)
        if (!res.flags[1][m] || !res.mappable[1][m] || !call.remote_out[m]) call.direct = false;
    }
    if (!call.direct)
      for (int m = 0; m < ci.nranks; ++m)
        if (!call.remote_recv[m])
          CD_PEER_ERROR("the workspace of a peer rank cannot be mapped over IPC (an allocation of 2-4 GiB, 6-8 GiB, ... cannot "
                        "be shared on this platform, nor can memory that is not a device allocation, nor -- reliably -- a "
                        "buffer that was freed and re-created at the same address): obtain it from cudecompMalloc");
  } else {
    call.remote_recv = pc.symmetric(ci, recv_area, "the workspace");
    call.direct = false;
  }
  call.epoch = pc.devEpoch(ci);
  if (pc.debug()) pc.dumpRow(ci, "begin");  // CUDECOMP_DEBUG_PEER=1 (host-synchronous): the row's counters as this call finds them
  FlagList begun;  // "my call has begun": where each member polls it (device flags) / my board cell (board mode)
  if (pc.deviceFlags()) {
    // (my own buffer too: a one-member communicator in the self-exchange test mode waits for itself)
    for (int m = 0; m < ci.nranks; ++m) begun.add(pc.dReadyAt(ci.barrier_slot, ci.global_ranks[m]));
  } else {
    begun.add(pc.dReadyAt(ci.barrier_slot, h->rank));
  }
  launchEpochBegin(call.epoch, begun, stream);
  return call;
}

namespace {

// The flags of one exchange, in the order the kernels walk them: `ready` of every destination (polled here: its receive area
// is free), `landed` at every destination (raised by me), `incoming` from every source (polled here).  Global ranks.
struct ExchangeFlags {
  FlagList ready, landed, incoming;
};
ExchangeFlags exchangeFlags(cudecompHandle_t h, PeerContext& pc, int slot, const std::vector<int>& dst, const std::vector<int>& src) {
  ExchangeFlags f;
  for (int d : dst) {
    f.ready.add(pc.dReady(slot, d));
    f.landed.add(pc.dLanded(slot, d, h->rank));
  }
  for (int s : src) f.incoming.add(pc.dLanded(slot, h->rank, s));
  return f;
}
// steps 1 .. P-1 of a pairwise schedule (entry 0 = self) as global ranks
std::vector<int> scheduleRanks(const cudecompCommInfo& ci, const std::vector<int>& schedule) {
  std::vector<int> ranks;
  for (int j = 1; j < ci.nranks; ++j) ranks.push_back(ci.global_ranks[schedule[j]]);
  return ranks;
}
// every global rank of `ranks` but mine
std::vector<int> allBut(int me, const std::vector<int>& ranks) {
  std::vector<int> others;
  for (int r : ranks)
    if (r != me) others.push_back(r);
  return others;
}

// One wait for "every receiver's receive area is free" on the CALLER's stream, then an event the copy streams wait
// for.  No copy stream ever parks a spinning wait kernel: the runtime multiplexes a process's streams onto a handful
// of hardware queues (GPU_MAX_HW_QUEUES, default 4), and a wait kernel parked on one of them would hold up the copies
// of every stream that shares its queue.  The pipelined exchange calls this right after the FIRST chunk is packed, so
// a receiver that is late delays nothing that could have run.
hipEvent_t peerReadyGate(cudecompHandle_t h, PeerContext& pc, int P, const PeerCall& call, const FlagList& ready, hipStream_t stream) {
  launchWait(call.epoch, ready, pc.dStatus(), h->peer_timeout_s, stream, kFlagBegun);
  hipEvent_t go = pc.copyEvent(2 * P);  // "go": receivers ready
  CD_CHECK_HIP(hipEventRecord(go, stream));
  return go;
}

// The send area as the move kernels address it (bufs[buf] + base elements) and as the copy engines do (send).
struct SendArea {
  void* const* bufs;
  BufId buf;
  i64 base;
  const char* send;
};

// One fan-out: slabs [n*k/K, n*(k+1)/K) of the n = send_n[d] slabs of the chunk for every peer d -- K == 0: the whole chunk --
// travel concurrently, then `step` is raised in the landed flag at every destination.  Copy engines: one hipMemcpyAsync per peer
// on a stream of its own (every link / SDMA queue busy), each followed by its signal.  Compute-unit copies: ONE launch whose
// workgroups serve the destinations round robin feeds every link for the whole launch, on ONE extra stream (a stream per peer
// brings nothing here and costs a hardware queue each), and one signal for all destinations -- issued also when nothing of any
// chunk falls into the range: the receivers wait for every step.  The copy streams wait for the events `packed` and `go` (null:
// not for that one), never for a flag (see peerReadyGate); `record`: leave the closing events joinCopies waits for.
void fanOutChunks(cudecompHandle_t h, PeerContext& pc, int P, const TransposePlan& p, const SendArea& area, int es, const PeerCall& call,
                  const ExchangeFlags& fl, int k, int K, int step, hipEvent_t packed, hipEvent_t go, bool record) {
  // elements [*lo, *lo + *count) of the chunk for member d
  auto range = [&](int d, i64* lo, i64* count) {
    const i64 n = K ? p.send_n[d] : 1, per = p.send_cnt[d] / n;
    *lo = K ? n * k / K * per : 0;
    *count = (K ? n * (k + 1) / K * per : per) - *lo;
  };
  auto waitFor = [&](hipStream_t cs) {
    if (packed) CD_CHECK_HIP(hipStreamWaitEvent(cs, packed, 0));
    if (go) CD_CHECK_HIP(hipStreamWaitEvent(cs, go, 0));
  };
  i64 lo = 0, count = 0;
  if (h->peer_copy_engine == 1 && P > 1) {
    hipStream_t cs = pc.copyStream(0);
    waitFor(cs);
    std::vector<Move3D> moves;
    std::vector<void*> dst_base;
    for (int j = 1; j < P; ++j) {
      const int d = p.schedule_dst[j];
      range(d, &lo, &count);
      if (count == 0) continue;
      moves.push_back(linearMove(area.buf, area.base + p.send_off[d] + lo, p.remote_recv_off[d] + lo, count, d));
      dst_base.push_back(call.remote_recv[d]);
    }
    if (!moves.empty()) launchMoves(moves.data(), (int)moves.size(), area.bufs, es, cs, &h->tuning, nullptr, dst_base.data());
    launchSignal(call.epoch, fl.landed, cs, step);
    if (record) CD_CHECK_HIP(hipEventRecord(pc.copyEvent(0), cs));
    return;
  }
  for (int j = 1; j < P; ++j) {
    const int d = p.schedule_dst[j];
    hipStream_t cs = pc.copyStream(j);
    waitFor(cs);
    range(d, &lo, &count);
    peerCopy(h, call.remote_recv[d] + (p.remote_recv_off[d] + lo) * es, area.send + (p.send_off[d] + lo) * es, (size_t)count * es, cs);
    FlagList landed;
    landed.add(fl.landed.f[j - 1]);
    launchSignal(call.epoch, landed, cs, step);
    if (record) CD_CHECK_HIP(hipEventRecord(pc.copyEvent(j), cs));
  }
}

// `stream` continues when every outgoing copy is done (the send area may be reused): the closing events of fanOutChunks
void joinCopies(cudecompHandle_t h, PeerContext& pc, int P, hipStream_t stream) {
  if (h->peer_copy_engine == 1 && P > 1) CD_CHECK_HIP(hipStreamWaitEvent(stream, pc.copyEvent(0), 0));
  else
    for (int j = 1; j < P; ++j) CD_CHECK_HIP(hipStreamWaitEvent(stream, pc.copyEvent(j), 0));
}

// my own chunk never leaves the device: a local copy (reference: comm_routines.h:405-410), or through the engine under test
void copySelfChunk(cudecompHandle_t h, const TransposePlan& p, const ExchangeBuffers& b, int es, hipStream_t stream, int engine) {
  const int me = p.comm_rank;
  if (p.send_cnt[me])
    peerCopy(h, b.recv + p.recv_off[me] * es, b.send + p.send_off[me] * es, (size_t)p.send_cnt[me] * es, stream, engine);
}

}  // namespace

// All chunks at once: they are packed (caller), the receivers' ready flags are awaited ONCE on `stream` (peerReadyGate), then
// the P-1 chunks travel concurrently (fanOutChunks).  `stream` continues when every incoming chunk has landed and every outgoing
// copy is done (the send area may be reused).
void peerAlltoall(cudecompHandle_t h, cudecompCommInfo& ci, const TransposePlan& p, const ExchangeBuffers& b, int es,
                  const PeerCall& call, hipStream_t stream) {
  PeerContext& pc = peerOf(h, ci);
  const int P = ci.nranks;
  const ExchangeFlags fl = exchangeFlags(h, pc, ci.barrier_slot, scheduleRanks(ci, p.schedule_dst), scheduleRanks(ci, p.schedule_src));
  hipEvent_t go = peerReadyGate(h, pc, P, call, fl.ready, stream);  // chunks packed, receivers ready
  void* bufs[3] = {b.send, nullptr, nullptr};
  fanOutChunks(h, pc, P, p, SendArea{bufs, BUF_IN, 0, b.send}, es, call, fl, 0, 0, kFlagDone, nullptr, go, true);
  copySelfChunk(h, p, b, es, stream, h->self_exchange ? -1 : 0);
  joinCopies(h, pc, P, stream);
  launchWait(call.epoch, fl.incoming, pc.dStatus(), h->peer_timeout_s, stream);
}

// "SM"-style exchange (NVSHMEM_SM enum): the pack kernels write each chunk straight into the receiver's memory over
// xGMI -- one launch feeds all links at once, and the send area, the copy engines and one full HBM pass disappear.
// With call.direct the destination is the receiver's OUTPUT pencil in its final layout and the unpack pass
// disappears as well: one read and one write per element for the whole transpose.  The reference's counterpart is the
// NVSHMEM block-put kernel (include/internal/cudecomp_kernels.cuh:86-122); here it is the ordinary move kernel with
// remote destinations and write-through stores.
void peerPutExchange(cudecompHandle_t h, cudecompCommInfo& ci, const TransposePlan& p, void* const bufs[3], int es,
                     const PeerCall& call, hipStream_t stream) {
  PeerContext& pc = peerOf(h, ci);
  const int P = ci.nranks;
  const ExchangeFlags fl = exchangeFlags(h, pc, ci.barrier_slot, allBut(h->rank, ci.global_ranks), allBut(h->rank, ci.global_ranks));
  launchWait(call.epoch, fl.ready, pc.dStatus(), h->peer_timeout_s, stream, kFlagBegun);  // every destination may be written
  std::vector<Move3D> moves;
  std::vector<void*> dst_base;
  if (call.direct) {
    for (const Move3D& m : p.direct) {
      moves.push_back(m);
      dst_base.push_back(call.remote_out[m.peer]);
    }
  } else if (!p.pack.empty()) {
    for (const Move3D& m : p.pack) {
      Move3D r = m;
      r.dst_off = p.remote_recv_off[m.peer];
      moves.push_back(r);
      dst_base.push_back(call.remote_recv[m.peer]);
    }
  } else {  // chunks already sit packed in the send buffer (skip-pack plans): plain copies to the peers
    for (int j = 0; j < P; ++j) {
      const int d = p.schedule_dst[j];
      moves.push_back(linearMove(p.send_buf, p.send_base + p.send_off[d], p.remote_recv_off[d], p.send_cnt[d], d));
      dst_base.push_back(call.remote_recv[d]);
    }
  }
  launchMoves(moves.data(), (int)moves.size(), bufs, es, stream, &h->tuning, nullptr, dst_base.data());
  launchSignal(call.epoch, fl.landed, stream);
  launchWait(call.epoch, fl.incoming, pc.dStatus(), h->peer_timeout_s, stream);
}

// ---- two-hop relay (plan.h RelayPlan) -----------------------------------------------------------
bool peerRelayApplies(cudecompHandle_t h, cudecompGridDesc_t gd, const TransposePlan& plan, cudecompTransposeCommBackend_t backend) {
  if (!h->two_hop_relay || backend != CUDECOMP_TRANSPOSE_COMM_NVSHMEM || !plan.exchange || h->self_exchange) return false;
  if (!relayWorthwhile(plan.nranks, h->nranks)) return false;
  // flags of a communicator of all ranks, all of them on this node and on the shared board
  return h->peer && gd->world.nranks == h->nranks && h->nranks <= kMaxFlags && h->peer->usable(gd->world);
}

bool peerRelayEnsureRegion(cudecompHandle_t h, const RelayPlan& rp, int es) {
  // the same number on every rank (it is derived from the whole decomposition), so this is collective by construction
  const size_t need = (size_t)rp.relayElements() * es;
  if (h->relay_buf && h->relay_bytes >= need) return true;
  if (h->relay_buf) {
    // Regrowing: my previous relayed call (possibly on another stream) and my peers' previous scatters into the region must be
    // over before it goes away.  Mine: the event every relayed call ends with (never recorded if that call threw before
    // its end -- a deliberate no-op then); the peers': a barrier after everybody has waited for its own.
    if (h->relay_last_call) CD_CHECK_HIP(hipEventSynchronize(h->relay_last_call));
    h->boot->barrier();
    workspaceFreeRaw(h, h->relay_buf);
  }
  h->relay_buf = nullptr;
  h->relay_bytes = 0;
  void* p = workspaceAllocRaw(h, need, true);
  PeerContext::Region* r = h->peer->find(p);
  bool ok = r != nullptr;
  for (int g = 0; ok && g < h->nranks; ++g) ok = r->peer_base[g] != nullptr;
  if (h->boot->allreduceOr(!ok)) {
    // agreed by all ranks: the relay is off for this handle from here on (no retry per call), exchanges go direct
    workspaceFreeRaw(h, p);
    h->two_hop_relay = false;
    if (h->rank == 0)
      fprintf(stderr, "CUDECOMP:WARN: the relay region of the two-hop exchange could not be mapped into every rank of the node; "
                      "CUDECOMP_TWO_HOP_RELAY is off for this handle.\n");
    return false;
  }
  h->relay_buf = p;
  h->relay_bytes = need;
  return true;
}

void peerRelayAlltoall(cudecompHandle_t h, cudecompCommInfo& world, const TransposePlan& p, const RelayPlan& rp,
                       const ExchangeBuffers& b, int es, const PeerCall& call, hipStream_t stream) {
  PeerContext& pc = peerOf(h, world);
  const int n = world.nranks, me = h->rank, slot = world.barrier_slot;
  PeerContext::Region* rr = pc.find(h->relay_buf);
  if (!rr) CD_INTERNAL_ERROR("two-hop relay without its relay region");
  std::vector<int> others;
  for (int q = 0; q < n; ++q)
    if (q != me) others.push_back(q);
  const ExchangeFlags fl = exchangeFlags(h, pc, slot, others, others);
  // every rank has begun this call: its relay slots (forwarded in its previous call, earlier on its stream) and its
  // receive area are free
  launchWait(call.epoch, fl.ready, pc.dStatus(), h->peer_timeout_s, stream, kFlagBegun);
  auto run = [&](const std::vector<RelayMove>& list, char* src_base) {
    std::vector<Move3D> moves;
    std::vector<void*> dst_base;
    for (const RelayMove& m : list) {
      moves.push_back(linearMove(BUF_IN, m.src_off, m.dst_off, m.count, m.dst_rank));
      dst_base.push_back(m.to_relay ? rr->peer_base[m.dst_rank] : call.remote_recv[m.dst_rank]);
    }
    void* bufs[3] = {src_base, nullptr, nullptr};
    if (!moves.empty()) launchMoves(moves.data(), (int)moves.size(), bufs, es, stream, &h->tuning, nullptr, dst_base.data());
  };
  // step 1: my slices to the relays (and the two direct slices of every chunk to its destination)
  run(rp.scatter, b.send);
  launchSignal(call.epoch, fl.landed, stream, 1);
  copySelfChunk(h, p, b, es, stream, 0);
  // step 2: what the others parked in my relay region goes on to its destinations
  launchWait(call.epoch, fl.incoming, pc.dStatus(), h->peer_timeout_s, stream, 1);
  run(rp.forward, static_cast<char*>(h->relay_buf));
  launchSignal(call.epoch, fl.landed, stream, kFlagDone);
  // everybody's direct slices (done before their step-1 signal) and forwards have reached my receive area
  launchWait(call.epoch, fl.incoming, pc.dStatus(), h->peer_timeout_s, stream, kFlagDone);
}

bool peerPipelineAvailable(cudecompHandle_t h, const cudecompCommInfo& ci) { return h->peer && h->peer->usable(ci); }

// Staged pipeline of the one-sided transport (NVSHMEM_PL / MPI_P2P_PL enums).
//
// The reference pipelines PER PEER (comm_routines.h:427-631, transpose.h:470-513, 683-744): one peer's chunk is packed,
// sent and unpacked after the other.  On a full xGMI mesh that is the wrong unit: every peer has a link of its own, so a
// per-peer pipeline keeps one link busy at a time while the others wait for their turn, and each per-peer unpack launch
// writes one slice of every destination row (a 2-KiB piece of every 8-KiB row leaves most DRAM channels idle:
// 0.54-0.57 of the HBM peak, profiles/r02_local_phases.json).  Here the pipeline runs over STAGES instead: all chunks
// are cut into K ranges along their slowest wire dim (contiguous sub-chunks in the send and receive areas), and stage k
//   pack(k): one launch, all destinations            [caller's stream, event per stage]
//   send(k): sub-chunk k to EVERY peer at once        [copy stream(s): all links busy in every stage] + landed = k
//   unpack(k): one launch, all sources, whole rows   [caller's stream, behind a wait for stage k of every source]
// overlaps pack(k+1) with send(k) and send(k+1) with unpack(k).  The receivers' "ready" is awaited once, on the
// caller's stream behind the first pack; no stream ever parks a spinning kernel in front of work that could run.
void peerStagedExchange(cudecompHandle_t h, cudecompCommInfo& ci, const TransposePlan& plan, void* const bufs[3],
                        const ExchangeBuffers& b, int es, const PeerCall& call, hipStream_t stream) {
  PeerContext& pc = peerOf(h, ci);
  const int P = plan.nranks, ax = plan.stage_axis;
  const int K = stageCount(plan, h->pipeline_stages, es, h->pipeline_min_stage_bytes);
  auto stepOf = [&](int k) { return k == K - 1 ? kFlagDone : k + 1; };
  // events: [0, P) last copy of each copy stream, 2P "go", then one "packed" event per stage
  auto packedEvent = [&](int k) { return pc.copyEvent(2 * P + 2 + k); };
  const ExchangeFlags fl = exchangeFlags(h, pc, ci.barrier_slot, scheduleRanks(ci, plan.schedule_dst), scheduleRanks(ci, plan.schedule_src));
  const SendArea area{bufs, plan.send_buf, plan.send_base, b.send};
  std::vector<Move3D> moves;
  for (int k = 0; k < K; ++k) {
    // ---- pack stage k (all destinations, self included) on the caller's stream
    if (!plan.pack.empty()) {
      moves.clear();
      for (const Move3D& m : plan.pack) moves.push_back(stageOfMove(m, ax, k, K));
      launchMoves(moves.data(), (int)moves.size(), bufs, es, stream, &h->tuning);
    }
    CD_CHECK_HIP(hipEventRecord(packedEvent(k), stream));
    // ---- send stage k to every peer; receivers ready? (once, behind the first pack)
    hipEvent_t go = k == 0 ? peerReadyGate(h, pc, P, call, fl.ready, stream) : nullptr;
    fanOutChunks(h, pc, P, plan, area, es, call, fl, k, K, stepOf(k), packedEvent(k), go, k == K - 1);
  }
  copySelfChunk(h, plan, b, es, stream, h->self_exchange ? -1 : 0);
  // ---- unpack stage by stage: every source's sub-chunk k has landed -> one launch that writes whole rows
  for (int k = 0; k < K; ++k) {
    launchWait(call.epoch, fl.incoming, pc.dStatus(), h->peer_timeout_s, stream, stepOf(k));
    moves.clear();
    for (const Move3D& m : plan.unpack) moves.push_back(stageOfMove(m, ax, k, K));
    if (!moves.empty()) launchMoves(moves.data(), (int)moves.size(), bufs, es, stream, &h->tuning);
  }
  joinCopies(h, pc, P, stream);  // send area reusable
}

// ================================================================================================
// halo faces
// ================================================================================================
// resolves where my two faces land: remote[i] = address of neighbour i's halo slot (1 - i) as written by me
PeerCall haloBegin(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloExchange& x, cudecompHaloCommBackend_t backend,
                   hipStream_t stream) {
  cudecompCommInfo& ci = gd->comm(x.comm_axis);
  // the NVSHMEM enums require a symmetric workspace from cudecompMalloc (as in the reference); the MPI enums take any
  // device buffer and pay a host rendezvous per call (the reference's MPI backends block the host as well)
  return peerBegin(h, ci, !haloBackendIsPeer(backend), x.recv, nullptr, false, stream);
}

namespace {
int memberOf(const cudecompCommInfo& ci, int global_rank) {
  for (int m = 0; m < ci.nranks; ++m)
    if (ci.global_ranks[m] == global_rank) return m;
  CD_INTERNAL_ERROR("halo neighbour is not a member of the exchanging communicator");
}
}  // namespace

// one wait for both neighbours' "my halo slots are free" on the caller's stream; returns the event the copy streams
// wait for (no copy stream parks a wait kernel, see peerReadyGate)
hipEvent_t haloReadyGate(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloExchange& x, const PeerCall& call, hipStream_t stream) {
  cudecompCommInfo& ci = gd->comm(x.comm_axis);
  PeerContext& pc = peerOf(h, ci);
  FlagList both;
  for (int i = 0; i < 2; ++i)
    if (x.neighbor[i] != -1 && (i == 0 || x.neighbor[1] != x.neighbor[0])) both.add(pc.dReady(ci.barrier_slot, x.neighbor[i]));
  launchWait(call.epoch, both, pc.dStatus(), h->peer_timeout_s, stream, kFlagBegun);
  hipEvent_t ready_ev = pc.copyEvent(2 * ci.nranks + 1);
  CD_CHECK_HIP(hipEventRecord(ready_ev, stream));
  return ready_ev;
}

// faces -> neighbours' halo slots.  packed[i] (may be null: face data ready on `stream` already) gates face i.
// Slot i of mine is filled by neighbour i, who raises landed[me][i]; I fill slot 1-i of neighbour i.
void peerHaloExchange(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloExchange& x, const PeerCall& call,
                      hipEvent_t* packed, hipEvent_t ready_ev, hipStream_t stream) {
  cudecompCommInfo& ci = gd->comm(x.comm_axis);
  PeerContext& pc = peerOf(h, ci);
  // plain sequence (packed == nullptr): the gate comes after both packs, then the two copies fan out;
  // overlapped sequence: the caller placed it behind the first pack, each face also waits for its own pack
  if (!ready_ev) ready_ev = haloReadyGate(h, gd, x, call, stream);
  FlagList incoming;
  const bool one_stream = h->peer_copy_engine == 1;  // kernel copies: both faces share one extra stream (see fanOutChunks)
  for (int i = 0; i < 2; ++i) {
    if (x.neighbor[i] == -1) continue;
    const int m = memberOf(ci, x.neighbor[i]);
    hipStream_t cs = pc.copyStream(one_stream ? 0 : i);
    if (packed) CD_CHECK_HIP(hipStreamWaitEvent(cs, packed[i], 0));
    CD_CHECK_HIP(hipStreamWaitEvent(cs, ready_ev, 0));
    FlagList landed;
    landed.add(pc.dLanded(ci.barrier_slot, x.neighbor[i], 1 - i));
    peerCopy(h, call.remote_recv[m] + x.remote_off[i], x.send + x.send_off[i], (size_t)x.bytes, cs);
    launchSignal(call.epoch, landed, cs);
    CD_CHECK_HIP(hipEventRecord(pc.copyEvent(i), cs));
    incoming.add(pc.dLanded(ci.barrier_slot, h->rank, i));
  }
  for (int i = 0; i < 2; ++i)
    if (x.neighbor[i] != -1) CD_CHECK_HIP(hipStreamWaitEvent(stream, pc.copyEvent(i), 0));
  launchWait(call.epoch, incoming, pc.dStatus(), h->peer_timeout_s, stream);
}

}  // namespace cudecomp
