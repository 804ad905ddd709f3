// peer_context.h -- what the transport sources share (transport.cc, peer_context.cc, workspace.cc, peer_exchange.cc,
// peer_diag.cc): the RCCL communicator, the registry behind the one-sided transport and the helpers of its exchanges.
// The rest of the library includes transport.h.
#pragma once
#include <rccl/rccl.h>

#include <atomic>
#include <cstring>

#include "errors.h"
#include "transport.h"

namespace cudecomp {

// the RCCL communicator over all ranks of a handle
class RcclContext {
 public:
  explicit RcclContext(cudecompHandle_t h) {
    ncclUniqueId id;
    std::memset(&id, 0, sizeof(id));
    if (h->rank == 0) CD_CHECK_RCCL(ncclGetUniqueId(&id));
    h->boot->bcast(&id, sizeof(id), 0);
    CD_CHECK_RCCL(ncclCommInitRank(&comm_, h->nranks, id, h->rank));
  }
  ~RcclContext() {
    if (comm_) ncclCommDestroy(comm_);
  }
  ncclComm_t comm() const { return comm_; }

 private:
  ncclComm_t comm_ = nullptr;
};

// PEER: IPC-mapped buffers + one-sided xGMI copies, ordered ON THE STREAM by flags in a shared board
//
// Platform quirk (ROCm 7.x, dmabuf IPC): hipIpcOpenMemHandle never returns for an allocation whose byte size has
// bit 31 set (2-4 GiB, 6-8 GiB, ...); every other size maps and transfers correctly (verified block by block with
// cudecompExtPeerProbe up to 17 GiB).  Library allocations are rounded up past such sizes; foreign buffers of
// such a size are reported as not mappable instead of hanging.
inline bool ipcSizeHangs(size_t bytes) { return (bytes & 0x80000000ull) != 0; }
inline size_t ipcSafeSize(size_t bytes) { return ipcSizeHangs(bytes) ? ((bytes >> 32) + 1) << 32 : bytes; }

using u64 = unsigned long long;
struct BufDesc;  // peer_context.cc: what a rank tells the other members of a communicator about one buffer of the current call
struct Mail;     // peer_context.cc: a rank's descriptors of one call, in the shared board
constexpr int kMailBufs = 2;

class PeerContext {
 public:
  struct Region {
    int64_t id = -1;
    char* base = nullptr;
    size_t bytes = 0;
    std::vector<char*> peer_base;  // by global rank; [my rank] = base
  };
  static constexpr int kSlots = 256;

  explicit PeerContext(cudecompHandle_t h);  // collective over the handle's communicator
  ~PeerContext();

  bool hasBoard() const { return board_ != nullptr; }

  // ---- library regions (cudecompMalloc): mapped into every rank of the node at allocation -------------------
  Region* find(const void* ptr);
  // collective over the handle's communicator
  // `stale` (optional): set when some member's NEW mapping of a peer's buffer does not lead to that buffer (page tags do
  // not read back); the region is then not registered and nullptr is returned -- agreed by all ranks.
  Region* registerRegion(void* base, size_t bytes, bool* stale = nullptr);
  void unregisterRegion(void* base);  // collective

  // ---- pool of released regions ---------------------------------------------------------------------------------
  // cudecompFree parks a library region -- allocation AND the peers' mappings stay -- and cudecompMalloc hands it out
  // again for requests it fits.  Two reasons: mapping a buffer into every rank of the node is the expensive part of
  // cudecompMalloc, and re-creating allocations is what exposes the platform's stale-IPC-mapping behaviour (DESIGN.md
  // section 9).  Every rank sees the same sequence of (collective) malloc / free calls with the same (max-reduced)
  // sizes, so the pools are identical everywhere and so is every decision taken from them.
  void* takeFromPool(size_t bytes);
  // returns the regions that must really be released now (oldest first) to stay under the pool's limit
  std::vector<void*> park(void* base);
  bool poolEnabled() const { return pool_limit_ > 0; }
  // The pools and their eviction lists must be identical on every rank (park / take decisions involve collectives): the
  // limit each rank derived from ITS device (or environment) is replaced by the smallest one.  Collective; called once,
  // when the transport comes up, before any park or take.
  void agreePoolLimit();
  size_t poolBytes() const { return pool_bytes_; }
  // Retired mappings of re-created user buffers (see map()) each keep the exporter's FREED memory referenced: keep the
  // newest `keep`, close the older ones.  Called where every rank has drained its device and nothing is being imported
  // (grid descriptor destruction), never right before an import -- that is the sequence section 9 A warns about.
  void trimRetiredImports(size_t keep);
  size_t retiredImports() const { return retired_imports_.size(); }
  std::vector<void*> drainPool();
  int64_t poolHits() const { return pool_hits_; }
  int64_t staleMappingsSeen() const { return stale_mappings_seen_; }

  // ---- host barrier among the members of a row / column communicator (set-up paths, probes) ---------------
  void barrier(cudecompCommInfo& ci);

  // ---- device view of the board ----------------------------------------------------------------------
  // The board is registered with the HIP runtime on first use (geometry-only runs never touch a device).
  void ensureDeviceView();
  bool usable(const cudecompCommInfo& ci) const { return board_ && ci.ngroups == 1 && ci.barrier_slot >= 0; }

  // Where the flags live.  Board mode (fallback): row `rank` of the host-pinned board holds ready[rank] and
  // landed[rank][*]; everybody polls and writes host memory (about 8 us per flag round trip between processes).
  // Device mode: every rank owns a small UNCACHED device buffer, IPC-mapped into all ranks of the node once, when the
  // transport comes up; a flag is always POLLED in the poller's own HBM and WRITTEN into the poller's buffer by whoever
  // raises it (one posted store over xGMI) -- the counterpart of the reference's NVSHMEM signals in the symmetric heap
  // (include/internal/cudecomp_kernels.cuh:51-84).  Row layout per slot: ready_from[nranks], landed[landed_n].
  //   dReady(slot, r)        address I poll to see rank r's "begun" flag
  //   dReadyAt(slot, m)      address rank m polls to see MINE (written by my epoch kernel)
  //   dLanded(slot, dst, i)  landed flag i of rank dst: polled by dst (dst == me: local), written by the sender
  u64* dReady(int slot, int rank) {
    if (flag_base_.empty()) return reinterpret_cast<u64*>(dboard_ + flagRowOff(slot, rank));
    return flag_base_[h_->rank] + (size_t)slot * flagRowWords() + rank;
  }
  u64* dReadyAt(int slot, int at_rank) {
    if (flag_base_.empty()) return reinterpret_cast<u64*>(dboard_ + flagRowOff(slot, h_->rank));
    return flag_base_[at_rank] + (size_t)slot * flagRowWords() + h_->rank;
  }
  u64* dLanded(int slot, int dst, int idx) {
    if (flag_base_.empty()) return reinterpret_cast<u64*>(dboard_ + flagRowOff(slot, dst)) + 1 + idx;
    return flag_base_[dst] + (size_t)slot * flagRowWords() + h_->nranks + idx;
  }
  bool deviceFlags() const { return !flag_base_.empty(); }

  // collective over the handle's communicator (called when the transport comes up on a job that has devices)
  void setupDeviceFlags();
  u64* dStatus() { return reinterpret_cast<u64*>(dboard_ + status_off_ + (size_t)h_->rank * 64); }
  // a wait kernel of an earlier call gave up: report it now (the data of that call is incomplete)
  void checkStatus();

  // Device call counter of a communicator: one cell per board row (slot) in a slab that lives as long as this context.
  // The cells used to be a hipMalloc / hipFree per communicator, so a communicator created right after another one was
  // destroyed got the SAME address back -- and with several processes on one GPU a compute die can keep serving a re-allocated
  // address's previous life (found on the test programs' data buffers).  A call counter read stale would
  // put a rank's call numbers out of step with its peers' and let flags of earlier calls satisfy its waits.  Never observed
  // (round 6 suspected it for a failure that turned out to be a test's own race, profiles/r06_pooled_suite_failure.md); kept
  // as the sturdier design: never re-allocated while the handle lives, uncached (no compute-die cache holds them), written
  // and read with system-scope atomics, and a communicator that takes over a row writes its agreed base into the row's cell.
  u64* devEpoch(cudecompCommInfo& ci);

  // ---- per-call rendezvous: every member publishes where its buffers are, then reads the others' ------------
  // Returns remote[b][m]: the address through which THIS rank writes member m's buffer b (nullptr: not reachable),
  // and flags[b][m] as posted by m.  Blocks the host until every member has ENTERED the same call (not until any
  // GPU work is done).  Handles buffers that are not from cudecompMalloc, at any offset of any allocation, and
  // notices when an allocation was freed and re-created at the same address.
  struct Resolved {
    std::vector<char*> remote[kMailBufs];
    std::vector<uint32_t> flags[kMailBufs], mappable[kMailBufs];
  };
  Resolved rendezvous(cudecompCommInfo& ci, const void* const* ptrs, const uint32_t* flags, int nbuf);

  // symmetric resolution without any host communication: the buffer must come from cudecompMalloc and sit at the same
  // offset of its region on every rank (the contract of the reference's NVSHMEM backends)
  std::vector<char*> symmetric(const cudecompCommInfo& ci, const void* ptr, const char* what);

  hipEvent_t copyEvent(int i);
  hipStream_t copyStream(int i);

  bool debug() const { return debug_; }
  // debugging aid (CUDECOMP_DEBUG_PEER=1): device call counter and the flags of my row, read on the host after a device sync
  void dumpRow(cudecompCommInfo& ci, const char* when);

  // highest counter value any rank may have left in row `slot` that involves me
  uint64_t slotHigh(int slot);

 private:
  Region* findById(int64_t id) {
    auto it = region_by_id_.find(id);
    return it == region_by_id_.end() ? nullptr : find(it->second);
  }
  // Best effort: a process that sees several GPUs (torchrun exposes all of them to every rank) turns on peer access
  // from its device to the others, so kernels and copy engines may address IPC-mapped memory of any of them.
  void enablePeerAccessOnce();
  void spinUntil(std::atomic<uint64_t>& a, uint64_t v, const char* what);
  size_t flagRowWords() const { return (size_t)h_->nranks + landed_n_; }

  // ---- foreign buffers: export on demand, cached per allocation; validated on every call ---------------------
  struct Export {
    size_t bytes = 0;
    unsigned long long buffer_id = 0;
    bool has_id = false;
    hipIpcMemHandle_t handle;
  };
  struct Import {
    hipIpcMemHandle_t handle;
    size_t bytes = 0;
    char* mapped = nullptr;
  };
  BufDesc describe(const void* ptr, uint32_t flags);
  char* map(int g, const BufDesc& d);
  void closePeers(Region& r) {
    for (int p = 0; p < (int)r.peer_base.size(); ++p)
      if (p != h_->rank && r.peer_base[p]) (void)hipIpcCloseMemHandle(r.peer_base[p]);
  }

  // ---- board layout ----------------------------------------------------------------------------------------
  //   cells   [kSlots][nranks] x 64 B    host barrier epochs
  //   flags   [kSlots][nranks] rows      u64 ready; u64 landed[max(nranks, 2)]   (row padded to 64 B)
  //   mail    [kSlots][nranks][2]        per-call buffer descriptors, double buffered by call parity
  //   status  [nranks] x 64 B            written by a wait kernel that gave up
  size_t flagRowOff(int slot, int rank) const { return flags_off_ + ((size_t)slot * h_->nranks + rank) * flag_row_bytes_; }
  std::atomic<uint64_t>& cell(int slot, int rank) {
    return *reinterpret_cast<std::atomic<uint64_t>*>(board_ + ((size_t)slot * h_->nranks + rank) * 64);
  }
  Mail& mail(int slot, int rank, int parity);
  void* mapBoard(int fd, size_t bytes);
  void unmapBoard(void* p, size_t bytes);
  void openBoard();

  cudecompHandle_t h_;
  std::map<char*, Region> regions_;
  std::map<int64_t, char*> region_by_id_;
  int64_t next_region_id_ = 0;
  std::map<char*, Export> exports_;
  std::map<std::pair<int, uint64_t>, Import> imports_;
  std::vector<char*> retired_imports_;
  std::vector<hipStream_t> copy_streams_;
  std::vector<hipEvent_t> copy_events_;
  std::vector<u64*> flag_base_;  // device-memory flags: base of every rank's flag buffer as mapped here (empty: board mode)
  u64* flag_mem_ = nullptr;      // my own
  static constexpr int kEpochStride = 8;  // u64 words between the epoch cells of two rows (one 64-byte unit each)
  u64* epoch_slab_ = nullptr;    // the communicators' device call counters, one cell per board row (see devEpoch)
  struct Parked {
    char* base;
    size_t bytes;
  };
  static constexpr int kMaxParked = 32;
  std::vector<Parked> pool_;
  size_t pool_bytes_ = 0, pool_limit_ = 0;
  int64_t pool_hits_ = 0, stale_mappings_seen_ = 0;
  bool verify_mappings_ = true;
  unsigned long long* verify_count_ = nullptr;
  bool peer_access_done_ = false;
  bool debug_ = false;
  bool board_registered_ = false;
  bool board_in_arena_ = false;
  char* board_ = nullptr;
  char* dboard_ = nullptr;
  size_t board_bytes_ = 0, flags_off_ = 0, mail_off_ = 0, status_off_ = 0, flag_row_bytes_ = 0;
  int landed_n_ = 2;
};

// ---- helpers of the exchanges (peer_exchange.cc) ----------------------------------------------------------------------
// the registry of a handle whose communicator `ci` can exchange one-sidedly, with the device view of the board in place
PeerContext& peerOf(cudecompHandle_t h, const cudecompCommInfo& ci);
// one copy into a peer's mapping: copy engines (hipMemcpyAsync; the runtime picks SDMA or a blit kernel from the
// pointers) or the library's own row-copy kernel with write-through stores, one engine per handle
void peerCopy(cudecompHandle_t h, char* dst, const char* src, size_t bytes, hipStream_t stream, int engine = -1);
// a contiguous run of `count` elements at src_off of buffer src_buf -> dst_off of member `peer`'s destination base
Move3D linearMove(BufId src_buf, i64 src_off, i64 dst_off, i64 count, int peer);

// ---- the exchanges transport.cc dispatches to (peer_exchange.cc) ---------------------------------------------------------
// all chunks of the plan at once, between the caller's pack and unpack; `call` = peerBegin's result
void peerAlltoall(cudecompHandle_t h, cudecompCommInfo& ci, const TransposePlan& p, const ExchangeBuffers& b, int es,
                  const PeerCall& call, hipStream_t stream);
// halo faces: peerBegin on the faces' communicator; the one wait for the neighbours' ready flags (returns the event the copy
// streams wait for); the exchange itself (ready_ev null: it places the gate itself, behind whatever `stream` holds)
PeerCall haloBegin(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloExchange& x, cudecompHaloCommBackend_t backend,
                   hipStream_t stream);
hipEvent_t haloReadyGate(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloExchange& x, const PeerCall& call, hipStream_t stream);
void peerHaloExchange(cudecompHandle_t h, cudecompGridDesc_t gd, const HaloExchange& x, const PeerCall& call,
                      hipEvent_t* packed, hipEvent_t ready_ev, hipStream_t stream);

}  // namespace cudecomp
