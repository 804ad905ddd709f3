// peer_context.cc -- PeerContext (peer_context.h): IPC region registry, workspace pool, shared board, device flags, per-call
// rendezvous, copy streams and events of the one-sided transport
#include "peer_context.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <thread>

#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>

namespace cudecomp {

// what a rank tells the other members of a communicator about one buffer of the current call
struct BufDesc {
  uint64_t offset;       // of the buffer inside its region / allocation
  uint64_t alloc_base;   // foreign buffers: identity of the allocation in the owner's address space
  uint64_t alloc_bytes;
  int64_t region_id;     // >= 0: library region (mapped everywhere since cudecompMalloc); -1: foreign allocation
  uint32_t mappable;     // 0: the owner could not export it
  uint32_t flags;        // call-specific bits
  hipIpcMemHandle_t handle;
};
struct Mail {
  std::atomic<uint64_t> seq;
  uint64_t nbuf;
  BufDesc buf[kMailBufs];
};
constexpr size_t kMailBytes = (sizeof(Mail) + 63) / 64 * 64;

PeerContext::PeerContext(cudecompHandle_t h) : h_(h) {
  debug_ = std::getenv("CUDECOMP_DEBUG_PEER") != nullptr;
  // CUDECOMP_WORKSPACE_POOL_MIB: how much released workspace memory stays parked (0 = none: every cudecompFree really
  // frees); default 1/8 of the device's memory, at most 32 GiB.  CUDECOMP_VERIFY_IPC_MAPPINGS=0 skips the page tags.
  pool_limit_ = (size_t)32 << 30;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) pool_limit_ = std::min(pool_limit_, total_b / 8);
  else (void)hipGetLastError();
  if (const char* v = std::getenv("CUDECOMP_WORKSPACE_POOL_MIB")) pool_limit_ = (size_t)std::strtoull(v, nullptr, 10) << 20;
  if (const char* v = std::getenv("CUDECOMP_VERIFY_IPC_MAPPINGS")) verify_mappings_ = std::strtol(v, nullptr, 10) != 0;
  openBoard();
}

PeerContext::~PeerContext() {
  if (board_registered_) (void)hipHostUnregister(board_);
  if (board_) unmapBoard(board_, board_bytes_);
  for (auto& kv : regions_) closePeers(kv.second);
  for (auto& pk : pool_) (void)hipFree(pk.base);  // parked workspaces: released with the library
  for (auto& kv : imports_)
    if (kv.second.mapped) (void)hipIpcCloseMemHandle(kv.second.mapped);
  for (char* q : retired_imports_) (void)hipIpcCloseMemHandle(q);
  for (int p = 0; p < (int)flag_base_.size(); ++p)
    if (p != h_->rank && flag_base_[p]) (void)hipIpcCloseMemHandle(flag_base_[p]);
  if (flag_mem_) (void)hipFree(flag_mem_);
  if (epoch_slab_) (void)hipFree(epoch_slab_);
  if (verify_count_) (void)hipFree(verify_count_);
  for (hipStream_t s : copy_streams_) (void)hipStreamDestroy(s);
  for (hipEvent_t e : copy_events_) (void)hipEventDestroy(e);
  (void)hipGetLastError();
}

PeerContext::Region* PeerContext::find(const void* ptr) {
  const char* p = static_cast<const char*>(ptr);
  auto it = regions_.upper_bound(const_cast<char*>(p));
  if (it == regions_.begin()) return nullptr;
  --it;
  Region& r = it->second;
  return (p >= r.base && p < r.base + r.bytes) ? &r : nullptr;
}

PeerContext::Region* PeerContext::registerRegion(void* base, size_t bytes, bool* stale) {
  struct Wire {
    hipIpcMemHandle_t handle;
    unsigned long long bytes;
    unsigned long long seed;  // of the page tags the owner stamped into the buffer
    int pid;
  };
  enablePeerAccessOnce();
  if (stale) *stale = false;
  // Failures are agreed on collectively (a rank that threw on its own would leave the others waiting in the
  // next collective): everybody tries, then everybody learns whether anybody failed.
  Wire mine{};
  std::string error;
  hipError_t e = hipIpcGetMemHandle(&mine.handle, base);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    error = std::string("hipIpcGetMemHandle failed: ") + hipGetErrorString(e);
  }
  mine.bytes = error.empty() ? bytes : 0;  // 0 = "I have nothing to offer"
  mine.pid = (int)::getpid();
  // Stamp every page before anybody maps it: an importer that ends up with a mapping of something else (the platform
  // can hand back the mapping of a PREDECESSOR of this allocation) must not go unnoticed.
  mine.seed = ((unsigned long long)mine.pid << 32) ^ (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count() ^
              ((unsigned long long)next_region_id_ << 20);
  if (verify_mappings_ && error.empty()) {
    bool launched = true;
    try {
      launchTagPages(base, bytes, mine.seed, nullptr);
    } catch (const Error&) {  // a local launch failure is agreed on below like every other failure
      launched = false;
    }
    if (!launched || hipDeviceSynchronize() != hipSuccess) {
      (void)hipGetLastError();
      error = "stamping the page tags of a new workspace failed";
      mine.bytes = 0;
    }
  }
  std::vector<Wire> all(h_->nranks);
  h_->boot->allgather(&mine, all.data(), sizeof(Wire));
  Region r;
  r.id = next_region_id_++;  // the same number on every rank: registrations are collective and ordered
  r.base = static_cast<char*>(base);
  r.bytes = bytes;
  r.peer_base.assign(h_->nranks, nullptr);
  for (int p = 0; p < h_->nranks && error.empty(); ++p) {
    if (p == h_->rank) {
      r.peer_base[p] = r.base;
      continue;
    }
    if (h_->hostnames[p] != h_->hostnames[h_->rank]) continue;  // no xGMI path: not mappable
    if (all[p].bytes == 0) {
      error = "a peer rank could not export its buffer over IPC";
      break;
    }
    void* mapped = nullptr;
    e = hipIpcOpenMemHandle(&mapped, all[p].handle, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      error = std::string("hipIpcOpenMemHandle failed: ") + hipGetErrorString(e) +
              " (is HSA_ENABLE_IPC_MODE_LEGACY=0 exported?)";
      break;
    }
    r.peer_base[p] = static_cast<char*>(mapped);
  }
  // read every peer's page tags back through the mapping just made
  bool my_stale = false;
  if (verify_mappings_ && error.empty()) {
    if (!verify_count_) (void)hipMalloc(reinterpret_cast<void**>(&verify_count_), sizeof(unsigned long long));
    for (int p = 0; p < h_->nranks && verify_count_; ++p) {
      if (p == h_->rank || !r.peer_base[p]) continue;
      unsigned long long bad = 0;
      if (hipMemcpy(verify_count_, &bad, sizeof(bad), hipMemcpyHostToDevice) != hipSuccess) break;
      bool launched = true;
      try {
        launchCheckPages(r.peer_base[p], (size_t)all[p].bytes, all[p].seed, verify_count_, nullptr);
      } catch (const Error&) {
        launched = false;
      }
      if (!launched || hipMemcpy(&bad, verify_count_, sizeof(bad), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        bad = 1;
      }
      if (bad) {
        my_stale = true;
        stale_mappings_seen_++;
        if (debug_ || std::getenv("CUDECOMP_VERBOSE"))
          fprintf(stderr, "CUDECOMP:WARN rank %d: the new IPC mapping of rank %d's workspace (%llu bytes) does not show its "
                          "page tags on %llu of %llu pages: stale mapping, the workspace will be re-created\n", h_->rank, p,
                  all[p].bytes, bad, all[p].bytes / 4096);
      }
    }
  }
  const bool anyone_failed = h_->boot->allreduceOr(!error.empty());  // also: everybody has finished mapping
  if (anyone_failed) {
    closePeers(r);
    CD_PEER_ERROR(error.empty() ? std::string("IPC mapping failed on another rank") : error);
  }
  if (verify_mappings_ && h_->boot->allreduceOr(my_stale)) {
    closePeers(r);
    h_->boot->barrier();  // everybody has let go of everybody's buffer: the owners may dispose of them
    if (stale) *stale = true;
    if (!stale) CD_PEER_ERROR("a new IPC mapping of a peer's workspace does not lead to that workspace (stale mapping)");
    return nullptr;
  }
  region_by_id_[r.id] = r.base;
  h_->region_generation++;
  auto ins = regions_.emplace(r.base, std::move(r));
  return &ins.first->second;
}

void PeerContext::enablePeerAccessOnce() {
  if (peer_access_done_) return;
  peer_access_done_ = true;
  int dev = -1, count = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  for (int d = 0; d < count; ++d) {
    int can = 0;
    if (d == dev || hipDeviceCanAccessPeer(&can, dev, d) != hipSuccess || !can) continue;
    (void)hipDeviceEnablePeerAccess(d, 0);  // "already enabled" is fine
  }
  (void)hipGetLastError();
}

void PeerContext::unregisterRegion(void* base) {
  auto it = regions_.find(static_cast<char*>(base));
  if (it == regions_.end()) return;
  (void)hipDeviceSynchronize();  // my copies into the peers' mappings are done ...
  h_->boot->barrier();           // ... and so are everybody else's into mine
  closePeers(it->second);
  region_by_id_.erase(it->second.id);
  regions_.erase(it);
  h_->region_generation++;
  h_->boot->barrier();
}

void* PeerContext::takeFromPool(size_t bytes) {
  int best = -1;
  for (int i = 0; i < (int)pool_.size(); ++i) {
    if (pool_[i].bytes < bytes || pool_[i].bytes > std::max(2 * bytes, bytes + ((size_t)64 << 20))) continue;
    if (best < 0 || pool_[i].bytes < pool_[best].bytes) best = i;
  }
  if (best < 0) return nullptr;
  void* p = pool_[best].base;
  pool_bytes_ -= pool_[best].bytes;
  pool_.erase(pool_.begin() + best);
  pool_hits_++;
  return p;
}
std::vector<void*> PeerContext::park(void* base) {
  std::vector<void*> evict;
  Region* r = find(base);
  if (!r || r->base != base) return evict;
  pool_.push_back(Parked{r->base, r->bytes});
  pool_bytes_ += r->bytes;
  while (pool_.size() > 1 && (pool_bytes_ > pool_limit_ || (int)pool_.size() > kMaxParked)) {
    evict.push_back(pool_.front().base);
    pool_bytes_ -= pool_.front().bytes;
    pool_.erase(pool_.begin());
  }
  if (pool_.size() == 1 && pool_bytes_ > pool_limit_) {  // larger than the whole pool: not kept at all
    evict.push_back(pool_.front().base);
    pool_bytes_ = 0;
    pool_.clear();
  }
  return evict;
}
void PeerContext::agreePoolLimit() {
  const int64_t mine = (int64_t)std::min<size_t>(pool_limit_, (size_t)1 << 62);
  pool_limit_ = (size_t)(-h_->boot->allreduceMaxI64(-mine));
}
void PeerContext::trimRetiredImports(size_t keep) {
  if (retired_imports_.size() <= keep) return;
  (void)hipDeviceSynchronize();  // nothing this rank enqueued may still be copying through them
  const size_t n = retired_imports_.size() - keep;
  for (size_t i = 0; i < n; ++i) (void)hipIpcCloseMemHandle(retired_imports_[i]);
  (void)hipGetLastError();
  retired_imports_.erase(retired_imports_.begin(), retired_imports_.begin() + n);
}
std::vector<void*> PeerContext::drainPool() {
  std::vector<void*> all;
  for (auto& p : pool_) all.push_back(p.base);
  pool_.clear();
  pool_bytes_ = 0;
  return all;
}

void PeerContext::barrier(cudecompCommInfo& ci) {
  if (!board_ || ci.ngroups != 1 || ci.barrier_slot < 0) {
    ci.boot->barrier();
    return;
  }
  const uint64_t epoch = ++ci.barrier_epoch;
  cell(ci.barrier_slot, h_->rank).store(epoch, std::memory_order_release);
  for (int m = 0; m < ci.nranks; ++m)
    spinUntil(cell(ci.barrier_slot, ci.global_ranks[m]), epoch, "the shared-memory barrier");
}

void PeerContext::ensureDeviceView() {
  if (dboard_) return;
  if (!board_) CD_PEER_ERROR("the shared-memory board of the peer transport could not be set up on this node");
  CD_CHECK_HIP(hipHostRegister(board_, board_bytes_, hipHostRegisterMapped | hipHostRegisterPortable));
  board_registered_ = true;
  void* d = nullptr;
  CD_CHECK_HIP(hipHostGetDevicePointer(&d, board_, 0));
  dboard_ = static_cast<char*>(d);
}

void PeerContext::setupDeviceFlags() {
  // OPT-IN (CUDECOMP_FLAGS_IN_DEVICE_MEMORY=1).  Measured with ranks sharing one GPU (profiles/r03_tuning.md): per
  // exchange the device flags are as fast or faster than the board, but eight ranks on one device ran the case sweeps
  // 2.7x slower with them and, rarely, a wait kernel never saw a flag that had been raised (30-s device-side
  // timeouts in two suite runs); the board has no such history, so it stays the default until the device flags can
  // be qualified on a node with a GPU per rank.
  const char* want = std::getenv("CUDECOMP_FLAGS_IN_DEVICE_MEMORY");
  if (!board_ || h_->nranks > 64 || !want || std::strtol(want, nullptr, 10) != 1) return;
  for (int r = 0; r < h_->nranks; ++r)
    if (h_->hostnames[r] != h_->hostnames[h_->rank]) return;  // (multi-node jobs keep the per-node board)
  if (h_->rank == 0)
    fprintf(stderr, "CUDECOMP:WARN: CUDECOMP_FLAGS_IN_DEVICE_MEMORY=1 is EXPERIMENTAL: not yet qualified with one GPU per rank "
                    "(profiles/r05_tuning.md); the default keeps the flags in host-pinned memory.\n");
  const auto t_setup = std::chrono::steady_clock::now();
  struct Wire {
    hipIpcMemHandle_t handle;
    int ok;
  };
  Wire mine{};
  const size_t bytes = ((size_t)kSlots * flagRowWords() * sizeof(u64) + 4095) / 4096 * 4096;
  u64* buf = nullptr;
  enablePeerAccessOnce();
  bool ok = hipExtMallocWithFlags(reinterpret_cast<void**>(&buf), bytes, hipDeviceMallocUncached) == hipSuccess && buf;
  if (ok) ok = hipMemset(buf, 0, bytes) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (ok) ok = hipIpcGetMemHandle(&mine.handle, buf) == hipSuccess;
  (void)hipGetLastError();
  mine.ok = ok ? 1 : 0;
  std::vector<Wire> all(h_->nranks);
  h_->boot->allgather(&mine, all.data(), sizeof(Wire));
  for (auto& w : all) ok = ok && w.ok;
  std::vector<u64*> base(h_->nranks, nullptr);
  if (ok) {
    for (int p = 0; p < h_->nranks && ok; ++p) {
      if (p == h_->rank) {
        base[p] = buf;
        continue;
      }
      void* m = nullptr;
      ok = hipIpcOpenMemHandle(&m, all[p].handle, hipIpcMemLazyEnablePeerAccess) == hipSuccess;
      base[p] = static_cast<u64*>(m);
    }
    (void)hipGetLastError();
  }
  const bool all_ok = !h_->boot->allreduceOr(!ok);  // also: everybody has finished mapping
  if (all_ok) {
    flag_base_ = base;
    flag_mem_ = buf;
  } else {
    for (int p = 0; p < h_->nranks; ++p)
      if (p != h_->rank && base[p]) (void)hipIpcCloseMemHandle(base[p]);
    if (buf) (void)hipFree(buf);
    (void)hipGetLastError();
  }
  h_->boot->barrier();
  if (h_->rank == 0 && std::getenv("CUDECOMP_VERBOSE"))
    fprintf(stderr, "CUDECOMP: one-sided exchange flags live in %s (set-up %.1f ms)\n",
            all_ok ? "device memory (polled locally, written by the peer)" : "the host-pinned board",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_setup).count());
}

void PeerContext::checkStatus() {
  if (!board_) return;
  auto& st = *reinterpret_cast<std::atomic<uint64_t>*>(board_ + status_off_ + (size_t)h_->rank * 64);
  const uint64_t v = st.load(std::memory_order_relaxed);
  if (v == 0) return;
  st.store(0, std::memory_order_relaxed);
  CD_PEER_ERROR("a one-sided exchange timed out on the device waiting for a peer's signal (call " +
                std::to_string(v >> 8) + ", flag " + std::to_string((v & 0xff) - 1) + "): a peer rank died or never "
                "entered the matching call; the results of that exchange are incomplete");
}

u64* PeerContext::devEpoch(cudecompCommInfo& ci) {
  if (!ci.dev_epoch) {
    if (ci.barrier_slot < 0) CD_INTERNAL_ERROR("one-sided exchange on a communicator without a board row");
    if (!epoch_slab_) {
      const size_t bytes = (size_t)kSlots * kEpochStride * sizeof(u64);
      if (hipExtMallocWithFlags(reinterpret_cast<void**>(&epoch_slab_), bytes, hipDeviceMallocUncached) != hipSuccess || !epoch_slab_) {
        (void)hipGetLastError();
        CD_CHECK_HIP(hipMalloc(reinterpret_cast<void**>(&epoch_slab_), bytes));
      }
      CD_CHECK_HIP(hipMemset(epoch_slab_, 0, bytes));
    }
    ci.dev_epoch = epoch_slab_ + (size_t)ci.barrier_slot * kEpochStride;
    const u64 base = ci.epoch_base;
    CD_CHECK_HIP(hipMemcpy(ci.dev_epoch, &base, sizeof(base), hipMemcpyHostToDevice));
    // the counter is first touched by a kernel on the CALLER's stream, which need not be ordered behind a synchronous
    // copy from pageable memory (it may return once the bytes are staged): make sure they are in place -- once per
    // communicator
    CD_CHECK_HIP(hipDeviceSynchronize());
  }
  return ci.dev_epoch;
}

PeerContext::Resolved PeerContext::rendezvous(cudecompCommInfo& ci, const void* const* ptrs, const uint32_t* flags, int nbuf) {
  if (!usable(ci)) CD_PEER_ERROR("the one-sided transport needs all members of the communicator on one node");
  const uint64_t seq = ++ci.mail_seq;
  Mail& mine = mail(ci.barrier_slot, h_->rank, (int)(seq & 1));
  // every descriptor of the mailbox is (re)written on every call: a member that posts fewer buffers than a peer asks
  // for must never show that peer what it posted two calls ago
  mine.nbuf = (uint64_t)nbuf;
  for (int b = 0; b < kMailBufs; ++b) mine.buf[b] = (b < nbuf) ? describe(ptrs[b], flags ? flags[b] : 0) : describe(nullptr, 0);
  mine.seq.store(seq, std::memory_order_release);
  Resolved out;
  for (int b = 0; b < nbuf; ++b) {
    out.remote[b].assign(ci.nranks, nullptr);
    out.flags[b].assign(ci.nranks, 0);
    out.mappable[b].assign(ci.nranks, 0);
  }
  for (int m = 0; m < ci.nranks; ++m) {
    const int g = ci.global_ranks[m];
    Mail& theirs = mail(ci.barrier_slot, g, (int)(seq & 1));
    spinUntil(theirs.seq, seq, "the per-call rendezvous of a one-sided exchange");
    const int their_nbuf = (int)std::min<uint64_t>(theirs.nbuf, (uint64_t)kMailBufs);
    for (int b = 0; b < nbuf; ++b) {
      // a buffer the member did not post counts as "not offered" (flags 0, not mappable): the members of a call may
      // disagree about optional buffers (the direct put's output pencil), never about what that means
      const BufDesc d = (b < their_nbuf) ? theirs.buf[b] : BufDesc{};
      out.flags[b][m] = d.flags;
      out.mappable[b][m] = d.mappable;
      if (g == h_->rank) out.remote[b][m] = static_cast<char*>(const_cast<void*>(ptrs[b]));
      else out.remote[b][m] = map(g, d);
      if (debug_)
        fprintf(stderr, "CUDECOMP:DEBUG rank %d slot %d seq %llu buf %d member %d (rank %d): region %lld base %llx bytes %llu "
                        "off %llu mappable %u flags %u -> %p\n", h_->rank, ci.barrier_slot, (unsigned long long)seq, b, m, g,
                (long long)d.region_id, (unsigned long long)d.alloc_base, (unsigned long long)d.alloc_bytes,
                (unsigned long long)d.offset, d.mappable, d.flags, (void*)out.remote[b][m]);
    }
  }
  return out;
}

std::vector<char*> PeerContext::symmetric(const cudecompCommInfo& ci, const void* ptr, const char* what) {
  Region* r = find(ptr);
  if (!r)
    CD_INVALID_USAGE(std::string(what) + " must be allocated with cudecompMalloc for the NVSHMEM backends (symmetric "
                     "one-sided access); use an MPI_* backend for arbitrary device buffers");
  std::vector<char*> out(ci.nranks);
  for (int m = 0; m < ci.nranks; ++m) {
    char* pb = r->peer_base[ci.global_ranks[m]];
    if (!pb) CD_PEER_ERROR("peer buffer is not reachable over xGMI/IPC (rank on another host?)");
    out[m] = pb + (static_cast<const char*>(ptr) - r->base);
  }
  return out;
}

hipEvent_t PeerContext::copyEvent(int i) {
  while ((int)copy_events_.size() <= i) {
    hipEvent_t e;
    CD_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    copy_events_.push_back(e);
  }
  return copy_events_[i];
}
hipStream_t PeerContext::copyStream(int i) {
  while ((int)copy_streams_.size() <= i) {
    hipStream_t s;
    CD_CHECK_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    copy_streams_.push_back(s);
  }
  return copy_streams_[i];
}

void PeerContext::dumpRow(cudecompCommInfo& ci, const char* when) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(nullptr, &cap);  // (never inside a capture: the dump synchronizes)
  if (hipGetLastError() != hipSuccess || cap != hipStreamCaptureStatusNone) return;
  if (hipDeviceSynchronize() != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  unsigned long long e = 0;
  if (ci.dev_epoch) (void)hipMemcpy(&e, ci.dev_epoch, sizeof(e), hipMemcpyDeviceToHost);
  char line[512];
  int n = snprintf(line, sizeof(line), "CUDECOMP:DEBUG rank %d %s slot %d P %d base %llu device epoch %llu ready", h_->rank, when,
                   ci.barrier_slot, ci.nranks, (unsigned long long)ci.epoch_base, e);
  if (board_ && ci.barrier_slot >= 0) {
    const u64* row = reinterpret_cast<const u64*>(board_ + flagRowOff(ci.barrier_slot, h_->rank));
    n += snprintf(line + n, sizeof(line) - n, " %llu landed", (unsigned long long)row[0]);
    for (int i = 0; i < landed_n_ && n < 480; ++i) n += snprintf(line + n, sizeof(line) - n, " %llu", (unsigned long long)row[1 + i]);
  }
  fprintf(stderr, "%s\n", line);
}

uint64_t PeerContext::slotHigh(int slot) {
  if (!board_ || slot < 0) return 0;
  uint64_t v = cell(slot, h_->rank).load(std::memory_order_relaxed);
  const u64* row = reinterpret_cast<const u64*>(board_ + flagRowOff(slot, h_->rank));
  for (int i = 0; i < 1 + landed_n_; ++i)  // (flags hold call * kFlagScale + step: round up to whole calls)
    v = std::max<uint64_t>(v, (reinterpret_cast<const std::atomic<uint64_t>*>(row + i)->load() + kFlagScale - 1) / kFlagScale);
  for (int par = 0; par < 2; ++par) v = std::max<uint64_t>(v, mail(slot, h_->rank, par).seq.load());
  // (flags in device memory are not read back: whatever anybody wrote into my buffer carries that rank's call number
  // on the communicator that used the slot, which that rank reports itself -- buildCommInfo reduces over ALL ranks)
  return v;
}

void PeerContext::spinUntil(std::atomic<uint64_t>& a, uint64_t v, const char* what) {
  const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(h_->peer_timeout_s);
  int spins = 0;
  while (a.load(std::memory_order_acquire) < v) {
    if (++spins > 2000) {
      std::this_thread::yield();
      if ((spins & 0xfff) == 0 && std::chrono::steady_clock::now() > deadline)
        CD_PEER_ERROR(std::string("timed out waiting for a peer rank in ") + what + " (did it die, or skip this call?)");
    }
  }
}

BufDesc PeerContext::describe(const void* ptr, uint32_t flags) {
  BufDesc d{};
  d.flags = flags;
  d.region_id = -1;
  if (!ptr) return d;
  if (Region* r = find(ptr)) {
    d.region_id = r->id;
    d.offset = (uint64_t)(static_cast<const char*>(ptr) - r->base);
    d.mappable = 1;
    return d;
  }
  void* base = nullptr;
  size_t bytes = 0;
  if (hipMemGetAddressRange(&base, &bytes, const_cast<void*>(ptr)) != hipSuccess || ipcSizeHangs(bytes)) {
    (void)hipGetLastError();
    return d;  // not a device allocation, or of a size this platform cannot share: mappable = 0
  }
  d.alloc_base = (uint64_t)(uintptr_t)base;
  d.alloc_bytes = bytes;
  d.offset = (uint64_t)(static_cast<const char*>(ptr) - static_cast<const char*>(base));
  // Same address and size as last time does not mean the same allocation (free + malloc can return it again): the
  // runtime's buffer id tells them apart; without one the handle is re-exported on every call.
  unsigned long long id = 0;
  const bool has_id = hipPointerGetAttribute(&id, HIP_POINTER_ATTRIBUTE_BUFFER_ID, const_cast<void*>(ptr)) == hipSuccess;
  if (!has_id) (void)hipGetLastError();
  auto it = exports_.find((char*)base);
  if (it == exports_.end() || it->second.bytes != bytes || !has_id || !it->second.has_id || it->second.buffer_id != id) {
    Export e;
    e.bytes = bytes;
    e.buffer_id = id;
    e.has_id = has_id;
    enablePeerAccessOnce();
    if (hipIpcGetMemHandle(&e.handle, base) != hipSuccess) {
      (void)hipGetLastError();
      exports_.erase((char*)base);
      return d;
    }
    it = exports_.insert_or_assign((char*)base, e).first;
  }
  d.handle = it->second.handle;
  d.mappable = 1;
  return d;
}

char* PeerContext::map(int g, const BufDesc& d) {
  if (!d.mappable) return nullptr;
  if (d.region_id >= 0) {
    Region* r = findById(d.region_id);
    if (!r || !r->peer_base[g] || d.offset >= r->bytes) return nullptr;
    return r->peer_base[g] + d.offset;
  }
  if (h_->hostnames[g] != h_->hostnames[h_->rank]) return nullptr;
  const auto key = std::make_pair(g, d.alloc_base);
  auto it = imports_.find(key);
  if (it != imports_.end() &&
      (it->second.bytes != d.alloc_bytes || std::memcmp(&it->second.handle, &d.handle, sizeof(d.handle)) != 0)) {
    // the owner freed that allocation and made a new one at the same address.  The old mapping is RETIRED, not closed:
    // closing a mapping right before importing its successor is the sequence that can hand back the predecessor's
    // memory on this platform, while importers that never close are safe (scripts/probe/ipc_remap_probe.cpp, modes
    // 1 vs 257).  Retired mappings are closed with the transport.
    (void)hipDeviceSynchronize();
    if (it->second.mapped) retired_imports_.push_back(it->second.mapped);
    imports_.erase(it);
    it = imports_.end();
  }
  if (it == imports_.end()) {
    Import im;
    im.handle = d.handle;
    im.bytes = d.alloc_bytes;
    void* mapped = nullptr;
    enablePeerAccessOnce();
    if (hipIpcOpenMemHandle(&mapped, d.handle, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    im.mapped = static_cast<char*>(mapped);
    it = imports_.emplace(key, im).first;
  }
  return it->second.mapped + d.offset;
}

Mail& PeerContext::mail(int slot, int rank, int parity) {
  return *reinterpret_cast<Mail*>(board_ + mail_off_ + (((size_t)slot * h_->nranks + rank) * 2 + parity) * kMailBytes);
}

// Where a board is mapped.  The board is registered with HIP and polled by kernels; a process that finalizes a handle and
// creates another (a job server, a long-lived test worker) would normally get the NEW board at the address the old one
// had.  Given what this platform does with recycled addresses when several processes share a GPU
// boards are placed in a reserved address arena, each at a fresh address, and a retired board's range stays reserved: no
// board address is ever used twice by a process.  A precaution, not the fix of an observed failure (round 6 suspected a
// recycled board for a failure that was a test's own race: arms with and without the arena failed alike,
// profiles/r06_pooled_suite_failure.md).  CUDECOMP_BOARD_FRESH_ADDRESS=0 restores plain mmap.
namespace {
constexpr size_t kArenaBytes = (size_t)4 << 30, kArenaAlign = (size_t)2 << 20;
char* arena_base = nullptr;  // of this process, whatever handles come and go
size_t arena_used = 0;
bool freshAddresses() {
  const char* v = std::getenv("CUDECOMP_BOARD_FRESH_ADDRESS");
  return !v || std::strtol(v, nullptr, 10) != 0;
}
}  // namespace

void* PeerContext::mapBoard(int fd, size_t bytes) {
  board_in_arena_ = false;
  if (freshAddresses()) {
    if (!arena_base) {
      void* a = ::mmap(nullptr, kArenaBytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
      if (a != MAP_FAILED) arena_base = static_cast<char*>(a);
    }
    const size_t need = (bytes + kArenaAlign - 1) / kArenaAlign * kArenaAlign;
    if (arena_base && arena_used + need <= kArenaBytes) {
      void* p = ::mmap(arena_base + arena_used, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_FIXED, fd, 0);
      if (p != MAP_FAILED) {
        arena_used += need;
        board_in_arena_ = true;
        return p;
      }
    }
  }
  return ::mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
}
void PeerContext::unmapBoard(void* p, size_t bytes) {
  // inside the arena the range goes back to "reserved, inaccessible": the shared pages are dropped, the address is not reused
  if (board_in_arena_) (void)::mmap(p, bytes, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE | MAP_FIXED, -1, 0);
  else ::munmap(p, bytes);
}

void PeerContext::openBoard() {
  // every host gets its own segment; its name is agreed through the bootstrap, the creator unlinks it as
  // soon as all local ranks have mapped it, so nothing is left behind even if a rank crashes later
  landed_n_ = std::max(h_->nranks, 2);
  flag_row_bytes_ = ((size_t)(1 + landed_n_) * sizeof(uint64_t) + 63) / 64 * 64;
  const size_t cells_bytes = (size_t)kSlots * h_->nranks * 64;
  flags_off_ = cells_bytes;
  mail_off_ = flags_off_ + (size_t)kSlots * h_->nranks * flag_row_bytes_;
  status_off_ = mail_off_ + (size_t)kSlots * h_->nranks * 2 * kMailBytes;
  board_bytes_ = (status_off_ + (size_t)h_->nranks * 64 + 4095) / 4096 * 4096;
  if (h_->nranks > 64) return;  // the flag lists of the wait / signal kernels hold 64 entries: no peer transport
  char name[128] = {0};
  if (h_->local_rank == 0)
    snprintf(name, sizeof(name), "/cudecomp_%d_%llx", (int)::getpid(),
             (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count());
  std::vector<char> all((size_t)128 * h_->nranks);
  h_->boot->allgather(name, all.data(), 128);
  int creator = -1;
  for (int r = 0; r < h_->nranks; ++r)
    if (h_->hostnames[r] == h_->hostnames[h_->rank] && h_->rank_to_local_rank[r] == 0) creator = r;
  const char* shm_name = all.data() + (size_t)128 * creator;
  int fd = -1;
  if (h_->local_rank == 0) {
    fd = ::shm_open(shm_name, O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd >= 0 && ::ftruncate(fd, (off_t)board_bytes_) != 0) {
      ::close(fd);
      fd = -1;
    }
  }
  h_->boot->barrier();
  if (h_->local_rank != 0) fd = ::shm_open(shm_name, O_RDWR, 0600);
  void* p = (fd >= 0) ? mapBoard(fd, board_bytes_) : MAP_FAILED;
  if (fd >= 0) ::close(fd);
  const bool ok = (p != MAP_FAILED);
  const bool all_ok = !h_->boot->allreduceOr(!ok);  // also: everybody has mapped it
  if (h_->local_rank == 0) ::shm_unlink(shm_name);
  if (ok && all_ok) board_ = static_cast<char*>(p);
  else if (ok) unmapBoard(p, board_bytes_);  // bootstrap barriers, no one-sided transport
}

}  // namespace cudecomp
