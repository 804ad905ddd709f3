// workspace.cc -- cudecompMalloc / cudecompFree: workspaces that every rank of the node can write (IPC regions of the PeerContext,
// peer_context.h), pooled with their mappings
#include <cstdio>

#include "peer_context.h"

namespace cudecomp {

void peerPoolCounters(cudecompHandle_t h, int64_t* pool_hits, int64_t* stale_mappings, int64_t* pool_bytes, int64_t* retired) {
  *pool_hits = h->peer ? h->peer->poolHits() : 0;
  *stale_mappings = h->peer ? h->peer->staleMappingsSeen() : 0;
  if (pool_bytes) *pool_bytes = h->peer ? (int64_t)h->peer->poolBytes() : 0;
  if (retired) *retired = h->peer ? (int64_t)h->peer->retiredImports() : 0;
}

void peerTrimRetiredImports(cudecompHandle_t h, size_t keep) {
  if (h->peer) h->peer->trimRetiredImports(keep);
}

namespace {
void releaseRegionForReal(cudecompHandle_t h, void* ptr) {
  h->peer->unregisterRegion(ptr);
  CD_CHECK_HIP(hipFree(ptr));
}
}  // namespace

void* workspaceAllocRaw(cudecompHandle_t h, size_t bytes, bool peer_capable) {
  void* ptr = nullptr;
  if ((h->nranks > 1 || h->self_exchange) && peer_capable) {
    // one-sided writes address the peer's workspace by offset: make it the same size everywhere
    bytes = (size_t)h->boot->allreduceMaxI64((int64_t)bytes);
    bytes = ipcSafeSize(bytes);
    prepareTransports(h, false, true);
    if (void* pooled = h->peer->takeFromPool(bytes)) return pooled;  // (the same decision on every rank)
    // A new allocation is mapped into every rank and the mappings are VERIFIED (page tags).  The platform can answer
    // hipIpcOpenMemHandle with the mapping of a predecessor of the allocation (freed, re-created at the same address,
    // DESIGN.md section 9); such a buffer is SET ASIDE -- so that the next attempt gets another address -- and
    // released as soon as a later candidate exists (at most one is alive beside the candidate: peak 2x the request) or
    // on any exit, also an exceptional one.
    struct SetAside {
      std::vector<void*> bufs;
      ~SetAside() {
        for (void* q : bufs) (void)hipFree(q);
      }
      void keepOnlyLatest() {
        while (bufs.size() > 1) {
          (void)hipFree(bufs.front());
          bufs.erase(bufs.begin());
        }
      }
    } set_aside;
    std::string failure;
    bool drained = false;
    for (int attempt = 0; attempt < 4 && !ptr; ++attempt) {
      void* cand = nullptr;
      // A failing hipMalloc is AGREED ON before anybody acts on it (a rank that threw on its own would leave the others
      // in registerRegion's collectives).  First remedy: everything the pool has parked is released -- collectively, the
      // pools are identical on every rank -- and the allocation is tried again.
      hipError_t me = hipMalloc(&cand, bytes);
      if (me != hipSuccess) {
        (void)hipGetLastError();
        cand = nullptr;
      }
      if (h->boot->allreduceOr(cand == nullptr)) {
        if (cand) (void)hipFree(cand);
        if (!drained) {
          drained = true;
          for (void* q : h->peer->drainPool()) releaseRegionForReal(h, q);
          --attempt;  // the retry after draining does not count as a mapping attempt
          continue;
        }
        CD_HIP_ERROR(std::string("cudecompMalloc: hipMalloc of ") + std::to_string(bytes) + " bytes failed on " +
                     (me != hipSuccess ? "this rank" : "another rank") + " (out of memory), also after releasing the workspace pool");
      }
      set_aside.keepOnlyLatest();
      bool stale = false;
      try {
        if (h->peer->registerRegion(cand, bytes, &stale)) ptr = cand;
      } catch (const Error& e) {
        // Agreed on by all ranks (registerRegion fails collectively): export or import refused.  The same platform
        // behaviour shows this way too ("invalid argument" / "invalid device pointer" for a re-created allocation), so
        // another address gets its chance before the library gives up on sharing the workspace.
        failure = e.what();
      }
      if (!ptr) set_aside.bufs.push_back(cand);
    }
    if (!ptr) {
      // not shared: still a valid workspace for the RCCL / MPI transports; an operation that needs the one-sided
      // transport will report the IPC problem itself
      if (failure.empty()) failure = "every attempt to map the workspace into the other ranks ended with a stale mapping";
      ptr = set_aside.bufs.back();
      set_aside.bufs.pop_back();
    } else {
      failure.clear();
    }
    if (!failure.empty()) {
      if (h->rank == 0 && !h->ipc_warned) {
        fprintf(stderr, "CUDECOMP:WARN: workspace could not be shared over IPC (%s); one-sided (NVSHMEM*/default MPI*) "
                        "backends are unavailable with it\n", failure.c_str());
      }
      h->ipc_warned = true;
    }
    return ptr;
  }
  CD_CHECK_HIP(hipMalloc(&ptr, bytes));
  return ptr;
}

void workspaceTrimPool(cudecompHandle_t h) {
  if (!h->peer) return;
  CD_CHECK_HIP(hipDeviceSynchronize());
  for (void* q : h->peer->drainPool()) releaseRegionForReal(h, q);
}

void workspaceFreeRaw(cudecompHandle_t h, void* ptr) {
  if (h->peer) {
    auto* r = h->peer->find(ptr);
    if (r && r->base == ptr) {
      // like hipFree, return only when everything this rank enqueued that may touch the buffer is done
      CD_CHECK_HIP(hipDeviceSynchronize());
      if (h->peer->poolEnabled()) {
        for (void* q : h->peer->park(ptr)) releaseRegionForReal(h, q);  // (the same list on every rank)
        return;
      }
      releaseRegionForReal(h, ptr);
      return;
    }
  }
  CD_CHECK_HIP(hipFree(ptr));
}

void* workspaceAlloc(cudecompHandle_t h, cudecompGridDesc_t gd, size_t bytes) {
  const bool peer_backend = !transposeBackendIsRccl(gd->config.transpose_comm_backend) ||
                            !haloBackendIsRccl(gd->config.halo_comm_backend);
  return workspaceAllocRaw(h, bytes, peer_backend);
}

void workspaceFree(cudecompHandle_t h, void* ptr) { workspaceFreeRaw(h, ptr); }

}  // namespace cudecomp
