"""Per-rank bodies of tests/test_gpu_sync_kernels.py: the six kernels of csrc/sync.hip launched one at a time through the
cudecompExtSync* / TagPages / CheckPages / Checksum harness entries and held, exactly, to tests/sync_reference.py; and the
exchange-verification aid (CUDECOMP_DEBUG_VERIFY_EXCHANGE) end to end.  Every body returns {"failures": [strings], ...figures}.

Memory for flags, epoch and status comes in the two kinds production uses (csrc/peer_context.cc): "device" -- an UNCACHED device
allocation (hipExtMallocWithFlags, as devEpoch and setupDeviceFlags make) -- and "pinned" -- page-aligned host memory registered
mapped and portable and addressed by its device pointer (as ensureDeviceView does with the board).  After every launch every word
of the whole area is compared: the cells the launch names and all sentinels around them."""
import ctypes as C
import os

import numpy as np

import cudecomp_amd as cd
from tests import sync_reference as R

U64 = np.uint64
CELLS = 80                  # flag cells
EPOCH, STATUS = 83, 91      # their cells in the same area, sentinels on both sides of each
AREA = 96
NEAR_2_40 = 2**40 - 3
SCATTER = [(37 * i + 5) % CELLS for i in range(R.MAX_FLAGS)]  # flag i -> cell: the list's order is not the cells' (37 is coprime to 80)
assert len(set(SCATTER)) == R.MAX_FLAGS


def sentinels():
    return (U64(0xA5A5000000000000) + np.arange(AREA, dtype=U64) * U64(0x0101)).astype(U64)


# ---- the HIP runtime the library itself is bound to, for the allocations torch does not make ---------------------------------------
_hip_lib = [None]
# hip_runtime_api.h, by the names they have there
hipSuccess = 0
hipDeviceMallocUncached = 0x3
hipHostRegisterPortable, hipHostRegisterMapped = 0x1, 0x2
hipMemcpyHostToDevice, hipMemcpyDeviceToHost = 1, 2
hipStreamNonBlocking = 0x1


def hip():
    if _hip_lib[0] is None:
        import torch  # noqa: F401  (brings the runtime in, see cudecomp_amd.lib())
        cd.lib()
        L = C.CDLL(None)   # by symbol, whatever file the runtime came from: the one libcudecomp.so resolves its own calls in
        if not hasattr(L, "hipExtMallocWithFlags"):  # (the runtime was not loaded into the global scope: by its mapping then)
            with open("/proc/self/maps") as f:
                path = [l.split(None, 5)[-1].strip() for l in f if "libamdhip64" in l][0]
            L = C.CDLL(path)
        vp = C.c_void_p
        L.hipExtMallocWithFlags.argtypes = [C.POINTER(vp), C.c_size_t, C.c_uint]
        L.hipFree.argtypes = [vp]
        L.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        L.hipHostRegister.argtypes = [vp, C.c_size_t, C.c_uint]
        L.hipHostUnregister.argtypes = [vp]
        L.hipHostGetDevicePointer.argtypes = [C.POINTER(vp), vp, C.c_uint]
        L.hipDeviceSynchronize.argtypes = []
        _hip_lib[0] = L
    return _hip_lib[0]


def _ok(code, what):
    if code != hipSuccess:
        raise RuntimeError("%s failed with hipError_t %d" % (what, code))


class Area:
    """AREA 64-bit cells in one of the two kinds of memory; write / read move the whole area and synchronise the device"""

    def __init__(self, kind):
        import torch
        torch.zeros(1, device="cuda")
        self.kind, self.bytes = kind, AREA * 8
        H = hip()
        p = C.c_void_p()
        if kind == "device":
            _ok(H.hipExtMallocWithFlags(C.byref(p), 4096, hipDeviceMallocUncached), "hipExtMallocWithFlags(hipDeviceMallocUncached)")
            self.base = p.value
        else:
            import mmap
            self.map = mmap.mmap(-1, 4096)
            self.host = np.frombuffer(self.map, dtype=U64, count=AREA)
            self.host_address = C.addressof(C.c_char.from_buffer(self.map))
            _ok(H.hipHostRegister(self.host_address, 4096, hipHostRegisterPortable | hipHostRegisterMapped), "hipHostRegister(portable | mapped)")
            _ok(H.hipHostGetDevicePointer(C.byref(p), self.host_address, 0), "hipHostGetDevicePointer")
            self.base = p.value

    def cell(self, i):
        return self.base + 8 * i

    def write(self, words):
        words = np.ascontiguousarray(words, dtype=U64)
        assert words.size == AREA
        _ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if self.kind == "device":
            _ok(hip().hipMemcpy(self.base, words.ctypes.data, self.bytes, hipMemcpyHostToDevice), "hipMemcpy to the device")
        else:
            self.host[:] = words
        _ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")

    def read(self):
        _ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if self.kind == "device":
            out = np.empty(AREA, dtype=U64)
            _ok(hip().hipMemcpy(out.ctypes.data, self.base, self.bytes, hipMemcpyDeviceToHost), "hipMemcpy to the host")
            return out
        return self.host.copy()

    def close(self):
        _ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if self.kind == "device":
            _ok(hip().hipFree(self.base), "hipFree")
        else:
            _ok(hip().hipHostUnregister(self.host_address), "hipHostUnregister")
            del self.host
            self.map = None


def differing(got, want, what, failures):
    """one failure string naming the flag words that differ (the text the can-fail tests look for)"""
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        failures.append("%s: %d flag words differ, first cell %d holds %#x, expected %#x" % (what, bad.size, i, int(got[i]), int(want[i])))


class LaunchWatch:
    """cudecompExtDataLaunchCount and cudecompExtLastKernelName must not change across the launches of a body"""

    def __init__(self):
        self.count, self.name = cd.cudecompExtDataLaunchCount(), cd.cudecompExtLastKernelName()

    def check(self, failures):
        now = (cd.cudecompExtDataLaunchCount(), cd.cudecompExtLastKernelName())
        if now != (self.count, self.name):
            failures.append("the data-launch count / last kernel name changed: %r -> %r" % ((self.count, self.name), now))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _maps():
    return (("identity", list(range(R.MAX_FLAGS))), ("scattered", SCATTER))


def flags_begin_signal(rank, nranks, args):
    """epoch_begin_k and signal_k for n in {0, 1, 2, 63, 64}, the epoch at 0 and near 2^40, steps 0, 1, 14, 15, the flags in cells
    0 .. n-1 and in scattered cells.  args["short_reference"]: the numpy side alone expects n - 1 flags (the can-fail test)."""
    failures, watch = [], LaunchWatch()
    area = Area(args["kind"])
    short = 1 if args.get("short_reference") else 0
    launches = 0
    for label, cells in _maps():
        for n in args.get("ns", (0, 1, 2, 63, 64)):
            flags = [area.cell(c) for c in cells[:n]]
            ref_cells = cells[:max(n - short, 0)]
            for e0 in (0, NEAR_2_40):
                want = sentinels()
                want[EPOCH] = e0
                area.write(want)
                cd.cudecompExtSyncEpochBegin(area.cell(EPOCH), flags, _stream())
                launches += 1
                want[EPOCH] = e0 + 1   # (n == 0 too)
                want[ref_cells] = R.flag_value(e0 + 1, 0)
                differing(area.read(), want, "begin %s %s n=%d E=%d" % (args["kind"], label, n, e0), failures)
                for step in (0, 1, 14, 15):
                    want = sentinels()
                    want[EPOCH] = e0 + 1
                    area.write(want)
                    cd.cudecompExtSyncSignal(area.cell(EPOCH), flags, step, _stream())
                    launches += 1
                    want[ref_cells] = R.flag_value(e0 + 1, step)   # (the epoch itself is unchanged; n == 0: nothing at all)
                    differing(area.read(), want, "signal %s %s n=%d E=%d step %d" % (args["kind"], label, n, e0 + 1, step), failures)
    area.close()
    watch.check(failures)
    return {"failures": failures, "launches": launches}


def _elapsed_s(fn, stream=None):
    """seconds between a pair of events around fn() on the current (or the given) stream; synchronises"""
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def flags_wait_satisfied(rank, nranks, args):
    """wait_k on flags that already hold enough: the exact target, a later step of the same call, any step of a later call; steps
    0, 1, 15; n in {0, 1, 2, 63, 64} (n = 0 launches nothing: the whole area, status included, stays as it was whatever the cells
    hold); the status cell unchanged from 0 and from a nonzero preset; the launch's time between two events."""
    failures, watch = [], LaunchWatch()
    area = Area(args["kind"])
    slowest = 0.0
    for label, cells in _maps():
        for n in (0, 1, 2, 63, 64):
            flags = [area.cell(c) for c in cells[:n]]
            for e in (5, NEAR_2_40):
                for step in (0, 1, 15):
                    values = {"the exact target": R.flag_value(e, step), "a later call, step 0": R.flag_value(e + 1, 0),
                              "a later call, step 7": R.flag_value(e + 3, 7)}
                    if step < 15:
                        values["a later step of the call"] = R.flag_value(e, step + 1)
                        values["the last step of the call"] = R.flag_value(e, 15)
                    for what, v in values.items():
                        for preset in (0, 0x1234):
                            want = sentinels()
                            want[EPOCH], want[STATUS] = e, preset
                            want[cells[:n]] = v
                            area.write(want)
                            t = _elapsed_s(lambda: cd.cudecompExtSyncWait(area.cell(EPOCH), flags, step, area.cell(STATUS), 0.05, _stream()))
                            slowest = max(slowest, t)
                            differing(area.read(), want, "satisfied wait %s %s n=%d E=%d step %d on %s, status preset %#x"
                                      % (args["kind"], label, n, e, step, what, preset), failures)
    area.close()
    watch.check(failures)
    return {"failures": failures, "slowest_s": slowest}


def flags_wait_timeout(rank, nranks, args):
    """wait_k that gives up after 0.05 s: one lane k of 64 one below the target (step 15: the step before; step 0: the previous
    call's "all landed"), two lanes short, and a signal queued behind the wait on the same stream."""
    failures, watch = [], LaunchWatch()
    area = Area(args["kind"])
    flags = [area.cell(c) for c in SCATTER]
    codes = []
    for e in (5, NEAR_2_40):
        for step in (15, 0):
            target = R.flag_value(e, step)
            for lanes in ((0,), (31,), (63,), (7, 40)):
                want = sentinels()
                want[EPOCH], want[STATUS] = e, 0
                want[SCATTER] = target
                for k in lanes:
                    want[SCATTER[k]] = target - 1
                if step == 0:
                    assert target - 1 == R.flag_value(e - 1, R.FLAG_DONE)
                area.write(want)
                cd.cudecompExtSyncWait(area.cell(EPOCH), flags, step, area.cell(STATUS), 0.05, _stream())
                cd.cudecompExtSyncSignal(area.cell(EPOCH), flags, 15, _stream())  # behind the wait: runs once the wait has given up
                got = area.read()
                status = int(got[STATUS])
                allowed = [R.status_code(e, k) for k in lanes]
                what = "unsatisfied wait %s E=%d step %d lanes %s" % (args["kind"], e, step, lanes)
                if status not in allowed:
                    failures.append("%s: status %#x, expected one of %s" % (what, status, [hex(a) for a in allowed]))
                elif R.decode_status(status) not in [(e, k) for k in lanes]:
                    failures.append("%s: status %#x decodes to %r" % (what, status, R.decode_status(status)))
                codes.append(status)
                want[STATUS] = status
                want[SCATTER] = R.flag_value(e, 15)
                differing(got, want, what + ", then signal", failures)
    area.close()
    watch.check(failures)
    return {"failures": failures, "codes": codes}


def wait_clock(rank, nranks, args):
    """the seconds an unsatisfied wait_k takes at timeout_s 0.05 and 0.20, between two events"""
    failures, watch = [], LaunchWatch()
    area = Area(args["kind"])
    flags = [area.cell(c) for c in SCATTER]
    seconds = {}
    for warm, timeout in ((True, 0.05), (False, 0.05), (False, 0.20)):  # (the first launch pays the code load: not measured)
        want = sentinels()
        want[EPOCH], want[STATUS] = 9, 0
        want[SCATTER] = R.flag_value(9, 15)
        want[SCATTER[17]] -= U64(1)
        area.write(want)
        t = _elapsed_s(lambda: cd.cudecompExtSyncWait(area.cell(EPOCH), flags, 15, area.cell(STATUS), timeout, _stream()))
        want[STATUS] = R.status_code(9, 17)
        differing(area.read(), want, "timed wait %s timeout %.2f" % (args["kind"], timeout), failures)
        if not warm:
            seconds["%.2f" % timeout] = t
    area.close()
    watch.check(failures)
    return {"failures": failures, "seconds": seconds}


def two_streams(rank, nranks, args):
    """the production pattern: wait_k (timeout 0.5 s, flags short) on stream A, then signal_k on stream B.  Both drain, the status
    stays 0, A is done in under 0.5 s.  Were the two streams serialised, the wait would time out after half a second.

    A is the process's default stream (the caller's), B the first stream the process creates, non-blocking, as the library makes its
    copy stream.  The test relies on these two landing on different hardware queues, which holds for the first streams of a process
    under the runtime's default of four queues ("Streams and hardware queues"): hence a process of its own.
    Runs every memory kind of args["kinds"] in turn; returns {kind: figures}."""
    import torch
    out = {}
    a = torch.cuda.default_stream()
    raw = C.c_void_p()
    H = hip()
    H.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    H.hipStreamDestroy.argtypes = [C.c_void_p]
    _ok(H.hipStreamCreateWithFlags(C.byref(raw), hipStreamNonBlocking), "hipStreamCreateWithFlags(hipStreamNonBlocking)")
    b = torch.cuda.ExternalStream(raw.value)
    for kind in args["kinds"]:
        failures, watch = [], LaunchWatch()
        area = Area(kind)
        flags = [area.cell(c) for c in SCATTER]
        want = sentinels()
        want[EPOCH], want[STATUS] = 12, 0
        want[SCATTER] = R.flag_value(12, 14)
        area.write(want)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record(a)
        cd.cudecompExtSyncWait(area.cell(EPOCH), flags, 15, area.cell(STATUS), 0.5, a.cuda_stream)
        e1.record(a)
        cd.cudecompExtSyncSignal(area.cell(EPOCH), flags, 15, b.cuda_stream)
        e2.record(b)
        b.synchronize()
        a.synchronize()
        seconds = e0.elapsed_time(e1) * 1e-3
        signalled = e0.elapsed_time(e2) * 1e-3   # (when the signal was done, on the wait's clock: tells a late signal from an unseen one)
        want[SCATTER] = R.flag_value(12, 15)
        differing(area.read(), want, "two streams %s" % kind, failures)
        area.close()
        watch.check(failures)
        out[kind] = {"failures": failures, "seconds": seconds, "signalled_s": signalled}
    del b
    _ok(H.hipStreamDestroy(raw), "hipStreamDestroy")
    return out


def graph_replay(rank, nranks, args):
    """begin, signal(step 15) and the wait they satisfy, captured on one stream (one branch) and replayed three times: epoch and
    flags advance by one call per replay, the status stays 0."""
    import torch
    failures, watch = [], LaunchWatch()
    area = Area(args["kind"])
    n = 64
    flags = [area.cell(c) for c in SCATTER[:n]]
    e0 = 40
    want = sentinels()
    want[EPOCH], want[STATUS] = e0, 0
    area.write(want)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = torch.cuda.current_stream().cuda_stream
        cd.cudecompExtSyncEpochBegin(area.cell(EPOCH), flags, s)
        cd.cudecompExtSyncSignal(area.cell(EPOCH), flags, 15, s)
        cd.cudecompExtSyncWait(area.cell(EPOCH), flags, 15, area.cell(STATUS), 0.05, s)
    differing(area.read(), want, "after the capture (nothing has run) %s" % args["kind"], failures)
    for replay in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        want[EPOCH] = e0 + replay
        want[SCATTER[:n]] = R.flag_value(e0 + replay, 15)
        differing(area.read(), want, "graph replay %d %s" % (replay, args["kind"]), failures)
    del graph
    area.close()
    watch.check(failures)
    return {"failures": failures}


# ---- page tags ---------------------------------------------------------------------------------------------------------------------
GUARD = 4096


def _host(t):
    return t.cpu().numpy()


def page_tags(rank, nranks, args):
    """tag_pages_k and check_pages_k on bytes = 4096 p + r, p in {0, 1, 255, 256, 257}, r in {0, 8, 4095}: every byte of the buffer
    and 4 KiB on both sides after the tag pass; the counts check_pages_k adds.  args["page_off_by_one"]: the numpy side alone numbers
    the pages from 1 (the can-fail test)."""
    import torch
    failures, watch = [], LaunchWatch()
    rng = np.random.default_rng(4096)
    shift = 1 if args.get("page_off_by_one") else 0
    seeds = [0, 1, 2**64 - 1]
    counts = torch.zeros(8, dtype=torch.int64, device="cuda")
    BAD = 3

    def check(base, nbytes, seed, preset):
        init = np.arange(100, 108, dtype=np.int64)
        init[BAD] = preset
        counts.copy_(torch.from_numpy(init))
        cd.cudecompExtCheckPages(base, nbytes, seed, counts.data_ptr() + 8 * BAD, _stream())
        torch.cuda.synchronize()
        got = _host(counts)
        added = int(got[BAD]) - preset
        init[BAD] = got[BAD]
        if not np.array_equal(got, init):
            failures.append("check_pages wrote beside its counter: %r" % got.tolist())
        return added

    for p in args.get("ps", (0, 1, 255, 256, 257)):
        for r in (0, 8, 4095):
            nbytes = 4096 * p + r
            seed = seeds.pop() if seeds and p > 0 else int(rng.integers(0, 2**64, dtype=np.uint64))
            what = "p=%d r=%d seed %#x" % (p, r, seed)
            payload = rng.integers(0, 256, 2 * GUARD + nbytes, dtype=np.uint8)
            dev = torch.from_numpy(payload.copy()).cuda()
            base = dev.data_ptr() + GUARD
            assert base % 8 == 0
            cd.cudecompExtTagPages(base, nbytes, seed, _stream())
            torch.cuda.synchronize()
            want = payload.copy()
            tags = R.page_tags(seed, np.arange(p, dtype=U64) + U64(shift))
            for i in range(p):
                want[GUARD + 4096 * i:GUARD + 4096 * i + 8] = np.frombuffer(tags[i:i + 1].tobytes(), dtype=np.uint8)
                assert int(tags[i]) == R.page_tag(seed, i + shift)
            got = _host(dev)
            bad = np.flatnonzero(got != want)
            if bad.size:
                failures.append("tag pass %s: %d bytes differ, first at byte %d of the buffer (page %d)"
                                % (what, bad.size, int(bad[0]) - GUARD, (int(bad[0]) - GUARD) // 4096))
                continue
            if shift:
                continue
            for preset in (0, 7):   # the kernel accumulates
                added = check(base, nbytes, seed, preset)
                if added != 0:
                    failures.append("check after the tag pass %s, counter preset %d: added %d, expected 0" % (what, preset, added))
            if p == 0:
                if check(base, nbytes, seed ^ 1, 0) != 0:
                    failures.append("check %s: no whole page, yet the counter moved" % what)
                continue
            added = check(base, nbytes, seed ^ (1 << 63), 7)
            if added != p:
                failures.append("check with another seed %s: added %d, expected %d" % (what, added, p))
            added = check(base + 4096, nbytes - 4096, seed, 0)   # the tag depends on the page NUMBER
            if added != p - 1:
                failures.append("check one page up %s: added %d, expected %d" % (what, added, p - 1))
            damaged = sorted({0, p - 1, p // 2})
            words = dev[GUARD:GUARD + 4096 * p].view(torch.int64)
            for i in damaged:
                words[512 * i] ^= 1 << (i % 63)
            torch.cuda.synchronize()
            for preset in (0, 7):
                added = check(base, nbytes, seed, preset)
                if added != len(damaged):
                    failures.append("check after damaging pages %s of %s, counter preset %d: added %d, expected %d"
                                    % (damaged, what, preset, added, len(damaged)))
            del words, dev
    watch.check(failures)
    return {"failures": failures}


def page_tags_large(rank, nranks, args):
    """p = 262144 + 3 pages (1 GiB + 12 KiB): the grid is capped at 1024 x 256 threads, so pages 262144 .. 262146 are stamped and
    checked in the stride loop's SECOND pass.  Nothing of the buffer goes to the host: the tags are compared on the device through a
    strided view with the vectorised reference, every other word (and 4 KiB on both sides) with the fill's closed form, 16 MiB at a
    time; then the last three pages are damaged."""
    import torch
    failures, watch = [], LaunchWatch()
    p = 262144 + 3
    seed = 0xC0FFEE0123456789
    guard = GUARD // 8
    total = 2 * guard + 512 * p
    k = 0x9E3779B97F4A7C15 - 2**64   # (as a signed 64-bit factor: torch's int64 product wraps like the unsigned one)
    chunk = 1 << 21                  # 16 MiB of words

    def fill(lo, hi):
        return torch.arange(lo, hi, dtype=torch.int64, device="cuda") * k + 1

    buf = torch.empty(total, dtype=torch.int64, device="cuda")
    for lo in range(0, total, chunk):
        buf[lo:min(total, lo + chunk)] = fill(lo, min(total, lo + chunk))
    base = buf.data_ptr() + GUARD
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    cd.cudecompExtTagPages(base, 4096 * p, seed, _stream())
    torch.cuda.synchronize()
    tags = torch.from_numpy(R.page_tags(seed, p).view(np.int64)).cuda()
    if int(tags[p - 1].item()) % 2**64 != R.page_tag(seed, p - 1):
        failures.append("the vectorised reference disagrees with the integer one at the last page")
    got_tags = buf[guard:guard + 512 * p:512]
    wrong = int((got_tags != tags).sum().item())
    if wrong:
        first = int((got_tags != tags).nonzero()[0].item())
        failures.append("large tag pass: %d of %d tags differ, first at page %d" % (wrong, p, first))
    others = 0
    for lo in range(0, total, chunk):
        hi = min(total, lo + chunk)
        exp = fill(lo, hi)
        first_page = max(0, -(-(lo - guard) // 512))
        last_page = min(p, -(-(hi - guard) // 512))   # pages whose word 0 lies in [lo, hi)
        if last_page > first_page:
            exp[guard + 512 * first_page - lo:guard + 512 * (last_page - 1) - lo + 1:512] = tags[first_page:last_page]
        others += int((buf[lo:hi] != exp).sum().item())
        del exp
    if others:
        failures.append("large tag pass: %d words of the buffer or its guards differ from what the pass should leave" % others)
    cd.cudecompExtCheckPages(base, 4096 * p, seed, counter.data_ptr(), _stream())
    torch.cuda.synchronize()
    if int(counter.item()) != 0:
        failures.append("large check after the tag pass: %d, expected 0" % int(counter.item()))
    for i in (p - 3, p - 2, p - 1):
        buf[guard + 512 * i] ^= 1
    counter.zero_()
    cd.cudecompExtCheckPages(base, 4096 * p, seed, counter.data_ptr(), _stream())
    torch.cuda.synchronize()
    bad = int(counter.item())
    if bad != 3:
        failures.append("large check after damaging the last three pages: %d, expected 3" % bad)
    del buf, tags, got_tags
    torch.cuda.empty_cache()
    watch.check(failures)
    return {"failures": failures, "bad": bad}


# ---- checksum ----------------------------------------------------------------------------------------------------------------------
SUM_GUARD = 256
BIG = 4 * (2048 * 1024 + 1) + 2   # the block cap plus a tail
SIZES = [0, 1, 2, 3, 4, 5, 7, 8] + [4 * w for w in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)] + [BIG]


class Summer:
    """checksum_k on host bytes: the payload between two guards on the device, out2 in cells 2, 3 of eight"""

    def __init__(self, failures):
        import torch
        self.torch, self.failures = torch, failures
        self.out = torch.zeros(8, dtype=torch.int64, device="cuda")

    def run(self, payload, offset=0, behind=None, preset=(0, 0)):
        """(s1, s2) the device leaves for `payload` (uint8) placed `offset` bytes behind a 256-byte boundary, out2 preset; `behind`:
        the bytes that follow the payload (default: random)"""
        torch = self.torch
        n = payload.size
        raw = np.random.default_rng(n).integers(0, 256, 2 * SUM_GUARD + offset + n, dtype=np.uint8)
        raw[SUM_GUARD + offset:SUM_GUARD + offset + n] = payload
        if behind is not None:
            raw[SUM_GUARD + offset + n:] = behind
        dev = torch.from_numpy(raw.copy()).cuda()
        assert dev.data_ptr() % 256 == 0
        init = np.arange(200, 208, dtype=U64)
        init[2], init[3] = preset
        self.out.copy_(torch.from_numpy(init.view(np.int64)))
        cd.cudecompExtChecksum(dev.data_ptr() + SUM_GUARD + offset, n, self.out.data_ptr() + 16, _stream())
        torch.cuda.synchronize()
        got = _host(self.out).view(U64)
        if not np.array_equal(got[[0, 1, 4, 5, 6, 7]], init[[0, 1, 4, 5, 6, 7]]):
            self.failures.append("checksum of %d bytes wrote beside out2: %r" % (n, got.tolist()))
        if not np.array_equal(_host(dev), raw):
            self.failures.append("checksum of %d bytes changed the bytes it read" % n)
        return (int(got[2]) - preset[0]) % 2**64, (int(got[3]) - preset[1]) % 2**64


def checksum(rank, nranks, args):
    """checksum_k on every size of SIZES: random payloads, all 0xFF on the largest (s2 wraps), out2 preset to 0 and to values within
    2^20 below 2^64 (the kernel adds), the 4 x 257 and 4 x 1025 sizes again from a base at 2 mod 4, and a 16-byte block moved.
    args["drop_last_word"]: the numpy side alone leaves the last word out (the can-fail test)."""
    failures, watch = [], LaunchWatch()
    rng = np.random.default_rng(2048)
    S = Summer(failures)
    drop = bool(args.get("drop_last_word"))

    def reference(payload):
        return R.checksum_np(payload[:(payload.size - 1) // 4 * 4] if drop and payload.size else payload)

    def hold(payload, what, offset=0):
        want = reference(payload)
        for preset in ((0, 0), (2**64 - 1 - int(rng.integers(0, 2**20)), 2**64 - 1 - int(rng.integers(0, 2**20)))):
            got = S.run(payload, offset, preset=preset)
            if got != want:
                failures.append("checksum %s, %d bytes, base at %d mod 4, out2 preset %s: sums differ, device %#x / %#x, reference %#x / %#x"
                                % (what, payload.size, offset % 4, "0" if preset == (0, 0) else "near 2^64", got[0], got[1], want[0], want[1]))
        return want

    for n in args.get("sizes", SIZES):
        hold(rng.integers(0, 256, n, dtype=np.uint8), "of random bytes")
    if not args.get("sizes"):
        ones = np.full(BIG, 0xFF, dtype=np.uint8)
        want = hold(ones, "of 0xFF bytes")
        words = BIG // 4
        if (2**32 - 1) * words * (words + 1) // 2 < 2**64 or want != R.checksum_of_words([2**32 - 1] * words + [0xFFFF]):
            failures.append("the all-0xFF payload does not wrap s2, or the two reference forms disagree on it")
        for n in (4 * 257, 4 * 1025):
            hold(rng.integers(0, 256, n, dtype=np.uint8), "of random bytes", offset=2)
        # moving one 16-byte block elsewhere changes the result (and the reference follows)
        payload = rng.integers(0, 256, 4 * 1025, dtype=np.uint8)
        moved = payload.copy()
        moved[160:176], moved[2000:2016] = payload[2000:2016], payload[160:176]
        assert not np.array_equal(payload[160:176], payload[2000:2016])
        a, b = S.run(payload), S.run(moved)
        if a == b or a[0] != b[0]:
            failures.append("a moved 16-byte block: sums %r and %r (s1 must agree, s2 must not)" % (a, b))
        if (a, b) != (reference(payload), reference(moved)):
            failures.append("a moved 16-byte block: the device's sums are not the reference's")
    watch.check(failures)
    return {"failures": failures}


def checksum_tail(rank, nranks, args):
    """The tail of 1 - 3 bytes is one more word: (1) two chunks of an ODD number of 2-byte elements that differ in the last element
    only, based at 2 mod 4 as peerVerifyExchange bases them, give different sums, each the reference's; (2) with different poison
    behind the range the sums are the same: no byte past `bytes` enters.  Returns the sums of (1)."""
    failures, watch = [], LaunchWatch()
    S = Summer(failures)
    rng = np.random.default_rng(105)
    chunk = rng.integers(0, 2**16, 105, dtype=np.uint16)      # 7 x 5 x 3 elements, 210 bytes
    other = chunk.copy()
    other[-1] ^= 0x8001
    a = S.run(chunk.view(np.uint8), offset=2)
    b = S.run(other.view(np.uint8), offset=2)
    if a == b:
        failures.append("odd-length chunk of 2-byte elements: the last element does not enter the sums (%#x / %#x both times)" % a)
    if a != R.checksum(chunk.tobytes()) or b != R.checksum(other.tobytes()):
        failures.append("odd-length chunk of 2-byte elements: device %r and %r, reference %r and %r"
                        % (a, b, R.checksum(chunk.tobytes()), R.checksum(other.tobytes())))
    for n in (1, 2, 3, 5, 6, 7, 4 * 1024 + 1, 4 * 1024 + 3):
        payload = rng.integers(0, 256, n, dtype=np.uint8)
        sums = {S.run(payload, behind=poison) for poison in (0x00, 0xFF, 0x5A)}
        if sums != {R.checksum(payload.tobytes())}:
            failures.append("%d bytes with three poisons behind them: sums %r, reference %r" % (n, sorted(sums), R.checksum(payload.tobytes())))
    watch.check(failures)
    return {"failures": failures, "sums": [list(a), list(b)], "without_tail": list(R.checksum(chunk.tobytes()[:208]))}


# ---- the exchange-verification aid ---------------------------------------------------------------------------------------------------
def sender_sum_index(member, destination, members):
    """where peerVerifyExchange finds "what `member` sent to `destination`" in the gathered array: [member][destination][2]"""
    return 2 * (member * members + destination)


def verify_exchange_aid(rank, nranks, args):
    """X->Y->Z->Y->X out of place on the one-sided backend whose exchanges are ordered by the device-side flag kernels, with
    CUDECOMP_DEBUG_VERIFY_EXCHANGE=1 (the caller's environment): after every exchange peerVerifyExchange (csrc/peer_diag.cc) sums
    each received chunk at the landed flag and again after a barrier, each sent chunk on its sender, and prints a CUDECOMP:VERIFY
    line for a chunk whose sums disagree.  Every member contributes its 2 P sender sums to an allgather, so the gathered array is
    indexed [member][destination][2]: receiver `me` reads what member s sent it at 2 * (s * P + me) (sender_sum_index).

    First a 2-byte type on a grid whose chunks hold odd numbers of elements (gdims (15, 9, 7) on pdims (2, 2): 7 x 5 x 3 = 105 among
    them, so chunks also start at 2 mod 4 and end in a half word), then DOUBLE.  File descriptor 2 goes to a temporary file around
    the calls; returns the transposes' failures against the numpy references (tests/half_bodies.py, the oracle), the lines that
    contain CUDECOMP:VERIFY, and ("ran") the line the aid prints per exchange under CUDECOMP_VERBOSE: the evidence that it ran."""
    import tempfile
    import sys
    from tests import gpu_bodies as B
    from tests import half_bodies as HB
    if os.environ.get("CUDECOMP_DEBUG_VERIFY_EXCHANGE") != "1":
        return {"failures": ["CUDECOMP_DEBUG_VERIFY_EXCHANGE is not set in the rank's environment"], "lines": [], "ran": []}
    common = {"gdims": args["gdims"], "pdims": args["pdims"], "transpose_backend": cd.TRANSPOSE_COMM_NVSHMEM, "out_of_place": [True]}
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            failures = HB.half_cycle(rank, nranks, dict(common, dtype=cd.HALF, expect_path=["peer_barrier"]))
            failures += B.transpose_chain(rank, nranks, dict(common, kind=1, expect_path=["peer_barrier"]))
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    sys.stderr.write(text)
    # with CUDECOMP_VERBOSE the aid says after every exchange it has looked at how many chunks it summed: that it ran at all
    ran = [l for l in text.splitlines() if l.startswith("CUDECOMP: exchange verification rank %d " % rank)]
    return {"failures": failures, "lines": [l for l in text.splitlines() if "CUDECOMP:VERIFY" in l], "ran": ran}
