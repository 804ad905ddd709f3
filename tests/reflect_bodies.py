"""Halo reflection (cudecomp_amd_reflect.h: cudecompAmdReflectHalos{X,Y,Z}): two numpy restatements of the contract -- the
definition cell by cell, and numpy.pad axis by axis -- and the per-rank bodies of tests/test_gpu_halo_reflect.py.  Everything is
compared byte for byte, whole buffers; there is no tolerance anywhere.

Pencils are uint8 arrays of shape (cells, element bytes).  parity -1 inverts the sign bit of every real: the top bit of the last
byte of every `rb` bytes (little endian), rb = the size of one real of the data type.  Buffers start filled with a poison byte
that occurs in no payload, and neither does the poison with its top bit inverted."""
import ctypes as C

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB

POISON = 0x5C
SLACK = 256  # poison bytes in front of and behind a pencil on the device
_ALLOWED = np.array([b for b in range(256) if b not in (POISON, POISON ^ 0x80)], dtype=np.uint8)

# reals with a meaning of their own, most significant byte first: -0, subnormals of both signs, the infinities, quiet and
# signalling NaNs with distinct payload bits and both signs.  A reflection moves them like any other bytes.
_SPECIAL = {
    ("fp16", 2): ["8000", "0001", "8003", "7C00", "FC00", "7E01", "7E02", "FE03", "7D01"],
    ("bf16", 2): ["8000", "0001", "8003", "7F80", "FF80", "7FC1", "7FC2", "FFC3", "7FA1"],
    ("fp32", 4): ["80000000", "00000001", "80000003", "7F800000", "FF800000", "7FC00001", "7FC00002", "FFC00003", "7FA00001"],
    ("fp64", 8): ["8000000000000000", "0000000000000001", "8000000000000003", "7FF0000000000000", "FFF0000000000000",
                  "7FF8000000000001", "7FF8000000000002", "FFF8000000000003", "7FF4000000000001"],
}


def flip_signs(cells, rb):
    """the sign bit of every real of `cells` (uint8, last axis = element bytes) inverted, in place"""
    cells[..., rb - 1::rb] ^= 0x80


def payload(dtype, cells, seed):
    """(cells, element bytes) of bytes that are never the poison (nor the poison with its sign flipped); the first reals are the
    special values of the data type's real, one per cell"""
    es, rb = AB.element_bytes(dtype), AB.real_bytes(dtype)
    rng = np.random.default_rng([int(seed), int(dtype) & 0xFF, int(cells)])  # (the extension types have negative codes)
    out = _ALLOWED[rng.integers(0, _ALLOWED.size, size=(int(cells), es))]
    special = _SPECIAL[(AB.kind_of(dtype), rb)]
    for i, word in enumerate(special[:int(cells)]):
        out[i, (i % (es // rb)) * rb:(i % (es // rb) + 1) * rb] = np.frombuffer(bytes.fromhex(word), dtype=np.uint8)[::-1]
    assert not np.any(out == POISON) and not np.any(out == POISON ^ 0x80)
    return out


def _dim_axis(p, dim):
    """(numpy axis of AB.pencil3's view, extent without padding) of global dim `dim` in pencil `p`"""
    k = [int(x) for x in p.order].index(dim)
    return 2 - k, int(p.shape[k]) - int(p.padding[dim])


def _unpadded(p):
    """index of AB.pencil3's view that leaves the padding out"""
    idx = [None] * 3
    for k in range(3):
        idx[2 - k] = slice(0, int(p.shape[k]) - int(p.padding[int(p.order[k])]))
    return idx


def reflect_reference(p, cells, halo, dim, has_neighbour, parity, centering, rb):
    """THE DEFINITION on one pencil (info `p`), in place on `cells` (uint8, (cells, element bytes)): for k in [0, h), on the
    sides without a neighbour (has_neighbour = (low, high)), cell(h-1-k) = s * cell(h+k+c) and cell(n-h+k) = s * cell(n-h-1-k-c)
    along `dim`, over the other two dims with their halos and without their padding"""
    h, c = int(halo[dim]), int(centering)
    if h == 0:
        return
    ax, n = _dim_axis(p, dim)
    v = AB.pencil3(p, cells)
    for side in (0, 1):
        if has_neighbour[side]:
            continue
        for k in range(h):
            dst, src = (h - 1 - k, h + k + c) if side == 0 else (n - h + k, n - h - 1 - k - c)
            assert h <= src < n - h, "the source of a mirrored cell lies outside the interior"
            d, s = _unpadded(p), _unpadded(p)
            d[ax], s[ax] = dst, src
            x = v[tuple(s)].copy()
            if parity < 0:
                flip_signs(x, rb)
            v[tuple(d)] = x


def wrap_reference(p, cells, halo, dim):
    """the periodic update of a rank that is its own neighbour along `dim`: L <- HF, H <- LF"""
    h = int(halo[dim])
    if h == 0:
        return
    v = AB.pencil3(p, cells)
    lo, hi = v[AB.slab(p, dim, "HF", h)].copy(), v[AB.slab(p, dim, "LF", h)].copy()
    v[AB.slab(p, dim, "L", h)] = lo
    v[AB.slab(p, dim, "H", h)] = hi


def padded_expectation(p, interior, halo, periods, parity, centering, rb, lo=None, fill=POISON):
    """THE OTHER RESTATEMENT, for the sequence (update, reflection) over dims 0, 1, 2: numpy.pad of the global array axis by
    axis -- wrap on periodic dims, symmetric (centering 0) or reflect (centering 1) on the others --, of which the pencil `p`
    holds the slice that begins at global cell lo - halo; a cell outside the domain along an odd number of non-periodic dims has
    its sign bits flipped (parity -1).  interior: uint8, (g0, g1, g2, element bytes), the global array (for a single rank: its
    interior).  Returns the pencil as (cells, element bytes); padding cells hold `fill`."""
    g = interior.shape[:3]
    ids = np.arange(g[0] * g[1] * g[2], dtype=np.int64).reshape(g)
    outside = np.zeros(g, dtype=np.int64)  # along how many non-periodic dims a cell lies outside the domain
    for dim in range(3):
        h = int(halo[dim])
        width = [(h, h) if d == dim else (0, 0) for d in range(3)]
        ids = np.pad(ids, width, mode="wrap" if periods[dim] else ("reflect" if centering else "symmetric"))
        outside = np.pad(outside, width, mode="edge")  # (what the other dims have counted so far travels along)
        if h and not periods[dim]:
            sl = [slice(None)] * 3
            for part in (slice(0, h), slice(outside.shape[dim] - h, None)):
                sl[dim] = part
                outside[tuple(sl)] += 1
    values = interior.reshape(-1, interior.shape[3])[ids]
    if parity < 0:
        odd = (outside % 2).astype(bool)
        flipped = values[odd]
        flip_signs(flipped, rb)
        values[odd] = flipped
    lo = [0, 0, 0] if lo is None else lo  # global index of the pencil's first interior cell
    take = tuple(slice(int(lo[d]), int(lo[d]) + _dim_axis(p, d)[1]) for d in range(3))
    mine = values[take]  # axes (dim 0, dim 1, dim 2, bytes): into memory order, slowest first
    order = [int(x) for x in p.order]
    out = np.full((int(p.size), interior.shape[3]), fill, dtype=np.uint8)
    AB.pencil3(p, out)[tuple(_unpadded(p))] = mine.transpose(order[2], order[1], order[0], 3)
    return out


def interior_index(p):
    """index of AB.pencil3's view that names the interior cells of pencil `p`"""
    idx = [None] * 3
    for k in range(3):
        o = int(p.order[k])
        idx[2 - k] = slice(int(p.halo_extents[o]), int(p.shape[k]) - int(p.padding[o]) - int(p.halo_extents[o]))
    return tuple(idx)


def first_difference(got, want, es):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else "%d bytes differ, first in cell %d (byte %d of it)" % (bad.size, bad[0] // es, bad[0] % es)


# ---- GPU bodies ------------------------------------------------------------------------------------------------------------
def _device_pencil(start):
    """the bytes of `start` on the device between two runs of poison; returns (whole buffer, pointer of the pencil)"""
    import torch
    raw = np.full(2 * SLACK + start.size, POISON, dtype=np.uint8)
    raw[SLACK:SLACK + start.size] = start.reshape(-1)
    dev = torch.from_numpy(raw).cuda()
    return dev, dev.data_ptr() + SLACK


def _with_slack(pencil):
    return np.concatenate([np.full(SLACK, POISON, dtype=np.uint8), pencil.reshape(-1), np.full(SLACK, POISON, dtype=np.uint8)])


def sequence_sweep(rank, nranks, args):
    """(update, reflection) over dims 0, 1, 2 on every rank of the job, for every case of args["cases"] = [[axis, halo, periods,
    padding, dtype, parity, centering], ...]: the pencil starts as poison everywhere but in its interior, which holds this rank's
    part of a global payload; afterwards EVERY byte of the pencil and of the slack around it is compared
      (a) single rank: against the definition applied dim by dim (wrap copy on periodic dims, mirror on the others),
      (b) always: against numpy.pad of the global array axis by axis (padded_expectation),
    so that no ghost cell holds poison any more and no interior cell has changed.  args["single_dims"]: also every dim alone
    (reflection only) on a freshly poisoned pencil, against the definition."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    gdims = [int(x) for x in args["gdims"]]
    failures = []
    wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, c[0], c[1]) * AB.element_bytes(c[4]) for c in args["cases"])
    work = cd.cudecompMalloc(h, gd, max(wsz, 16))  # one workspace serves every case
    for case in args["cases"]:
        axis, halo, periods, padding, dtype, parity, centering = case
        es, rb = AB.element_bytes(dtype), AB.real_bytes(dtype)
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        info = g.pencil_info(rank, axis, halo, padding)
        what = "rank %d axis %d %s halo %s periods %s padding %s parity %d centering %d" % (
            rank, axis, AB.NAMES[dtype], tuple(halo), tuple(periods), tuple(padding), parity, centering)
        if info.as_dict() != p.as_dict():
            failures.append(what + ": pencil info differs from the oracle")
            continue
        world = payload(dtype, gdims[0] * gdims[1] * gdims[2], 7).reshape(gdims[2], gdims[1], gdims[0], es).transpose(2, 1, 0, 3)
        lo = [0, 0, 0]
        for k in range(3):
            lo[int(p.order[k])] = int(p.lo[k])
        mine = world[tuple(slice(lo[d], lo[d] + _dim_axis(p, d)[1] - 2 * int(halo[d])) for d in range(3))]
        order = [int(x) for x in p.order]
        start = np.full((int(p.size), es), POISON, dtype=np.uint8)
        AB.pencil3(p, start)[interior_index(p)] = mine.transpose(order[2], order[1], order[0], 3)
        neighbours = [[g.shifted_rank(rank, axis, dim, side, bool(periods[dim])) >= 0 for side in (-1, 1)] for dim in range(3)]
        dev, ptr = _device_pencil(start)
        for dim in range(3):
            cd.cudecompUpdateHalos(axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream)
            cd.cudecompReflectHalos(axis, h, gd, ptr, dtype, parity, centering, halo, periods, dim, padding, stream)
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        # the global array padded by the halos: this rank's pencil begins at global cell lo (padded coordinates)
        want = padded_expectation(p, world, halo, periods, parity, centering, rb, lo=lo)
        diff = first_difference(got, _with_slack(want), es)
        if diff:
            failures.append(what + ", against numpy.pad: " + diff + "; last kernel " + cd.cudecompExtLastKernelName())
        inside = AB.pencil3(p, got[SLACK:SLACK + start.size].reshape(-1, es))[interior_index(p)]
        if not np.array_equal(inside, AB.pencil3(p, start)[interior_index(p)]):
            failures.append(what + ": an interior cell changed")
        ghosts = np.ones(int(p.size), dtype=bool)
        AB.pencil3(p, ghosts)[interior_index(p)] = False
        unpadded = np.zeros(int(p.size), dtype=bool)
        AB.pencil3(p, unpadded)[tuple(_unpadded(p))] = True
        if np.any(np.all(got[SLACK:SLACK + start.size].reshape(-1, es)[ghosts & unpadded] == POISON, axis=1)):
            failures.append(what + ": a ghost cell still holds the poison")
        if nranks == 1:
            ref = start.copy()
            for dim in range(3):
                if periods[dim]:
                    wrap_reference(p, ref, halo, dim)
                reflect_reference(p, ref, halo, dim, neighbours[dim], parity, centering, rb)
            diff = first_difference(got, _with_slack(ref), es)
            if diff:
                failures.append(what + ", against the definition: " + diff)
        if args.get("single_dims"):
            for dim in range(3):
                dev, ptr = _device_pencil(start)
                cd.cudecompReflectHalos(axis, h, gd, ptr, dtype, parity, centering, halo, periods, dim, padding, stream)
                torch.cuda.synchronize()
                ref = start.copy()
                reflect_reference(p, ref, halo, dim, neighbours[dim], parity, centering, rb)
                diff = first_difference(dev.cpu().numpy(), _with_slack(ref), es)
                if diff:
                    failures.append(what + " dim %d alone: " % dim + diff + "; last kernel " + cd.cudecompExtLastKernelName())
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, sptr):
    """(update, reflection) over dims 0, 1, 2 through the C entry points"""
    up, rf = getattr(L, "cudecompUpdateHalos" + "XYZ"[axis]), getattr(L, "cudecompAmdReflectHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    per = b3(*[bool(x) for x in periods])
    for dim in range(3):
        rc = up(h, gd, ptr, work, dtype, i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc
        rc = rf(h, gd, ptr, dtype, parity, centering, i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc


def _single_rank_case(h, gd, g, args, seed):
    axis, dtype = args.get("axis", 0), args.get("dtype", cd.DOUBLE)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    es = AB.element_bytes(dtype)
    p = g.pencil_info(0, axis, halo, padding)
    gdims = [int(x) for x in args["gdims"]]
    world = payload(dtype, gdims[0] * gdims[1] * gdims[2], seed).reshape(gdims[2], gdims[1], gdims[0], es).transpose(2, 1, 0, 3)
    order = [int(x) for x in p.order]
    start = np.full((int(p.size), es), POISON, dtype=np.uint8)
    AB.pencil3(p, start)[interior_index(p)] = world.transpose(order[2], order[1], order[0], 3)
    want = padded_expectation(p, world, halo, periods, args.get("parity", -1), args.get("centering", 0), AB.real_bytes(dtype))
    return p, start, want


def graph_replay(rank, nranks, args):
    """The three-dim sequence (update, reflection) captured from the caller's stream into one hipGraph after an eager warm-up,
    replayed on fresh data: every replay leaves the pencil numpy.pad names for the data it found."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype = args.get("axis", 0), args.get("dtype", cd.DOUBLE)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    parity, centering = args.get("parity", -1), args.get("centering", 0)
    es = AB.element_bytes(dtype)
    L = cd.lib()
    p, start, want = _single_rank_case(h, gd, g, args, 11)
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * es)
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    dev, ptr = _device_pencil(start)
    with torch.cuda.stream(stream):
        _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, torch.cuda.current_stream().cuda_stream)
    for it in range(args.get("replays", 2)):
        p, start, want = _single_rank_case(h, gd, g, args, 100 + it)  # fresh data every time
        with torch.cuda.stream(stream):
            dev.copy_(torch.from_numpy(_with_slack(start)))
            graph.replay()
            stream.synchronize()
        diff = first_difference(dev.cpu().numpy(), _with_slack(want), es)
        if diff:
            failures.append("replay %d: %s" % (it, diff))
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """A long run of kernels is enqueued on a stream, then reflections along all three dims: the calls return while that work is
    still running (an event recorded behind them has not completed), and the pencil is right once it has."""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], (0, 0, 0)
    es = 8
    p, start, want = _single_rank_case(h, gd, g, dict(args, parity=-1, centering=1), 5)
    dev, ptr = _device_pencil(start)
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    for dim in range(3):  # warm-up: first-use work happens before the timed part
        cd.cudecompReflectHalos(0, h, gd, ptr, cd.DOUBLE, -1, 1, halo, periods, dim, padding, stream.cuda_stream)
    dev.copy_(torch.from_numpy(_with_slack(start)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.get("kernels", 100)):
        big.add_(1.0)
    t1 = time.perf_counter()
    for dim in range(3):
        cd.cudecompReflectHalos(0, h, gd, ptr, cd.DOUBLE, -1, 1, halo, periods, dim, padding, stream.cuda_stream)
    t2 = time.perf_counter()
    done = torch.cuda.Event()
    done.record(stream)
    pending = not done.query()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    diff = first_difference(dev.cpu().numpy(), _with_slack(want), es)
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": [diff] if diff else [], "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3,
            "reflect_host_ms": (t2 - t1) * 1e3, "total_ms": (t3 - t0) * 1e3}


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out
