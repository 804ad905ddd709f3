"""Halo fill (cudecomp_amd_fill.h: cudecompAmdFillHalos{X,Y,Z}): the numpy restatement of the contract and the per-rank bodies
of tests/test_gpu_halo_fill.py.  Everything is compared byte for byte, whole buffers; there is no tolerance anywhere.

Fill values: all bytes of the element distinct (0xA0 + i), so a vector stored at the wrong element phase shows; and NULL (zero
bytes).  Buffers start filled with a poison byte that occurs in neither."""
import ctypes as C

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB

POISON = 0x5C


def value_bytes(es):
    return bytes(0xA0 + i for i in range(es))


def fill_reference(g, rank, axis, halo, periods, dim, info, cells, value):
    """the contract on rank `rank`'s pencil, in place on `cells` (uint8, shape (cells, element bytes)): the low halo where
    there is a low neighbour, the high halo where there is a high one, receive the bytes of `value` (None: zero bytes)"""
    h = int(halo[dim])
    if h == 0:
        return
    v = np.frombuffer(value, dtype=np.uint8) if value is not None else np.zeros(cells.shape[1], dtype=np.uint8)
    for side, which in ((-1, "L"), (+1, "H")):
        if g.shifted_rank(rank, axis, dim, side, bool(periods[dim])) >= 0:
            AB.pencil3(info, cells)[AB.slab(info, dim, which, h)] = v


def _first_difference(got, want, es):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else "%d bytes differ, first in cell %d (byte %d of it)" % (bad.size, bad[0] // es, bad[0] % es)


def fill_sweep(rank, nranks, args):
    """cudecompAmdFillHalos for every axis of args["axes"], type of args["dtypes"], dim and value, each call on a freshly
    poisoned pencil: the whole pencil (halo and padding cells included) against the restatement.  args["all_dims"]: also dims
    0, 1, 2 in turn on one pencil (and in the order 2, 0, 1: the same bytes)."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for axis in args.get("axes", [0, 1, 2]):
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        info = g.pencil_info(rank, axis, halo, padding)
        if info.as_dict() != p.as_dict():
            failures.append("rank %d axis %d: pencil info differs from the oracle" % (rank, axis))
            continue
        for dtype in args.get("dtypes", AB.ALL_TYPES):
            es = AB.element_bytes(dtype)
            data = torch.empty(int(p.size) * es, dtype=torch.uint8, device="cuda")
            for value in (value_bytes(es), None):
                for dims in [(0,), (1,), (2,)] + ([(0, 1, 2), (2, 0, 1)] if args.get("all_dims") else []):
                    data.fill_(POISON)
                    want = np.full((int(p.size), es), POISON, dtype=np.uint8)
                    for dim in dims:
                        cd.cudecompFillHalos(axis, h, gd, data.data_ptr(), dtype, halo, periods, dim, padding, value, stream)
                        fill_reference(g, rank, axis, halo, periods, dim, info, want, value)
                    torch.cuda.synchronize()
                    diff = _first_difference(data.cpu().numpy(), want.reshape(-1), es)
                    if diff:
                        failures.append("rank %d axis %d %s halo %s periods %s padding %s dims %s value %s: %s; last kernel %s" %
                                        (rank, axis, AB.NAMES[dtype], tuple(halo), tuple(periods), tuple(padding), dims,
                                         "NULL" if value is None else "bytes", diff, cd.cudecompExtLastKernelName()))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def update_as_oracle(rank, nranks, args):
    """The set of bytes cudecompUpdateHalos changes must be the set the fill changes on a poisoned pencil.  For the update to
    SHOW every cell it writes, every cell it reads must differ from what it overwrites: the pencil holds the poison in every cell
    whose coordinate along `dim` lies in the two halos, and another byte everywhere else (the interior, and the halo and
    padding cells of the other two dims beside it -- the faces span those)."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for axis in args.get("axes", [0, 1, 2]):
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
        for dtype in args.get("dtypes", [cd.DOUBLE]):
            es = AB.element_bytes(dtype)
            work = cd.cudecompMalloc(h, gd, wsz * es)
            for dim in range(3):
                start = np.full((int(p.size), es), POISON, dtype=np.uint8)
                k = [int(x) for x in p.order].index(dim)
                idx = [slice(None)] * 3
                idx[2 - k] = slice(int(halo[dim]), int(p.shape[k]) - int(p.padding[dim]) - int(halo[dim]))
                AB.pencil3(p, start)[tuple(idx)] = 0x11
                start = start.reshape(-1)
                updated = torch.from_numpy(start.copy()).cuda()
                cd.cudecompUpdateHalos(axis, h, gd, updated.data_ptr(), work, dtype, halo, periods, dim, padding, stream)
                filled = torch.full((int(p.size) * es,), POISON, dtype=torch.uint8, device="cuda")
                cd.cudecompFillHalos(axis, h, gd, filled.data_ptr(), dtype, halo, periods, dim, padding, value_bytes(es), stream)
                torch.cuda.synchronize()
                by_update = updated.cpu().numpy() != start
                by_fill = filled.cpu().numpy() != POISON
                if not np.array_equal(by_update, by_fill):
                    failures.append("rank %d axis %d %s dim %d: the update changed %d bytes, the fill %d, %d differ" %
                                    (rank, axis, AB.NAMES[dtype], dim, by_update.sum(), by_fill.sum(), (by_update != by_fill).sum()))
            cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def deposit_loop(rank, nranks, args):
    """What the feature is for.  One time step: fill dims 0, 1, 2 with zero; pencil += w on every cell, ghosts included (the
    deposit; w holds integers 0..2, so every sum stays exact: at most 27 * 2 per step, 162 after three, below bf16's 256);
    accumulate along dims 2, 1, 0.  The pencil starts with zero in the interior and the poison everywhere else.  After every
    step the interior must have grown by exactly what tests/accumulate_bodies.py restates for THAT step's deposit alone: a ghost
    cell the fill missed still holds the poison, or the previous step's deposit, and lands in an interior cell."""
    import torch
    from tests import gpu_bodies as B
    from tests.half_bodies import global_index
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    stream = torch.cuda.current_stream().cuda_stream
    tdt = {cd.DOUBLE: torch.float64, cd.BFLOAT16: torch.bfloat16}
    failures = []
    for axis in args.get("axes", [0, 1, 2]):
        infos = [g.pencil_info(r, axis, halo, padding) for r in range(g.nranks)]
        p = infos[rank]
        inside = torch.from_numpy(global_index(p, g.gdims) >= 0).cuda()
        wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
        for dtype in args["dtypes"]:
            es = AB.element_bytes(dtype)
            work = cd.cudecompMalloc(h, gd, wsz * es)
            raw = torch.full((int(p.size) * es,), POISON, dtype=torch.uint8, device="cuda")
            pencil = raw.view(tdt[dtype])
            pencil[inside] = 0
            for step in range(3):
                w = [AB.initial_cells(1000 * step + 17, r, axis, infos[r].size, 1) % 3 for r in range(g.nranks)]
                before = pencil[inside].to(torch.float64).cpu().numpy()
                for dim in (0, 1, 2):
                    cd.cudecompFillHalos(axis, h, gd, raw.data_ptr(), dtype, halo, periods, dim, padding, None, stream)
                pencil += torch.from_numpy(w[rank].reshape(-1).astype(np.float64)).cuda().to(tdt[dtype])
                for dim in (2, 1, 0):
                    cd.cudecompAccumulateHalos(axis, h, gd, raw.data_ptr(), work, dtype, halo, periods, dim, padding, stream)
                torch.cuda.synchronize()
                want = [a.copy() for a in w]
                for dim in (2, 1, 0):
                    AB.accumulate_reference(g, axis, halo, periods, dim, infos, want)
                grown = pencil[inside].to(torch.float64).cpu().numpy() - before
                expected = want[rank].reshape(-1)[inside.cpu().numpy()].astype(np.float64)
                if not np.array_equal(grown, expected):
                    failures.append("rank %d axis %d %s step %d: %d interior cells grew by something else than this step's deposit" %
                                    (rank, axis, AB.NAMES[dtype], step, int((grown != expected).sum())))
            cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def _fill_all_dims(L, axis, h, gd, ptr, dtype, value, halo, periods, padding, sptr):
    """the C entry point itself, so that `value` can be a buffer the caller changes afterwards"""
    fn = getattr(L, "cudecompAmdFillHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    for dim in range(3):
        rc = fn(h, gd, ptr, dtype, value, i3(*halo), b3(*[bool(x) for x in periods]), dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc


def graph_replay(rank, nranks, args):
    """A fill of all three dims captured from the caller's stream into one hipGraph after an eager warm-up; the host value is
    overwritten after the capture; every replay, on a re-poisoned pencil, still stores the captured value."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    axis, dtype = args.get("axis", 0), args.get("dtype", cd.DOUBLE)
    es = AB.element_bytes(dtype)
    info = g.pencil_info(rank, axis, halo, padding)
    L = cd.lib()
    captured = value_bytes(es)
    value = (C.c_uint8 * es)(*captured)
    want = np.full((int(info.size), es), POISON, dtype=np.uint8)
    for dim in range(3):
        fill_reference(g, rank, axis, halo, periods, dim, info, want, captured)
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    data = torch.full((int(info.size) * es,), POISON, dtype=torch.uint8, device="cuda")
    with torch.cuda.stream(stream):
        _fill_all_dims(L, axis, h, gd, data.data_ptr(), dtype, value, halo, periods, padding, stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        _fill_all_dims(L, axis, h, gd, data.data_ptr(), dtype, value, halo, periods, padding, torch.cuda.current_stream().cuda_stream)
    for i in range(es):
        value[i] = 0xEE  # the caller's value changes after the capture
    for it in range(args.get("replays", 2)):
        with torch.cuda.stream(stream):
            data.fill_(POISON)
            graph.replay()
            stream.synchronize()
        diff = _first_difference(data.cpu().numpy(), want.reshape(-1), es)
        if diff:
            failures.append("replay %d: %s" % (it, diff))
    del graph
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """A long run of kernels is enqueued on a stream, then fills along all three dims: the calls return while that work is still
    running (an event recorded behind them has not completed), and the pencil is right once it has."""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], (0, 0, 0)
    es = 8
    info = g.pencil_info(rank, 0, halo, padding)
    data = torch.full((int(info.size) * es,), POISON, dtype=torch.uint8, device="cuda")
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    for dim in range(3):  # warm-up: first-use work happens before the timed part
        cd.cudecompFillHalos(0, h, gd, data.data_ptr(), cd.DOUBLE, halo, periods, dim, padding, None, stream.cuda_stream)
    data.fill_(POISON)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.get("kernels", 100)):
        big.add_(1.0)
    t1 = time.perf_counter()
    for dim in range(3):
        cd.cudecompFillHalos(0, h, gd, data.data_ptr(), cd.DOUBLE, halo, periods, dim, padding, value_bytes(es), stream.cuda_stream)
    t2 = time.perf_counter()
    done = torch.cuda.Event()
    done.record(stream)
    pending = not done.query()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    want = np.full((int(info.size), es), POISON, dtype=np.uint8)
    for dim in range(3):
        fill_reference(g, rank, 0, halo, periods, dim, info, want, value_bytes(es))
    diff = _first_difference(data.cpu().numpy(), want.reshape(-1), es)
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": [diff] if diff else [], "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3,
            "fill_host_ms": (t2 - t1) * 1e3, "total_ms": (t3 - t0) * 1e3}


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out
