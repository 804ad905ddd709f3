"""Wall values (cudecomp_halo_wall_values.h: cudecompAmdSetWallHalos{X,Y,Z}): the numpy restatement of the contract -- the
definition applied dim by dim to the global array, with AB.typed_add for the one addition per ghost cell and RB.flip_signs for
parity -1 -- and the per-rank bodies of tests/test_gpu_halo_wall_values.py.  Everything is compared byte for byte, whole buffers
with the poison slack around them; there is no tolerance anywhere.  Payloads are finite draws (AB.typed_cells), so no result is
a NaN; the edge-value test of the GPU file is the one place that compares through AB.mismatches.

Arrays of cells are uint8 of shape (..., element bytes); addends are element bytes (the doubles the call takes are chosen exact in
every type, so that this file does not restate the conversion: tests/test_halo_wall_values_plan.py does)."""
import ctypes as C

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import reflect_bodies as RB

POISON, SLACK = RB.POISON, RB.SLACK


def add_element(dtype, cells, element):
    """cells + element, real by real in the arithmetic of `dtype`: cells uint8 (..., es), element `es` bytes; returns uint8"""
    u = AB.FORMATS[AB.kind_of(dtype)][0]
    a = np.ascontiguousarray(cells).view(u)
    b = np.ascontiguousarray(np.broadcast_to(np.frombuffer(bytes(element), dtype=u), a.shape))
    return np.ascontiguousarray(AB.typed_add(dtype, a, b).astype(u)).view(np.uint8)


def wall_cells(dtype, src, parity, element):
    """THE DEFINITION for one ghost layer: s * src + a -- flip first, add second"""
    x = np.array(src, dtype=np.uint8, copy=True)
    if parity < 0:
        RB.flip_signs(x, AB.real_bytes(dtype))
    return add_element(dtype, x, element)


def layer_values(dim, side, h, nc, salt=0):
    """the doubles of one call's side: h * nc small multiples of 1/4, distinct per layer, side, dim and component, exact in every
    one of the seven types (bf16 holds 8 significant bits)"""
    return [(-1.0) ** (k + side) * (0.75 * (k + 1) + 0.25 * c) + 8.0 * side + 16.0 * ((dim + salt) % 3) for k in range(h) for c in range(nc)]


def elements_of(dtype, values, nc):
    """the element bytes of every layer of `values` (doubles, nc per layer)"""
    return [AB.to_bytes(np.array(values[k * nc:(k + 1) * nc], dtype=np.float64), dtype).tobytes() for k in range(len(values) // nc)]


def typed_world(dtype, gdims, seed):
    """finite, non-integer reals of `dtype` for every cell of the global array: uint8 (g0, g1, g2, es)"""
    nc, es = AB.TYPES[dtype][1], AB.element_bytes(dtype)
    n = int(gdims[0]) * int(gdims[1]) * int(gdims[2])
    flat = np.ascontiguousarray(AB.bits_of(dtype, AB.typed_cells(dtype, seed, 0, 0, n, nc))).view(np.uint8).reshape(n, es)
    return flat.reshape(int(gdims[2]), int(gdims[1]), int(gdims[0]), es).transpose(2, 1, 0, 3)


def global_reference(dtype, world, halo, periods, steps):
    """The sequence (update, wall values) over dims 0, 1, 2 on the GLOBAL array as one rank would hold it: uint8
    (g0 + 2 h0, g1 + 2 h1, g2 + 2 h2, es), poison outside the interior at the start.  Per dim: the periodic wrap where the dim is
    periodic; otherwise every call of steps[dim] = [(parity, centering, sides, low values, high values), ...] in order, by the
    definition: cell(h-1-k) = s * cell(h+k+c) + a_low[k], cell(n-h+k) = s * cell(n-h-1-k-c) + a_high[k] over the other two dims
    with their halos.  A rank's pencil is a slice of the result (rank_slice)."""
    es, nc = world.shape[3], AB.TYPES[dtype][1]
    g = world.shape[:3]
    out = np.full((g[0] + 2 * halo[0], g[1] + 2 * halo[1], g[2] + 2 * halo[2], es), POISON, dtype=np.uint8)
    out[tuple(slice(halo[d], halo[d] + g[d]) for d in range(3))] = world
    for dim in range(3):
        h, n = int(halo[dim]), g[dim] + 2 * int(halo[dim])
        if h == 0:
            continue
        at = lambda i: tuple(i if d == dim else slice(None) for d in range(3))
        if periods[dim]:
            for k in range(h):
                out[at(k)] = out[at(n - 2 * h + k)]
                out[at(n - h + k)] = out[at(h + k)]
            continue
        for parity, c, sides, low, high in steps[dim]:
            for side, values in ((0, low), (1, high)):
                if not sides & (1 << side):
                    continue
                elems = elements_of(dtype, values, nc)
                for k in range(h):
                    dst, src = (h - 1 - k, h + k + c) if side == 0 else (n - h + k, n - h - 1 - k - c)
                    assert h <= src < n - h
                    out[at(dst)] = wall_cells(dtype, out[at(src)], parity, elems[k])
    return out


def rank_slice(p, padded, lo):
    """the pencil `p` (first interior cell at global `lo`) cut out of the padded global array: uint8 (cells, es), padding poison"""
    take = tuple(slice(int(lo[d]), int(lo[d]) + RB._dim_axis(p, d)[1]) for d in range(3))
    order = [int(x) for x in p.order]
    out = np.full((int(p.size), padded.shape[3]), POISON, dtype=np.uint8)
    AB.pencil3(p, out)[tuple(RB._unpadded(p))] = padded[take].transpose(order[2], order[1], order[0], 3)
    return out


def _start_and_lo(p, world, halo):
    lo = [0, 0, 0]
    for k in range(3):
        lo[int(p.order[k])] = int(p.lo[k])
    mine = world[tuple(slice(lo[d], lo[d] + RB._dim_axis(p, d)[1] - 2 * int(halo[d])) for d in range(3))]
    order = [int(x) for x in p.order]
    start = np.full((int(p.size), world.shape[3]), POISON, dtype=np.uint8)
    AB.pencil3(p, start)[RB.interior_index(p)] = mine.transpose(order[2], order[1], order[0], 3)
    return start, lo


def steps_of(dtype, halo, parity, centering, sides, salt=0):
    """one call per dim: the case's parity, centering and sides with layer_values as addends"""
    nc = AB.TYPES[dtype][1]
    return [[(parity, centering, sides, layer_values(dim, 0, int(halo[dim]), nc, salt), layer_values(dim, 1, int(halo[dim]), nc, salt))]
            for dim in range(3)]


def wall_sweep(rank, nranks, args):
    """(update, wall values) over dims 0, 1, 2 on every rank of the job, for every case of args["cases"] = [[axis, halo, periods,
    padding, dtype, parity, centering, sides], ...]: the pencil starts as poison everywhere but in its interior, which holds this
    rank's part of a global payload of finite reals; afterwards EVERY byte of the pencil and of the slack around it against the
    definition applied dim by dim to the global array.  Ghost cells of a side that `sides` leaves out stay poison (and travel as
    poison through the later updates) in both."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    gdims = [int(x) for x in args["gdims"]]
    failures = []
    wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, c[0], c[1]) * AB.element_bytes(c[4]) for c in args["cases"])
    work = cd.cudecompMalloc(h, gd, max(wsz, 16))
    worlds = {}
    for case in args["cases"]:
        axis, halo, periods, padding, dtype, parity, centering, sides = case
        es = AB.element_bytes(dtype)
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        what = "rank %d axis %d %s halo %s periods %s padding %s parity %d centering %d sides %d" % (
            rank, axis, AB.NAMES[dtype], tuple(halo), tuple(periods), tuple(padding), parity, centering, sides)
        if g.pencil_info(rank, axis, halo, padding).as_dict() != p.as_dict():
            failures.append(what + ": pencil info differs from the oracle")
            continue
        if dtype not in worlds:
            worlds[dtype] = typed_world(dtype, gdims, 7)  # (computed once, never changed)
        world = worlds[dtype]
        start, lo = _start_and_lo(p, world, halo)
        steps = steps_of(dtype, halo, parity, centering, sides)
        dev, ptr = RB._device_pencil(start)
        for dim in range(3):
            cd.cudecompUpdateHalos(axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream)
            _, c, s, low, high = steps[dim][0]
            cd.cudecompAmdSetWallHalos(axis, h, gd, ptr, dtype, parity, c, s, low if s & 1 else None, high if s & 2 else None, halo, periods,
                                       dim, padding, stream)
        torch.cuda.synchronize()
        want = rank_slice(p, global_reference(dtype, world, halo, periods, steps), lo)
        diff = RB.first_difference(dev.cpu().numpy(), RB._with_slack(want), es)
        if diff:
            failures.append(what + ": " + diff + "; last kernel " + cd.cudecompExtLastKernelName())
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def _f64(values):
    return (C.c_double * max(1, len(values)))(*values)


def _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, arrays, sptr):
    """(update, wall values) over dims 0, 1, 2 through the C entry points; arrays[dim] = (low, high) ctypes arrays of doubles"""
    up, wv = getattr(L, "cudecompUpdateHalos" + "XYZ"[axis]), getattr(L, "cudecompAmdSetWallHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    per = b3(*[bool(x) for x in periods])
    for dim in range(3):
        rc = up(h, gd, ptr, work, dtype, i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc
        rc = wv(h, gd, ptr, dtype, parity, centering, 3, arrays[dim][0], arrays[dim][1], i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc


def graph_replay(rank, nranks, args):
    """The three-dim sequence (update, wall values) captured from the caller's stream into one hipGraph after an eager warm-up; the
    host arrays of addends are OVERWRITTEN after the capture; every replay, on fresh data, applies the addends that were captured."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype = args.get("axis", 0), args.get("dtype", cd.DOUBLE)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    parity, centering = args.get("parity", -1), args.get("centering", 0)
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    gdims = [int(x) for x in args["gdims"]]
    L = cd.lib()
    p = g.pencil_info(0, axis, halo, padding)
    steps = steps_of(dtype, halo, parity, centering, 3)
    arrays = [(_f64(steps[dim][0][3]), _f64(steps[dim][0][4])) for dim in range(3)]
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * es)
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    start, lo = _start_and_lo(p, typed_world(dtype, gdims, 11), halo)
    dev, ptr = RB._device_pencil(start)
    with torch.cuda.stream(stream):
        _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, arrays, stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, arrays, torch.cuda.current_stream().cuda_stream)
    for low, high in arrays:  # the host arrays now hold other numbers: a replay must not look at them
        for a in (low, high):
            for i in range(len(a)):
                a[i] = 1000.0 + i
    for it in range(args.get("replays", 2)):
        world = typed_world(dtype, gdims, 100 + it)  # fresh data every time
        start, lo = _start_and_lo(p, world, halo)
        with torch.cuda.stream(stream):
            dev.copy_(torch.from_numpy(RB._with_slack(start)))
            graph.replay()
            stream.synchronize()
        want = rank_slice(p, global_reference(dtype, world, halo, periods, steps), lo)
        diff = RB.first_difference(dev.cpu().numpy(), RB._with_slack(want), es)
        if diff:
            failures.append("replay %d: %s" % (it, diff))
    # ... and an eager call after the overwrite does apply the new numbers (so the check above can fail)
    with torch.cuda.stream(stream):
        dev.copy_(torch.from_numpy(RB._with_slack(start)))
        _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, arrays, stream.cuda_stream)
        stream.synchronize()
    if any(halo[d] and not periods[d] for d in range(3)) and RB.first_difference(dev.cpu().numpy(), RB._with_slack(want), es) is None:
        failures.append("the eager call after the overwrite still applied the old addends")
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """A long run of kernels is enqueued on a stream, then wall values along all three dims: the calls return while that work is
    still running (an event recorded behind them has not completed), and the pencil is right once it has."""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding, dtype = args["halo"], args["periods"], (0, 0, 0), cd.DOUBLE
    gdims = [int(x) for x in args["gdims"]]
    p = g.pencil_info(0, 0, halo, padding)
    world = typed_world(dtype, gdims, 5)
    start, lo = _start_and_lo(p, world, halo)
    steps = steps_of(dtype, halo, -1, 1, 3)
    want = rank_slice(p, global_reference(dtype, world, halo, periods, steps), lo)
    dev, ptr = RB._device_pencil(start)
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def calls():
        for dim in range(3):
            cd.cudecompAmdSetWallHalos(0, h, gd, ptr, dtype, -1, 1, 3, steps[dim][0][3], steps[dim][0][4], halo, periods, dim, padding,
                                       stream.cuda_stream)

    calls()  # warm-up: first-use work happens before the timed part
    dev.copy_(torch.from_numpy(RB._with_slack(start)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.get("kernels", 100)):
        big.add_(1.0)
    t1 = time.perf_counter()
    calls()
    t2 = time.perf_counter()
    done = torch.cuda.Event()
    done.record(stream)
    pending = not done.query()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    diff = RB.first_difference(dev.cpu().numpy(), RB._with_slack(want), 8)
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": [diff] if diff else [], "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3,
            "wall_host_ms": (t2 - t1) * 1e3, "total_ms": (t3 - t0) * 1e3}
