"""Wall planes (cudecomp_halo_wall_planes.h: cudecompAmdSetWallPlaneHalos{X,Y,Z}): the numpy restatement of the contract -- the
definition applied dim by dim to the global array, with AB.typed_add for the one addition per ghost cell and RB.flip_signs for
parity -1 -- and the per-rank bodies of tests/test_gpu_halo_wall_planes.py.  Everything is compared byte for byte, whole buffers
with the poison slack around them, the plane buffers included (they are only read); there is no tolerance anywhere.  Payloads are
finite draws (AB.typed_cells), so no result is a NaN; the edge-value test of the GPU file is the one place that compares through
AB.mismatches.

Arrays of cells are uint8 of shape (..., element bytes).  Plane entries are exact small multiples of 1/4 in every one of the seven
types, a seeded function of the GLOBAL position (k; p, q) with the other dims' halos counted in, so corner entries are defined and a
rank's plane is its slab of the global one."""
import ctypes as C

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import reflect_bodies as RB
from tests import wall_values_bodies as WB

POISON, SLACK = RB.POISON, RB.SLACK


def entries(dtype, index):
    """plane entries for the integer array `index` (any shape): uint8 (..., es).  Multiples of 1/4 with at most 8 significant bits
    for the 2-byte types (509 distinct values, neighbours in index differ), 65521 distinct values for the wider ones; the second
    real of a complex element comes from the index shifted"""
    nc = AB.TYPES[dtype][1]
    wide = AB.real_bytes(dtype) > 2
    idx = np.asarray(index, dtype=np.int64)[..., None] * nc + np.arange(nc)
    v = ((idx * 7 + 3) % 65521 - 32760) * 0.25 if wide else ((idx * 7 + 3) % 509 - 254) * 0.25
    return AB.to_bytes(v, dtype).reshape(idx.shape[:-1] + (AB.element_bytes(dtype),))


def add_cells(dtype, cells, plane):
    """cells + plane, real by real in the arithmetic of `dtype`: both uint8 (..., es); returns uint8"""
    u = AB.FORMATS[AB.kind_of(dtype)][0]
    a, b = np.ascontiguousarray(cells).view(u), np.ascontiguousarray(plane).view(u)
    return np.ascontiguousarray(AB.typed_add(dtype, a, b).astype(u)).view(np.uint8)


def wall_cells(dtype, src, parity, plane):
    """THE DEFINITION for a set of ghost cells: s * src + plane entry -- flip first, add second"""
    x = np.array(src, dtype=np.uint8, copy=True)
    if parity < 0:
        RB.flip_signs(x, AB.real_bytes(dtype))
    return add_cells(dtype, x, plane)


def global_planes(dtype, gdims, halo, salt=0):
    """planes[dim][side]: uint8 of the padded global array's shape with the extent along `dim` replaced by halo[dim] (+ es): the
    entry of (k; p, q), k the ghost layer counted from the wall outward"""
    full = [int(gdims[d]) + 2 * int(halo[d]) for d in range(3)]
    out = []
    for dim in range(3):
        shape = [int(halo[dim]) if d == dim else full[d] for d in range(3)]
        n = shape[0] * shape[1] * shape[2]
        out.append([entries(dtype, np.arange(n).reshape(shape) + 1000 * (2 * dim + side) + 77 * salt) for side in (0, 1)])
    return out


def global_reference(dtype, world, halo, periods, steps, planes):
    """The sequence (update, wall planes) over dims 0, 1, 2 on the GLOBAL array as one rank would hold it: uint8
    (g0 + 2 h0, g1 + 2 h1, g2 + 2 h2, es), poison outside the interior at the start.  Per dim: the periodic wrap where the dim is
    periodic; otherwise every call of steps[dim] = [(parity, centering, sides), ...] in order, by the definition:
    cell(h-1-k; p,q) = s * cell(h+k+c; p,q) + planes_low(k; p,q), cell(n-h+k; p,q) = s * cell(n-h-1-k-c; p,q) + planes_high(k; p,q)
    over the other two dims with their halos."""
    es = world.shape[3]
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
        for parity, c, sides in steps[dim]:
            for side in (0, 1):
                if not sides & (1 << side):
                    continue
                for k in range(h):
                    dst, src = (h - 1 - k, h + k + c) if side == 0 else (n - h + k, n - h - 1 - k - c)
                    assert h <= src < n - h
                    out[at(dst)] = wall_cells(dtype, out[at(src)], parity, planes[dim][side][at(k)])
    return out


def rank_plane(p, plane, lo, dim, h):
    """the plane of pencil `p` (first interior cell at global `lo`) cut out of the global plane of `dim`: uint8 (elements, es) in the
    layout the contract states -- the pencil's shape in memory order with the extent along `dim` replaced by h; entries at padding
    positions hold poison (they are never read)"""
    order = [int(x) for x in p.order]
    shape = [int(x) for x in p.shape]
    a = order.index(dim)
    shape[a] = int(h)
    take = tuple(slice(0, int(h)) if d == dim else slice(int(lo[d]), int(lo[d]) + RB._dim_axis(p, d)[1]) for d in range(3))
    out = np.full((shape[0] * shape[1] * shape[2], plane.shape[3]), POISON, dtype=np.uint8)
    idx = RB._unpadded(p)
    idx[2 - a] = slice(0, int(h))
    out.reshape(shape[2], shape[1], shape[0], -1)[tuple(idx)] = plane[take].transpose(order[2], order[1], order[0], 3)
    assert out.shape[0] == cd.wall_plane_shape(p, dim, [h if d == dim else 0 for d in range(3)])[1]
    return out


def device_planes(p, planes, lo, halo):
    """per dim the (device buffer, pointer, host copy with slack) of the low and the high plane of pencil `p`; None where h == 0"""
    out = []
    for dim in range(3):
        if int(halo[dim]) == 0:
            out.append(None)
            continue
        sides = []
        for side in (0, 1):
            host = rank_plane(p, planes[dim][side], lo, dim, int(halo[dim]))
            dev, ptr = RB._device_pencil(host)
            sides.append((dev, ptr, RB._with_slack(host)))
        out.append(sides)
    return out


def planes_unchanged(dev_planes):
    for dim, sides in enumerate(dev_planes):
        for side, (dev, _, host) in enumerate(sides or []):
            if not np.array_equal(dev.cpu().numpy(), host):
                return "the %s plane of dim %d was written" % (("low", "high")[side], dim)
    return None


def plane_move(extent, ss, mirrored, soff, doff, side, ps=None, poff=0):
    """(move, operand) of a wall-plane list (cudecompExtRunMoves / cudecompExtDescribeMoves, modes 13 / 14): the source block
    (strides `ss`, all positive here; the destination has them too) begins `soff` elements into buffer 0 and is read backwards along
    `mirrored`, the destination block begins at `doff`; the plane block (strides `ps`, default `ss`) begins `poff` elements into the
    side's plane and is read backwards along `mirrored` on the low side (0), forwards on the high side (1)"""
    ps = list(ss if ps is None else ps)
    signed = list(ss)
    signed[mirrored] = -ss[mirrored]
    m = cd.make_move(extent, signed, ss, soff + (extent[mirrored] - 1) * ss[mirrored], doff, 0, 0)
    m.peer = side
    if side == 0:
        poff += (extent[mirrored] - 1) * ps[mirrored]
        ps[mirrored] = -ps[mirrored]
    return m, (poff, tuple(ps))


def plane_sweep(rank, nranks, args):
    """(update, wall planes) over dims 0, 1, 2 on every rank of the job, for every case of args["cases"] = [[axis, halo, periods,
    padding, dtype, parity, centering, sides], ...]: the pencil starts as poison everywhere but in its interior, which holds this
    rank's part of a global payload of finite reals; the rank's planes are its slabs of the global planes, poison at padding
    positions and around them; afterwards EVERY byte of the pencil and of the slack around it against the definition applied dim by
    dim to the global array, and every byte of the plane buffers against what they held."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    gdims = [int(x) for x in args["gdims"]]
    failures = []
    wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, c[0], c[1]) * AB.element_bytes(c[4]) for c in args["cases"])
    work = cd.cudecompMalloc(h, gd, max(wsz, 16))
    worlds, plane_sets, on_device = {}, {}, {}  # (the planes are only read: one set on the device per pencil geometry and type)
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
            worlds[dtype] = WB.typed_world(dtype, gdims, 7)  # (computed once, never changed)
        if (dtype, tuple(halo)) not in plane_sets:
            plane_sets[(dtype, tuple(halo))] = global_planes(dtype, gdims, halo)
        world, planes = worlds[dtype], plane_sets[(dtype, tuple(halo))]
        start, lo = WB._start_and_lo(p, world, halo)
        steps = [[(parity, centering, sides)] for _ in range(3)]
        dev, ptr = RB._device_pencil(start)
        key = (axis, dtype, tuple(halo), tuple(padding))
        if key not in on_device:
            on_device[key] = device_planes(p, planes, lo, halo)
        dplanes = on_device[key]
        for dim in range(3):
            cd.cudecompUpdateHalos(axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream)
            low, high = (dplanes[dim][0][1], dplanes[dim][1][1]) if dplanes[dim] else (ptr, ptr)  # (h == 0: checked for NULL only)
            cd.cudecompAmdSetWallPlaneHalos(axis, h, gd, ptr, dtype, parity, centering, sides, low if sides & 1 else None,
                                            high if sides & 2 else None, halo, periods, dim, padding, stream)
        torch.cuda.synchronize()
        want = WB.rank_slice(p, global_reference(dtype, world, halo, periods, steps, planes), lo)
        diff = RB.first_difference(dev.cpu().numpy(), RB._with_slack(want), es)
        if diff:
            failures.append(what + ": " + diff + "; last kernel " + cd.cudecompExtLastKernelName())
    for key, dplanes in on_device.items():
        diff = planes_unchanged(dplanes)
        if diff:
            failures.append("rank %d %s: %s" % (rank, key, diff))
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, dplanes, sptr):
    """(update, wall planes) over dims 0, 1, 2 through the C entry points"""
    up, wp = getattr(L, "cudecompUpdateHalos" + "XYZ"[axis]), getattr(L, "cudecompAmdSetWallPlaneHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    per = b3(*[bool(x) for x in periods])
    for dim in range(3):
        rc = up(h, gd, ptr, work, dtype, i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc
        rc = wp(h, gd, ptr, dtype, parity, centering, 3, dplanes[dim][0][1], dplanes[dim][1][1], i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc


def graph_replay(rank, nranks, args):
    """The three-dim sequence (update, wall planes) captured from the caller's stream into one hipGraph after an eager warm-up.  First
    replay: the definition with the contents the planes held at capture.  Then the plane CONTENTS are overwritten on the stream --
    same pointers, no re-capture -- and the second replay equals the definition with the new contents."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype = args.get("axis", 0), args.get("dtype", cd.DOUBLE)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    parity, centering = args.get("parity", -1), args.get("centering", 0)
    es = AB.element_bytes(dtype)
    gdims = [int(x) for x in args["gdims"]]
    L = cd.lib()
    p = g.pencil_info(0, axis, halo, padding)
    steps = [[(parity, centering, 3)] for _ in range(3)]
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * es)
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    world = WB.typed_world(dtype, gdims, 11)
    start, lo = WB._start_and_lo(p, world, halo)
    old, new = global_planes(dtype, gdims, halo, 0), global_planes(dtype, gdims, halo, 5)
    dev, ptr = RB._device_pencil(start)
    dplanes = device_planes(p, old, lo, halo)
    fresh = [[torch.from_numpy(RB._with_slack(rank_plane(p, new[dim][side], lo, dim, halo[dim]))).cuda() for side in (0, 1)] for dim in range(3)]
    with torch.cuda.stream(stream):
        _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, dplanes, stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        _sequence(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, dplanes, torch.cuda.current_stream().cuda_stream)
    for it, planes in enumerate((old, new)):
        with torch.cuda.stream(stream):
            dev.copy_(torch.from_numpy(RB._with_slack(start)))
            if it == 1:  # the contents change on the stream; the pointers, and the graph, stay
                for dim in range(3):
                    for side in (0, 1):
                        dplanes[dim][side][0].copy_(fresh[dim][side], non_blocking=True)
            graph.replay()
            stream.synchronize()
        want = WB.rank_slice(p, global_reference(dtype, world, halo, periods, steps, planes), lo)
        diff = RB.first_difference(dev.cpu().numpy(), RB._with_slack(want), es)
        if diff:
            failures.append("replay %d: %s" % (it, diff))
    # (so that the two checks above cannot both pass with one set of contents)
    if any(halo[d] and not periods[d] for d in range(3)):
        first = WB.rank_slice(p, global_reference(dtype, world, halo, periods, steps, old), lo)
        if np.array_equal(first, want):
            failures.append("the two sets of plane contents give one result")
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """A long run of kernels is enqueued on a stream, then wall planes along all three dims: the calls return while that work is
    still running (an event recorded behind them has not completed), and the pencil is right once it has."""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding, dtype = args["halo"], args["periods"], (0, 0, 0), cd.DOUBLE
    gdims = [int(x) for x in args["gdims"]]
    p = g.pencil_info(0, 0, halo, padding)
    world = WB.typed_world(dtype, gdims, 5)
    start, lo = WB._start_and_lo(p, world, halo)
    planes = global_planes(dtype, gdims, halo)
    steps = [[(-1, 1, 3)] for _ in range(3)]
    want = WB.rank_slice(p, global_reference(dtype, world, halo, periods, steps, planes), lo)
    dev, ptr = RB._device_pencil(start)
    dplanes = device_planes(p, planes, lo, halo)
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def calls():
        for dim in range(3):
            cd.cudecompAmdSetWallPlaneHalos(0, h, gd, ptr, dtype, -1, 1, 3, dplanes[dim][0][1], dplanes[dim][1][1], halo, periods, dim,
                                            padding, stream.cuda_stream)

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
