"""Multi-field wall values (cudecomp_halo_wall_value_fields.h: cudecompAmdSetWallFieldHalos{X,Y,Z}): the per-rank bodies of
tests/test_gpu_halo_wall_value_fields.py.  The contract is "every field byte for byte what the single call makes of it alone", so
the reference of every body here is cudecompAmdSetWallHalos* on a clone of each field (tests/test_gpu_halo_wall_values.py holds the
single call to numpy); whole buffers are compared, poison slack included, without any tolerance.  Payloads are finite draws and the
poison is a finite number in every type, so no result is a NaN."""
import ctypes as C

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import reflect_bodies as RB
from tests import wall_values_bodies as WB

TABLE = 2048


def addend_values(f, side, h, nc, salt=0):
    """the doubles of field f's side: h * nc multiples of 1/4 below 32 in magnitude -- exact in all seven types -- that differ from
    field to field, side to side, layer to layer and component to component, so that a wrong table index shows"""
    return [((f * 37 + side * 101 + k * 13 + c * 59 + salt * 7) % 255 - 127) / 4.0 for k in range(h) for c in range(nc)]


def field_values(n_fields, side, h, nc, salt=0):
    """values_low or values_high of a call: field-major"""
    return [x for f in range(n_fields) for x in addend_values(f, side, h, nc, salt)]


def parities_of(n_fields, salt):
    """mixed parities: never all equal for two fields or more"""
    return [-1 if (f + salt) % 3 == 0 or (f * salt) % 5 == 2 else 1 for f in range(n_fields)]


def launches_expected(n_fields, sides_written, h, es):
    if sides_written == 0 or h == 0:
        return 0
    if n_fields == 1:
        return 1
    per = min(32, TABLE // (sides_written * h * es))
    return -(-n_fields // per)


def _launch_count():
    n = C.c_int64(-1)
    assert cd.lib().cudecompExtDataLaunchCount(C.byref(n)) == cd.RESULT_SUCCESS
    return n.value


def fields_sweep(rank, nranks, args):
    """For every case of args["cases"] = [[axis, halo, periods, padding, dtype, centering, sides, n_fields], ...]: n_fields pencils,
    poison everywhere but in their interiors, which hold this rank's part of a payload of their own; over dims 0, 1, 2 one multi-field
    call on the fields and n_fields single calls on their clones, each field with its parity and its addends.  Afterwards EVERY byte
    of every field and of the slack around it against its clone; the launches of every multi-field call against the launch rule;
    and the walls were written at all (the fields differ from their start where the rank has a wall)."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    gdims = [int(x) for x in args["gdims"]]
    failures, worlds = [], {}
    written = 0
    for number, case in enumerate(args["cases"]):
        axis, halo, periods, padding, dtype, centering, sides, n_fields = case
        es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        what = "rank %d case %d axis %d %s halo %s periods %s padding %s centering %d sides %d fields %d" % (
            rank, number, axis, AB.NAMES[dtype], tuple(halo), tuple(periods), tuple(padding), centering, sides, n_fields)
        parities = parities_of(n_fields, number)
        starts = []
        for f in range(n_fields):
            if (dtype, f) not in worlds:
                worlds[(dtype, f)] = WB.typed_world(dtype, gdims, 20 + f)  # (computed once, never changed)
            starts.append(WB._start_and_lo(p, worlds[(dtype, f)], halo)[0])
        multi = [RB._device_pencil(s) for s in starts]
        clones = [RB._device_pencil(s) for s in starts]
        for dim in range(3):
            hd = int(halo[dim])
            low, high = field_values(n_fields, 0, hd, nc, dim), field_values(n_fields, 1, hd, nc, dim)
            shifted = [cd.cudecompGetShiftedRank(h, gd, axis, dim, d, bool(periods[dim])) for d in (-1, 1)]
            walls = 0 if periods[dim] else sum(1 for side in (0, 1) if shifted[side] < 0 and sides & (1 << side))
            before = _launch_count()
            cd.cudecompAmdSetWallFieldHalos(axis, h, gd, [m[1] for m in multi], dtype, parities, centering, sides, low if sides & 1 else None,
                                            high if sides & 2 else None, halo, periods, dim, padding, stream)
            made = _launch_count() - before
            if made != launches_expected(n_fields, walls, hd, es):
                failures.append(what + ": dim %d made %d launches, the rule says %d" % (dim, made, launches_expected(n_fields, walls, hd, es)))
            name = cd.cudecompExtLastKernelName()
            if made and not name.startswith(("rows_fields_wall_kernel<", "generic_fields_wall_kernel<") if n_fields > 1
                                            else ("rows_wall_kernel<", "generic_wall_kernel<")):
                failures.append(what + ": dim %d ran %s" % (dim, name))
            written += made
            for f in range(n_fields):
                per = hd * nc
                cd.cudecompAmdSetWallHalos(axis, h, gd, clones[f][1], dtype, parities[f], centering, sides,
                                           low[f * per:(f + 1) * per] if sides & 1 else None, high[f * per:(f + 1) * per] if sides & 2 else None,
                                           halo, periods, dim, padding, stream)
        torch.cuda.synchronize()
        changed = False
        for f in range(n_fields):
            got, want = multi[f][0].cpu().numpy(), clones[f][0].cpu().numpy()
            diff = RB.first_difference(got, want, es)
            if diff:
                failures.append(what + ": field %d (parity %d): %s" % (f, parities[f], diff))
            changed = changed or not np.array_equal(want, RB._with_slack(starts[f]))
        if not changed and any(halo[d] and not periods[d] for d in range(3)) and nranks == 1:
            failures.append(what + ": the single calls wrote nothing")
    cd.cudecompGridDescDestroy(h, gd)
    if args.get("must_launch") and written == 0:
        failures.append("rank %d: no call launched anything" % rank)
    return failures


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def _f64(values):
    return (C.c_double * max(1, len(values)))(*values)


def _multi(L, axis, h, gd, table, n_fields, dtype, par, centering, halo, periods, padding, arrays, sptr):
    fn = getattr(L, "cudecompAmdSetWallFieldHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    for dim in range(3):
        rc = fn(h, gd, table, n_fields, dtype, par, centering, 3, arrays[dim][0], arrays[dim][1], i3(*halo), b3(*[bool(x) for x in periods]),
                dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc


def _clone_reference(axis, h, gd, starts, dtype, parities, centering, halo, periods, padding, nc, salt, stream):
    """the single calls over dims 0, 1, 2 on fresh copies of `starts`: the bytes the multi-field sequence must leave"""
    import torch
    out = []
    for f, start in enumerate(starts):
        dev, ptr = RB._device_pencil(start)
        for dim in range(3):
            hd = int(halo[dim])
            cd.cudecompAmdSetWallHalos(axis, h, gd, ptr, dtype, parities[f], centering, 3, addend_values(f, 0, hd, nc, dim + salt),
                                       addend_values(f, 1, hd, nc, dim + salt), halo, periods, dim, padding, stream)
        torch.cuda.synchronize()
        out.append(dev.cpu().numpy())
    return out


def graph_replay(rank, nranks, args):
    """The calls along dims 0, 1, 2 captured into one hipGraph after an eager warm-up; the host arrays -- pointers, parities and
    addends -- are OVERWRITTEN after the capture; every replay, on fresh data, applies what was captured."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype, n_fields = args.get("axis", 0), args.get("dtype", cd.DOUBLE), args.get("n_fields", 3)
    halo, periods, padding, centering = args["halo"], args["periods"], args.get("padding", (0, 0, 0)), args.get("centering", 0)
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    gdims = [int(x) for x in args["gdims"]]
    L = cd.lib()
    p = g.pencil_info(0, axis, halo, padding)
    parities = parities_of(n_fields, 1)
    arrays = [(_f64(field_values(n_fields, 0, int(halo[dim]), nc, dim)), _f64(field_values(n_fields, 1, int(halo[dim]), nc, dim))) for dim in range(3)]
    par = (C.c_int32 * n_fields)(*parities)
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    starts = [WB._start_and_lo(p, WB.typed_world(dtype, gdims, 40 + f), halo)[0] for f in range(n_fields)]
    devs = [RB._device_pencil(s) for s in starts]
    table = (C.c_void_p * n_fields)(*[d[1] for d in devs])
    with torch.cuda.stream(stream):
        _multi(L, axis, h, gd, table, n_fields, dtype, par, centering, halo, periods, padding, arrays, stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        _multi(L, axis, h, gd, table, n_fields, dtype, par, centering, halo, periods, padding, arrays, torch.cuda.current_stream().cuda_stream)
    for low, high in arrays:  # the host arrays now hold other numbers: a replay must not look at them
        for a in (low, high):
            for i in range(len(a)):
                a[i] = 1000.0 + i
    for f in range(n_fields):
        par[f] = -par[f]
        table[f] = None
    for it in range(args.get("replays", 2)):
        starts = [WB._start_and_lo(p, WB.typed_world(dtype, gdims, 100 + 10 * it + f), halo)[0] for f in range(n_fields)]  # fresh data
        with torch.cuda.stream(stream):
            for d, s in zip(devs, starts):
                d[0].copy_(torch.from_numpy(RB._with_slack(s)))
            graph.replay()
            stream.synchronize()
        want = _clone_reference(axis, h, gd, starts, dtype, parities, centering, halo, periods, padding, nc, 0, torch.cuda.current_stream().cuda_stream)
        for f in range(n_fields):
            diff = RB.first_difference(devs[f][0].cpu().numpy(), want[f], es)
            if diff:
                failures.append("replay %d field %d: %s" % (it, f, diff))
    del graph
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """A long run of kernels is enqueued on a stream, then multi-field wall values along all three dims: the calls return while that
    work is still running (an event recorded behind them has not completed), and the fields are right once it has."""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding, dtype, n_fields = args["halo"], args["periods"], (0, 0, 0), cd.DOUBLE, 5
    gdims = [int(x) for x in args["gdims"]]
    p = g.pencil_info(0, 0, halo, padding)
    parities = parities_of(n_fields, 2)
    starts = [WB._start_and_lo(p, WB.typed_world(dtype, gdims, 60 + f), halo)[0] for f in range(n_fields)]
    stream = torch.cuda.current_stream()
    want = _clone_reference(0, h, gd, starts, dtype, parities, 1, halo, periods, padding, 1, 0, stream.cuda_stream)
    devs = [RB._device_pencil(s) for s in starts]
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")

    def calls():
        for dim in range(3):
            hd = int(halo[dim])
            cd.cudecompAmdSetWallFieldHalos(0, h, gd, [d[1] for d in devs], dtype, parities, 1, 3, field_values(n_fields, 0, hd, 1, dim),
                                            field_values(n_fields, 1, hd, 1, dim), halo, periods, dim, padding, stream.cuda_stream)

    calls()  # warm-up: first-use work happens before the timed part
    for d, s in zip(devs, starts):
        d[0].copy_(torch.from_numpy(RB._with_slack(s)))
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
    diffs = [RB.first_difference(d[0].cpu().numpy(), w, 8) for d, w in zip(devs, want)]
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": [d for d in diffs if d], "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3,
            "wall_host_ms": (t2 - t1) * 1e3, "total_ms": (t3 - t0) * 1e3}
