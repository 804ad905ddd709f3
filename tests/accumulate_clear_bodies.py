"""Halo accumulate-and-clear (cudecomp_amd_fill.h: cudecompAmdAccumulateAndClearHalos{X,Y,Z}): the numpy restatement of the
contract, the runner of take-move lists (modes 3 and 4 of cudecompExtRunMoves) and the per-rank bodies of
tests/test_gpu_halo_accumulate_clear.py.  Everything is compared byte for byte, whole buffers with poison slack on both sides;
there is no tolerance anywhere.

The fused call is DEFINED as  accumulate(dim); fill(dim, NULL)  with the same arguments, so every pencil is held against two
references: (a) the library's own two calls on a copy, (b) numpy -- AB.accumulate_reference on the pencils of all ranks, then
zero bytes into the cells FB.fill_reference names.  Payloads are the finite draws of AB.typed_cells (every sum rounds, no NaN
arises) and AB.initial_cells (integers, exact in every type)."""
import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fill_bodies as FB
from tests import move_lists as ML

SLACK = 256  # poison bytes before and after every device buffer
POISON = FB.POISON
TAKE_KINDS = {12: "rows_take", 13: "generic_take", 14: "rows_add_take", 15: "generic_add_take"}
ARITH_NAMES = {1: "_Float16", 2: "__bf16", 3: "float", 4: "double"}
ARITH_BYTES = {1: 2, 2: 2, 3: 4, 4: 8}


def kernel_name_of(launch):
    """the template spelling of a described launch of kinds 12-15 (csrc/kernels.cc kernelName)"""
    k, es, vec, access, arith = (launch[x] for x in ("kind", "es", "vec", "access", "arith"))
    if k == 12:
        return "rows_take_kernel<%d,%d>" % (vec, access)
    if k == 13:
        return "generic_take_kernel<%d>" % es
    if k == 14:
        return "rows_accumulate_take_kernel<%s,%d,%d>" % (ARITH_NAMES[arith], vec, access)
    assert k == 15, launch
    return "generic_accumulate_take_kernel<%s,%d>" % (ARITH_NAMES[arith], es // ARITH_BYTES[arith])


# ---- numpy: lists of take-moves ------------------------------------------------------------------------------------------------
def finite_bytes(dtype, n_elements, seed):
    """n elements of finite non-integer reals of `dtype` (AB.typed_cells) as bytes"""
    nc = AB.TYPES[dtype][1]
    return AB.bits_of(dtype, AB.typed_cells(dtype, seed, 0, 0, n_elements, nc)).view(np.uint8).reshape(-1).copy()


def host_buffers(moves, es, mode, dtype, seed):
    """buffers 0 (sources) and 1 (destinations) sized for the list, SLACK poison bytes on both sides.  Mode 3: random bytes.
    Mode 4: finite reals in EVERY cell, so every sum is finite and the comparison is byte for byte."""
    n = ML.buffer_lengths(moves)
    rng = np.random.default_rng(seed)
    out = []
    for b in (0, 1):
        body = rng.integers(0, 256, n[b] * es, dtype=np.uint8) if mode == cd.MOVES_TAKE else finite_bytes(dtype, n[b], seed + b)
        out.append(np.concatenate([np.full(SLACK, POISON, np.uint8), body, np.full(SLACK, POISON, np.uint8)]))
    return out


def expected_buffers(moves, es, mode, dtype, bufs):
    """the two buffers after the list ran, one move after the other: dst = src (mode 3) or dst = dst + src in the arithmetic of
    `dtype` (mode 4, AB.typed_add), then zero bytes into the source cells"""
    exp = [b.copy() for b in bufs]
    if mode == cd.MOVES_TAKE:
        src, dst = (e[SLACK:e.size - SLACK].reshape(-1, es) for e in exp)
    else:
        u, nc = AB.FORMATS[AB.kind_of(dtype)][0], AB.TYPES[dtype][1]
        src, dst = (e[SLACK:e.size - SLACK].view(u).reshape(-1, nc) for e in exp)
    for m in moves:
        if 0 in tuple(m.extent):
            continue
        cs, cdst = ML.cells(m.extent, m.ss, m.src_off), ML.cells(m.extent, m.ds, m.dst_off)
        dst[cdst] = src[cs] if mode == cd.MOVES_TAKE else AB.typed_add(dtype, dst[cdst], src[cs])
        src[cs] = 0
    return exp


def assert_disjoint(moves):
    """sources disjoint from each other (they live in buffer 0, destinations in buffer 1), destinations from each other"""
    ML.assert_disjoint_destinations(moves)
    c = [ML.cells(m.extent, m.ss, m.src_off) for m in moves if 0 not in tuple(m.extent)]
    if c:
        c = np.concatenate(c)
        assert np.unique(c).size == c.size, "source cells of the list overlap"
    assert all(m.src_buf == 0 and m.dst_buf == 1 for m in moves)


def run_take_lists(lists, es, mode, dtype=0, seed=0, check_cells=True):
    """GPU.  lists: [(moves, flags)], all over ONE pair of buffers (the regions of different lists disjoint): every list is one
    cudecompExtRunMoves call, in order; then EVERY byte of both buffers, slack included, against numpy.  The launches each call
    makes must be those cudecompExtDescribeMoves predicts for the same addresses, and the kernel that ran the one it names.
    Returns per list the described launches."""
    import torch
    every = [m for moves, _ in lists for m in moves]
    if check_cells:
        assert_disjoint(every)
    bufs = host_buffers(every, es, mode, dtype, seed)
    exp = expected_buffers(every, es, mode, dtype, bufs)
    dev = [torch.from_numpy(b).cuda() for b in bufs]
    assert all(t.data_ptr() % 256 == 0 for t in dev)
    ptrs = [dev[0].data_ptr() + SLACK, dev[1].data_ptr() + SLACK, None]
    stream = torch.cuda.current_stream().cuda_stream
    described = []
    for moves, flags in lists:
        want = ML.describe(moves, ptrs, es, mode, dtype, flags)
        launches, elements, total = cd.cudecompExtRunMoves(moves, ptrs, es, mode, dtype, None, flags, None, stream)
        what = (es, mode, dtype, flags, [(l["kind"], l["vec"], l["n"], l["interleave"], l["blocks"]) for l in want])
        assert total == len(want) and launches == [sum(1 for l in want if l["cls"] == c) for c in range(3)], what
        assert elements == [sum(l["elements"] for l in want if l["cls"] == c) for c in range(3)], what
        assert all(l["kind"] in TAKE_KINDS for l in want), what
        if want:
            assert cd.cudecompExtLastKernelName() == kernel_name_of(want[-1]), (cd.cudecompExtLastKernelName(), what)
        described.append(want)
    torch.cuda.synchronize()
    for name, got, ref in (("source buffer", dev[0], exp[0]), ("destination buffer", dev[1], exp[1])):
        g = got.cpu().numpy()
        bad = np.flatnonzero(g != ref)
        assert bad.size == 0, (name, es, mode, dtype, "%d bytes differ, first at byte %d of %d (slack: %d on both sides); lists: %s"
                               % (bad.size, bad[0], ref.size, SLACK, [(f, [(tuple(m.extent), tuple(m.ss), tuple(m.ds), m.src_off, m.dst_off)
                                                                           for m in mv][:3]) for mv, f in lists][:4]))
    return described


# ---- numpy: the contract ---------------------------------------------------------------------------------------------------------
def fused_reference(g, axis, halo, periods, dim, infos, pencils, add=None):
    """one fused call along `dim` on every rank, in place on `pencils` ((cells, nc) arrays of reals or of bit patterns): the
    accumulation of AB.accumulate_reference, then zero into L / H on the sides that have a neighbour"""
    AB.accumulate_reference(g, axis, halo, periods, dim, infos, pencils, add)
    h = int(halo[dim])
    if h == 0:
        return
    for r in range(len(pencils)):
        for side, which in ((-1, "L"), (+1, "H")):
            if g.shifted_rank(r, axis, dim, side, bool(periods[dim])) >= 0:
                AB.pencil3(infos[r], pencils[r])[AB.slab(infos[r], dim, which, h)] = 0


def _payload(dtype, typed, seed, rank, axis, cells, nc):
    """bit patterns (cells, nc) of rank `rank`'s initial pencil"""
    if typed:
        return AB.bits_of(dtype, AB.typed_cells(dtype, seed, rank, axis, cells, nc)).copy()
    u = AB.FORMATS[AB.kind_of(dtype)][0]
    return AB.to_bytes(AB.initial_cells(seed, rank, axis, cells, nc), dtype).view(u).reshape(-1, nc).copy()


def _guarded(raw):
    import torch
    return torch.from_numpy(np.concatenate([np.full(SLACK, POISON, np.uint8), raw, np.full(SLACK, POISON, np.uint8)])).cuda()


def _diff(got, want, es, what):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    return "%s: %d bytes differ, first at byte %d (cell %d; the pencil begins at byte %d)" % (what, bad.size, bad[0], (int(bad[0]) - SLACK) // es, SLACK)


SEQUENCES = {"fused": "F2 F1 F0", "accumulate_then_fill": "A2 A1 A0 Z0 Z1 Z2", "interleaved": "A2 Z2 A1 Z1 A0 Z0"}


def _run(ops, axis, h, gd, ptr, work, dtype, halo, periods, padding, stream):
    """ops: words of F (fused), A (accumulate), Z (fill with zero bytes) + dim"""
    for op in ops.split():
        dim = int(op[1])
        if op[0] == "F":
            cd.cudecompAccumulateAndClearHalos(axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream)
        elif op[0] == "A":
            cd.cudecompAccumulateHalos(axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream)
        else:
            cd.cudecompFillHalos(axis, h, gd, ptr, dtype, halo, periods, dim, padding, None, stream)


def fused_sweep(rank, nranks, args):
    """For every axis of args["axes"], type of args["dtypes"] and dim: the fused call on a guarded pencil; the WHOLE buffer
    (pencil, halo and padding cells, slack) against (a) the library's accumulate then fill(NULL) on a copy and (b) the all-ranks
    numpy restatement.  args["sequence"]: also fused 2, 1, 0 against accumulate 2, 1, 0 then fill 0, 1, 2, against accumulate /
    fill interleaved per dim, and against the restatement of three fused calls.  Payload: args["payload"] "typed" (default) or
    "ints"."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    typed = args.get("payload", "typed") == "typed"
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for axis in args.get("axes", [0, 1, 2]):
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        infos = [g.pencil_info(r, axis, halo, padding) for r in range(g.nranks)]
        if infos[rank].as_dict() != p.as_dict():
            failures.append("rank %d axis %d: pencil info differs from the oracle" % (rank, axis))
            continue
        wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
        for dtype in args.get("dtypes", AB.ALL_TYPES):
            nc, es = AB.TYPES[dtype][1], AB.element_bytes(dtype)
            add = (lambda x, y: AB.typed_add(dtype, x, y))  # noqa: E731  (bit patterns in, bit patterns out)
            work = cd.cudecompMalloc(h, gd, wsz * es)
            init = [_payload(dtype, typed, args.get("seed", 5), r, axis, infos[r].size, nc) for r in range(g.nranks)]
            mine = init[rank].view(np.uint8).reshape(-1)
            runs = [("dim %d" % d, "F%d" % d, "A%d Z%d" % (d, d), (d,)) for d in args.get("dims", (0, 1, 2))]
            if args.get("sequence"):
                runs.append(("dims 2 1 0", SEQUENCES["fused"], SEQUENCES["accumulate_then_fill"], (2, 1, 0)))
                runs.append(("dims 2 1 0 interleaved", SEQUENCES["fused"], SEQUENCES["interleaved"], (2, 1, 0)))
            for label, fused_ops, two_call_ops, dims in runs:
                where = "rank %d axis %d %s halo %s periods %s padding %s %s" % (rank, axis, AB.NAMES[dtype], tuple(halo), tuple(periods),
                                                                              tuple(padding), label)
                fused, twice = _guarded(mine), _guarded(mine)
                _run(fused_ops, axis, h, gd, fused.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream)
                kernel = cd.cudecompExtLastKernelName()
                _run(two_call_ops, axis, h, gd, twice.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream)
                torch.cuda.synchronize()
                want = [a.copy() for a in init]
                for dim in dims:
                    fused_reference(g, axis, halo, periods, dim, infos, want, add)
                restated = np.concatenate([np.full(SLACK, POISON, np.uint8), want[rank].view(np.uint8).reshape(-1), np.full(SLACK, POISON, np.uint8)])
                got = fused.cpu().numpy()
                for d in (_diff(got, twice.cpu().numpy(), es, "against the library's two calls"), _diff(got, restated, es, "against numpy")):
                    if d:
                        failures.append("%s: %s; last kernel %s" % (where, d, kernel))
            cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def deposit_loop(rank, nranks, args):
    """What the feature is for.  The existing loop (tests/fill_bodies.py): every step fill 0, 1, 2 -- deposit -- accumulate 2, 1,
    0.  The fused loop: fill 0, 1, 2 ONCE, then every step deposit -- fused 2, 1, 0.  Both start from the same pencil (zero in the
    interior, poison elsewhere) and deposit the same integers (exact in bf16 over three steps).  After every step the fused
    pencil must equal, over the whole guarded buffer, the existing loop's pencil with its ghost cells cleared (fill 0, 1, 2 on a
    copy: the clear the existing loop does at the start of its next step)."""
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
            n = int(p.size) * es
            old_raw = torch.full((2 * SLACK + n,), POISON, dtype=torch.uint8, device="cuda")
            old = old_raw[SLACK:SLACK + n].view(tdt[dtype])
            old[inside] = 0
            new_raw = old_raw.clone()
            new = new_raw[SLACK:SLACK + n].view(tdt[dtype])
            _run("Z0 Z1 Z2", axis, h, gd, new_raw.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream)
            for step in range(3):
                w = AB.initial_cells(1000 * step + 17, rank, axis, p.size, 1) % 3
                deposit = torch.from_numpy(w.reshape(-1).astype(np.float64)).cuda().to(tdt[dtype])
                _run("Z0 Z1 Z2", axis, h, gd, old_raw.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream)
                old += deposit
                _run("A2 A1 A0", axis, h, gd, old_raw.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream)
                new += deposit
                _run("F2 F1 F0", axis, h, gd, new_raw.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream)
                cleared = old_raw.clone()
                _run("Z0 Z1 Z2", axis, h, gd, cleared.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream)
                torch.cuda.synchronize()
                d = _diff(new_raw.cpu().numpy(), cleared.cpu().numpy(), es, "fused loop against the existing loop")
                if d:
                    failures.append("rank %d axis %d %s step %d: %s" % (rank, axis, AB.NAMES[dtype], step, d))
                if not bool((new[inside] == old[inside]).all()) or not bool((old[inside] > 0).any()):
                    failures.append("rank %d axis %d %s step %d: interiors differ, or nothing was deposited" % (rank, axis, AB.NAMES[dtype], step))
            cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def graph_replay(rank, nranks, args):
    """The three fused calls (dims 2, 1, 0) captured from the caller's stream into ONE hipGraph after an eager warm-up, replayed
    on fresh data: whole guarded pencils against the numpy restatement and against the library's two-call form run eagerly."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    axis, dtype = args.get("axis", 0), cd.DOUBLE
    es, nc = 8, 1
    infos = [g.pencil_info(r, axis, halo, padding) for r in range(g.nranks)]
    n = int(infos[rank].size) * es
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * es)
    add = lambda x, y: AB.typed_add(dtype, x, y)  # noqa: E731
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    data = torch.full((2 * SLACK + n,), POISON, dtype=torch.uint8, device="cuda")
    data[SLACK:SLACK + n] = 0
    with torch.cuda.stream(stream):
        _run(SEQUENCES["fused"], axis, h, gd, data.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        _run(SEQUENCES["fused"], axis, h, gd, data.data_ptr() + SLACK, work, dtype, halo, periods, padding, torch.cuda.current_stream().cuda_stream)
    for it in range(args.get("replays", 3)):
        want = [_payload(dtype, True, 100 + it, r, axis, infos[r].size, nc) for r in range(g.nranks)]
        mine = want[rank].view(np.uint8).reshape(-1).copy()
        for dim in (2, 1, 0):
            fused_reference(g, axis, halo, periods, dim, infos, want, add)
        restated = np.concatenate([np.full(SLACK, POISON, np.uint8), want[rank].view(np.uint8).reshape(-1), np.full(SLACK, POISON, np.uint8)])
        with torch.cuda.stream(stream):
            data.copy_(_guarded(mine))
            graph.replay()
            stream.synchronize()
            twice = _guarded(mine)
            _run(SEQUENCES["accumulate_then_fill"], axis, h, gd, twice.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream.cuda_stream)
            stream.synchronize()
        got = data.cpu().numpy()
        for d in (_diff(got, restated, es, "replay %d against numpy" % it), _diff(got, twice.cpu().numpy(), es, "replay %d against the two calls" % it)):
            if d:
                failures.append("rank %d: %s" % (rank, d))
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """A long run of kernels is enqueued on a stream, then the fused call along all three dims: the calls return while that work
    is still running (an event recorded behind them has not completed), and the pencil is right once it has."""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], (0, 0, 0)
    dtype, es = cd.DOUBLE, 8
    info = g.pencil_info(rank, 0, halo, padding)
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, 0, halo), 1) * es)
    init = _payload(dtype, True, 3, rank, 0, info.size, 1)
    mine = init.view(np.uint8).reshape(-1)
    data = _guarded(mine)
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    _run(SEQUENCES["fused"], 0, h, gd, data.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream.cuda_stream)  # warm-up
    data.copy_(_guarded(mine))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.get("kernels", 100)):
        big.add_(1.0)
    t1 = time.perf_counter()
    _run(SEQUENCES["fused"], 0, h, gd, data.data_ptr() + SLACK, work, dtype, halo, periods, padding, stream.cuda_stream)
    t2 = time.perf_counter()
    done = torch.cuda.Event()
    done.record(stream)
    pending = not done.query()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    want = [init.copy()]
    for dim in (2, 1, 0):
        fused_reference(g, 0, halo, periods, dim, [info], want, lambda x, y: AB.typed_add(dtype, x, y))
    restated = np.concatenate([np.full(SLACK, POISON, np.uint8), want[0].view(np.uint8).reshape(-1), np.full(SLACK, POISON, np.uint8)])
    diff = _diff(data.cpu().numpy(), restated, es, "against numpy")
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": [diff] if diff else [], "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3,
            "fused_host_ms": (t2 - t1) * 1e3, "total_ms": (t3 - t0) * 1e3}


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out
