"""Bodies of the multi-field wall halo tests (cudecomp_halo_wall_fields.h), run in the test process or on several ranks through
tests/mp.py.  The reference of everything here is the single calls (cudecompAmdReflectHalos*, cudecompAmdFoldHalos*) on clones of
the same fields, whose own definitions tests/reflect_bodies.py and tests/fold_bodies.py hold; every comparison is byte for byte over
the whole pencil and the slack around it."""
import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fold_bodies as FB
from tests import reflect_bodies as RB

SLACK = FB.SLACK
OPS = (("reflect", 0), ("fold", 0), ("fold", 1))  # (operation, clear)


def parities_of(n, k=0):
    """mixed for every n >= 2: -1, +1, -1, -1, +1, ... shifted by k"""
    return [1 if (f + k) % 3 == 1 else -1 for f in range(n)]


def _single(op, clear, axis, h, gd, ptr, dtype, parity, centering, halo, periods, dim, padding, stream):
    if op == "reflect":
        cd.cudecompReflectHalos(axis, h, gd, ptr, dtype, parity, centering, halo, periods, dim, padding, stream)
    else:
        cd.cudecompFoldHalos(axis, h, gd, ptr, dtype, parity, centering, clear, halo, periods, dim, padding, stream)


def _fields(op, clear, axis, h, gd, ptrs, dtype, parities, centering, halo, periods, dim, padding, stream):
    if op == "reflect":
        cd.cudecompReflectFieldHalos(axis, h, gd, ptrs, dtype, parities, centering, halo, periods, dim, padding, stream)
    else:
        cd.cudecompFoldFieldHalos(axis, h, gd, ptrs, dtype, parities, centering, clear, halo, periods, dim, padding, stream)


def _sides(g, rank, axis, periods, halo, dim):
    """sides of this rank along `dim` that are walls and have ghost cells"""
    nb = FB.neighbours_of(g, rank, axis, periods)[dim]
    return 0 if int(halo[dim]) == 0 else sum(1 for has in nb if not has)


def wall_sweep(rank, nranks, args):
    """For every axis, dim, centering, operation (reflection, fold, fold that clears), data type and field count of args: single calls
    with parities[f] on clones (made on the device), ONE field call on the originals, whole buffers compared.  A tuple the single call
    refuses must be refused by the field call with the same code and leave the fields alone.  Launches, by the data-launch counter: 0
    where there is no wall side, else 1 -- 2 for a fold whose sides add onto the same cells (n < 4h + 2c, both sides walls), in which
    case the single call makes 2 as well; a call without a wall side must leave every field as it found it ("idle" counts them).
    Returns {"failures", "drawn", "accepted", "launching", "ordered", "idle"}."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    out = {"failures": [], "drawn": 0, "accepted": 0, "launching": 0, "ordered": 0, "idle": 0}
    fails = out["failures"]
    most = max(args["n_fields"])
    for axis in args.get("axes", range(3)):
        p = g.pencil_info(rank, axis, halo, padding)
        for dtype in args["dtypes"]:
            es = AB.element_bytes(dtype)
            base = [torch.from_numpy(FB.guarded(FB.start_pencil(p, dtype, 31 + 7 * f + rank))).cuda() for f in range(most)]
            for dim, centering, (op, clear), n in ((d, c, o, n) for d in args.get("dims", range(3)) for c in args.get("centerings", (0, 1))
                                                   for o in OPS for n in args["n_fields"]):
                out["drawn"] += 1
                what = "rank %d axis %d dim %d %s %s clear %d centering %d, %d fields" % (rank, axis, dim, AB.NAMES[dtype], op, clear, centering, n)
                parities = args.get("parities") or parities_of(n, dim + centering)
                ones = [b.clone() for b in base[:n]]
                refused = None
                count = cd.cudecompExtDataLaunchCount()
                try:
                    for f in range(n):
                        _single(op, clear, axis, h, gd, ones[f].data_ptr() + SLACK, dtype, parities[f], centering, halo, periods, dim, padding, stream)
                except cd.CudecompError as e:
                    refused = e.code
                single_launches = (cd.cudecompExtDataLaunchCount() - count) // n if refused is None else 0
                single_name = cd.cudecompExtLastKernelName()
                many = [b.clone() for b in base[:n]]
                count = cd.cudecompExtDataLaunchCount()
                try:
                    _fields(op, clear, axis, h, gd, [t.data_ptr() + SLACK for t in many], dtype, parities, centering, halo, periods, dim, padding, stream)
                    code = None
                except cd.CudecompError as e:
                    code = e.code
                launches = cd.cudecompExtDataLaunchCount() - count
                name = cd.cudecompExtLastKernelName()
                torch.cuda.synchronize()
                if refused is not None or code is not None:
                    if refused != code:
                        fails.append("%s: the single call answers %s, the field call %s" % (what, refused, code))
                    if launches or any(not torch.equal(many[f], base[f]) for f in range(n)):
                        fails.append("%s: a refused call launched or wrote" % what)
                    continue
                out["accepted"] += 1
                for f in range(n):
                    if not torch.equal(many[f], ones[f]):
                        diff = FB.first_difference(many[f].cpu().numpy(), ones[f].cpu().numpy(), es)
                        fails.append("%s, field %d (parity %+d): %s; kernel %s, the single call's %s" % (what, f, parities[f], diff, name, single_name))
                sides = _sides(g, rank, axis, periods, halo, dim)
                n_ext = RB._dim_axis(p, dim)[1]
                ordered = op == "fold" and sides == 2 and n_ext < 4 * int(halo[dim]) + 2 * centering
                want = 0 if sides == 0 else (2 if ordered else 1)
                out["launching"] += sides > 0
                if sides == 0:
                    out["idle"] += 1
                    if any(not torch.equal(many[f], base[f]) for f in range(n)):
                        fails.append("%s: no wall side, yet a field changed" % what)
                out["ordered"] += ordered
                if launches != want or single_launches != want:
                    fails.append("%s: %d launches (the single call %d), expected %d" % (what, launches, single_launches, want))
                family = name.split("_fields_")[1].split("_kernel")[0] if "_fields_" in name else name
                if sides and n >= 2 and not (name.startswith(("rows_fields_", "generic_fields_")) and family == op):
                    fails.append("%s: kernel %s" % (what, name))
                if sides and n == 1 and name != single_name:
                    fails.append("%s: one field ran %s, the single call %s" % (what, name, single_name))
    cd.cudecompGridDescDestroy(h, gd)
    return out


def plan_cache(rank, nranks, args):
    """two field calls that differ only in their parities add ONE plan to the descriptor's cache; another field count, centering,
    `clear` or operation adds another; one field with another parity adds another (the single call's plan carries its sign)"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    halo, periods, dtype = (2, 1, 1), (False, True, False), cd.DOUBLE
    p = g.pencil_info(rank, 0, halo, (0, 0, 0))
    dev = [torch.from_numpy(FB.guarded(FB.start_pencil(p, dtype, 3 + f))).cuda() for f in range(3)]
    ptrs = [t.data_ptr() + SLACK for t in dev]
    steps = []

    def grew(call):
        before = cd.cudecompExtHaloPlanCount(h, gd)
        call()
        steps.append(cd.cudecompExtHaloPlanCount(h, gd) - before)

    grew(lambda: cd.cudecompReflectFieldHalos(0, h, gd, ptrs, dtype, [1, 1, 1], 0, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompReflectFieldHalos(0, h, gd, ptrs, dtype, [-1, 1, -1], 0, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompReflectFieldHalos(0, h, gd, ptrs, dtype, [-1, -1, -1], 0, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompFoldFieldHalos(0, h, gd, ptrs, dtype, [1, -1, 1], 0, 1, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompFoldFieldHalos(0, h, gd, ptrs, dtype, [-1, -1, 1], 0, 1, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompFoldFieldHalos(0, h, gd, ptrs, dtype, [-1, -1, 1], 0, 0, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompReflectFieldHalos(0, h, gd, ptrs, dtype, [-1, 1, -1], 1, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompReflectFieldHalos(0, h, gd, ptrs[:2], dtype, [-1, 1], 0, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompReflectFieldHalos(0, h, gd, ptrs[:1], dtype, [1], 0, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompReflectFieldHalos(0, h, gd, ptrs[:1], dtype, [-1], 0, halo, periods, 0, None, stream))
    grew(lambda: cd.cudecompReflectHalos(0, h, gd, ptrs[0], dtype, -1, 0, halo, periods, 0, None, stream))  # (the same plan)
    torch.cuda.synchronize()
    cd.cudecompGridDescDestroy(h, gd)
    return steps


def sequence(rank, nranks, args):
    """single rank, fp64, positive integers in the interior and poison elsewhere: (update, field reflection) for dims 0, 1, 2 fills
    every ghost cell of every field; a cell reached through r reflected dims carries parities[f] ** r times the interior value numpy's
    pad names (symmetric for centering 0, reflect for centering 1; wrap along the periodic dims)"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    halo, periods, axis, dtype = args["halo"], args["periods"], args.get("axis", 0), cd.DOUBLE
    parities = args["parities"]
    n = len(parities)
    p = g.pencil_info(rank, axis, halo, (0, 0, 0))
    work = cd.cudecompMalloc(h, gd, n * max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * 8)  # (n single workspaces)
    failures = []
    for centering in (0, 1):
        rng = np.random.default_rng([5, centering])
        inner = RB.interior_index(p)
        starts, wants = [], []
        for f in range(n):
            v = np.full(int(p.size), np.nan)
            cube = AB.pencil3(p, v)
            cube[inner] = rng.integers(1, 100, size=cube[inner].shape)
            want, sign = cube[inner].copy(), np.ones(cube[inner].shape)
            for dim in range(3):
                ax, hd = RB._dim_axis(p, dim)[0], int(halo[dim])
                pad = [(hd, hd) if a == ax else (0, 0) for a in range(3)]
                mode = "wrap" if periods[dim] else ("symmetric" if centering == 0 else "reflect")
                want, sign = np.pad(want, pad, mode=mode), np.pad(sign, pad, mode=mode)
                if not periods[dim] and hd:  # (the ghost slabs of a reflected dim: the sign of the cell they mirror, times the parity)
                    lo, hi = [slice(None)] * 3, [slice(None)] * 3
                    lo[ax], hi[ax] = slice(0, hd), slice(sign.shape[ax] - hd, sign.shape[ax])
                    sign[tuple(lo)] *= parities[f]
                    sign[tuple(hi)] *= parities[f]
            starts.append(v)
            wants.append(want * sign)
        dev = [torch.from_numpy(FB.guarded(s.view(np.uint64).reshape(-1, 1))).cuda() for s in starts]
        ptrs = [t.data_ptr() + SLACK for t in dev]
        for dim in range(3):
            cd.cudecompUpdateFieldHalos(axis, h, gd, ptrs, work, dtype, halo, periods, dim, None, stream)
            cd.cudecompReflectFieldHalos(axis, h, gd, ptrs, dtype, parities, centering, halo, periods, dim, None, stream)
        torch.cuda.synchronize()
        for f in range(n):
            raw = dev[f].cpu().numpy()
            got = AB.pencil3(p, raw[SLACK:raw.size - SLACK].view(np.float64))
            if got.shape != wants[f].shape or not np.array_equal(got.view(np.uint64), wants[f].view(np.uint64)):
                failures.append("centering %d field %d (parity %+d): %d cells differ" % (
                    centering, f, parities[f], -1 if got.shape != wants[f].shape else int((got.view(np.uint64) != wants[f].view(np.uint64)).sum())))
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def adjoint(rank, nranks, args):
    """small integers in fp64: sum over the fields of <R x_f, y_f> against sum of <x_f, F y_f>, R the field reflections along dims 0,
    1, 2, F the field folds (clear 0) along dims 2, 1, 0; x is zero outside the interior (as tests/fold_bodies.py adjoint has it), y
    lives in every non-padding cell.  Also with one field's parity flipped in F only: what the identity must tell apart.  Returns
    [[lhs, rhs, broken], ...] per centering."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    halo, periods, padding, axis, dtype = args["halo"], args["periods"], args.get("padding", (0, 0, 0)), args.get("axis", 0), cd.DOUBLE
    parities = args["parities"]
    n = len(parities)
    p = g.pencil_info(rank, axis, halo, padding)
    inside, cells = FB.interior_mask(p), FB.nonpadding_mask(p)
    out = []

    def run(ints, fold, par, centering):
        dev = [torch.from_numpy(FB.guarded(FB.int_bits(dtype, a))).cuda() for a in ints]
        ptrs = [t.data_ptr() + SLACK for t in dev]
        for dim in ((2, 1, 0) if fold else (0, 1, 2)):
            if fold:
                cd.cudecompFoldFieldHalos(axis, h, gd, ptrs, dtype, par, centering, 0, halo, periods, dim, padding, stream)
            else:
                cd.cudecompReflectFieldHalos(axis, h, gd, ptrs, dtype, par, centering, halo, periods, dim, padding, stream)
        torch.cuda.synchronize()
        res = []
        for t in dev:
            raw = t.cpu().numpy()
            res.append(FB.values_of(dtype, raw[SLACK:raw.size - SLACK].view(FB.unsigned_of(dtype)).reshape(-1, 1)))
        return res

    for centering in (0, 1):
        rng = np.random.default_rng([43, centering])
        xs = [rng.integers(-3, 4, size=(int(p.size), 1)) * inside[:, None] for _ in range(n)]
        ys = [rng.integers(-3, 4, size=(int(p.size), 1)) * cells[:, None] for _ in range(n)]
        rx, fy = run(xs, False, parities, centering), run(ys, True, parities, centering)
        other = [-parities[0]] + list(parities[1:])
        gy = run(ys, True, other, centering)
        lhs = sum(int((rx[f][cells] * ys[f][cells]).sum()) for f in range(n))
        rhs = sum(int((xs[f][inside] * fy[f][inside]).sum()) for f in range(n))
        broken = sum(int((xs[f][inside] * gy[f][inside]).sum()) for f in range(n))
        out.append([lhs, rhs, broken])
    cd.cudecompGridDescDestroy(h, gd)
    return out


def graph_replay(rank, nranks, args):
    """a field reflection and a field fold (args["clear"]) along every walled dim captured from the caller's stream into one hipGraph
    after an eager warm-up; the host arrays of pointers and parities are temporaries that are gone before the replays; every replay,
    on refilled fields, leaves what the single calls make of clones"""
    import gc

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype, clear = args.get("axis", 0), args.get("dtype", cd.DOUBLE), args["clear"]
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    parities, centering = args["parities"], args.get("centering", 0)
    n = len(parities)
    es = AB.element_bytes(dtype)
    p = g.pencil_info(0, axis, halo, padding)
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    dev = [torch.from_numpy(FB.guarded(FB.start_pencil(p, dtype, 1 + f))).cuda() for f in range(n)]

    def both(sptr):
        ptrs = [t.data_ptr() + SLACK for t in dev]  # (fresh host arrays inside the wrappers: gone when they return)
        for dim in (2, 1, 0):
            cd.cudecompReflectFieldHalos(axis, h, gd, ptrs, dtype, list(parities), centering, halo, periods, dim, padding, sptr)
            cd.cudecompFoldFieldHalos(axis, h, gd, ptrs, dtype, list(parities), centering, clear, halo, periods, dim, padding, sptr)
        del ptrs

    with torch.cuda.stream(stream):
        both(stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        both(torch.cuda.current_stream().cuda_stream)
    gc.collect()
    for it in range(args.get("replays", 2)):
        starts = [torch.from_numpy(FB.guarded(FB.start_pencil(p, dtype, 100 + 10 * it + f))).cuda() for f in range(n)]
        ones = [s.clone() for s in starts]
        cur = torch.cuda.current_stream().cuda_stream
        for f in range(n):
            for dim in (2, 1, 0):
                _single("reflect", 0, axis, h, gd, ones[f].data_ptr() + SLACK, dtype, parities[f], centering, halo, periods, dim, padding, cur)
                _single("fold", clear, axis, h, gd, ones[f].data_ptr() + SLACK, dtype, parities[f], centering, halo, periods, dim, padding, cur)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            for f in range(n):
                dev[f].copy_(starts[f])
            graph.replay()
            stream.synchronize()
        for f in range(n):
            if torch.equal(dev[f], starts[f]):
                failures.append("replay %d field %d: nothing was written" % (it, f))
            if not torch.equal(dev[f], ones[f]):
                failures.append("replay %d field %d: %s" % (it, f, FB.first_difference(dev[f].cpu().numpy(), ones[f].cpu().numpy(), es)))
    del graph
    cd.cudecompGridDescDestroy(h, gd)
    return failures
