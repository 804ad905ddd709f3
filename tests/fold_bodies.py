"""Halo folding (cudecomp_halo_fold.h: cudecompAmdFoldHalos{X,Y,Z}): the numpy restatement of the contract -- the definition cell
by cell, with the additions of tests/accumulate_bodies.py (typed_add) -- and the per-rank bodies of tests/test_gpu_halo_fold.py.
Everything is compared byte for byte, whole buffers with poison slack on both sides; there is no tolerance anywhere.

Pencils are arrays of BIT PATTERNS of shape (cells, reals per element), of the unsigned type as wide as one real.  Payloads are
finite: the non-integer draws of AB.typed_cells (every sum rounds, none overflows) with zeros of both signs and subnormals of
both signs in every seventh real; no NaN, no infinity, so every sum is specified to the bit.  Padding cells and the slack hold a
poison byte and must still hold it afterwards."""
import ctypes as C

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import accumulate_clear_bodies as ACB
from tests import reflect_bodies as RB

POISON = RB.POISON
SLACK = RB.SLACK
K_ROWS_FOLD, K_GENERIC_FOLD, K_ROWS_FOLD_TAKE, K_GENERIC_FOLD_TAKE = 18, 19, 20, 21
FOLD_MARK, NEGATE_MARK, ORDERED_MARK, CLEAR_MARK = 1 << 14, 1 << 13, 2, 1 << 9
ARITH_NAMES = ACB.ARITH_NAMES
TF = {False: "false", True: "true"}


def unsigned_of(dtype):
    return AB.FORMATS[AB.kind_of(dtype)][0]


def sign_bit(dtype):
    u, m, e = AB.FORMATS[AB.kind_of(dtype)]
    return u(1 << (m + e))


def arith_name(dtype):
    return {"fp16": "_Float16", "bf16": "__bf16", "fp32": "float", "fp64": "double"}[AB.kind_of(dtype)]


def rows_name(dtype, vb, stream, take):
    return "rows_fold_kernel<%s,%d,%d,%s>" % (arith_name(dtype), vb, stream, TF[bool(take)])


def generic_name(dtype, take):
    return "generic_fold_kernel<%s,%d,%s>" % (arith_name(dtype), AB.TYPES[dtype][1], TF[bool(take)])


_DRAWS = {}


def finite_bits(dtype, cells, seed):
    """the draw of _finite_bits, computed once per (type, cells, seed) and handed out as a copy"""
    key = (int(dtype), int(cells), int(seed))
    if key not in _DRAWS:
        if len(_DRAWS) > 256:
            _DRAWS.clear()
        _DRAWS[key] = _finite_bits(dtype, cells, seed)
    return _DRAWS[key].copy()


def _finite_bits(dtype, cells, seed):
    """(cells, reals per element) bit patterns of finite reals: AB.typed_cells, and in every seventh real one of +0, -0, the
    smallest subnormal, -3 of them, the largest subnormal of either sign"""
    u, m, e = AB.FORMATS[AB.kind_of(dtype)]
    nc = AB.TYPES[dtype][1]
    bits = AB.bits_of(dtype, AB.typed_cells(dtype, seed, 0, 0, int(cells), nc)).copy().reshape(-1)
    sign, ones = 1 << (m + e), (1 << m) - 1
    table = np.array([0, sign, 1, sign | 3, ones, sign | ones], dtype=u)
    at = np.arange(0, bits.size, 7)
    bits[at] = table[(at // 7) % 6]
    cls = AB.classes(AB.kind_of(dtype), bits)
    assert not cls["nan"].any() and not cls["inf"].any()
    return bits.reshape(-1, nc)


def int_bits(dtype, ints):
    """bit patterns (cells, nc) of an integer array (cells, nc)"""
    return AB.to_bytes(ints, dtype).view(unsigned_of(dtype)).reshape(ints.shape).copy()


def values_of(dtype, bits):
    """int64 values of bit patterns that hold small integers"""
    kind = AB.kind_of(dtype)
    if kind == "bf16":
        f = (np.ascontiguousarray(bits).astype(np.uint32) << 16).view(np.float32)
    else:
        f = np.ascontiguousarray(bits).view(AB._FLOAT_OF_KIND[kind])
    out = f.astype(np.int64)
    assert np.array_equal(out.astype(np.float64), f.astype(np.float64)), "a cell holds no integer"
    return out


def fold_add(dtype, dst, src, negate):
    """dst + src, or dst + (src with every sign bit flipped), on bit patterns: the flip first, then the addition of the type"""
    x = np.ascontiguousarray(src).copy()
    if negate:
        x ^= sign_bit(dtype)
    return AB.typed_add(dtype, np.ascontiguousarray(dst), x)


def fold_reference(p, bits, halo, dim, has_neighbour, parity, centering, clear, dtype):
    """THE DEFINITION on one pencil (info `p`), in place on `bits` ((cells, nc) bit patterns): on the sides without a neighbour
    (has_neighbour = (low, high)), the low side first: for k in [0, h) cell(h+k+c) += s * cell(h-1-k), then cell(n-h-1-k-c) += s *
    cell(n-h+k) along `dim`, over the other two dims with their halos and without their padding; with `clear` the ghost cells
    read hold zero bytes afterwards.  Returns the number of sides folded."""
    h, c = int(halo[dim]), int(centering)
    if h == 0:
        return 0
    ax, n = RB._dim_axis(p, dim)
    v = AB.pencil3(p, bits)
    sides = 0
    for side in (0, 1):
        if has_neighbour[side]:
            continue
        sides += 1
        for k in range(h):
            dst, src = (h + k + c, h - 1 - k) if side == 0 else (n - h - 1 - k - c, n - h + k)
            assert h <= dst < n - h, "the destination of a folded cell lies outside the interior"
            d, s = RB._unpadded(p), RB._unpadded(p)
            d[ax], s[ax] = dst, src
            v[tuple(d)] = fold_add(dtype, v[tuple(d)], v[tuple(s)], parity < 0)
            if clear:
                v[tuple(s)] = 0
    return sides


def nonpadding_mask(p):
    m = np.zeros(int(p.size), dtype=bool)
    AB.pencil3(p, m)[tuple(RB._unpadded(p))] = True
    return m


def interior_mask(p):
    m = np.zeros(int(p.size), dtype=bool)
    AB.pencil3(p, m)[RB.interior_index(p)] = True
    return m


def start_pencil(p, dtype, seed, payload=None):
    """(bit patterns (cells, nc), the same as bytes): finite payload in every non-padding cell, poison bytes in the padding"""
    u, nc = unsigned_of(dtype), AB.TYPES[dtype][1]
    bits = np.frombuffer(bytes([POISON]) * (int(p.size) * AB.element_bytes(dtype)), dtype=u).reshape(-1, nc).copy()
    keep = nonpadding_mask(p)
    bits[keep] = (finite_bits(dtype, int(p.size), seed) if payload is None else payload)[keep]
    return bits


def guarded(bits):
    raw = np.ascontiguousarray(bits).view(np.uint8).reshape(-1)
    return np.concatenate([np.full(SLACK, POISON, np.uint8), raw, np.full(SLACK, POISON, np.uint8)])


def first_difference(got, want, es):
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    return "%d bytes differ, first at byte %d (cell %d, byte %d of it; the pencil begins at byte %d)" % (
        bad.size, bad[0], (int(bad[0]) - SLACK) // es, (int(bad[0]) - SLACK) % es, SLACK)


def neighbours_of(g, rank, axis, periods):
    return [[g.shifted_rank(rank, axis, dim, side, bool(periods[dim])) >= 0 for side in (-1, 1)] for dim in range(3)]


# ---- GPU bodies ------------------------------------------------------------------------------------------------------------
def fold_sweep(rank, nranks, args):
    """cudecompAmdFoldHalos* on every rank of the job for every case of args["cases"] = [[axis, halo, periods, padding, dtype,
    parity, centering, clear], ...]: the fold along dims 2, 1, 0 in turn on a guarded pencil of finite reals; afterwards EVERY byte
    of the pencil and of the slack around it against the definition applied dim by dim.  args["single_dims"]: also every dim alone
    on a fresh pencil; and there, for the cases with clear = 1, the library's own clear = 0 result with zero bytes written into
    exactly the ghost slabs that were read (the sides without a neighbour along that dim) must equal the clear = 1 result.  A case
    the library refuses is a failure."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for n, case in enumerate(args["cases"]):
        axis, halo, periods, padding, dtype, parity, centering, clear = case
        es = AB.element_bytes(dtype)
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        info = g.pencil_info(rank, axis, halo, padding)
        what = "rank %d axis %d %s halo %s periods %s padding %s parity %d centering %d clear %d" % (
            rank, axis, AB.NAMES[dtype], tuple(halo), tuple(periods), tuple(padding), parity, centering, clear)
        if info.as_dict() != p.as_dict():
            failures.append(what + ": pencil info differs from the oracle")
            continue
        nb = neighbours_of(g, rank, axis, periods)
        start = start_pencil(p, dtype, 11 + n % 5)
        runs = [("dims 2 1 0", (2, 1, 0))] + ([("dim %d alone" % d, (d,)) for d in range(3)] if args.get("single_dims") else [])
        for label, dims in runs:
            dev = torch.from_numpy(guarded(start)).cuda()
            ptr = dev.data_ptr() + SLACK
            try:
                for dim in dims:
                    cd.cudecompFoldHalos(axis, h, gd, ptr, dtype, parity, centering, clear, halo, periods, dim, padding, stream)
            except cd.CudecompError as e:
                failures.append("%s %s: refused with code %d" % (what, label, e.code))
                continue
            kernel = cd.cudecompExtLastKernelName()
            torch.cuda.synchronize()
            got = dev.cpu().numpy()
            want = start.copy()
            for dim in dims:
                fold_reference(p, want, halo, dim, nb[dim], parity, centering, clear, dtype)
            diff = first_difference(got, guarded(want), es)
            if diff:
                failures.append("%s %s, against the definition: %s; last kernel %s" % (what, label, diff, kernel))
            if clear and len(dims) == 1:
                dim = dims[0]
                other = torch.from_numpy(guarded(start)).cuda()
                cd.cudecompFoldHalos(axis, h, gd, other.data_ptr() + SLACK, dtype, parity, centering, 0, halo, periods, dim, padding, stream)
                torch.cuda.synchronize()
                kept = other.cpu().numpy()
                body = kept[SLACK:kept.size - SLACK].reshape(-1, es)
                for side, which in ((0, "L"), (1, "H")):
                    if int(halo[dim]) and not nb[dim][side]:
                        AB.pencil3(p, body)[AB.slab(p, dim, which, int(halo[dim]))] = 0
                diff = first_difference(got, kept, es)
                if diff:
                    failures.append("%s %s, against clear = 0 and zero bytes into the ghost cells read: %s" % (what, label, diff))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def adjoint(rank, nranks, args):
    """<S x, y> and <x, S^T y> of this rank, in int64 on the host, for every case of args["cases"] = [[axis, halo, periods,
    padding, dtype, parity, centering], ...].  S: (update, reflection) for dims 0, 1, 2 on x, integers in [-3, 3] in the interior
    and zero elsewhere.  S^T: (accumulation, fold with clear = 0) for dims 2, 1, 0 on y, integers in [-3, 3] in every non-padding
    cell.  <S x, y> runs over the non-padding cells, <x, S^T y> over the interior.  Every value that arises is an integer of
    magnitude below 256: exact in every type, bf16 included.  Also <x, S'^T y> with the fold LEFT OUT of the first non-periodic dim
    that has a halo (None when there is none): what the identity must be able to tell from S^T.  All of it for TWO independent
    draws of x, so that a chance equality of two integer sums in one of them (about one in a few hundred) cannot hide that.
    Returns one [[lhs, rhs, broken], [lhs, rhs, broken]] per case; the caller adds them over the ranks."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    wsz = max(max(cd.cudecompGetHaloWorkspaceSize(h, gd, c[0], c[1]) for c in args["cases"]), 1)
    work = cd.cudecompMalloc(h, gd, wsz * 16)
    for n, case in enumerate(args["cases"]):
        axis, halo, periods, padding, dtype, parity, centering = case
        nc = AB.TYPES[dtype][1]
        p = g.pencil_info(rank, axis, halo, padding)
        rng = np.random.default_rng([41, n, rank])
        inside, cells = interior_mask(p), nonpadding_mask(p)
        xs = [rng.integers(-3, 4, size=(int(p.size), nc)) * inside[:, None] for _ in range(2)]
        y = rng.integers(-3, 4, size=(int(p.size), nc)) * cells[:, None]

        def run(ints, ops):
            dev = torch.from_numpy(guarded(int_bits(dtype, ints))).cuda()
            ptr = dev.data_ptr() + SLACK
            for op, dim in ops:
                if op == "U":
                    cd.cudecompUpdateHalos(axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream)
                elif op == "R":
                    cd.cudecompReflectHalos(axis, h, gd, ptr, dtype, parity, centering, halo, periods, dim, padding, stream)
                elif op == "A":
                    cd.cudecompAccumulateHalos(axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream)
                else:
                    cd.cudecompFoldHalos(axis, h, gd, ptr, dtype, parity, centering, 0, halo, periods, dim, padding, stream)
            torch.cuda.synchronize()
            raw = dev.cpu().numpy()
            return values_of(dtype, raw[SLACK:raw.size - SLACK].view(unsigned_of(dtype)).reshape(-1, nc))

        transposed = [(op, dim) for dim in (2, 1, 0) for op in "AF"]
        sty = run(y, transposed)
        walls = [d for d in range(3) if not periods[d] and int(halo[d])]
        left_out = run(y, [o for o in transposed if o != ("F", walls[0])]) if walls else None
        draws = []
        for x in xs:
            sx = run(x, [(op, dim) for dim in (0, 1, 2) for op in "UR"])
            lhs = int((sx[cells] * y[cells]).sum())
            rhs = int((x[inside] * sty[inside]).sum())
            draws.append([lhs, rhs, int((x[inside] * left_out[inside]).sum()) if walls else None])
        out.append(draws)
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return out


def _scatter_close(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, sptr):
    """what closes a wall-bounded scatter step, through the C entry points: (accumulate-and-clear, fold with clear = 1) for dims
    2, 1, 0"""
    acc, fold = getattr(L, "cudecompAmdAccumulateAndClearHalos" + "XYZ"[axis]), getattr(L, "cudecompAmdFoldHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    per = b3(*[bool(x) for x in periods])
    for dim in (2, 1, 0):
        rc = acc(h, gd, ptr, work, dtype, i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc
        rc = fold(h, gd, ptr, dtype, parity, centering, 1, i3(*halo), per, dim, i3(*padding), sptr)
        assert rc == cd.RESULT_SUCCESS, rc


def _scatter_close_reference(g, p, start, axis, halo, periods, parity, centering, dtype):
    """... and in numpy, single rank: the fused accumulation of tests/accumulate_clear_bodies.py, then the fold's definition"""
    want = [start.copy()]
    nb = neighbours_of(g, 0, axis, periods)
    keep = start.copy()
    for dim in (2, 1, 0):
        ACB.fused_reference(g, axis, halo, periods, dim, [p], want, lambda a, b: AB.typed_add(dtype, a, b))
        fold_reference(p, want[0], halo, dim, nb[dim], parity, centering, 1, dtype)
    # (the accumulation's slabs exclude the padding, whose poison therefore stays)
    pad = ~nonpadding_mask(p)
    assert np.array_equal(want[0][pad], keep[pad])
    return want[0]


def graph_replay(rank, nranks, args):
    """(accumulate-and-clear, fold with clear = 1) for dims 2, 1, 0 captured from the caller's stream into one hipGraph after an
    eager warm-up, replayed on fresh data: every replay leaves the pencil numpy names for the data it found -- and no non-zero
    ghost cell."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype = args.get("axis", 0), args.get("dtype", cd.DOUBLE)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    parity, centering = args.get("parity", -1), args.get("centering", 0)
    es = AB.element_bytes(dtype)
    L = cd.lib()
    p = g.pencil_info(0, axis, halo, padding)
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * es)
    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    dev = torch.from_numpy(guarded(start_pencil(p, dtype, 1))).cuda()
    ptr = dev.data_ptr() + SLACK
    with torch.cuda.stream(stream):
        _scatter_close(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        _scatter_close(L, axis, h, gd, ptr, work, dtype, parity, centering, halo, periods, padding, torch.cuda.current_stream().cuda_stream)
    ghosts = nonpadding_mask(p) & ~interior_mask(p)
    for it in range(args.get("replays", 2)):
        start = start_pencil(p, dtype, 100 + it)  # fresh data every time
        want = _scatter_close_reference(g, p, start, axis, halo, periods, parity, centering, dtype)
        with torch.cuda.stream(stream):
            dev.copy_(torch.from_numpy(guarded(start)))
            graph.replay()
            stream.synchronize()
        got = dev.cpu().numpy()
        diff = first_difference(got, guarded(want), es)
        if diff:
            failures.append("replay %d: %s" % (it, diff))
        if np.any(got[SLACK:got.size - SLACK].reshape(-1, es)[ghosts]):
            failures.append("replay %d: a ghost cell is not zero after the scatter step was closed" % it)
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """A long run of kernels is enqueued on a stream, then folds along all three dims: the calls return while that work is still
    running (an event recorded behind them has not completed), and the pencil is right once it has."""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], (0, 0, 0)
    dtype, es = cd.DOUBLE, 8
    p = g.pencil_info(0, 0, halo, padding)
    start = start_pencil(p, dtype, 5)
    nb = neighbours_of(g, 0, 0, periods)
    want = start.copy()
    for dim in (2, 1, 0):
        fold_reference(p, want, halo, dim, nb[dim], -1, 1, 1, dtype)
    dev = torch.from_numpy(guarded(start)).cuda()
    ptr = dev.data_ptr() + SLACK
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    for dim in (2, 1, 0):  # warm-up: first-use work happens before the timed part
        cd.cudecompFoldHalos(0, h, gd, ptr, dtype, -1, 1, 1, halo, periods, dim, padding, stream.cuda_stream)
    dev.copy_(torch.from_numpy(guarded(start)))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.get("kernels", 100)):
        big.add_(1.0)
    t1 = time.perf_counter()
    for dim in (2, 1, 0):
        cd.cudecompFoldHalos(0, h, gd, ptr, dtype, -1, 1, 1, halo, periods, dim, padding, stream.cuda_stream)
    t2 = time.perf_counter()
    done = torch.cuda.Event()
    done.record(stream)
    pending = not done.query()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    diff = first_difference(dev.cpu().numpy(), guarded(want), es)
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": [diff] if diff else [], "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3,
            "fold_host_ms": (t2 - t1) * 1e3, "total_ms": (t3 - t0) * 1e3}


# ---- refusals through the C ABI (no kernel runs: callable with and without a device) ----------------------------------------
def check_entry_points():
    """what the reflection refuses is refused here with the reflection's code, whatever `clear` is; a tuple the reflection accepts
    is INVALID_USAGE for clear -1 / 2, also when every halo is zero; a mirror that reaches beyond the interior is refused only
    where a side would be folded"""
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    refused = [(h, gd, 1, cd.FLOAT, None, None, 0, None, None),                  # halo_extents NULL
               (h, gd, None, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),        # input NULL
               (h, gd, 1, cd.FLOAT, i3(1, 1, 1), None, 3, None, None),           # dim out of range
               (h, gd, 1, cd.FLOAT, i3(1, 1, 1), None, -1, None, None),
               (h, gd, 1, 99, i3(1, 1, 1), None, 0, None, None),                 # unknown data type
               (h, None, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),         # no descriptor
               (None, gd, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),        # no handle
               (h, gd, None, 99, None, None, 5, None, None)]                     # several at once: the first check decides
    accepted = [(h, gd, None, cd.FLOAT, i3(0, 0, 0), None, 0, None, None),        # all halos zero: success before input is looked at
                (h, gd, None, cd.FLOAT, i3(0, 0, 0), None, 7, None, None),
                (h, gd, 1, cd.DOUBLE, i3(1, 0, 1), None, 1, i3(1, 2, 0), None),   # h == 0 along dim: success, no effect
                (h, gd, 1, cd.FLOAT, i3(9, 0, 0), b3(True, False, False), 0, None, None)]  # periodic: nothing to fold
    mirrors = [(1, 0), (-1, 1), (0, 0), (2, 1), (1, -1), (-1, 2)]
    for name in cd.AMD_FOLD_SYMBOLS:
        fn, reflect = getattr(L, name), getattr(L, name.replace("Fold", "Reflect"))
        for hh, g, inp, dtype, halo, per, dim, pad, stream in refused:
            for parity, centering in mirrors:
                want = reflect(hh, g, inp, dtype, parity, centering, halo, per, dim, pad, stream)
                assert want != cd.RESULT_SUCCESS
                for clear in (0, 1, 2, -1):
                    assert fn(hh, g, inp, dtype, parity, centering, clear, halo, per, dim, pad, stream) == want, (name, dim, parity, centering, clear)
        for hh, g, inp, dtype, halo, per, dim, pad, stream in accepted:
            for parity, centering in mirrors:
                want = reflect(hh, g, inp, dtype, parity, centering, halo, per, dim, pad, stream)
                assert want == (cd.RESULT_SUCCESS if (parity, centering) in mirrors[:2] else cd.RESULT_INVALID_USAGE)
                for clear in (0, 1):
                    assert fn(hh, g, inp, dtype, parity, centering, clear, halo, per, dim, pad, stream) == want, (name, dim, parity, centering, clear)
                for clear in (2, -1):
                    assert fn(hh, g, inp, dtype, parity, centering, clear, halo, per, dim, pad, stream) == cd.RESULT_INVALID_USAGE
        # h + centering one above the interior (X: 9 cells, h = 9, centering 1): refused before the device or the pointer is looked
        # at, whatever `clear` is -- unless the dim is periodic and nothing would be folded
        for parity, clear in ((1, 0), (-1, 1), (1, 2)):
            assert fn(h, gd, 1, cd.FLOAT, parity, 1, clear, i3(9, 0, 0), None, 0, None, None) == cd.RESULT_INVALID_USAGE
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out
