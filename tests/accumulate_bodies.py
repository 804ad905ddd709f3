"""Halo accumulation (cudecomp_amd.h: cudecompAmdAccumulateHalos{X,Y,Z}): the numpy restatement of the contract, payloads in
all seven data types, and the per-rank bodies of tests/test_gpu_halo_accumulate.py.

The restatement works on INTEGER arrays of shape (cells, reals per element): the test payload is an integer 0..7 in every
cell (halos and padding included), any cell ends up as a sum of at most 27 cells (<= 189), and such integers are exact in
every element type, bf16 included (8 significand bits hold up to 256) -- so the expected pencil is computed once in int64 and
compared bit for bit in the type under test.  Every rank can build every rank's initial pencil (seeded by rank and axis) and
therefore the expected value of every cell of its own pencil.

What is ADDED is stated a second time, without the code under test and without torch: typed_add (IEEE addition of numpy for
fp16 / fp32 / fp64; bf16 from numpy integers and fp32 alone), pinned by tests/test_accumulate_reference.py.  It serves the edge
value payloads of the kernel tests (edge_table, all_pairs, the three dense draws) and the payload="typed" mode of the
restatement: non-integer reals, every sum rounds, so the ORDER of the two additions on overlapping faces shows in the bits.
Comparison rule of everything typed (mismatches): where the expected real is a NaN the device real must be a NaN -- sign and
payload are unspecified by the contract --, every other real is compared bit for bit."""
import numpy as np

import cudecomp_amd as cd

# dtype -> (numpy type of one real, reals per element)
TYPES = {cd.FLOAT: (np.float32, 1), cd.DOUBLE: (np.float64, 1), cd.FLOAT_COMPLEX: (np.float32, 2),
         cd.DOUBLE_COMPLEX: (np.float64, 2), cd.HALF: (np.float16, 1), cd.BFLOAT16: ("bf16", 1), cd.HALF_COMPLEX: (np.float16, 2)}
NAMES = {cd.FLOAT: "fp32", cd.DOUBLE: "fp64", cd.FLOAT_COMPLEX: "complex64", cd.DOUBLE_COMPLEX: "complex128", cd.HALF: "fp16",
         cd.BFLOAT16: "bf16", cd.HALF_COMPLEX: "complex_fp16"}
ALL_TYPES = list(TYPES)


def real_bytes(dtype):
    return 2 if TYPES[dtype][0] == "bf16" else np.dtype(TYPES[dtype][0]).itemsize


def element_bytes(dtype):
    return real_bytes(dtype) * TYPES[dtype][1]


def to_bytes(values, dtype):
    """bit patterns (uint8 array) of float64 / integer `values` (any shape) converted to the reals of `dtype`; bf16 by
    truncating fp32 -- exact for everything the tests store (the callers round beforehand where they need rounding)"""
    real = TYPES[dtype][0]
    v = np.ascontiguousarray(values)
    if real == "bf16":
        f = v.astype(np.float32)
        assert np.all((f.view(np.uint32) & 0xffff) == 0), "value is not a bf16 number"
        return np.ascontiguousarray((f.view(np.uint32) >> 16).astype(np.uint16)).view(np.uint8).reshape(-1)
    out = v.astype(real)
    assert np.array_equal(out.astype(np.float64), v.astype(np.float64)), "value is not exact in the element type"
    return out.view(np.uint8).reshape(-1)


# ---- the arithmetic in numpy ------------------------------------------------------------------------------------------------
# real kind -> (unsigned type of its bit pattern, significand bits stored, exponent bits)
FORMATS = {"fp16": (np.uint16, 10, 5), "bf16": (np.uint16, 7, 8), "fp32": (np.uint32, 23, 8), "fp64": (np.uint64, 52, 11)}
_KIND_OF_REAL = {np.float16: "fp16", "bf16": "bf16", np.float32: "fp32", np.float64: "fp64"}
_FLOAT_OF_KIND = {"fp16": np.float16, "fp32": np.float32, "fp64": np.float64}


def kind_of(dtype):
    """"fp16" / "bf16" / "fp32" / "fp64": the format of one real of `dtype`"""
    return _KIND_OF_REAL[TYPES[dtype][0]]


def typed_add(dtype, a, b):
    """a + b, real by real, in the arithmetic the contract states for `dtype`.  a, b: arrays of the
    reals' bit patterns (unsigned integers of the real's width; the only form for bf16) or of the native numpy type; the result
    has the form of `a`.  fp16 / fp32 / fp64: numpy's IEEE addition.  bf16: widen by << 16, add in fp32, round to nearest even
    with integers; a NaN sum gives the quiet NaN 0x7fc0 (which NaN comes out is unspecified: compare NaNs by class)."""
    kind = kind_of(dtype)
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(all="ignore"):
        if kind != "bf16":
            f = _FLOAT_OF_KIND[kind]
            if a.dtype == f:
                return a + b.astype(f, copy=False)
            assert a.dtype == FORMATS[kind][0] and b.dtype == a.dtype, (a.dtype, b.dtype)
            return (a.view(f) + b.view(f)).view(a.dtype)
        assert a.dtype == np.uint16 and b.dtype == np.uint16, (a.dtype, b.dtype)
        s = (a.astype(np.uint32) << 16).view(np.float32) + (b.astype(np.uint32) << 16).view(np.float32)
        u = np.ascontiguousarray(s).view(np.uint32).astype(np.uint64)
        r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        return np.where(np.isnan(s), np.uint16(0x7fc0), r)


def bits_of(dtype, x):
    """the bit patterns (unsigned integers) of an array of reals in either form typed_add takes"""
    x = np.ascontiguousarray(x)
    return x if x.dtype.kind == "u" else x.view(FORMATS[kind_of(dtype)][0])


def classes(kind, bits):
    """dict of boolean masks nan / inf / zero / subnormal of an array of bit patterns -- from the patterns (numpy has no bf16)"""
    u, m, e = FORMATS[kind]
    bits = np.asarray(bits, dtype=u)
    expo = (bits >> u(m)) & u((1 << e) - 1)
    mant = bits & u((1 << m) - 1)
    top = u((1 << e) - 1)
    return {"nan": (expo == top) & (mant != 0), "inf": (expo == top) & (mant == 0), "zero": (expo == 0) & (mant == 0),
            "subnormal": (expo == 0) & (mant != 0)}


def mismatches(kind, got, want):
    """boolean mask of the reals (bit patterns) that break the comparison rule: expected NaN -> any NaN; otherwise bit-identical"""
    want_nan = classes(kind, want)["nan"]
    return np.where(want_nan, ~classes(kind, got)["nan"], np.asarray(got) != np.asarray(want))


def edge_table(kind):
    """24 bit patterns built from the format's parameters: the values at which an addition changes regime"""
    u, m, e = FORMATS[kind]
    bias, top = (1 << (e - 1)) - 1, (1 << e) - 1
    ones = (1 << m) - 1

    def pat(sign, expo, mant):
        return (sign << (m + e)) | (expo << m) | mant

    t = []
    for expo, mant in ((0, 0), (0, 1), (0, ones), (1, 0), (bias, 0)):  # zero, smallest / largest subnormal, smallest normal, one
        t += [pat(0, expo, mant), pat(1, expo, mant)]
    t += [pat(0, bias, 1), pat(0, bias - m - 1, 0)]                    # 1 + ulp, half an ulp of 1
    t += [pat(0, top - 1, ones), pat(1, top - 1, ones), pat(0, top - 1 - m - 1, 0)]  # +- largest finite, half its ulp
    t += [pat(0, top, 0), pat(1, top, 0), pat(0, top, 1 << (m - 1)), pat(0, top, 1)]  # +- inf, a quiet NaN, NaN with payload 1
    # ordinary values: 1.5, -2.75, about 0.3, about -106.6, the largest number below 1
    t += [pat(0, bias, 1 << (m - 1)), pat(1, bias + 1, 3 << (m - 3)), pat(0, bias - 2, 0x3333333333333 >> (52 - m)),
          pat(1, bias + 6, 0xaaaaaaaaaaaaa >> (52 - m)), pat(0, bias - 1, ones)]
    assert len(t) == 24 and len(set(t)) == 24
    return np.array(t, dtype=u)


def all_pairs(table):
    """(a, b) with a[i*K + j] = table[i], b[i*K + j] = table[j]: consecutive reals always differ in class on the b side"""
    k = len(table)
    return np.repeat(table, k), np.tile(table, k)


def dense_draws(kind, n, seed):
    """three draws of n operand pairs as bit patterns, {"uniform", "cancelling", "subnormal"}:
    uniform    uniformly random patterns; in one pair of eight b takes the exponent field of a, and in half of those both keep
               only the top four significand bits -- uniform patterns alone overflow, cancel and underflow (almost) never in the
               wide formats (two fp64 exponents coincide once in 2048 pairs), so a uniform draw alone would not test those;
    cancelling b = -a with the pattern of b moved up by 0..3 ulps: exact zeros and subnormal differences;
    subnormal  both operands subnormal or zero, in one pair of eight b = -a."""
    u, m, e = FORMATS[kind]
    rng = np.random.default_rng([seed, m, e])
    width = 1 + m + e
    sign, emask, low = u(1 << (m + e)), u(((1 << e) - 1) << m), u((1 << (m - 4)) - 1)

    def patterns(bits):
        return rng.integers(0, 1 << bits, size=n, dtype=np.uint64).astype(u)

    a, b = patterns(width), patterns(width)
    pick = rng.integers(0, 8, n) == 0
    b = np.where(pick, (b & ~emask) | (a & emask), b)
    coarse = pick & (rng.integers(0, 2, n) == 0)
    a, b = np.where(coarse, a & ~low, a), np.where(coarse, b & ~low, b)
    draws = {"uniform": (a, b)}
    a = patterns(width)
    draws["cancelling"] = (a, ((a ^ sign) + rng.integers(0, 4, n).astype(u)).astype(u))
    a = patterns(m) | (patterns(1) << u(m + e))
    b = patterns(m) | (patterns(1) << u(m + e))
    draws["subnormal"] = (a, np.where(rng.integers(0, 8, n) == 0, a ^ sign, b))
    return draws


def typed_cells(dtype, seed, rank, axis, cells, nc):
    """non-integer random reals of `dtype` in every cell of rank `rank`'s pencil of axis `axis`, in the form typed_add takes
    (native numpy type; bf16: bit patterns).  fp32 / fp64: standard normal.  fp16 / bf16: random sign and significand,
    magnitudes spread over [2^-6, 2^6) -- sums of neighbours in magnitude and sums across it both round."""
    rng = np.random.default_rng([int(seed), int(rank), int(axis), 77])
    kind = kind_of(dtype)
    shape = (int(cells), nc)
    if kind in ("fp32", "fp64"):
        return rng.standard_normal(shape).astype(_FLOAT_OF_KIND[kind])
    u, m, e = FORMATS[kind]
    bias = (1 << (e - 1)) - 1
    bits = (rng.integers(0, 2, shape) << (m + e)) | (rng.integers(bias - 6, bias + 6, shape) << m) | rng.integers(0, 1 << m, shape)
    bits = bits.astype(u)
    return bits if kind == "bf16" else bits.view(np.float16)


def initial_cells(seed, rank, axis, cells, nc):
    """integers 0..7 in every cell of rank `rank`'s pencil of axis `axis`"""
    return np.random.default_rng([int(seed), int(rank), int(axis)]).integers(0, 8, size=(int(cells), nc), dtype=np.int64)


# ---- the contract in numpy -------------------------------------------------------------------------------------------------
def pencil3(p, arr):
    """3-D (+ trailing) view of a pencil's cells: numpy axis 2 - k is memory position k"""
    s = [int(x) for x in p.shape]
    return arr.reshape([s[2], s[1], s[0]] + list(arr.shape[1:]))


def slab(p, dim, which, h):
    """index of slab `which` (L, LF, HF, H) along global dim `dim` of thickness h: the other two dims with their halos,
    without padding"""
    idx = [None] * 3
    for k in range(3):
        o = int(p.order[k])
        n = int(p.shape[k]) - int(p.padding[o])
        lo, hi = (0, n) if o != dim else {"L": (0, h), "LF": (h, 2 * h), "HF": (n - 2 * h, n - h), "H": (n - h, n)}[which]
        idx[2 - k] = slice(lo, hi)
    return tuple(idx)


def accumulate_reference(g, axis, halo, periods, dim, infos, pencils, add=None, swapped=False):
    """one accumulation along `dim` on every rank of oracle grid `g`, in place on `pencils` (one (cells, nc) array per rank):
    LF += H(low neighbour), then HF += L(high neighbour); halos are read as they were before the call.  add(x, y): the
    addition (default: the arrays' own +).  swapped: the two additions in the OPPOSITE order -- not the contract; what a test
    of the order must be able to tell from it."""
    h = int(halo[dim])
    if h == 0:
        return
    old = [a.copy() for a in pencils]
    sides = ((-1, "LF", "H"), (+1, "HF", "L"))
    for r in range(len(pencils)):
        for side, mine, theirs in (sides[::-1] if swapped else sides):
            nb = g.shifted_rank(r, axis, dim, side, bool(periods[dim]))
            if nb < 0:
                continue
            dst, src = pencil3(infos[r], pencils[r]), pencil3(infos[nb], old[nb])[slab(infos[nb], dim, theirs, h)]
            if add is None:
                dst[slab(infos[r], dim, mine, h)] += src
            else:
                dst[slab(infos[r], dim, mine, h)] = add(dst[slab(infos[r], dim, mine, h)], src)


def update_reference(g, axis, halo, periods, dim, infos, pencils):
    """the update along `dim` in the same words: L <- HF(low neighbour), H <- LF(high neighbour)"""
    h = int(halo[dim])
    if h == 0:
        return
    old = [a.copy() for a in pencils]
    for r in range(len(pencils)):
        for side, mine, theirs in ((-1, "L", "HF"), (+1, "H", "LF")):
            nb = g.shifted_rank(r, axis, dim, side, bool(periods[dim]))
            if nb < 0:
                continue
            pencil3(infos[r], pencils[r])[slab(infos[r], dim, mine, h)] = pencil3(infos[nb], old[nb])[slab(infos[nb], dim, theirs, h)]


def expected_after(g, axis, halo, periods, padding, seed, nc, dims=(2, 1, 0), typed=None, swapped=False):
    """(pencil infos, initial pencils, pencils after accumulating along `dims` in turn) of every rank.  typed: a data type --
    cells from typed_cells, every addition through typed_add in that type, in the documented order (swapped: in the other)"""
    infos = [g.pencil_info(r, axis, halo, padding) for r in range(g.nranks)]
    if typed is None:
        init, add = [initial_cells(seed, r, axis, infos[r].size, nc) for r in range(g.nranks)], None
    else:
        init = [typed_cells(typed, seed, r, axis, infos[r].size, nc) for r in range(g.nranks)]
        add = lambda x, y: typed_add(typed, x, y)  # noqa: E731
    want = [a.copy() for a in init]
    for dim in dims:
        accumulate_reference(g, axis, halo, periods, dim, infos, want, add, swapped)
    return infos, init, want


# ---- GPU bodies ------------------------------------------------------------------------------------------------------------
def _dev(raw):
    import torch
    return torch.from_numpy(np.ascontiguousarray(raw)).cuda()


def _first_difference(got, want, es):
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    return "%d bytes differ, first in cell %d" % (bad.size, bad[0] // es)


def accumulate_sweep(rank, nranks, args):
    """cudecompAmdAccumulateHalos along dims 2, 1, 0 for every axis of args["axes"] and every type of args["dtypes"]: the whole
    pencil (halo and padding cells included) against the all-ranks numpy restatement, bit for bit.  args["adjoint"]: also
    <U x, y> == <x, A y> (fp64, integers) with the library's own cudecompUpdateHalos as the witness.
    args["payload"] == "typed": non-integer reals of the element type instead of the integers, the restatement in that type's
    arithmetic (typed_add) in the documented order.  args["overlap"]: the faces of some rank overlap -- the restatement with the
    two additions swapped must then differ from the expected pencils (of all ranks together) in at least one cell, or the case
    could not see a swap."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for axis in args.get("axes", [0, 1, 2]):
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
        for dtype in args.get("dtypes", ALL_TYPES):
            nc, es = TYPES[dtype][1], element_bytes(dtype)
            typed = dtype if args.get("payload", "ints") == "typed" else None
            infos, init, want = expected_after(g, axis, halo, periods, padding, args.get("seed", 5), nc, typed=typed)
            if infos[rank].as_dict() != p.as_dict():
                failures.append("rank %d axis %d: pencil info differs from the oracle" % (rank, axis))
                continue
            if typed is not None and args.get("overlap"):
                other = expected_after(g, axis, halo, periods, padding, args.get("seed", 5), nc, typed=typed, swapped=True)[2]
                if all(np.array_equal(bits_of(dtype, a), bits_of(dtype, b)) for a, b in zip(want, other)):
                    failures.append("rank %d axis %d %s: swapping the two additions changes no cell: this seed cannot see the order" %
                                    (rank, axis, NAMES[dtype]))
            work_ptr = cd.cudecompMalloc(h, gd, wsz * es)
            raw = (lambda a: to_bytes(a, dtype)) if typed is None else (lambda a: bits_of(dtype, a).view(np.uint8).reshape(-1))
            data = _dev(raw(init[rank]))
            for dim in (2, 1, 0):
                cd.cudecompAccumulateHalos(axis, h, gd, data.data_ptr(), work_ptr, dtype, halo, periods, dim, padding, stream)
            torch.cuda.synchronize()
            got = data.cpu().numpy()
            if typed is None:
                diff = _first_difference(got, raw(want[rank]), es)
            else:  # the rule of everything typed: NaN by class (none arises from these magnitudes), all else bit for bit
                bad = np.nonzero(mismatches(kind_of(dtype), got.view(FORMATS[kind_of(dtype)][0]), bits_of(dtype, want[rank]).reshape(-1)))[0]
                diff = "%d reals differ, first in cell %d" % (bad.size, bad[0] // nc) if bad.size else None
            if diff:
                failures.append("rank %d axis %d %s halo %s periods %s padding %s: %s; last kernel %s" %
                                (rank, axis, NAMES[dtype], tuple(halo), tuple(periods), tuple(padding), diff,
                                 cd.cudecompExtLastKernelName()))
            cd.cudecompFree(h, gd, work_ptr)
        if args.get("adjoint"):
            failures.extend(_adjoint(rank, h, gd, g, axis, halo, periods, padding, wsz, stream))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def _adjoint(rank, h, gd, g, axis, halo, periods, padding, wsz, stream):
    """single rank: sum over ALL cells of (U x) * y == sum over INTERIOR cells of x * (A y), x zero outside the interior, U =
    cudecompUpdateHalos along 0, 1, 2, A = accumulation along 2, 1, 0; small integers, exact in fp64"""
    import torch
    from tests.half_bodies import global_index
    if g.nranks != 1:
        return []
    p = g.pencil_info(rank, axis, halo, padding)
    rng = np.random.default_rng(11 + axis)
    inside = global_index(p, g.gdims) >= 0
    x = np.where(inside, rng.integers(1, 8, size=int(p.size)), 0).astype(np.float64)
    y = rng.integers(0, 8, size=int(p.size)).astype(np.float64)
    work_ptr = cd.cudecompMalloc(h, gd, wsz * 8)
    ux, ay = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for dim in (0, 1, 2):
        cd.cudecompUpdateHalos(axis, h, gd, ux.data_ptr(), work_ptr, cd.DOUBLE, halo, periods, dim, padding, stream)
    for dim in (2, 1, 0):
        cd.cudecompAccumulateHalos(axis, h, gd, ay.data_ptr(), work_ptr, cd.DOUBLE, halo, periods, dim, padding, stream)
    torch.cuda.synchronize()
    lhs = float(np.dot(ux.cpu().numpy(), y))
    rhs = float(np.dot(x[inside], ay.cpu().numpy()[inside]))
    cd.cudecompFree(h, gd, work_ptr)
    return [] if lhs == rhs else ["axis %d halo %s periods %s: <U x, y> = %r but <x, A y> = %r" % (axis, tuple(halo), tuple(periods), lhs, rhs)]


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out


def _pattern(n, shift, device):
    """integers 0..7, a fixed function of the cell number, built on the device"""
    import torch
    i = torch.arange(n, dtype=torch.int64, device=device)
    return (((i * 2654435761 + shift) >> 7) & 7).to(torch.float64)


def _torch_reference(p, halo, t):
    """single rank, every dim periodic: the accumulation along 2, 1, 0 on a device tensor, in the words of
    accumulate_reference (the rank is its own neighbour)"""
    v = pencil3(p, t)
    for dim in (2, 1, 0):
        hh = int(halo[dim])
        if hh == 0:
            continue
        lo, hi = v[slab(p, dim, "L", hh)].clone(), v[slab(p, dim, "H", hh)].clone()
        v[slab(p, dim, "LF", hh)] += hi
        v[slab(p, dim, "HF", hh)] += lo


def full_size(rank, nranks, args):
    """One rank, a pencil of args["gdims"] interior cells, fp64, periodic: dims 2, 1, 0, every cell compared on the device."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, dict(args, pdims=(1, 1)))
    halo, periods = args["halo"], (1, 1, 1)
    axis = args.get("axis", 0)
    p = cd.cudecompGetPencilInfo(h, gd, axis, halo)
    n = int(p.size)
    work_ptr = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * 8)
    data = _pattern(n, 12345, "cuda")
    want = data.clone()
    _torch_reference(p, halo, want)
    kernels = []
    for dim in (2, 1, 0):
        cd.cudecompAccumulateHalos(axis, h, gd, data.data_ptr(), work_ptr, cd.DOUBLE, halo, periods, dim, None,
                                   torch.cuda.current_stream().cuda_stream)
        kernels.append(cd.cudecompExtLastKernelName())
    torch.cuda.synchronize()
    bad = (data != want).nonzero().flatten()
    failures = []
    if bad.numel():
        failures.append("%d of %d cells differ, first %s" % (bad.numel(), n, bad[:3].tolist()))
    changed = int((want != _pattern(n, 12345, "cuda")).sum())
    del data, want
    cd.cudecompFree(h, gd, work_ptr)
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": failures, "kernels": kernels, "cells": n, "changed": changed}


def graph_and_interleave(rank, nranks, args):
    """(1) Accumulation along 2, 1, 0 captured from the caller's stream into ONE hipGraph after an eager warm-up, replayed on
    fresh data; (2) an update and an accumulation interleaved on one workspace and one stream give the sequential result."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    axis, dtype = args.get("axis", 0), cd.DOUBLE
    infos = [g.pencil_info(r, axis, halo, padding) for r in range(g.nranks)]
    p = infos[rank]
    work_ptr = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * 8)
    failures = []

    def pencils(seed):
        return [initial_cells(seed, r, axis, infos[r].size, 1) for r in range(g.nranks)]

    def accumulate(t, sptr):
        for dim in (2, 1, 0):
            cd.cudecompAccumulateHalos(axis, h, gd, t.data_ptr(), work_ptr, dtype, halo, periods, dim, padding, sptr)

    if args.get("capture", True):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        data = torch.zeros(int(p.size), dtype=torch.float64, device="cuda")
        with torch.cuda.stream(stream):
            accumulate(data, stream.cuda_stream)  # warm-up: first-use allocations and mappings happen outside the capture
            stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            accumulate(data, torch.cuda.current_stream().cuda_stream)
        for it in range(args.get("replays", 3)):
            want = pencils(100 + it)
            mine = want[rank].astype(np.float64).reshape(-1)
            for dim in (2, 1, 0):
                accumulate_reference(g, axis, halo, periods, dim, infos, want)
            with torch.cuda.stream(stream):
                data.copy_(torch.from_numpy(mine).cuda())
                graph.replay()
                stream.synchronize()
            if not np.array_equal(data.cpu().numpy(), want[rank].astype(np.float64).reshape(-1)):
                failures.append("rank %d replay %d: captured accumulation differs from the restatement" % (rank, it))
        del graph
    # interleaved: U(0) A(2) U(1) A(1) U(2) A(0) on one stream and one workspace
    want = pencils(7)
    mine = want[rank].astype(np.float64).reshape(-1)
    sptr = torch.cuda.current_stream().cuda_stream
    t = torch.from_numpy(mine).cuda()
    for du, da in ((0, 2), (1, 1), (2, 0)):
        cd.cudecompUpdateHalos(axis, h, gd, t.data_ptr(), work_ptr, dtype, halo, periods, du, padding, sptr)
        update_reference(g, axis, halo, periods, du, infos, want)
        cd.cudecompAccumulateHalos(axis, h, gd, t.data_ptr(), work_ptr, dtype, halo, periods, da, padding, sptr)
        accumulate_reference(g, axis, halo, periods, da, infos, want)
    torch.cuda.synchronize()
    if not np.array_equal(t.cpu().numpy(), want[rank].astype(np.float64).reshape(-1)):
        failures.append("rank %d: interleaved updates and accumulations differ from the sequential restatement" % rank)
    cd.cudecompFree(h, gd, work_ptr)
    cd.cudecompGridDescDestroy(h, gd)
    return failures
