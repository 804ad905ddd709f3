"""Halo accumulation (cudecomp_amd.h: cudecompAmdAccumulateHalos{X,Y,Z}): the numpy restatement of the contract, payloads in
all seven data types, and the per-rank bodies of tests/test_gpu_halo_accumulate.py.

The restatement works on INTEGER arrays of shape (cells, reals per element): the test payload is an integer 0..7 in every
cell (halos and padding included), any cell ends up as a sum of at most 27 cells (<= 189), and such integers are exact in
every element type, bf16 included (8 significand bits hold up to 256) -- so the expected pencil is computed once in int64 and
compared bit for bit in the type under test.  Every rank can build every rank's initial pencil (seeded by rank and axis) and
therefore the expected value of every cell of its own pencil."""
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


def accumulate_reference(g, axis, halo, periods, dim, infos, pencils):
    """one accumulation along `dim` on every rank of oracle grid `g`, in place on `pencils` (one (cells, nc) array per rank):
    LF += H(low neighbour), then HF += L(high neighbour); halos are read as they were before the call"""
    h = int(halo[dim])
    if h == 0:
        return
    old = [a.copy() for a in pencils]
    for r in range(len(pencils)):
        for side, mine, theirs in ((-1, "LF", "H"), (+1, "HF", "L")):
            nb = g.shifted_rank(r, axis, dim, side, bool(periods[dim]))
            if nb < 0:
                continue
            pencil3(infos[r], pencils[r])[slab(infos[r], dim, mine, h)] += pencil3(infos[nb], old[nb])[slab(infos[nb], dim, theirs, h)]


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


def expected_after(g, axis, halo, periods, padding, seed, nc, dims=(2, 1, 0)):
    """(pencil infos, initial pencils, pencils after accumulating along `dims` in turn) of every rank"""
    infos = [g.pencil_info(r, axis, halo, padding) for r in range(g.nranks)]
    init = [initial_cells(seed, r, axis, infos[r].size, nc) for r in range(g.nranks)]
    want = [a.copy() for a in init]
    for dim in dims:
        accumulate_reference(g, axis, halo, periods, dim, infos, want)
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
    <U x, y> == <x, A y> (fp64, integers) with the library's own cudecompUpdateHalos as the witness."""
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
            infos, init, want = expected_after(g, axis, halo, periods, padding, args.get("seed", 5), nc)
            if infos[rank].as_dict() != p.as_dict():
                failures.append("rank %d axis %d: pencil info differs from the oracle" % (rank, axis))
                continue
            work_ptr = cd.cudecompMalloc(h, gd, wsz * es)
            data = _dev(to_bytes(init[rank], dtype))
            for dim in (2, 1, 0):
                cd.cudecompAccumulateHalos(axis, h, gd, data.data_ptr(), work_ptr, dtype, halo, periods, dim, padding, stream)
            torch.cuda.synchronize()
            diff = _first_difference(data.cpu().numpy(), to_bytes(want[rank], dtype), es)
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
