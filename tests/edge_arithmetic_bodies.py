"""The public calls that add -- cudecompAmdFoldHalos{X,Y,Z}, cudecompAmdFoldFieldHalos{X,Y,Z}, cudecompAmdAccumulateFieldHalos{X,Y,Z}
-- on pencils of IEEE edge values: the per-rank bodies of tests/test_gpu_halo_edge_arithmetic.py.  The kernel tests of that module
prove the arithmetic of every instantiation; these prove that the plans hand the kernels every cell they should, and that no NaN or
infinity of a ghost cell lands anywhere else.

Every cell of a pencil -- interior, ghost cells, padding -- holds an element of the 24 x 24 pairs of tests/edge_arithmetic.py, walked
cyclically with a stride coprime to their number.  Expected pencils: the definitions in numpy (FB.fold_reference, AB.accumulate_reference
and ACB.fused_reference with AB.typed_add), one call along one dim on a fresh pencil.  Comparison: the whole buffer with its slack;
the reals whose expected value is a NaN under AB.mismatches (any NaN of the type), every other byte identical.  `cases` needs no GPU:
tests/test_edge_arithmetic_table.py holds the expected pencils to the classes of results they are there for."""
import itertools

import numpy as np

import cudecomp_amd as cd
from oracle import oracle as orc
from tests import accumulate_bodies as AB
from tests import accumulate_clear_bodies as ACB
from tests import edge_arithmetic as EA
from tests import fold_bodies as FB

SLACK = FB.SLACK
STRIDE = 175  # cells step through the 1152 elements (a and b of the 576 pairs, interleaved) by this: coprime to 576 and to 1152
PARITIES = (1, -1, 1)  # of the three fields
# the pencils of tests/test_gpu_halo_edge_arithmetic.py: all three axes and every dim of them, in both memory orders
PENCILS = {"gdims": (11, 9, 7), "pdims": (1, 1), "halo": (2, 1, 3), "periods": (0, 1, 0), "padding": (1, 2, 0),
           "dtypes": [cd.HALF, cd.BFLOAT16, cd.FLOAT_COMPLEX, cd.DOUBLE]}
ORDERS = {"default": None, "mixed": ((1, 0, 2), (2, 1, 0), (0, 2, 1))}


def grid_of(args):
    return orc.Grid(args["gdims"], args["pdims"], mem_order=args.get("mem_order"))


def fill(p, dtype, field=0):
    """(cells, nc) bit patterns for EVERY cell of the pencil, ghost cells and padding included"""
    a, b = EA.pairs(dtype)
    pool = np.stack([a, b], axis=1).reshape(2 * len(a), -1)
    return pool[(np.arange(int(p.size), dtype=np.int64) * STRIDE + 101 * field) % len(pool)].copy()


def _ones(p, dtype):
    """the element (1, 1) in every cell: what a reference changes of it are the cells it adds into"""
    u, m, e = AB.FORMATS[AB.kind_of(dtype)]
    return np.full((int(p.size), AB.TYPES[dtype][1]), ((1 << (e - 1)) - 1) << m, dtype=u)


def cases(call, args):
    """every case of a call family as (label, axis, dtype, dim, parameters, start pencils, expected pencils, result masks) --
    one pencil per field; result mask: the cells the call adds into.  Parameters: fold (parity, centering, clear), fold_fields
    (centering, clear), accumulate_fields (clear,)."""
    g = grid_of(args)
    halo, periods, padding = args["halo"], args["periods"], args["padding"]
    for axis, dtype, dim in itertools.product(range(3), args["dtypes"], range(3)):
        p = g.pencil_info(0, axis, halo, padding)
        nb = FB.neighbours_of(g, 0, axis, periods)
        add = lambda x, y, dtype=dtype: AB.typed_add(dtype, x, y)  # noqa: E731
        if call == "accumulate_fields":
            for clear in (0, 1):
                start = [fill(p, dtype, f) for f in range(3)]
                want = [s.copy() for s in start]
                for w in want:  # every field by itself: what the single call makes of it
                    (ACB.fused_reference if clear else AB.accumulate_reference)(g, axis, halo, periods, dim, [p], [w], add)
                ones = _ones(p, dtype)
                AB.accumulate_reference(g, axis, halo, periods, dim, [p], [ones], add)
                mask = (ones != _ones(p, dtype)).any(axis=1)
                yield "axis %d %s dim %d clear %d" % (axis, AB.NAMES[dtype], dim, clear), axis, dtype, dim, (clear,), start, want, [mask] * 3
            continue
        for centering, clear in itertools.product((0, 1), (0, 1)):
            ones = _ones(p, dtype)
            FB.fold_reference(p, ones, halo, dim, nb[dim], 1, centering, 0, dtype)
            mask = (ones != _ones(p, dtype)).any(axis=1)
            if call == "fold":
                for parity in (1, -1):
                    start = [fill(p, dtype)]
                    want = [start[0].copy()]
                    FB.fold_reference(p, want[0], halo, dim, nb[dim], parity, centering, clear, dtype)
                    yield ("axis %d %s dim %d parity %+d centering %d clear %d" % (axis, AB.NAMES[dtype], dim, parity, centering, clear),
                           axis, dtype, dim, (parity, centering, clear), start, want, [mask])
            else:
                start = [fill(p, dtype, f) for f in range(3)]
                want = [s.copy() for s in start]
                for f, w in enumerate(want):
                    FB.fold_reference(p, w, halo, dim, nb[dim], PARITIES[f], centering, clear, dtype)
                yield ("axis %d %s dim %d centering %d clear %d" % (axis, AB.NAMES[dtype], dim, centering, clear), axis, dtype, dim,
                       (centering, clear), start, want, [mask] * 3)


def result_classes(call, args):
    """{data type: {"reals", "nan", "inf", "zero", "subnormal"}} over the cells the calls of a family add into, all cases together"""
    out = {}
    for _, _, dtype, _, _, _, want, masks in cases(call, args):
        tally = out.setdefault(dtype, {"reals": 0, "nan": 0, "inf": 0, "zero": 0, "subnormal": 0})
        for w, m in zip(want, masks):
            tally["reals"] += int(w[m].size)
            for k, v in AB.classes(AB.kind_of(dtype), w[m]).items():
                tally[k] += int(v.sum())
    return out


def class_failures(call, args):
    """the expected pencils of a family must contain NaN, infinite, zero and subnormal results, and NaNs in under a quarter of them"""
    out = []
    for dtype, t in result_classes(call, args).items():
        if not (t["nan"] and t["inf"] and t["zero"] and t["subnormal"]) or 4 * t["nan"] >= t["reals"]:
            out.append("%s %s: the results of the expected pencils are %s" % (call, AB.NAMES[dtype], t))
    return out


def _run(call, rank, nranks, args):
    import torch
    from tests import gpu_bodies as B
    assert nranks == 1
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    out = {"failures": class_failures(call, args), "compared": 0, "launching": 0}
    work = {}
    for label, axis, dtype, dim, params, start, want, masks in cases(call, args):
        es, kind, u = AB.element_bytes(dtype), AB.kind_of(dtype), AB.FORMATS[AB.kind_of(dtype)][0]
        p = g.pencil_info(0, axis, halo, padding)
        if p.as_dict() != cd.cudecompGetPencilInfo(h, gd, axis, halo, padding).as_dict():
            out["failures"].append("%s: pencil info differs from the oracle" % label)
            continue
        dev = [torch.from_numpy(FB.guarded(s)).cuda() for s in start]
        ptrs = [t.data_ptr() + SLACK for t in dev]
        before = cd.cudecompExtDataLaunchCount()
        try:
            if call == "fold":
                parity, centering, clear = params
                cd.cudecompFoldHalos(axis, h, gd, ptrs[0], dtype, parity, centering, clear, halo, periods, dim, padding, stream)
            elif call == "fold_fields":
                centering, clear = params
                cd.cudecompFoldFieldHalos(axis, h, gd, ptrs, dtype, list(PARITIES), centering, clear, halo, periods, dim, padding, stream)
            else:
                if (axis, dtype) not in work:
                    work[(axis, dtype)] = cd.cudecompMalloc(h, gd, 3 * max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * es)
                cd.cudecompAccumulateFieldHalos(axis, h, gd, ptrs, work[(axis, dtype)], dtype, halo, periods, dim, padding, params[0], stream)
        except cd.CudecompError as e:
            out["failures"].append("%s: refused with code %d" % (label, e.code))
            continue
        torch.cuda.synchronize()
        launched = cd.cudecompExtDataLaunchCount() - before
        kernel = cd.cudecompExtLastKernelName()
        out["launching"] += launched > 0
        if bool(launched) != bool(masks[0].any()):
            out["failures"].append("%s: %d launches, and %d cells to add into" % (label, launched, int(masks[0].sum())))
        for f, (t, w) in enumerate(zip(dev, want)):
            got, ref = t.cpu().numpy(), FB.guarded(w)
            out["compared"] += 1
            nan = np.zeros(got.size, dtype=bool)  # the BYTES of the reals whose expected value is a NaN
            nan[SLACK:got.size - SLACK] = np.repeat(AB.classes(kind, w)["nan"].reshape(-1), np.dtype(u).itemsize)
            diff = FB.first_difference(np.where(nan, 0, got), np.where(nan, 0, ref), es)
            bad = AB.mismatches(kind, got[SLACK:got.size - SLACK].view(u).reshape(w.shape), w)
            if diff or bad.any():
                c = int(np.argwhere(bad)[0][0]) if bad.any() else -1
                out["failures"].append("%s field %d: %s; %d reals break the NaN rule%s; last kernel %s" % (
                    label, f, diff, int(bad.sum()), " (first in cell %d: %s, expected %s)" % (
                        c, [hex(int(x)) for x in got[SLACK:got.size - SLACK].view(u).reshape(w.shape)[c]], [hex(int(x)) for x in w[c]]) if c >= 0 else "",
                    kernel))
    for ptr in work.values():
        cd.cudecompFree(h, gd, ptr)
    cd.cudecompGridDescDestroy(h, gd)
    return out


def fold(rank, nranks, args):
    """cudecompAmdFoldHalos*: parity +-1, centering 0 and 1, clear 0 and 1, every axis and dim"""
    return _run("fold", rank, nranks, args)


def fold_fields(rank, nranks, args):
    """cudecompAmdFoldFieldHalos*: three fields with parities (+1, -1, +1), each held to the single call's definition"""
    return _run("fold_fields", rank, nranks, args)


def accumulate_fields(rank, nranks, args):
    """cudecompAmdAccumulateFieldHalos* with and without clear, three fields, each held to the single call's definition"""
    return _run("accumulate_fields", rank, nranks, args)
