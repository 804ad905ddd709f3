"""The public calls that add -- cudecompAmdFoldHalos{X,Y,Z}, cudecompAmdFoldFieldHalos{X,Y,Z}, cudecompAmdAccumulateFieldHalos{X,Y,Z},
cudecompAmdSetWallHalos{X,Y,Z}, cudecompAmdSetWallFieldHalos{X,Y,Z}, cudecompAmdSetWallPlaneHalos{X,Y,Z} -- on pencils of IEEE edge
values: the per-rank bodies of tests/test_gpu_halo_edge_arithmetic.py.  The kernel tests of that module prove the arithmetic of every
instantiation; these prove that the plans hand the kernels every cell they should, and that no NaN or infinity -- of a ghost cell,
a mirror cell, an addend or a plane -- lands anywhere but in the ghost cell the contract names.

Every cell of a pencil -- interior, ghost cells, padding -- holds an element of the 24 x 24 pairs of tests/edge_arithmetic.py, walked
cyclically with a stride coprime to their number; so does every entry of a wall plane, with another stride and offset; the addends
of the wall-value calls are entries of the edge table, as doubles.  Expected pencils: the definitions in numpy (FB.fold_reference,
AB.accumulate_reference and ACB.fused_reference with AB.typed_add; the walls: RB.reflect_reference for the cells and their mirrors,
WB.wall_cells / WPB.wall_cells for what they receive), one call along one dim on a fresh pencil.  Comparison: the whole buffer with its slack;
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
from tests import reflect_bodies as RB
from tests import wall_planes_bodies as WPB
from tests import wall_values_bodies as WB

SLACK = FB.SLACK
STRIDE = 175  # cells step through the 1152 elements (a and b of the 576 pairs, interleaved) by this: coprime to 576 and to 1152
PLANE_STRIDE, PLANE_OFFSET = 281, 59  # ... the entries of a wall plane by this, from this element on (281 is prime)
PARITIES = (1, -1, 1)  # of the three fields
WALLS = list(itertools.product((1, -1), (0, 1), (1, 2, 3)))  # (parity, centering, sides) of the wall-value and wall-plane calls
WALL_CALLS = ("wall_values", "wall_fields", "wall_planes")
# the pencils of tests/test_gpu_halo_edge_arithmetic.py: all three axes and every dim of them, in both memory orders
PENCILS = {"gdims": (11, 9, 7), "pdims": (1, 1), "halo": (2, 1, 3), "periods": (0, 1, 0), "padding": (1, 2, 0),
           "dtypes": [cd.HALF, cd.BFLOAT16, cd.FLOAT_COMPLEX, cd.DOUBLE]}
ORDERS = {"default": None, "mixed": ((1, 0, 2), (2, 1, 0), (0, 2, 1))}


def grid_of(args):
    return orc.Grid(args["gdims"], args["pdims"], mem_order=args.get("mem_order"))


def _pool(dtype):
    """the 1152 elements every cell is filled from: a and b of the 576 pairs, interleaved"""
    a, b = EA.pairs(dtype)
    return np.stack([a, b], axis=1).reshape(2 * len(a), -1)


def fill(p, dtype, field=0):
    """(cells, nc) bit patterns for EVERY cell of the pencil, ghost cells and padding included"""
    pool = _pool(dtype)
    return pool[(np.arange(int(p.size), dtype=np.int64) * STRIDE + 101 * field) % len(pool)].copy()


def fill_plane(elements, dtype, side):
    """(elements, nc) bit patterns for EVERY entry of a wall plane, padding positions included: the pencils' pool, walked with
    another stride and offset, and another offset per side"""
    pool = _pool(dtype)
    return pool[(np.arange(int(elements), dtype=np.int64) * PLANE_STRIDE + PLANE_OFFSET + 211 * side) % len(pool)].copy()


def addend_indices(number, dim, side, h, nc, field=0):
    """the entries of AB.edge_table a wall-value call adds, h * nc of them (re and im interleaved): cyclic in the dim, the side,
    the ghost layer, the part of the element, the field and the NUMBER of the case among those of its data type -- over the cases of
    a type every entry of the table is an addend"""
    return [(number + 7 * dim + 11 * side + 5 * k + 13 * c + 3 * field) % 24 for k in range(h) for c in range(nc)]


def _bytes_of(bits):
    """(cells, nc) bit patterns as uint8 (cells, es), the SAME memory: what RB and WB work on"""
    assert bits.flags["C_CONTIGUOUS"]
    return bits.view(np.uint8).reshape(len(bits), -1)


def wall_call(p, cells, halo, dim, has_neighbour, centering, sides, value):
    """ONE wall call along `dim`, in place on `cells` (uint8, (cells, element bytes)), from the definitions that exist:
    RB.reflect_reference says which ghost cells such a call writes and which mirror each of them takes (with parity +1 the mirror's
    bytes arrive as they are), on the sides that `sides` names and that have no neighbour; ghost layer k, counted from the wall
    outward, then becomes value(side, k, those bytes, index of the layer in AB.pencil3's view) -- WB.wall_cells or WPB.wall_cells"""
    skip = [bool(has_neighbour[s]) or not sides & (1 << s) for s in (0, 1)]
    RB.reflect_reference(p, cells, halo, dim, skip, 1, centering, 1)
    h = int(halo[dim])
    ax, n = RB._dim_axis(p, dim)
    v = AB.pencil3(p, cells)
    for side in (0, 1):
        for k in range(0 if skip[side] else h):
            at = RB._unpadded(p)
            at[ax] = h - 1 - k if side == 0 else n - h + k
            v[tuple(at)] = value(side, k, v[tuple(at)], at)


def written_mask(p, halo, dim, has_neighbour, centering, sides):
    """the ghost cells ONE wall call along `dim` writes"""
    marks = np.zeros((int(p.size), 1), dtype=np.uint8)
    wall_call(p, marks, halo, dim, has_neighbour, centering, sides, lambda side, k, x, at: np.ones_like(x))
    return marks[:, 0] == 1


def plane_layer(p, plane, dim, h, k, at):
    """the entries of ghost layer k of a plane ((elements, nc) bit patterns in the layout of cd.wall_plane_shape: the pencil's shape
    in memory order with the extent along `dim` replaced by h) for the ghost cells at index `at` of AB.pencil3's view, as bytes"""
    shape, elements = cd.wall_plane_shape(p, dim, [h if d == dim else 0 for d in range(3)])
    assert elements == len(plane)
    ax = RB._dim_axis(p, dim)[0]
    idx = list(at)
    idx[ax] = k
    return _bytes_of(plane).reshape(shape[2], shape[1], shape[0], -1)[tuple(idx)]


def _ones(p, dtype):
    """the element (1, 1) in every cell: what a reference changes of it are the cells it adds into"""
    u, m, e = AB.FORMATS[AB.kind_of(dtype)]
    return np.full((int(p.size), AB.TYPES[dtype][1]), ((1 << (e - 1)) - 1) << m, dtype=u)


def cases(call, args):
    """every case of a call family as (label, axis, dtype, dim, parameters, start pencils, expected pencils, result masks) --
    one pencil per field; result mask: the cells the call adds into.  Parameters: fold (parity, centering, clear), fold_fields
    (centering, clear), accumulate_fields (clear,), wall_values (parity, centering, sides, table entries of the low addends, of the
    high ones), wall_fields (centering, sides, the same two lists for all fields, field-major), wall_planes (parity, centering, sides,
    the low plane, the high plane as (elements, nc) bit patterns); result mask of these three: the ghost cells the call writes."""
    g = grid_of(args)
    halo, periods, padding = args["halo"], args["periods"], args["padding"]
    numbers = {}  # wall values: the cases of a data type so far
    for axis, dtype, dim in itertools.product(range(3), args["dtypes"], range(3)):
        p = g.pencil_info(0, axis, halo, padding)
        nb = FB.neighbours_of(g, 0, axis, periods)
        add = lambda x, y, dtype=dtype: AB.typed_add(dtype, x, y)  # noqa: E731
        if call in WALL_CALLS:
            yield from _wall_cases(call, p, nb[dim], axis, dtype, dim, halo, numbers)
            continue
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


def _wall_cases(call, p, has_neighbour, axis, dtype, dim, halo, numbers):
    """the cases of a wall family on ONE pencil and dim: every expected pencil is wall_call -- one call along one dim -- on a fresh
    pencil, with WB.wall_cells per ghost layer (the two value calls; every field by itself) or WPB.wall_cells (the planes)"""
    nc, h = AB.TYPES[dtype][1], int(halo[dim])
    table = AB.edge_table(AB.kind_of(dtype))
    element = lambda idx, k: table[idx[k * nc:(k + 1) * nc]].tobytes()  # noqa: E731
    if call == "wall_planes":
        planes = [fill_plane(cd.wall_plane_shape(p, dim, halo)[1], dtype, side) for side in (0, 1)]
    for parity, centering, sides in WALLS:
        if call == "wall_fields" and parity < 0:  # (the fields bring their parities)
            continue
        mask = written_mask(p, halo, dim, has_neighbour, centering, sides)
        number = numbers[dtype] = numbers.get(dtype, -1) + 1
        label = "axis %d %s dim %d centering %d sides %d" % (axis, AB.NAMES[dtype], dim, centering, sides)
        if call == "wall_planes":
            start = [fill(p, dtype)]
            want = [start[0].copy()]
            wall_call(p, _bytes_of(want[0]), halo, dim, has_neighbour, centering, sides,
                      lambda side, k, x, at: WPB.wall_cells(dtype, x, parity, plane_layer(p, planes[side], dim, h, k, at)))
            yield label + " parity %+d" % parity, axis, dtype, dim, (parity, centering, sides, planes[0], planes[1]), start, want, [mask]
            continue
        signs = (parity,) if call == "wall_values" else PARITIES
        idx = [[addend_indices(number, dim, side, h, nc, f) for side in (0, 1)] for f in range(len(signs))]
        start = [fill(p, dtype, f) for f in range(len(signs))]
        want = [s.copy() for s in start]
        for f, w in enumerate(want):  # every field by itself: what the single definition makes of it
            wall_call(p, _bytes_of(w), halo, dim, has_neighbour, centering, sides,
                      lambda side, k, x, at, f=f: WB.wall_cells(dtype, x, signs[f], element(idx[f][side], k)))
        low, high = ([i for per_field in idx for i in per_field[side]] for side in (0, 1))
        if call == "wall_values":
            yield label + " parity %+d" % parity, axis, dtype, dim, (parity, centering, sides, low, high), start, want, [mask]
        else:
            yield label, axis, dtype, dim, (centering, sides, low, high), start, want, [mask] * 3


def addend_entries(call, args):
    """{data type: the set of table entries that are an addend in some case of a wall-value family}"""
    out = {}
    for _, _, dtype, _, params, _, _, masks in cases(call, args):
        for side in (0, 1):
            if masks[0].any() and params[-3] & (1 << side):  # (a wall the call does write)
                out.setdefault(dtype, set()).update(params[-2 + side])
    return out


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
        planes = []
        if call == "wall_planes":  # (elements, nc) bit patterns between their slack, like the pencils; they are only read
            planes = [(torch.from_numpy(FB.guarded(x)).cuda(), FB.guarded(x)) for x in params[3:]]
        elif call in WALL_CALLS:  # the table entries as the doubles the calls take
            doubles = EA.edge_doubles(dtype)[0]
            low, high = ([float(doubles[i]) for i in idx] for idx in params[-2:])
        before = cd.cudecompExtDataLaunchCount()
        try:
            if call == "wall_planes":
                parity, centering, sides = params[:3]
                cd.cudecompAmdSetWallPlaneHalos(axis, h, gd, ptrs[0], dtype, parity, centering, sides,
                                                planes[0][0].data_ptr() + SLACK if sides & 1 else None,
                                                planes[1][0].data_ptr() + SLACK if sides & 2 else None, halo, periods, dim, padding, stream)
            elif call == "wall_values":
                parity, centering, sides = params[:3]
                cd.cudecompAmdSetWallHalos(axis, h, gd, ptrs[0], dtype, parity, centering, sides, low if sides & 1 else None,
                                           high if sides & 2 else None, halo, periods, dim, padding, stream)
            elif call == "wall_fields":
                centering, sides = params[:2]
                cd.cudecompAmdSetWallFieldHalos(axis, h, gd, ptrs, dtype, list(PARITIES), centering, sides, low if sides & 1 else None,
                                                high if sides & 2 else None, halo, periods, dim, padding, stream)
            elif call == "fold":
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
        for side, (t, host) in enumerate(planes):
            if not np.array_equal(t.cpu().numpy(), host):
                out["failures"].append("%s: the %s plane, or the slack around it, was written" % (label, ("low", "high")[side]))
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


def wall_values(rank, nranks, args):
    """cudecompAmdSetWallHalos*: parity +-1, centering 0 and 1, sides 1, 2 and 3, every axis and dim; the addends of the ghost layers
    are entries of the edge table, handed over as the doubles they are"""
    return _run("wall_values", rank, nranks, args)


def wall_fields(rank, nranks, args):
    """cudecompAmdSetWallFieldHalos*: three fields with parities (+1, -1, +1) and addends of their own, each held to the single
    definition"""
    return _run("wall_fields", rank, nranks, args)


def wall_planes(rank, nranks, args):
    """cudecompAmdSetWallPlaneHalos*: parity +-1, centering 0 and 1, sides 1, 2 and 3; both planes device arrays of edge values that
    must stay as they are"""
    return _run("wall_planes", rank, nranks, args)
