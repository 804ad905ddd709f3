"""Halo fill (cudecomp_amd_fill.h: cudecompAmdFillHalos{X,Y,Z}) without a GPU.  The product's planner (cudecompExtPlanHaloFill,
the buildHaloFillPlan the executor runs) is asked for the plan of EVERY rank, axis and dim of randomly drawn decompositions,
and three statements of "the cells a fill writes" must name the same cells:
  (a) the destination cells of the fill plan's moves;
  (b) the pencil cells the product's UPDATE plan (cudecompExtPlanHalo) writes: the pencil destinations of its wrap copies or
      unpacks, or its receive ranges when the update exchanges whole faces directly;
  (c) a numpy restatement from the pencil info and cudecompExtShiftedRank alone: the low halo where there is a low neighbour,
      the high halo where there is a high one, each spanning the other two dims with their halos and without padding.
Cells are compared as sets of element offsets into the pencil: nothing is executed, so there is no tolerance anywhere."""
import ctypes as C
import hashlib
import itertools
import os
import re

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import cudecomp_amd as cd
from tests import accumulate_bodies as AB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMS = list(itertools.permutations((0, 1, 2)))
INVALID_USAGE, NOT_SUPPORTED = 1, 2
FILL_MARK = 256  # cudecompExtHaloPlan_t::reserved, bit 8


@st.composite
def decompositions(draw, max_ranks=12):
    # (the strategy of tests/test_halo_accumulate_plan.py and tests/test_plan_sim.py, restated)
    pdims = draw(st.sampled_from([(a, b) for a in range(1, 7) for b in range(1, 7) if a * b <= max_ranks]))
    lo = max(pdims)  # no empty pencils: that case has its own test
    gdims = tuple(draw(st.integers(lo, lo + 9)) for _ in range(3))
    if draw(st.booleans()):
        mem_order = tuple(draw(st.sampled_from(PERMS)) for _ in range(3))
    else:
        ac = tuple(draw(st.booleans()) for _ in range(3))
        mem_order = tuple(tuple((ax + i) % 3 if ac[ax] else i for i in range(3)) for ax in range(3))
    gdims_dist = None
    if draw(st.booleans()):
        gdims_dist = tuple(draw(st.integers(max(lo, g - 3), g)) for g in gdims)
    return {"gdims": gdims, "pdims": pdims, "mem_order": mem_order, "gdims_dist": gdims_dist,
            "col_major": draw(st.booleans())}


small3 = st.tuples(st.integers(0, 2), st.integers(0, 2), st.integers(0, 2))


def _dst_cells(m):
    k = np.indices([int(e) for e in m.extent]).reshape(3, -1)
    return m.dst_off + k[0] * m.ds[0] + k[1] * m.ds[1] + k[2] * m.ds[2]


def _planned(call):
    """(plan, None) or (None, result code of the refusal)"""
    try:
        return call(), None
    except cd.CudecompError as e:
        return None, e.code


def fill_cells(plan, size):
    """(a): per move the sorted destination cells; checks the shape of a fill plan on the way"""
    assert plan.kind in (0, 1) and plan.n_post == 0 and 0 <= plan.n_pre <= 2
    if plan.kind == 0:
        assert plan.n_pre == 0
        return []
    assert plan.reserved == FILL_MARK, "not marked as a fill plan (or marked as something else too)"
    assert plan.n_pre >= 1
    out = []
    for i in range(plan.n_pre):
        m = plan.pre[i]
        assert m.dst_buf == 0 and m.row_pitch == 0, "a fill-move targets the pencil and never claims the cells between rows"
        assert m.src_buf == 0 and m.src_off == 0 and list(m.ss) == [0, 0, 0], "a fill-move has no source"
        cells = np.sort(_dst_cells(m))
        assert cells.size and np.all(np.diff(cells) > 0) and cells[0] >= 0 and cells[-1] < size
        out.append(cells)
    if len(out) == 2:
        assert out[0][0] < out[1][0], "the low side comes first"
        assert np.intersect1d(out[0], out[1]).size == 0, "the two moves of a plan share a cell"
    return out


def update_cells(plan):
    """(b): the pencil cells an update plan writes"""
    if plan.kind == 0:
        return np.zeros(0, dtype=np.int64)
    if plan.kind == 3:  # direct: what arrives lands in the pencil itself
        assert plan.xbuf == 0
        parts = [np.arange(plan.recv_off[i], plan.recv_off[i] + plan.face_elements) for i in range(2) if plan.neighbor[i] >= 0]
    else:
        moves = [plan.pre[i] for i in range(plan.n_pre)] + [plan.post[i] for i in range(plan.n_post)]
        parts = [_dst_cells(m) for m in moves if m.dst_buf == 0]
    cells = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    assert np.unique(cells).size == cells.size
    return np.sort(cells)


def restated_cells(spec, rank, axis, halo, periods, dim, padding):
    """(c): from the pencil info and the neighbour query alone"""
    p = cd.cudecompExtPencilInfo(spec, rank, axis, halo, padding)
    mask = np.zeros(int(p.size), dtype=bool)
    h = int(halo[dim])
    if h:
        for side, which in ((-1, "L"), (+1, "H")):
            if cd.cudecompExtShiftedRank(spec, rank, axis, dim, side, periods[dim]) >= 0:
                AB.pencil3(p, mask)[AB.slab(p, dim, which, h)] = True
    return np.nonzero(mask)[0], int(p.size)


def check_case(d, halo, periods, padding, force_packed):
    """every rank, axis and dim of one drawn decomposition; returns (plans compared, plans both planners refused)"""
    spec = cd.make_grid_spec(d["gdims"], d["pdims"], d["mem_order"], d["gdims_dist"], d["col_major"])
    compared = refused = 0
    for rank in range(d["pdims"][0] * d["pdims"][1]):
        for axis in range(3):
            for dim in range(3):
                where = (d, rank, axis, dim, halo, periods, padding, force_packed)
                fill, fcode = _planned(lambda: cd.cudecompExtPlanHaloFill(spec, rank, axis, halo, periods, dim, padding, force_packed))
                upd, ucode = _planned(lambda: cd.cudecompExtPlanHalo(spec, rank, axis, halo, periods, dim, padding, force_packed))
                assert fcode == ucode, ("the fill's refusal is not the update's", fcode, ucode, where)
                if fcode is not None:
                    assert fcode in (INVALID_USAGE, NOT_SUPPORTED), where
                    refused += 1
                    continue
                want, size = restated_cells(spec, rank, axis, halo, periods, dim, padding)
                moves = fill_cells(fill, size)
                got = np.sort(np.concatenate(moves)) if moves else np.zeros(0, dtype=np.int64)
                assert np.array_equal(got, update_cells(upd)), ("fill plan and update plan name different cells", where)
                assert np.array_equal(got, want), ("fill plan and restatement name different cells", where)
                assert list(fill.neighbor) == list(upd.neighbor), where
                compared += 1
    return compared, refused


def test_fill_plans_random_decompositions():
    seen = {"examples": 0, "compared": 0, "refused": 0}

    @settings(max_examples=200, deadline=None, suppress_health_check=list(HealthCheck), database=None)
    @given(d=decompositions(), halo=small3, periods=st.tuples(st.booleans(), st.booleans(), st.booleans()), padding=small3,
           force_packed=st.booleans())
    def run(d, halo, periods, padding, force_packed):
        compared, refused = check_case(d, halo, periods, padding, force_packed)
        seen["examples"] += 1
        seen["compared"] += compared
        seen["refused"] += refused

    run()
    print("halo fill plans: %(examples)d decompositions, %(compared)d plans compared, %(refused)d refused by both planners" % seen)
    assert seen["examples"] >= 200
    assert seen["compared"] >= 10 * seen["examples"] and 3 * seen["refused"] <= seen["compared"], seen


def test_the_three_update_kinds_and_the_layout_of_a_plan():
    order = ((0, 1, 2),) * 3
    one = cd.make_grid_spec((5, 6, 7), (1, 1), order)
    four = cd.make_grid_spec((6, 6, 6), (2, 2), order)
    # wrap onto myself (update kind 1), packed (2: a split dim that is not the slowest, or padding), direct (3: whole faces)
    for spec, rank, halo, per, dim, pad, packed, kind in ((one, 0, (1, 2, 1), (True,) * 3, 1, None, False, 1),
                                                          (four, 0, (1, 1, 1), (True,) * 3, 1, None, False, 2),
                                                          (four, 0, (1, 1, 1), (True,) * 3, 2, None, False, 3),
                                                          (four, 0, (1, 1, 1), (True,) * 3, 2, None, True, 2),
                                                          (four, 3, (1, 2, 2), (True,) * 3, 2, (0, 1, 0), False, 2)):
        assert cd.cudecompExtPlanHalo(spec, rank, 0, halo, per, dim, pad, packed).kind == kind
        p = cd.cudecompExtPlanHaloFill(spec, rank, 0, halo, per, dim, pad, packed)
        assert p.kind == 1 and p.n_pre == 2 and p.n_post == 0 and p.reserved == FILL_MARK
        want, size = restated_cells(spec, rank, 0, halo, per, dim, pad or (0, 0, 0))
        assert np.array_equal(np.sort(np.concatenate(fill_cells(p, size))), want)
    # an edge rank of a non-periodic dim keeps its outer side: one move; no neighbour at all, or h == 0: nothing
    p = cd.cudecompExtPlanHaloFill(four, 0, 0, (1, 1, 1), (False,) * 3, 1)
    assert p.kind == 1 and p.n_pre == 1 and sorted(p.neighbor)[0] == -1
    assert cd.cudecompExtPlanHaloFill(one, 0, 0, (1, 1, 1), (False,) * 3, 2).kind == 0
    assert cd.cudecompExtPlanHaloFill(four, 0, 0, (1, 0, 1), (True,) * 3, 1).kind == 0
    # update and accumulation plans carry no fill mark
    assert cd.cudecompExtPlanHalo(four, 0, 0, (1, 1, 1), (True,) * 3, 1).reserved == 0
    assert cd.cudecompExtPlanHaloAccumulate(four, 0, 0, (1, 1, 1), (True,) * 3, 1).reserved & FILL_MARK == 0


def test_refusals_are_the_updates():
    order = ((0, 1, 2),) * 3

    def codes(spec, rank, axis, halo, per, dim):
        f = _planned(lambda: cd.cudecompExtPlanHaloFill(spec, rank, axis, halo, per, dim))[1]
        u = _planned(lambda: cd.cudecompExtPlanHalo(spec, rank, axis, halo, per, dim))[1]
        return f, u

    four = cd.make_grid_spec((4, 4, 4), (2, 2), order)
    assert codes(four, 0, 0, (0, 3, 0), (True,) * 3, 1) == (INVALID_USAGE, INVALID_USAGE)  # wider than a neighbour's slab
    assert codes(four, 0, 0, (0, 2, 0), (True,) * 3, 1) == (None, None)
    uneven = cd.make_grid_spec((4, 7, 4), (3, 1), order)  # Y split 3 + 2 + 2 for X pencils
    assert codes(uneven, 0, 0, (0, 3, 0), (False,) * 3, 1) == (INVALID_USAGE, INVALID_USAGE)
    empty = cd.make_grid_spec((3, 8, 8), (4, 1), order)
    assert codes(empty, 0, 1, (1, 1, 1), (True,) * 3, 0) == (NOT_SUPPORTED, NOT_SUPPORTED)
    # planner arguments
    for call in (lambda: cd.cudecompExtPlanHaloFill(four, 4, 0, (1, 1, 1), None, 0), lambda: cd.cudecompExtPlanHaloFill(four, 0, 3, (1, 1, 1), None, 0),
                 lambda: cd.cudecompExtPlanHaloFill(four, 0, 0, (1, 1, 1), None, 3), lambda: cd.cudecompExtPlanHaloFill(four, 0, 0, None, None, 0)):
        assert _planned(call)[1] == INVALID_USAGE


def test_entry_points_check_their_arguments_like_the_updates():
    """the bad-argument tuples of tests/test_halo_accumulate_plan.py with `work` removed (the update gets a non-NULL one), a
    value or none; every return code is the update's"""
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    value = bytes(range(0xA0, 0xA4))
    tuples = [(h, gd, 1, cd.FLOAT, None, None, 0, None, None),                  # halo_extents NULL
              (h, gd, None, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),        # input NULL
              (h, gd, 1, cd.FLOAT, i3(1, 1, 1), None, 3, None, None),           # dim out of range
              (h, gd, 1, cd.FLOAT, i3(1, 1, 1), None, -1, None, None),
              (h, gd, 1, 99, i3(1, 1, 1), None, 0, None, None),                 # unknown data type
              (h, None, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),         # no descriptor
              (None, gd, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),        # no handle
              (h, gd, None, 99, None, None, 5, None, None),                     # several at once: the first check decides
              (h, gd, None, cd.FLOAT, i3(1, 1, 1), None, 3, None, None),
              (h, gd, None, cd.FLOAT, i3(0, 0, 0), None, 0, None, None),        # all halos zero: success before input is looked at
              (h, gd, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),           # non-periodic single rank: nothing to do
              (h, gd, 1, cd.DOUBLE, i3(1, 0, 1), b3(True, True, True), 1, i3(1, 2, 0), None)]  # h == 0 along dim: success, no effect
    for name in cd.AMD_FILL_SYMBOLS:
        fn, up = getattr(L, name), getattr(L, name.replace("AmdFill", "Update"))
        for hh, g, inp, dtype, halo, per, dim, pad, stream in tuples:
            want = up(hh, g, inp, 1, dtype, halo, per, dim, pad, stream)
            for v in (None, value):
                assert fn(hh, g, inp, dtype, v, halo, per, dim, pad, stream) == want, (name, inp, dtype, dim, v)
    assert L.cudecompAmdFillHalosX(h, gd, None, cd.FLOAT, None, i3(0, 0, 0), None, 0, None, None) == cd.RESULT_SUCCESS
    assert L.cudecompAmdFillHalosX(h, gd, None, cd.FLOAT, None, i3(1, 1, 1), None, 0, None, None) == cd.RESULT_INVALID_USAGE
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def test_with_cells_to_write_the_result_is_the_updates_with_or_without_a_device():
    """a periodic single rank has ghost cells to write on every dim: without a device both calls answer
    CUDECOMP_RESULT_CUDA_ERROR (the pointers are never looked at), with one both succeed on real buffers"""
    import torch
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    halo, value = (1, 2, 1), bytes(range(0xA0, 0xA4))
    for axis, name in enumerate(cd.AMD_FILL_SYMBOLS):
        fn, up = getattr(L, name), getattr(L, name.replace("AmdFill", "Update"))
        if torch.cuda.is_available():
            data = torch.zeros(int(cd.cudecompGetPencilInfo(h, gd, axis, halo).size), dtype=torch.float32, device="cuda")
            work = torch.zeros(max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1), dtype=torch.float32, device="cuda")
            inp, wk, expected = data.data_ptr(), work.data_ptr(), cd.RESULT_SUCCESS
        else:
            inp, wk, expected = 1, 1, cd.RESULT_CUDA_ERROR
        for dim in range(3):
            want = up(h, gd, inp, wk, cd.FLOAT, i3(*halo), b3(True, True, True), dim, None, None)
            assert want == expected, (name, dim, want)
            for v in (None, value):
                assert fn(h, gd, inp, cd.FLOAT, v, i3(*halo), b3(True, True, True), dim, None, None) == want, (name, dim, v)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def test_python_wrapper_checks_the_value_size():
    with pytest.raises(ValueError):
        cd.cudecompFillHalos(0, None, None, 1, cd.DOUBLE, (1, 1, 1), None, 0, value=np.float32(1))
    with pytest.raises(ValueError):
        cd.cudecompExtFill3D(1, 8, b"\x01\x02", (1, 1, 1), (1, 0, 0))


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(cudecomp\w+)\s*\(", src))


def test_header_declares_and_library_exports_the_symbols():
    assert _declared("cudecomp_amd_fill.h") == set(cd.AMD_FILL_SYMBOLS) == {"cudecompAmdFillHalos" + a for a in "XYZ"}
    assert '#include "cudecomp_amd.h"' in open(os.path.join(ROOT, "include", "cudecomp_amd_fill.h")).read()
    L = cd.lib()
    for name in cd.AMD_FILL_SYMBOLS + ["cudecompExtPlanHaloFill", "cudecompExtFill3D"]:
        assert hasattr(L, name), name
    assert {"cudecompExtPlanHaloFill", "cudecompExtFill3D"} <= _declared("cudecomp_ext.h")
    # cudecomp_amd.h is the file the accumulation change left: the fill lives in its own header
    assert cd.AMD_SYMBOLS == ["cudecompAmdAccumulateHalos" + a for a in "XYZ"]
    digest = hashlib.sha256(open(os.path.join(ROOT, "include", "cudecomp_amd.h"), "rb").read()).hexdigest()
    assert digest == "59ee86fb255c4ec48c5ce5a29a8a2ae32ec4a8ac2de41de07cb8cd1134d170e8"


def test_arguments_are_checked_in_the_stated_order(capfd):
    from tests import halo_check_order
    halo_check_order.check("fill", capfd)
