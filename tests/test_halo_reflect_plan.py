"""Halo reflection (cudecomp_amd_reflect.h: cudecompAmdReflectHalos{X,Y,Z}) without a GPU.  The product's planner
(cudecompExtPlanHaloReflect, the buildHaloReflectPlan the executor runs) is asked for the plan of EVERY rank, axis and dim of a
deterministic sweep of decompositions:
  * the destination cells of reflect(dim) and of fill(dim) with the same periods are disjoint, and their union is the cell set of
    fill(dim) with all periods true: the reflection is the exact complement of the update along `dim`;
  * the plan executed in numpy is the definition (tests/reflect_bodies.py reflect_reference), byte for byte on whole pencils;
  * on single-rank grids the sequence over dims 0, 1, 2 -- the update's wrap copies on periodic dims, the reflection on the
    others -- is numpy.pad of the interior axis by axis (wrap / symmetric / reflect), with the sign rule for parity -1.
Refusals and result codes, the kernel choices of mirror-moves (cudecompExtDescribeMoves, modes 5 / 6), the header and the Python
wrapper follow.  Nothing here has a tolerance."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import move_lists as ML
from tests import reflect_bodies as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CFLAGS = ["-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]
PERMS = list(itertools.permutations((0, 1, 2)))
INVALID_USAGE, NOT_SUPPORTED, INTERNAL_ERROR = 1, 2, 3
REFLECT_MARK, NEGATE_MARK = 1 << 12, 1 << 13
K_ROWS_REFLECT, K_GENERIC_REFLECT = 16, 17

# pdims -> ragged gdims whose smallest slab along every dim holds 4 cells: h + centering <= interior for every halo below
GRIDS = {(1, 1): (5, 6, 7), (1, 4): (16, 17, 18), (2, 2): (8, 9, 11), (2, 3): (12, 13, 14)}
HALOS = [(1, 1, 1), (2, 1, 3), (3, 3, 3)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
PERIODS = list(itertools.product((False, True), repeat=3))
ES, RB_ = 4, 2  # the numpy executions move complex-fp16 elements: two sign bits per element


def _cells(m, side):
    k = np.indices([int(e) for e in m.extent]).reshape(3, -1)
    off, st = (m.dst_off, m.ds) if side == "dst" else (m.src_off, m.ss)
    return off + k[0] * st[0] + k[1] * st[1] + k[2] * st[2]


def _planned(call):
    try:
        return call(), None
    except cd.CudecompError as e:
        return None, e.code


def _dst_cells(plan):
    parts = [_cells(plan.pre[i], "dst") for i in range(plan.n_pre)]
    cells = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    assert np.unique(cells).size == cells.size, "two moves of a plan share a destination cell"
    return np.sort(cells)


def check_shape_of_a_reflect_plan(plan, negate, size):
    assert plan.kind in (0, 1) and plan.n_post == 0 and 0 <= plan.n_pre <= 2
    if plan.kind == 0:
        assert plan.n_pre == 0
        return
    assert plan.reserved == REFLECT_MARK | (NEGATE_MARK if negate else 0), "not marked as a reflection plan (or as something else too)"
    assert plan.n_pre >= 1
    for i in range(plan.n_pre):
        m = plan.pre[i]
        assert m.src_buf == 0 and m.dst_buf == 0 and m.row_pitch == 0, "a reflect-move stays in the pencil and claims no cells between rows"
        assert sum(1 for s in m.ss if s < 0) == 1 and all(d > 0 for d in m.ds), "exactly the source of one dim runs backwards"
        src, dst = _cells(m, "src"), _cells(m, "dst")
        assert min(src.min(), dst.min()) >= 0 and max(src.max(), dst.max()) < size
        both = np.concatenate([src, dst])
        assert np.unique(both).size == both.size, "a reflect-move reads what it writes, or visits a cell twice"
    if plan.n_pre == 2:
        assert plan.pre[0].dst_off < plan.pre[1].dst_off, "the low side comes first"


def execute(plan, cells, rb):
    """the moves of a reflection plan in numpy, one after the other, in place on `cells` (uint8, (cells, element bytes))"""
    for i in range(plan.n_pre):
        m = plan.pre[i]
        x = cells[_cells(m, "src")].copy()
        if plan.reserved & NEGATE_MARK:
            RB.flip_signs(x, rb)
        cells[_cells(m, "dst")] = x


def execute_wrap(plan, cells):
    """the two wrap copies of a single-rank periodic update plan in numpy"""
    assert plan.kind in (0, 1)
    old = cells.copy()
    for i in range(plan.n_pre):
        m = plan.pre[i]
        assert m.src_buf == 0 and m.dst_buf == 0
        cells[_cells(m, "dst")] = old[_cells(m, "src")]


@pytest.mark.parametrize("pdims", list(GRIDS), ids=["%dx%d" % p for p in GRIDS])
def test_reflection_is_the_complement_of_the_fill_and_runs_as_defined(pdims):
    """every rank, axis, dim and memory order; halos, padding, all eight period mixes, both centerings (parity alternates with the
    case number: it changes no cell set, and the numpy execution sees both)"""
    gdims, n = GRIDS[pdims], 0
    for order in PERMS:
        spec = cd.make_grid_spec(gdims, pdims, (order,) * 3)
        for rank, axis, halo, padding in itertools.product(range(pdims[0] * pdims[1]), range(3), HALOS, PADDINGS):
            p = cd.cudecompExtPencilInfo(spec, rank, axis, halo, padding)
            size = int(p.size)
            start = RB.payload(cd.HALF_COMPLEX, size, rank)
            for dim in range(3):
                everywhere = _dst_cells(cd.cudecompExtPlanHaloFill(spec, rank, axis, halo, (True,) * 3, dim, padding))
                for periods, centering in itertools.product(PERIODS, (0, 1)):
                    if centering == 0:
                        filled = _dst_cells(cd.cudecompExtPlanHaloFill(spec, rank, axis, halo, periods, dim, padding))
                        has = [cd.cudecompExtShiftedRank(spec, rank, axis, dim, side, periods[dim]) >= 0 for side in (-1, 1)]
                    negate = bool(n & 1)
                    n += 1
                    where = (gdims, pdims, order, rank, axis, halo, padding, dim, periods, centering, negate)
                    plan = cd.cudecompExtPlanHaloReflect(spec, rank, axis, halo, periods, dim, padding, centering, negate)
                    check_shape_of_a_reflect_plan(plan, negate, size)
                    mirrored = _dst_cells(plan)
                    assert np.intersect1d(mirrored, filled).size == 0, ("reflection and fill share a cell", where)
                    assert np.array_equal(np.sort(np.concatenate([mirrored, filled])), everywhere), ("not the complement", where)
                    assert [plan.neighbor[0] >= 0, plan.neighbor[1] >= 0] == has, where
                    got, want = start.copy(), start.copy()
                    execute(plan, got, RB_)
                    RB.reflect_reference(p, want, halo, dim, has, -1 if negate else 1, centering, RB_)
                    assert np.array_equal(got, want), ("the plan does not compute the definition", where)
                    if mirrored.size:
                        assert not np.array_equal(got, start), where
    assert n == 6 * pdims[0] * pdims[1] * 3 * len(HALOS) * len(PADDINGS) * 3 * 16


@pytest.mark.parametrize("parity", [1, -1], ids=["even", "odd"])
@pytest.mark.parametrize("h", [1, 2, 3])
def test_single_rank_sequences_are_numpy_pad(h, parity):
    """dims 0, 1, 2: the update's wrap copies on periodic dims, the reflection on the others -- against numpy.pad of the
    interior axis by axis (wrap / symmetric / reflect); parity -1: the sign bits flipped where an odd number of reflected dims
    was crossed.  Every axis, memory order, period mix and both centerings; halos (h, h, h) and a mixed one."""
    gdims = GRIDS[(1, 1)]
    for order, axis, halo, padding, periods, centering in itertools.product(PERMS, range(3), [(h, h, h), (h, 1, 4 - h)], PADDINGS,
                                                                            PERIODS, (0, 1)):
        spec = cd.make_grid_spec(gdims, (1, 1), (order,) * 3)
        p = cd.cudecompExtPencilInfo(spec, 0, axis, halo, padding)
        world = RB.payload(cd.HALF_COMPLEX, gdims[0] * gdims[1] * gdims[2], 3).reshape(gdims[2], gdims[1], gdims[0], ES).transpose(2, 1, 0, 3)
        got = np.full((int(p.size), ES), RB.POISON, dtype=np.uint8)
        mem = [int(x) for x in p.order]
        AB.pencil3(p, got)[RB.interior_index(p)] = world.transpose(mem[2], mem[1], mem[0], 3)
        for dim in range(3):
            execute_wrap(cd.cudecompExtPlanHalo(spec, 0, axis, halo, periods, dim, padding), got)
            execute(cd.cudecompExtPlanHaloReflect(spec, 0, axis, halo, periods, dim, padding, centering, parity < 0), got, RB_)
        want = RB.padded_expectation(p, world, halo, periods, parity, centering, RB_)
        assert np.array_equal(got, want), (order, axis, halo, padding, periods, centering)


def test_numpy_pad_restatement_against_a_hand_written_line():
    """the restatement itself, on one line of five cells a..e with h = 2: symmetric b a | a b c d e | e d, reflect c b | a .. e | d c"""
    spec = cd.make_grid_spec((5, 1, 1), (1, 1), ((0, 1, 2),) * 3)
    p = cd.cudecompExtPencilInfo(spec, 0, 0, (2, 0, 0), None)
    line = np.array([[0x10 + i, i] for i in range(5)], dtype=np.uint8).reshape(5, 1, 1, 2)
    plus = lambda ids: [[0x10 + i, i] for i in ids]
    minus = lambda ids: [[0x10 + i, i ^ 0x80] for i in ids]
    got = RB.padded_expectation(p, line, (2, 0, 0), (False,) * 3, 1, 0, 2)
    assert got.tolist() == plus([1, 0, 0, 1, 2, 3, 4, 4, 3])
    got = RB.padded_expectation(p, line, (2, 0, 0), (False,) * 3, -1, 1, 2)
    assert got.tolist() == minus([2, 1]) + plus([0, 1, 2, 3, 4]) + minus([3, 2])
    got = RB.padded_expectation(p, line, (2, 0, 0), (True,) * 3, -1, 1, 2)
    assert got.tolist() == plus([3, 4, 0, 1, 2, 3, 4, 0, 1])


# ---- refusals and result codes --------------------------------------------------------------------------------------------
def test_planner_refusals():
    order = ((0, 1, 2),) * 3
    one = cd.make_grid_spec((5, 6, 7), (1, 1), order)
    code = lambda call: _planned(call)[1]
    # h + centering against the interior (gdims of a single rank ARE its interior): refused one above it, served at it
    for gx, h, c, want in ((9, 3, 0, None), (9, 3, 1, None), (4, 3, 1, None), (3, 3, 1, INVALID_USAGE), (3, 3, 0, None),
                           (2, 3, 0, INVALID_USAGE), (2, 1, 1, None), (1, 1, 1, INVALID_USAGE), (1, 1, 0, None)):
        spec = cd.make_grid_spec((gx, 6, 7), (1, 1), order)
        assert code(lambda: cd.cudecompExtPlanHaloReflect(spec, 0, 0, (h, 0, 0), (False,) * 3, 0, None, c)) == want, (gx, h, c)
        # ... but not where nothing would be written: the dim is periodic
        assert code(lambda: cd.cudecompExtPlanHaloReflect(spec, 0, 0, (h, 0, 0), (True,) * 3, 0, None, c)) is None
    # ... nor on a rank away from the edge, and only on the ranks that write: 1 x 3 ranks along Z of X pencils, slabs of 2
    three = cd.make_grid_spec((4, 4, 6), (1, 3), order)
    assert cd.cudecompExtPlanHaloReflect(three, 1, 0, (0, 0, 2), (False,) * 3, 2, None, 1).kind == 0
    for rank in (0, 2):
        assert code(lambda: cd.cudecompExtPlanHaloReflect(three, rank, 0, (0, 0, 2), (False,) * 3, 2, None, 1)) == INVALID_USAGE
        assert cd.cudecompExtPlanHaloReflect(three, rank, 0, (0, 0, 2), (False,) * 3, 2, None, 0).n_pre == 1
    # centering
    for c in (-1, 2):
        assert code(lambda: cd.cudecompExtPlanHaloReflect(one, 0, 0, (1, 1, 1), (False,) * 3, 0, None, c)) == INVALID_USAGE
    # the update's refusals come first, with the update's code
    four = cd.make_grid_spec((4, 4, 4), (2, 2), order)
    empty = cd.make_grid_spec((3, 8, 8), (4, 1), order)
    for spec, rank, axis, halo, per, dim in ((four, 0, 0, (0, 3, 0), (True,) * 3, 1), (empty, 0, 1, (1, 1, 1), (True,) * 3, 0)):
        want = code(lambda: cd.cudecompExtPlanHaloFill(spec, rank, axis, halo, per, dim))
        assert want in (INVALID_USAGE, NOT_SUPPORTED)
        for c in (0, 1, 7):
            assert code(lambda: cd.cudecompExtPlanHaloReflect(spec, rank, axis, halo, per, dim, None, c)) == want
    assert code(lambda: cd.cudecompExtPlanHaloReflect(empty, 0, 1, (1, 1, 1), (True,) * 3, 0, None, 7)) == NOT_SUPPORTED
    # planner arguments
    for call in (lambda: cd.cudecompExtPlanHaloReflect(four, 4, 0, (1, 1, 1), None, 0), lambda: cd.cudecompExtPlanHaloReflect(four, 0, 3, (1, 1, 1), None, 0),
                 lambda: cd.cudecompExtPlanHaloReflect(four, 0, 0, (1, 1, 1), None, 3), lambda: cd.cudecompExtPlanHaloReflect(four, 0, 0, None, None, 0)):
        assert code(call) == INVALID_USAGE
    # no other plan carries the marks
    for p in (cd.cudecompExtPlanHalo(one, 0, 0, (1, 1, 1), (True,) * 3, 1), cd.cudecompExtPlanHaloFill(one, 0, 0, (1, 1, 1), (True,) * 3, 1),
              cd.cudecompExtPlanHaloAccumulate(one, 0, 0, (1, 1, 1), (True,) * 3, 1)):
        assert p.reserved & (REFLECT_MARK | NEGATE_MARK) == 0


def test_entry_points_check_their_arguments():
    """the fill's bad-argument tuples: every return code is the fill's, whatever parity and centering are; a tuple the fill accepts
    is INVALID_USAGE for parity 0 / 2 and centering -1 / 2, also when every halo is zero"""
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
               (h, gd, None, 99, None, None, 5, None, None),                     # several at once: the first check decides
               (h, gd, None, cd.FLOAT, i3(1, 1, 1), None, 3, None, None)]
    accepted = [(h, gd, None, cd.FLOAT, i3(0, 0, 0), None, 0, None, None),        # all halos zero: success before input is looked at
                (h, gd, None, cd.FLOAT, i3(0, 0, 0), None, 7, None, None),
                (h, gd, 1, cd.DOUBLE, i3(1, 0, 1), None, 1, i3(1, 2, 0), None)]   # h == 0 along dim: success, no effect
    good = [(1, 0), (-1, 0), (1, 1), (-1, 1)]
    bad = [(0, 0), (2, 1), (1, -1), (-1, 2), (0, 2)]
    for name in cd.AMD_REFLECT_SYMBOLS:
        fn, fill = getattr(L, name), getattr(L, name.replace("Reflect", "Fill"))
        for hh, g, inp, dtype, halo, per, dim, pad, stream in refused:
            want = fill(hh, g, inp, dtype, None, halo, per, dim, pad, stream)
            assert want != cd.RESULT_SUCCESS
            for parity, centering in good + bad:
                assert fn(hh, g, inp, dtype, parity, centering, halo, per, dim, pad, stream) == want, (name, inp, dtype, dim, parity, centering)
        for hh, g, inp, dtype, halo, per, dim, pad, stream in accepted:
            assert fill(hh, g, inp, dtype, None, halo, per, dim, pad, stream) == cd.RESULT_SUCCESS
            for parity, centering in good:
                assert fn(hh, g, inp, dtype, parity, centering, halo, per, dim, pad, stream) == cd.RESULT_SUCCESS, (name, dim, parity, centering)
            for parity, centering in bad:
                assert fn(hh, g, inp, dtype, parity, centering, halo, per, dim, pad, stream) == cd.RESULT_INVALID_USAGE, (name, dim, parity, centering)
    # periodic along dim: nothing to mirror, so no device is needed either (the fill has cells to write there)
    for parity, centering in good + bad:
        want = cd.RESULT_SUCCESS if (parity, centering) in good else cd.RESULT_INVALID_USAGE
        assert L.cudecompAmdReflectHalosY(h, gd, 1, cd.FLOAT, parity, centering, i3(1, 1, 1), b3(True, True, True), 0, None, None) == want
    # h + centering one above the interior (X: 9 cells, h = 9, centering 1): refused before the device is looked at -- unless the
    # dim is periodic and nothing would be written
    for parity in (1, -1):
        assert L.cudecompAmdReflectHalosX(h, gd, 1, cd.FLOAT, parity, 1, i3(9, 0, 0), None, 0, None, None) == cd.RESULT_INVALID_USAGE
        assert L.cudecompAmdReflectHalosX(h, gd, 1, cd.FLOAT, parity, 1, i3(9, 0, 0), b3(True, False, False), 0, None, None) == cd.RESULT_SUCCESS
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def test_with_and_without_cells_to_write_on_this_device():
    """a non-periodic single rank has ghost cells to mirror on every dim: without a device the call answers
    CUDECOMP_RESULT_CUDA_ERROR (the pointer is never looked at), with one it succeeds on a real buffer; with nothing to write
    (periodic dims) it succeeds either way"""
    import torch
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    halo = (1, 2, 1)
    for axis, name in enumerate(cd.AMD_REFLECT_SYMBOLS):
        fn = getattr(L, name)
        if torch.cuda.is_available():
            data = torch.zeros(int(cd.cudecompGetPencilInfo(h, gd, axis, halo).size), dtype=torch.float32, device="cuda")
            inp, expected = data.data_ptr(), cd.RESULT_SUCCESS
        else:
            inp, expected = 1, cd.RESULT_CUDA_ERROR
        for dim, (parity, centering) in itertools.product(range(3), ((1, 0), (-1, 1))):
            assert fn(h, gd, inp, cd.FLOAT, parity, centering, i3(*halo), b3(False, False, False), dim, None, None) == expected, (name, dim)
            assert fn(h, gd, inp, cd.FLOAT, parity, centering, i3(*halo), b3(True, True, True), dim, None, None) == cd.RESULT_SUCCESS
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def test_python_wrapper_rejects_bad_parity_and_centering():
    for parity, centering in ((0, 0), (2, 0), (1, -1), (1, 2), (-1, 2)):
        with pytest.raises(ValueError):
            cd.cudecompReflectHalos(0, None, None, 1, cd.DOUBLE, parity, centering, (1, 1, 1), None, 0)


# ---- kernel choices (cudecompExtDescribeMoves, modes 5 / 6) --------------------------------------------------------------
def _mirror(extent, ss, ds, mirrored, soff=0, doff=0, row_pitch=0):
    """a mirror-move inside one buffer: the source block at soff, its `mirrored` dim read backwards, the destination at doff"""
    ss = list(ss)
    soff += (extent[mirrored] - 1) * ss[mirrored]
    ss[mirrored] = -ss[mirrored]
    return cd.make_move(extent, ss, ds, soff, doff, 0, 0, row_pitch)


def test_both_sides_share_one_launch_of_the_row_kernel():
    """the two moves of a plan -- mirrored dim the middle or the slowest memory axis -- are siblings of one interleaved launch of
    kind 16; with parity -1 the launch carries the real type; 32 MiB and more stream"""
    spec = cd.make_grid_spec((40, 36, 30), (1, 1), ((0, 1, 2),) * 3)
    for dim, halo, dtype, negate in itertools.product((1, 2), ((1, 1, 1), (2, 3, 2)), (cd.DOUBLE, cd.HALF, cd.FLOAT_COMPLEX), (False, True)):
        plan = cd.cudecompExtPlanHaloReflect(spec, 0, 0, halo, (False,) * 3, dim, None, 1, negate)
        moves = [plan.pre[i] for i in range(plan.n_pre)]
        es = AB.element_bytes(dtype)
        (l,) = ML.describe(moves, ML.FAKE, es, cd.MOVES_REFLECT_NEGATE if negate else cd.MOVES_REFLECT, dtype)
        assert (l["kind"], l["cls"], l["n"], l["interleave"], l["access"]) == (K_ROWS_REFLECT, 0, 2, 1, 0), (dim, halo, l)
        assert l["arith"] == ({cd.DOUBLE: 4, cd.HALF: 1, cd.FLOAT_COMPLEX: 3}[dtype] if negate else 0)
        assert l["vec"] >= es and l["elements"] == 2 * plan.face_elements
    big = _mirror((2048, 1024, 2), (1, 2048, 2048 * 1024 * 2), (1, 2048, 2048 * 1024), 2, soff=0, doff=2048 * 1024 * 8)
    (l,) = ML.describe([big], ML.FAKE, 8, cd.MOVES_REFLECT)
    assert (l["kind"], l["vec"], l["access"]) == (K_ROWS_REFLECT, 16, 1)
    small = _mirror((2048, 1024, 2), (1, 2048, 2048 * 1024 * 2), (1, 2048, 2048 * 1024), 2, doff=2048 * 1024 * 8)
    (l,) = ML.describe([small], ML.FAKE, 4, cd.MOVES_REFLECT)
    assert (l["kind"], l["vec"], l["access"]) == (K_ROWS_REFLECT, 16, 0)
    (l,) = ML.describe([small], ML.FAKE, 4, cd.MOVES_REFLECT, flags=2)
    assert l["access"] == 1


def test_two_byte_rows_at_two_mod_four_take_two_byte_lanes():
    for soff, doff, pitch, want in ((0, 4000, 64, 16), (1, 4000, 64, 2), (0, 4001, 64, 2), (0, 4000, 65, 2), (2, 4002, 66, 4)):
        m = _mirror((32 if want != 4 else 30, 5, 3), (1, pitch, pitch * 8), (1, pitch, pitch * 8), 1, soff, doff)
        for mode, dtype in ((cd.MOVES_REFLECT, 0), (cd.MOVES_REFLECT_NEGATE, cd.HALF), (cd.MOVES_REFLECT_NEGATE, cd.BFLOAT16)):
            (l,) = ML.describe([m], ML.FAKE, 2, mode, dtype)
            assert (l["kind"], l["vec"]) == (K_ROWS_REFLECT, want), (soff, doff, pitch, l)


def test_a_mirrored_fastest_dim_is_always_element_wise():
    """dim as the fastest memory axis: rows of h elements reversed in themselves, a row pitch apart"""
    spec = cd.make_grid_spec((40, 36, 30), (1, 1), ((0, 1, 2),) * 3)
    for h, es, negate in itertools.product((1, 2, 3, 5), (2, 4, 8, 16), (False, True)):
        dtype = {2: cd.HALF, 4: cd.FLOAT, 8: cd.DOUBLE, 16: cd.DOUBLE_COMPLEX}[es]
        plan = cd.cudecompExtPlanHaloReflect(spec, 0, 0, (h, 1, 1), (False,) * 3, 0, None, 0, negate)
        moves = [plan.pre[i] for i in range(plan.n_pre)]
        (l,) = ML.describe(moves, ML.FAKE, es, cd.MOVES_REFLECT_NEGATE if negate else cd.MOVES_REFLECT, dtype)
        assert (l["kind"], l["cls"], l["n"], l["vec"], l["access"]) == (K_GENERIC_REFLECT, 2, 2, es, 0), (h, es, l)
    for extent in ((5, 1, 1), (5, 7, 3), (2, 300, 1)):
        m = _mirror(extent, (1, 40, 40 * 400), (1, 40, 40 * 400), 0, soff=10, doff=0)
        (l,) = ML.describe([m], ML.FAKE, 8, cd.MOVES_REFLECT, flags=2)
        assert (l["kind"], l["access"]) == (K_GENERIC_REFLECT, 0), extent
    # forced (flag bit 0), and a move with no contiguous dim at all
    m = _mirror((32, 5, 3), (1, 64, 640), (1, 64, 640), 2, doff=4000)
    assert ML.describe([m], ML.FAKE, 8, cd.MOVES_REFLECT, flags=1)[0]["kind"] == K_GENERIC_REFLECT
    m = _mirror((32, 5, 3), (2, 64, 640), (2, 64, 640), 1, doff=4000)
    assert ML.describe([m], ML.FAKE, 8, cd.MOVES_REFLECT)[0]["kind"] == K_GENERIC_REFLECT


def test_what_a_reflect_move_never_carries():
    m = _mirror((32, 5, 3), (1, 64, 640), (1, 64, 640), 1, doff=4000)
    assert ML.describe([m], ML.FAKE, 8, cd.MOVES_REFLECT)[0]["kind"] == K_ROWS_REFLECT
    code = lambda call: _planned(call)[1]
    with_pitch = _mirror((32, 5, 3), (1, 64, 640), (1, 64, 640), 1, doff=4000, row_pitch=64)
    for mode, dtype in ((cd.MOVES_REFLECT, 0), (cd.MOVES_REFLECT_NEGATE, cd.DOUBLE)):
        assert code(lambda: ML.describe([with_pitch], ML.FAKE, 8, mode, dtype)) == INTERNAL_ERROR
        assert code(lambda: ML.describe([m], ML.FAKE, 8, mode, dtype, base_addresses=[1 << 44])) == INTERNAL_ERROR
    two = cd.make_move((32, 5, 3), (1, -64, -640), (1, 64, 640), 2000, 4000, 0, 0)
    assert code(lambda: ML.describe([two], ML.FAKE, 8, cd.MOVES_REFLECT)) == INTERNAL_ERROR  # two mirrored dims
    assert code(lambda: ML.describe([m], ML.FAKE, 8, cd.MOVES_REFLECT_NEGATE, cd.FLOAT)) == INVALID_USAGE  # the type's size is not es
    assert code(lambda: ML.describe([m], ML.FAKE, 8, 7)) == INVALID_USAGE  # no such mode
    # every other mode answers for the same geometry without the mirror as before; the mirror modes refuse it: no dim is named
    plain = cd.make_move((32, 5, 3), (1, 64, 640), (1, 64, 640), 0, 4000, 0, 0)
    assert ML.describe([plain], ML.FAKE, 8, cd.MOVES_COPY)[0]["kind"] == 0
    for mode, dtype in ((cd.MOVES_REFLECT, 0), (cd.MOVES_REFLECT_NEGATE, cd.DOUBLE)):
        assert code(lambda: ML.describe([plain], ML.FAKE, 8, mode, dtype)) == INVALID_USAGE
    # a mirrored dim one cell thick still names itself
    thin = _mirror((32, 1, 3), (1, 64, 640), (1, 64, 640), 1, doff=4000)
    assert ML.describe([thin], ML.FAKE, 8, cd.MOVES_REFLECT)[0]["kind"] == K_ROWS_REFLECT


# ---- header, exports ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_alone(tmp_path, lang):
    src = tmp_path / ("t.c" if lang == "c99" else "t.cc")
    src.write_text('#include "cudecomp_amd_reflect.h"\nint main(void) { return cudecompAmdReflectHalosX == 0; }\n')
    cc = ["gcc", "-std=c99"] if lang == "c99" else ["g++", "-std=c++17"]
    r = subprocess.run(cc + ["-Wall", "-Werror", "-pedantic-errors", "-Wno-address", "-fsyntax-only"] + CFLAGS + [str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(cudecomp\w+)\s*\(", src))


def test_header_declares_and_library_exports_the_symbols():
    assert _declared("cudecomp_amd_reflect.h") == set(cd.AMD_REFLECT_SYMBOLS) == {"cudecompAmdReflectHalos" + a for a in "XYZ"}
    assert '#include "cudecomp_amd.h"' in open(os.path.join(ROOT, "include", "cudecomp_amd_reflect.h")).read()
    L = cd.lib()
    ext = ["cudecompExtPlanHaloReflect", "cudecompExtReflect3D"]
    for name in cd.AMD_REFLECT_SYMBOLS + ext:
        assert hasattr(L, name), name
    assert set(ext) <= _declared("cudecomp_ext.h") and set(ext) <= set(cd.EXT_SYMBOLS)
    # the older headers stay as they were: the reflection lives in a header of its own
    assert _declared("cudecomp_amd_fill.h") == set(cd.AMD_FILL_SYMBOLS)
    assert "Reflect" not in open(os.path.join(ROOT, "include", "cudecomp_amd.h")).read()


def test_arguments_are_checked_in_the_stated_order(capfd):
    from tests import halo_check_order
    halo_check_order.check("reflect", capfd)
