"""Halo accumulate-and-clear (cudecomp_amd_fill.h: cudecompAmdAccumulateAndClearHalos{X,Y,Z}) without a GPU.

The fused call is accumulation whose moves out of the pencil also store zero bytes to what they have read.  So, over every rank
of a sweep of grids (ragged ones, all axes, three sets of memory orders, three halos, the period mixes and paddings of the fill
tests, packed and not): the fused plan (cudecompExtPlanHaloAccumulateClear) IS the accumulation plan
(cudecompExtPlanHaloAccumulate) in kind, neighbours, offsets and every move's geometry; the source-clearing marks sit on exactly
the moves whose source buffer is the pencil and on no move after the exchange; and the cells they clear are, cell for cell, the
destinations of the fill plan (cudecompExtPlanHaloFill) for the same arguments.  The fused plans of all ranks are then executed
on host arrays with numpy, the exchange simulated, and whole pencils compared with AB.accumulate_reference followed by zeroing
the fill plan's cells.  Further: the kernel choice of take-moves (cudecompExtDescribeMoves modes 3 and 4) and the validation of
the three entry points.  Nothing here has a tolerance."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import move_lists as ML
from tests import test_halo_accumulate_plan as TAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_USAGE, NOT_SUPPORTED, INTERNAL_ERROR = cd.RESULT_INVALID_USAGE, cd.RESULT_NOT_SUPPORTED, cd.RESULT_INTERNAL_ERROR
FUSED_MARK, TAKE_SHIFT = 512, 10  # cudecompExtHaloPlan_t::reserved: bit 9; bits 10, 11: pre[0], pre[1] clear their source
ORDERS = {"default": ((0, 1, 2),) * 3, "contiguous": ((0, 1, 2), (1, 2, 0), (2, 0, 1)), "mixed": ((1, 0, 2), (2, 1, 0), (0, 2, 1))}
HALOS = [(1, 1, 1), (2, 0, 3), (3, 2, 1)]
PERIODS = [(1, 1, 1), (1, 0, 1), (0, 0, 0)]    # (tests/test_gpu_halo_fill.py)
PADDINGS = [(0, 0, 0), (1, 2, 0)]
GRIDS = [((11, 9, 7), (1, 1)), ((10, 9, 11), (2, 1)), ((10, 9, 11), (2, 2)), ((11, 13, 10), (3, 2)), ((9, 14, 11), (1, 3))]
MOVE_FIELDS = ("src_buf", "dst_buf", "src_off", "dst_off", "peer", "row_pitch")


def _planned(call):
    try:
        return call(), None
    except cd.CudecompError as e:
        return None, e.code


def _move(m):
    return tuple(getattr(m, f) for f in MOVE_FIELDS) + (tuple(m.extent), tuple(m.ss), tuple(m.ds))


def _geometry(p):
    return (p.kind, p.comm_axis, tuple(p.neighbor), p.xbuf, p.n_pre, p.n_post, p.face_elements, tuple(p.send_off), tuple(p.recv_off),
            tuple(_move(p.pre[i]) for i in range(p.n_pre)), tuple(_move(p.post[i]) for i in range(p.n_post)))


def cleared_cells(p):
    """the source cells of the moves marked as clearing their source"""
    parts = [TAP._cells(p.pre[i], "src_off", "ss") for i in range(p.n_pre) if (p.reserved >> (TAKE_SHIFT + i)) & 1]
    cells = np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    assert np.unique(cells).size == cells.size, "two moves clear the same cell"
    return np.sort(cells)


def fill_cells(p):
    parts = [TAP._cells(p.pre[i], "dst_off", "ds") for i in range(p.n_pre)]
    return np.sort(np.concatenate(parts)) if parts else np.zeros(0, dtype=np.int64)


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("gdims,pdims", GRIDS, ids=["%dx%d" % g[1] for g in GRIDS])
def test_fused_plan_is_the_accumulation_plan_with_marks(gdims, pdims, layout):
    spec = cd.make_grid_spec(gdims, pdims, ORDERS[layout])
    compared = refused = marked = packed = wrapped = one_sided = 0
    for rank, axis, dim, halo, periods, padding, fp in itertools.product(range(pdims[0] * pdims[1]), range(3), range(3), HALOS, PERIODS,
                                                                         PADDINGS, (False, True)):
        where = (gdims, pdims, layout, rank, axis, dim, halo, periods, padding, fp)
        fused, fcode = _planned(lambda: cd.cudecompExtPlanHaloAccumulateClear(spec, rank, axis, halo, periods, dim, padding, fp))
        acc, acode = _planned(lambda: cd.cudecompExtPlanHaloAccumulate(spec, rank, axis, halo, periods, dim, padding, fp))
        assert fcode == acode, ("the fused plan's refusal is not the accumulation's", fcode, acode, where)
        if fcode is not None:
            assert fcode in (INVALID_USAGE, NOT_SUPPORTED), where
            refused += 1
            continue
        assert _geometry(fused) == _geometry(acc), where
        compared += 1
        # the marks: the accumulation's own, bit 9, and bits 10 / 11 on exactly the moves that read the pencil
        takes = sum(1 << (TAKE_SHIFT + i) for i in range(fused.n_pre) if fused.pre[i].src_buf == 0)
        assert fused.reserved == acc.reserved | FUSED_MARK | takes, (bin(fused.reserved), bin(acc.reserved), where)
        assert acc.reserved & (FUSED_MARK | (3 << TAKE_SHIFT)) == 0
        for i in range(fused.n_post):
            assert fused.post[i].src_buf == 2, ("a move after the exchange reads the pencil", where)
        if fused.kind == 0:
            assert takes == 0
        else:
            assert takes == sum(1 << (TAKE_SHIFT + i) for i in range(fused.n_pre)) and fused.n_pre >= 1, where
            for i in range(fused.n_pre):
                assert fused.pre[i].row_pitch == 0, "a take-move never claims the cells between rows"
                assert bool((fused.reserved >> (4 + i)) & 1) == (fused.kind == 1), "wrap moves add, packs copy"
            marked += fused.n_pre
            packed += fused.kind == 2
            wrapped += fused.kind == 1
            one_sided += fused.n_pre == 1
        # what is cleared is what the fill names
        fill = cd.cudecompExtPlanHaloFill(spec, rank, axis, halo, periods, dim, padding, fp)
        assert np.array_equal(cleared_cells(fused), fill_cells(fill)), ("cleared cells differ from the fill plan's destinations", where)
        assert list(fill.neighbor) == list(fused.neighbor), where
    assert compared > 10 * refused and marked > 0, (compared, refused, marked)
    split = pdims != (1, 1)  # packed plans and one-sided ones (edge ranks of a non-periodic dim) need a split dim; every grid wraps somewhere
    assert (packed > 0) == split and wrapped > 0 and (one_sided > 0) == split, (packed, wrapped, one_sided)


# ---- numpy execution of the fused plans -------------------------------------------------------------------------------------------
def run_moves(moves, n, add_bits, take_bits, bufs, ordered):
    """TAP.run_moves, with take-moves: after a move has read its source cells it stores zero to them"""
    live = [moves[i] for i in range(n) if 0 not in list(moves[i].extent)]
    if len(live) == 2 and live[0].dst_buf == live[1].dst_buf:
        shared = np.intersect1d(TAP._cells(live[0], "dst_off", "ds"), TAP._cells(live[1], "dst_off", "ds")).size
        assert shared == 0 or ordered, "two moves of one phase write the same cells and the plan does not say so"
    if take_bits:  # a cleared cell is no destination and no other move's source
        src = [TAP._cells(m, "src_off", "ss") for m in live if m.src_buf == 0]
        dst = [TAP._cells(m, "dst_off", "ds") for m in live if m.dst_buf == 0]
        assert np.unique(np.concatenate(src)).size == sum(s.size for s in src), "sources of one phase overlap"
        if dst:
            assert np.intersect1d(np.concatenate(src), np.concatenate(dst)).size == 0, "a cleared cell is also written"
    for i in range(n):
        m = moves[i]
        if 0 in list(m.extent):
            continue
        src_view = TAP._view(bufs[m.src_buf], m.src_off, m.extent, m.ss)
        src = src_view.copy()
        dst = TAP._view(bufs[m.dst_buf], m.dst_off, m.extent, m.ds)
        if (add_bits >> i) & 1:
            assert m.dst_buf == 0 and m.row_pitch == 0
            dst[...] += src
        else:
            dst[...] = src
        if (take_bits >> i) & 1:
            assert m.src_buf == 0
            src_view[...] = 0


def execute(plans, data, work, wsz):
    n = len(plans)
    for r in range(n):
        p = plans[r]
        assert p.kind in (0, 1, 2)
        if p.kind == 0:
            continue
        assert p.reserved & 1 and p.reserved & FUSED_MARK
        if p.kind == 2:
            assert p.xbuf == 2
            for i in range(2):
                assert 0 <= p.send_off[i] and p.send_off[i] + p.face_elements <= wsz[r]
                assert 0 <= p.recv_off[i] and p.recv_off[i] + p.face_elements <= wsz[r]
        run_moves(p.pre, p.n_pre, (p.reserved >> 4) & 3, (p.reserved >> TAKE_SHIFT) & 3, [data[r], data[r], work[r]], bool(p.reserved & 2))
    flights = []
    for r in range(n):
        p = plans[r]
        if p.kind != 2:
            continue
        for i in range(2):
            nb = p.neighbor[i]
            if nb < 0:
                continue
            q = plans[nb]
            assert q.kind == 2 and q.neighbor[1 - i] == r and q.face_elements == p.face_elements
            flights.append((nb, q.recv_off[1 - i], work[r][p.send_off[i]:p.send_off[i] + p.face_elements].copy()))
    for nb, off, face in flights:
        assert not (face == TAP.POISON).any(), "a send slot travels with cells nobody packed"
        work[nb][off:off + face.size] = face
    for r in range(n):
        p = plans[r]
        if p.kind == 2:
            run_moves(p.post, p.n_post, (p.reserved >> 6) & 3, 0, [data[r], data[r], work[r]], bool(p.reserved & 2))


SIMULATED = [((11, 9, 7), (1, 1)), ((10, 9, 11), (2, 1)), ((10, 9, 11), (2, 2)),
             ((3, 5, 4), (1, 1)), ((5, 3, 3), (1, 1))]  # (the last two: interior narrower than two halos, tests/test_gpu_halo_accumulate.py)


@pytest.mark.parametrize("gdims,pdims", SIMULATED, ids=["g%d_%d_%d_%dx%d" % (g[0] + g[1]) for g in SIMULATED])
def test_fused_plans_executed_in_numpy(gdims, pdims):
    """dims 2, 1, 0 in turn on every rank; after every call whole pencils equal AB.accumulate_reference followed by zero into the
    fill plan's cells -- and, at the end, the accumulation along 2, 1, 0 followed by the fills along 0, 1, 2"""
    narrow = min(gdims) <= 5
    halos = [(2, 2, 2), (3, 2, 3)][gdims == (5, 3, 3):][:1] if narrow else HALOS
    ran = ordered = 0
    for layout, halo, periods, padding, fp, axis in itertools.product(ORDERS, halos, PERIODS, PADDINGS, (False, True), range(3)):
        d = {"gdims": gdims, "pdims": pdims, "mem_order": ORDERS[layout], "gdims_dist": None, "col_major": False}
        spec, g = TAP._grids(d)
        n = g.nranks
        infos = [g.pencil_info(r, axis, halo, padding) for r in range(n)]
        wsz = [max(g.halo_workspace_size(r, axis, halo), 1) for r in range(n)]
        init = [AB.initial_cells(7, r, axis, infos[r].size, 1).reshape(-1) + 1 for r in range(n)]  # 1..8: no cell starts at zero
        data = [a.copy() for a in init]
        want = [a.copy().reshape(-1, 1) for a in init]
        late = [a.copy().reshape(-1, 1) for a in init]  # accumulate 2, 1, 0, THEN fill 0, 1, 2
        fills = {}
        try:
            for dim in (2, 1, 0):
                plans = [cd.cudecompExtPlanHaloAccumulateClear(spec, r, axis, halo, periods, dim, padding, fp) for r in range(n)]
                fills[dim] = [fill_cells(cd.cudecompExtPlanHaloFill(spec, r, axis, halo, periods, dim, padding, fp)) for r in range(n)]
                work = [np.full(wsz[r], TAP.POISON, dtype=np.int64) for r in range(n)]
                execute(plans, data, work, wsz)
                ordered += any(p.reserved & 2 for p in plans)
                AB.accumulate_reference(g, axis, halo, periods, dim, infos, want)
                AB.accumulate_reference(g, axis, halo, periods, dim, infos, late)
                for r in range(n):
                    want[r][fills[dim][r]] = 0
                    assert np.array_equal(data[r], want[r].reshape(-1)), ("rank %d differs after dim %d" % (r, dim), layout, halo, periods, padding, fp, axis)
        except cd.CudecompError as e:
            assert e.code == INVALID_USAGE and not narrow, (e.code, layout, halo, periods, padding, fp, axis)
            continue
        for dim in (0, 1, 2):
            for r in range(n):
                late[r][fills[dim][r]] = 0
        for r in range(n):
            assert np.array_equal(data[r], late[r].reshape(-1)), ("rank %d: fused 2 1 0 differs from accumulate 2 1 0, fill 0 1 2" % r, layout, halo, periods, padding, fp, axis)
        ran += 1
    assert ran >= 50, ran
    assert ordered > 0 or not narrow, "no plan of an interior narrower than two halos was ordered"


# ---- kernel choice of take-moves --------------------------------------------------------------------------------------------------
def _choices(moves, es, mode, dtype=0, flags=0):
    return [(l["kind"], l["vec"], l["access"], l["arith"], l["cls"]) for l in ML.describe(moves, ML.FAKE, es, mode, dtype, flags)]


TYPE_OF_ES = {2: cd.HALF, 4: cd.FLOAT, 8: cd.DOUBLE, 16: cd.DOUBLE_COMPLEX}


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_take_moves_follow_the_rule_of_the_add_moves(es):
    """kinds 12-15: the row / element-wise choice, the lane width and the access mode the add-move of the same geometry gets
    (kind 8 -> 14 and 12, 9 -> 15 and 13) -- whatever the copy of that geometry would take (shifted, dense, transposing forms)"""
    dtype = TYPE_OF_ES[es]
    seen = set()
    cands = list(ML.row_candidates(es, [1, 2, 3, 4, 8, 12, 16, 33, 64, 130, 1031], soff=0, doff=0)) + \
        list(ML.row_candidates(es, [2, 16, 33, 256], soff=1, doff=3)) + list(ML.row_candidates(es, [64, 512], doff=1, pitch=False))
    # a source that is not unit-stride, a transposed destination, a face one element thick on either side
    cands += [((64, 8, 2), (2, 128, 1024), (1, 64, 512), 0, 0, 0), ((64, 64, 2), (1, 64, 4096), (64, 1, 4096), 0, 0, 0),
              ((1, 9, 7), (1, 13, 13 * 12), (1, 1, 9), 0, 0, 0), ((1, 9, 7), (1, 1, 9), (1, 13, 13 * 12), 2, 1, 0)]
    for (extent, ss, ds, soff, doff, pitch), flags in itertools.product(cands, (0, 1, 2, 4)):
        m = [cd.make_move(extent, ss, ds, soff, doff, 0, 1, 0)]
        (add,) = _choices(m, es, cd.MOVES_ADD, dtype, flags)
        (take,) = _choices(m, es, cd.MOVES_TAKE, 0, flags)
        (add_take,) = _choices(m, es, cd.MOVES_ADD_TAKE, dtype, flags)
        assert add[0] in (8, 9)
        assert add_take == (add[0] + 6,) + add[1:], (extent, ss, ds, soff, doff, flags, add, add_take)
        assert take == (add[0] + 4, add[1], add[2], 0, add[4]), (extent, ss, ds, soff, doff, flags, add, take)
        if flags & 1:
            assert take[0] == 13 and add_take[0] == 15
        seen.add(take[:3])
    assert {k for k, _, _ in seen} == {12, 13} and {v for k, v, _ in seen if k == 12} == {v for v in (16, 8, 4, 2) if v >= es}
    assert {a for k, _, a in seen if k == 12} == {0, 1} and {a for k, _, a in seen if k == 13} == {0}
    # 2-byte elements at 2 mod 4 take 2-byte lanes; the size threshold of the streaming instantiation
    if es == 2:
        assert _choices([cd.make_move((64, 8, 2), (1, 64, 512), (1, 66, 600), 1, 0)], 2, cd.MOVES_TAKE)[0][:2] == (12, 2)
        assert _choices([cd.make_move((64, 8, 2), (1, 64, 512), (1, 67, 670), 0, 0)], 2, cd.MOVES_ADD_TAKE, cd.BFLOAT16)[0][:2] == (14, 2)
    n = (32 << 20) // es
    assert _choices([cd.make_move((n, 1, 1), (1, 0, 0), (1, 0, 0))], es, cd.MOVES_TAKE)[0][:3] == (12, 16, 1)
    assert _choices([cd.make_move((n - 1, 1, 1), (1, 0, 0), (1, 0, 0))], es, cd.MOVES_TAKE)[0][2] == 0
    assert _choices([cd.make_move((n, 1, 1), (1, 0, 0), (1, 0, 0))], es, cd.MOVES_ADD_TAKE, dtype)[0][:3] == (14, 16, 1)


def test_take_moves_are_regrouped_apart_split_at_eight_and_interleaved():
    es, dtype = 8, cd.DOUBLE
    p = ML.Packer(gap=3, align=256)
    for w in (64, 63, 64, 1, 64, 63, 64, 64, 64, 64, 64, 64):  # vec 16, vec 8, element-wise (w == 1 with a pitch), ...
        p.add((w, 5, 3), (1, w + 6, (w + 6) * 6), (1, w + 2, (w + 2) * 7))
    for mode, kinds in ((cd.MOVES_TAKE, (12, 13)), (cd.MOVES_ADD_TAKE, (14, 15))):
        ls = ML.describe(p.moves, ML.FAKE, es, mode, dtype)
        same = ML.describe(p.moves, ML.FAKE, es, cd.MOVES_ADD, dtype)
        # the grouping of additions: vec 16 (8 of them, the split at eight), vec 8 (two), element-wise (one), the ninth vec 16
        assert [(l["kind"], l["vec"], l["n"], l["interleave"], l["index"]) for l in ls] == \
            [(l["kind"] + (6 if mode == cd.MOVES_ADD_TAKE else 4), l["vec"], l["n"], l["interleave"], l["index"]) for l in same]
        assert [(l["kind"], l["vec"], l["n"], l["interleave"]) for l in ls] == [(kinds[0], 16, 8, 1), (kinds[0], 8, 2, 1), (kinds[1], 8, 1, 0),
                                                                                 (kinds[0], 16, 1, 0)]
        assert ls[0]["index"] == [0, 2, 4, 6, 7, 8, 9, 10][:8] and ls[0]["blocks"] == 8 * max(b - a for a, b in zip(ls[0]["first_block"], ls[0]["first_block"][1:]))
    # take-moves never share a launch with plain moves: the choice differs by kind, whatever else agrees
    take = ML.choice_of(ML.describe(p.moves[:1], ML.FAKE, es, cd.MOVES_TAKE)[0])
    copy = ML.choice_of(ML.describe(p.moves[:1], ML.FAKE, es, cd.MOVES_COPY)[0])
    assert take[0] == 12 and copy[0] == 0 and take[1:3] == copy[1:3]
    # no remote destination, no whole-line form
    for mode in (cd.MOVES_TAKE, cd.MOVES_ADD_TAKE):
        with pytest.raises(cd.CudecompError) as e:
            ML.describe(p.moves[:2], ML.FAKE, es, mode, dtype, 0, [1 << 44, 1 << 45])
        assert e.value.code == INTERNAL_ERROR
        with pytest.raises(cd.CudecompError) as e:
            ML.describe([cd.make_move((64, 5, 3), (1, 70, 420), (1, 66, 462), 0, 0, 0, 1, 66)], ML.FAKE, es, mode, dtype)
        assert e.value.code == INTERNAL_ERROR
    # mode 4 checks the data type as mode 1 does; mode 5 does not exist
    for mode, dt in ((cd.MOVES_ADD_TAKE, cd.FLOAT), (5, cd.DOUBLE)):
        with pytest.raises(cd.CudecompError) as e:
            ML.describe(p.moves[:1], ML.FAKE, es, mode, dt)
        assert e.value.code == INVALID_USAGE
    assert (cd.MOVES_TAKE, cd.MOVES_ADD_TAKE) == (3, 4)


# ---- the entry points -------------------------------------------------------------------------------------------------------------
def test_entry_points_validate_like_accumulation():
    """the tuples tests/test_abi.py uses for halo calls (NULL arrays, bad dim, bad data type, h == 0) and a halo wider than the
    interior, several faults at once so that the ORDER of the checks shows: every code is the accumulate entry's"""
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    per = b3(True, True, True)
    tuples = [(h, gd, 1, 1, cd.FLOAT, None, None, 0, None, None),                # halo_extents NULL
              (h, gd, None, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),      # input NULL
              (h, gd, 1, None, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),      # work NULL
              (h, gd, 1, 1, cd.FLOAT, i3(1, 1, 1), None, 3, None, None),         # dim out of range
              (h, gd, 1, 1, cd.FLOAT, i3(1, 1, 1), None, -1, None, None),
              (h, gd, 1, 1, 99, i3(1, 1, 1), None, 0, None, None),               # unknown data type
              (h, None, 1, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),       # no descriptor
              (None, gd, 1, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),      # no handle
              (h, gd, None, None, 99, None, None, 5, None, None),                # several at once: the first check decides
              (h, gd, None, None, cd.FLOAT, i3(1, 1, 1), None, 3, None, None),
              (h, gd, None, None, cd.FLOAT, i3(0, 0, 0), None, 0, None, None),   # all halos zero: success before the pointers are looked at
              (h, gd, 1, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),         # non-periodic single rank: nothing to do
              (h, gd, 1, 1, cd.DOUBLE, i3(1, 0, 1), per, 1, i3(1, 2, 0), None),  # h == 0 along dim: success, no effect
              (h, gd, 8, 8, cd.DOUBLE, i3(10, 0, 0), per, 0, None, None),        # wider than the interior: refused before device work
              (h, gd, 8, 8, cd.DOUBLE, i3(0, 11, 0), per, 1, None, None)]
    expected = {0: INVALID_USAGE, 3: INVALID_USAGE, 5: INVALID_USAGE, 10: cd.RESULT_SUCCESS, 12: cd.RESULT_SUCCESS, 13: INVALID_USAGE}
    for axis, name in enumerate(cd.AMD_ACCUMULATE_CLEAR_SYMBOLS):
        assert name == "cudecompAmdAccumulateAndClearHalos" + "XYZ"[axis]
        fn, acc = getattr(L, name), getattr(L, "cudecompAmdAccumulateHalos" + "XYZ"[axis])
        for i, args in enumerate(tuples):
            want = acc(*args)
            assert fn(*args) == want, (name, i, want)
            if i in expected:
                assert want == expected[i], (name, i, want)
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def test_with_cells_to_clear_the_result_is_accumulations_with_or_without_a_device():
    import torch
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    halo = (1, 2, 1)
    for axis, name in enumerate(cd.AMD_ACCUMULATE_CLEAR_SYMBOLS):
        fn, acc = getattr(L, name), getattr(L, "cudecompAmdAccumulateHalos" + "XYZ"[axis])
        if torch.cuda.is_available():
            data = torch.zeros(int(cd.cudecompGetPencilInfo(h, gd, axis, halo).size), dtype=torch.float32, device="cuda")
            work = torch.zeros(max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1), dtype=torch.float32, device="cuda")
            inp, wk, expected = data.data_ptr(), work.data_ptr(), cd.RESULT_SUCCESS
        else:
            inp, wk, expected = 1, 1, cd.RESULT_CUDA_ERROR
        for dim in range(3):
            want = acc(h, gd, inp, wk, cd.FLOAT, i3(*halo), b3(True, True, True), dim, None, None)
            assert want == expected, (name, dim, want)
            assert fn(h, gd, inp, wk, cd.FLOAT, i3(*halo), b3(True, True, True), dim, None, None) == want, (name, dim)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(cudecomp\w+)\s*\(", src))


def test_headers_declare_and_library_exports_the_symbols():
    names = {"cudecompAmdAccumulateAndClearHalos" + a for a in "XYZ"}
    assert _declared("cudecomp_amd_accumulate_clear.h") == set(cd.AMD_ACCUMULATE_CLEAR_SYMBOLS) == names
    fill = open(os.path.join(ROOT, "include", "cudecomp_amd_fill.h")).read()
    assert '#include "cudecomp_amd_accumulate_clear.h"' in fill  # a solver that includes the fill header gets the fused call
    assert "is accumulate-and-clear." not in fill and "Sequences over dims." in fill and "Addend order." in fill
    L = cd.lib()
    for name in sorted(names) + ["cudecompExtPlanHaloAccumulateClear"]:
        assert hasattr(L, name), name
    assert "cudecompExtPlanHaloAccumulateClear" in _declared("cudecomp_ext.h")
    assert callable(cd.cudecompAccumulateAndClearHalos)


def test_arguments_are_checked_in_the_stated_order(capfd):
    from tests import halo_check_order
    halo_check_order.check("accumulate_clear", capfd)
