"""Halo folding (cudecomp_halo_fold.h: cudecompAmdFoldHalos{X,Y,Z}) without a GPU.  The product's planner
(cudecompExtPlanHaloFold, the buildHaloFoldPlan the executor runs) is asked for the plan of EVERY rank, axis and dim of a
deterministic sweep of decompositions:
  * the source cells of fold(dim) are the destination cells of reflect(dim) with the same arguments and the other way round, with
    the same pairing k of ghost and interior cell: the fold is the transpose of the reflection;
  * `ordered` is set exactly when both sides are present and n < 4h + 2c, the moves clear their source exactly with `clear`;
  * the plan executed in numpy, one move after the other, is the definition (tests/fold_bodies.py fold_reference), bit for bit
    on whole pencils -- the overlapping sides included.
Refusals and result codes, the kernel choices of fold-moves (cudecompExtDescribeMoves, modes 7 ... 10) and the Python wrapper
follow.  Nothing here has a tolerance."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fold_bodies as FB
from tests import move_lists as ML

PERMS = list(itertools.permutations((0, 1, 2)))
INVALID_USAGE, NOT_SUPPORTED, INTERNAL_ERROR = 1, 2, 3
REFLECT_MARK = 1 << 12
MODES = (cd.MOVES_FOLD, cd.MOVES_FOLD_NEGATE, cd.MOVES_FOLD_TAKE, cd.MOVES_FOLD_NEGATE_TAKE)

# pdims -> ragged gdims whose smallest slab along every dim holds 4 cells: h + centering <= interior for every halo below
GRIDS = {(1, 1): (5, 6, 7), (1, 4): (16, 17, 18), (2, 2): (8, 9, 11), (2, 3): (12, 13, 14)}
HALOS = [(1, 1, 1), (2, 1, 3), (3, 3, 3)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
PERIODS = list(itertools.product((False, True), repeat=3))
DTYPE = cd.HALF_COMPLEX  # the numpy executions add complex-fp16 elements: two reals per element, every sum rounds


def _cells(m, side):
    k = np.indices([int(e) for e in m.extent]).reshape(3, -1)
    off, st = (m.dst_off, m.ds) if side == "dst" else (m.src_off, m.ss)
    return off + k[0] * st[0] + k[1] * st[1] + k[2] * st[2]


def _planned(call):
    try:
        return call(), None
    except cd.CudecompError as e:
        return None, e.code


def check_shape_of_a_fold_plan(plan, negate, clear, size):
    assert plan.kind in (0, 1) and plan.n_post == 0 and 0 <= plan.n_pre <= 2
    if plan.kind == 0:
        assert plan.n_pre == 0
        return
    marks = FB.FOLD_MARK | (FB.NEGATE_MARK if negate else 0) | (FB.CLEAR_MARK if clear else 0)
    takes = sum(1024 << i for i in range(plan.n_pre)) if clear else 0  # "take is set exactly when clear"
    assert plan.reserved & ~FB.ORDERED_MARK == marks | takes, "not marked as a fold plan (or as something else too)"
    assert plan.n_pre >= 1
    for i in range(plan.n_pre):
        m = plan.pre[i]
        assert m.src_buf == 0 and m.dst_buf == 0 and m.row_pitch == 0, "a fold-move stays in the pencil and claims no cells between rows"
        assert sum(1 for s in m.ss if s < 0) == 1 and all(d > 0 for d in m.ds), "exactly the source of one dim runs backwards"
        src, dst = _cells(m, "src"), _cells(m, "dst")
        assert min(src.min(), dst.min()) >= 0 and max(src.max(), dst.max()) < size
        both = np.concatenate([src, dst])
        assert np.unique(both).size == both.size, "a fold-move reads what it writes, or visits a cell twice"
    if plan.n_pre == 2:
        assert plan.pre[0].src_off < plan.pre[1].src_off and plan.pre[0].dst_off <= plan.pre[1].dst_off, "the low side comes first"
        sources = np.concatenate([_cells(plan.pre[i], "src") for i in range(2)])
        assert np.unique(sources).size == sources.size
        assert np.intersect1d(sources, np.concatenate([_cells(plan.pre[i], "dst") for i in range(2)])).size == 0


def execute(plan, bits):
    """the moves of a fold plan in numpy, one after the other, in place on `bits` ((cells, nc) bit patterns)"""
    for i in range(plan.n_pre):
        m = plan.pre[i]
        src, dst = _cells(m, "src"), _cells(m, "dst")
        bits[dst] = FB.fold_add(DTYPE, bits[dst], bits[src], bool(plan.reserved & FB.NEGATE_MARK))
        if plan.reserved & (1024 << i):
            bits[src] = 0


@pytest.mark.parametrize("pdims", list(GRIDS), ids=["%dx%d" % p for p in GRIDS])
def test_fold_is_the_transpose_of_the_reflection_and_runs_as_defined(pdims):
    """every rank, axis, dim and memory order; halos, padding, all eight period mixes, both centerings; parity and clear alternate
    with the case number (they change no cell set, and the numpy execution sees all four combinations)"""
    gdims, n, ordered_seen = GRIDS[pdims], 0, 0
    for order in PERMS:
        spec = cd.make_grid_spec(gdims, pdims, (order,) * 3)
        for rank, axis, halo, padding in itertools.product(range(pdims[0] * pdims[1]), range(3), HALOS, PADDINGS):
            p = cd.cudecompExtPencilInfo(spec, rank, axis, halo, padding)
            size = int(p.size)
            start = FB.finite_bits(DTYPE, size, rank)
            for dim in range(3):
                extent = int(p.shape[[int(x) for x in p.order].index(dim)]) - int(padding[dim])  # n of the contract
                for periods, centering in itertools.product(PERIODS, (0, 1)):
                    negate, clear = bool(n & 1), (n >> 1) & 1
                    n += 1
                    where = (gdims, pdims, order, rank, axis, halo, padding, dim, periods, centering, negate, clear)
                    has = [cd.cudecompExtShiftedRank(spec, rank, axis, dim, side, periods[dim]) >= 0 for side in (-1, 1)]
                    mirror = cd.cudecompExtPlanHaloReflect(spec, rank, axis, halo, periods, dim, padding, centering, negate)
                    plan = cd.cudecompExtPlanHaloFold(spec, rank, axis, halo, periods, dim, padding, centering, negate, clear)
                    check_shape_of_a_fold_plan(plan, negate, clear, size)
                    assert (plan.kind, plan.n_pre, plan.face_elements) == (mirror.kind, mirror.n_pre, mirror.face_elements), where
                    assert [plan.neighbor[0] >= 0, plan.neighbor[1] >= 0] == has and list(plan.neighbor) == list(mirror.neighbor), where
                    for i in range(plan.n_pre):
                        ghost_r, inner_r = _cells(mirror.pre[i], "dst"), _cells(mirror.pre[i], "src")
                        ghost_f, inner_f = _cells(plan.pre[i], "src"), _cells(plan.pre[i], "dst")
                        a, b = np.argsort(ghost_r), np.argsort(ghost_f)
                        assert np.array_equal(ghost_r[a], ghost_f[b]), ("the fold does not read the cells the reflection writes", where)
                        assert np.array_equal(inner_r[a], inner_f[b]), ("... or pairs them with other interior cells", where)
                    h = halo[dim]
                    overlap = plan.n_pre == 2 and extent < 4 * h + 2 * centering
                    assert bool(plan.reserved & FB.ORDERED_MARK) == overlap, ("ordered", where, extent)
                    if plan.n_pre == 2:
                        shared = np.intersect1d(_cells(plan.pre[0], "dst"), _cells(plan.pre[1], "dst")).size
                        assert (shared > 0) == overlap, where
                    ordered_seen += overlap
                    got, want = start.copy(), start.copy()
                    execute(plan, got)
                    FB.fold_reference(p, want, halo, dim, has, -1 if negate else 1, centering, clear, DTYPE)
                    assert np.array_equal(got, want), ("the plan does not compute the definition", where)
                    if plan.n_pre:
                        assert not np.array_equal(got, start), where
    assert n == 6 * pdims[0] * pdims[1] * 3 * len(HALOS) * len(PADDINGS) * 3 * 16
    # a rank alone along the dim whose interior is below 2h + 2c cells: only the single-rank grid (5, 6, 7) has such dims
    assert (ordered_seen > 0) == (pdims == (1, 1))


# ---- refusals and result codes --------------------------------------------------------------------------------------------
def test_planner_refusals_are_the_reflections_plus_clear():
    order = ((0, 1, 2),) * 3
    code = lambda call: _planned(call)[1]
    # h + centering against the interior: refused one above it, served at it -- as the reflection, for either clear
    for gx, h, c in ((9, 3, 0), (9, 3, 1), (4, 3, 1), (3, 3, 1), (3, 3, 0), (2, 3, 0), (2, 1, 1), (1, 1, 1), (1, 1, 0)):
        spec = cd.make_grid_spec((gx, 6, 7), (1, 1), order)
        for per in ((False,) * 3, (True,) * 3):
            want = code(lambda: cd.cudecompExtPlanHaloReflect(spec, 0, 0, (h, 0, 0), per, 0, None, c))
            for clear in (0, 1):
                assert code(lambda: cd.cudecompExtPlanHaloFold(spec, 0, 0, (h, 0, 0), per, 0, None, c, False, clear)) == want, (gx, h, c)
            assert code(lambda: cd.cudecompExtPlanHaloFold(spec, 0, 0, (h, 0, 0), per, 0, None, c, False, 2)) == INVALID_USAGE
    assert code(lambda: cd.cudecompExtPlanHaloFold(cd.make_grid_spec((3, 6, 7), (1, 1), order), 0, 0, (3, 0, 0), None, 0, None, 1)) == INVALID_USAGE
    # ... only on the ranks that fold: 1 x 3 ranks along Z of X pencils, slabs of 2
    three = cd.make_grid_spec((4, 4, 6), (1, 3), order)
    assert cd.cudecompExtPlanHaloFold(three, 1, 0, (0, 0, 2), (False,) * 3, 2, None, 1).kind == 0
    for rank in (0, 2):
        assert code(lambda: cd.cudecompExtPlanHaloFold(three, rank, 0, (0, 0, 2), (False,) * 3, 2, None, 1)) == INVALID_USAGE
        assert cd.cudecompExtPlanHaloFold(three, rank, 0, (0, 0, 2), (False,) * 3, 2, None, 0).n_pre == 1
    one = cd.make_grid_spec((5, 6, 7), (1, 1), order)
    for c in (-1, 2):
        assert code(lambda: cd.cudecompExtPlanHaloFold(one, 0, 0, (1, 1, 1), (False,) * 3, 0, None, c)) == INVALID_USAGE
    for clear in (-1, 2, 3):
        assert code(lambda: cd.cudecompExtPlanHaloFold(one, 0, 0, (1, 1, 1), (False,) * 3, 0, None, 0, False, clear)) == INVALID_USAGE
    # the update's refusals come first, with the update's code -- before `clear` is looked at
    four = cd.make_grid_spec((4, 4, 4), (2, 2), order)
    empty = cd.make_grid_spec((3, 8, 8), (4, 1), order)
    for spec, rank, axis, halo, per, dim in ((four, 0, 0, (0, 3, 0), (True,) * 3, 1), (empty, 0, 1, (1, 1, 1), (True,) * 3, 0)):
        want = code(lambda: cd.cudecompExtPlanHaloReflect(spec, rank, axis, halo, per, dim))
        assert want in (INVALID_USAGE, NOT_SUPPORTED)
        for c, clear in ((0, 0), (1, 1), (7, 2)):
            assert code(lambda: cd.cudecompExtPlanHaloFold(spec, rank, axis, halo, per, dim, None, c, False, clear)) == want
    assert code(lambda: cd.cudecompExtPlanHaloFold(empty, 0, 1, (1, 1, 1), (True,) * 3, 0, None, 0, False, 2)) == NOT_SUPPORTED
    # planner arguments
    for call in (lambda: cd.cudecompExtPlanHaloFold(four, 4, 0, (1, 1, 1), None, 0), lambda: cd.cudecompExtPlanHaloFold(four, 0, 3, (1, 1, 1), None, 0),
                 lambda: cd.cudecompExtPlanHaloFold(four, 0, 0, (1, 1, 1), None, 3), lambda: cd.cudecompExtPlanHaloFold(four, 0, 0, None, None, 0)):
        assert code(call) == INVALID_USAGE
    # no other plan carries the mark, and a fold plan does not carry the reflection's
    for p in (cd.cudecompExtPlanHalo(one, 0, 0, (1, 1, 1), (True,) * 3, 1), cd.cudecompExtPlanHaloFill(one, 0, 0, (1, 1, 1), (True,) * 3, 1),
              cd.cudecompExtPlanHaloAccumulate(one, 0, 0, (1, 1, 1), (True,) * 3, 1), cd.cudecompExtPlanHaloReflect(one, 0, 0, (1, 1, 1), None, 1)):
        assert p.reserved & FB.FOLD_MARK == 0
    assert cd.cudecompExtPlanHaloFold(one, 0, 0, (1, 1, 1), None, 1).reserved & REFLECT_MARK == 0


def test_entry_points_check_their_arguments():
    FB.check_entry_points()


def test_with_and_without_cells_to_fold_on_this_device():
    """a non-periodic single rank has ghost cells to fold on every dim: without a device the call answers
    CUDECOMP_RESULT_CUDA_ERROR (the pointer is never looked at), with one it succeeds on a real buffer; with nothing to fold
    (periodic dims) it succeeds either way"""
    import torch
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    halo = (1, 2, 1)
    for axis, name in enumerate(cd.AMD_FOLD_SYMBOLS):
        fn = getattr(L, name)
        if torch.cuda.is_available():
            data = torch.zeros(int(cd.cudecompGetPencilInfo(h, gd, axis, halo).size), dtype=torch.float32, device="cuda")
            inp, expected = data.data_ptr(), cd.RESULT_SUCCESS
        else:
            inp, expected = 1, cd.RESULT_CUDA_ERROR
        for dim, (parity, centering, clear) in itertools.product(range(3), ((1, 0, 0), (-1, 1, 1))):
            assert fn(h, gd, inp, cd.FLOAT, parity, centering, clear, i3(*halo), b3(False, False, False), dim, None, None) == expected, (name, dim)
            assert fn(h, gd, inp, cd.FLOAT, parity, centering, clear, i3(*halo), b3(True, True, True), dim, None, None) == cd.RESULT_SUCCESS
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def test_python_wrapper_rejects_bad_parity_centering_and_clear():
    for parity, centering, clear in ((0, 0, 0), (2, 0, 0), (1, -1, 0), (1, 2, 1), (1, 0, 2), (-1, 1, -1)):
        with pytest.raises(ValueError):
            cd.cudecompFoldHalos(0, None, None, 1, cd.DOUBLE, parity, centering, clear, (1, 1, 1), None, 0)


# ---- kernel choices (cudecompExtDescribeMoves, modes 7 ... 10) -------------------------------------------------------------
def _fold_move(extent, ss, ds, mirrored, soff=0, doff=0, row_pitch=0):
    """a fold-move inside one buffer: the source block at soff, its `mirrored` dim read backwards, the destination at doff"""
    ss = list(ss)
    soff += (extent[mirrored] - 1) * ss[mirrored]
    ss[mirrored] = -ss[mirrored]
    return cd.make_move(extent, ss, ds, soff, doff, 0, 0, row_pitch)


def _kinds(mode):
    """(rows kind, generic kind) of a fold mode"""
    return (20, 21) if mode in (cd.MOVES_FOLD_TAKE, cd.MOVES_FOLD_NEGATE_TAKE) else (18, 19)


def test_kinds_18_to_21_and_both_sides_in_one_launch():
    """the two moves of a plan -- mirrored dim the middle or the slowest memory axis -- are siblings of one interleaved launch of
    the row kind of their mode, which carries the real type whatever the parity; 32 MiB and more stream their source"""
    spec = cd.make_grid_spec((40, 36, 30), (1, 1), ((0, 1, 2),) * 3)
    arith = {cd.DOUBLE: 4, cd.HALF: 1, cd.FLOAT_COMPLEX: 3, cd.BFLOAT16: 2}
    for dim, halo, dtype, mode in itertools.product((1, 2), ((1, 1, 1), (2, 3, 2)), arith, MODES):
        negate, clear = mode in (cd.MOVES_FOLD_NEGATE, cd.MOVES_FOLD_NEGATE_TAKE), int(mode >= cd.MOVES_FOLD_TAKE)
        plan = cd.cudecompExtPlanHaloFold(spec, 0, 0, halo, (False,) * 3, dim, None, 1, negate, clear)
        assert not plan.reserved & FB.ORDERED_MARK
        moves = [plan.pre[i] for i in range(plan.n_pre)]
        es = AB.element_bytes(dtype)
        (l,) = ML.describe(moves, ML.FAKE, es, mode, dtype)
        assert (l["kind"], l["cls"], l["n"], l["interleave"], l["access"]) == (_kinds(mode)[0], 0, 2, 1, 0), (dim, halo, l)
        assert l["arith"] == arith[dtype] and l["vec"] >= es and l["elements"] == 2 * plan.face_elements
    # the mirrored dim as the fastest memory axis: element-wise, whatever is forced
    for h, dtype, mode in itertools.product((1, 2, 3, 5), (cd.HALF, cd.FLOAT, cd.DOUBLE, cd.DOUBLE_COMPLEX), MODES):
        plan = cd.cudecompExtPlanHaloFold(spec, 0, 0, (h, 1, 1), (False,) * 3, 0, None, 0, False, int(mode >= cd.MOVES_FOLD_TAKE))
        moves = [plan.pre[i] for i in range(plan.n_pre)]
        es = AB.element_bytes(dtype)
        for flags in (0, 2):
            (l,) = ML.describe(moves, ML.FAKE, es, mode, dtype, flags)
            assert (l["kind"], l["cls"], l["n"], l["vec"], l["access"]) == (_kinds(mode)[1], 2, 2, es, 0), (h, es, l)
    big = _fold_move((2048, 1024, 2), (1, 2048, 2048 * 1024 * 2), (1, 2048, 2048 * 1024), 2, soff=0, doff=2048 * 1024 * 8)
    for mode in MODES:
        (l,) = ML.describe([big], ML.FAKE, 8, mode, cd.DOUBLE)
        assert (l["kind"], l["vec"], l["access"]) == (_kinds(mode)[0], 16, 1)
        (l,) = ML.describe([big], ML.FAKE, 4, mode, cd.FLOAT)  # (16 MiB)
        assert (l["kind"], l["vec"], l["access"]) == (_kinds(mode)[0], 16, 0)
        (l,) = ML.describe([big], ML.FAKE, 4, mode, cd.FLOAT, flags=2)
        assert l["access"] == 1
        (l,) = ML.describe([big], ML.FAKE, 4, mode, cd.FLOAT, flags=1)
        assert (l["kind"], l["access"]) == (_kinds(mode)[1], 0)


def test_two_byte_rows_at_two_mod_four_take_two_byte_lanes():
    for soff, doff, pitch, want in ((0, 4000, 64, 16), (1, 4000, 64, 2), (0, 4001, 64, 2), (0, 4000, 65, 2), (2, 4002, 66, 4)):
        m = _fold_move((32 if want != 4 else 30, 5, 3), (1, pitch, pitch * 8), (1, pitch, pitch * 8), 1, soff, doff)
        for mode, dtype in itertools.product(MODES, (cd.HALF, cd.BFLOAT16)):
            (l,) = ML.describe([m], ML.FAKE, 2, mode, dtype)
            assert (l["kind"], l["vec"]) == (_kinds(mode)[0], want), (soff, doff, pitch, l)


@pytest.mark.parametrize("mode", MODES)
def test_lists_never_share_a_launch_with_another_kind_and_split_at_eight(mode):
    """nineteen sibling row moves: launches of 8, 8 and 3; row moves, element-wise moves and rows of another lane width in one
    list: one launch per kernel choice, each of one kind; the same list in another fold mode shares no kind with this one"""
    rows, generic = _kinds(mode)
    moves, at = [], 0
    for i in range(19):
        moves.append(_fold_move((32, 5 + i, 3), (1, 32, 32 * 40), (1, 32, 32 * 40), 1, at, at + 4000))
        at += 8000
    ls = ML.describe(moves, ML.FAKE, 8, mode, cd.DOUBLE)
    assert [(l["kind"], l["n"]) for l in ls] == [(rows, 8), (rows, 8), (rows, 3)]
    assert [l["index"][:l["n"]] for l in ls] == [list(range(8)), list(range(8, 16)), list(range(16, 19))]
    mixed = moves[:3] + [_fold_move((3, 9, 7), (1, 13, 130), (1, 13, 130), 0, at, at + 3)] + \
        [_fold_move((33, 4, 2), (1, 35, 150), (1, 35, 150), 2, at + 2000, at + 3000)] + moves[3:5]
    ls = ML.describe(mixed, ML.FAKE, 8, mode, cd.DOUBLE)
    assert sorted((l["kind"], l["vec"], l["n"]) for l in ls) == sorted([(rows, 16, 5), (generic, 8, 1), (rows, 8, 1)])
    assert sorted(i for l in ls for i in l["index"][:l["n"]]) == list(range(7))
    for other in MODES:
        if _kinds(other) != _kinds(mode):
            assert not {l["kind"] for l in ML.describe(mixed, ML.FAKE, 8, other, cd.DOUBLE)} & {l["kind"] for l in ls}
    # nothing of a fold list is ever a copy, an addition, a take or a reflection
    assert {l["kind"] for l in ls} <= {18, 19, 20, 21}


def test_what_a_fold_move_never_carries():
    m = _fold_move((32, 5, 3), (1, 64, 640), (1, 64, 640), 1, doff=4000)
    code = lambda call: _planned(call)[1]
    with_pitch = _fold_move((32, 5, 3), (1, 64, 640), (1, 64, 640), 1, doff=4000, row_pitch=64)
    plain = cd.make_move((32, 5, 3), (1, 64, 640), (1, 64, 640), 0, 4000, 0, 0)
    two = cd.make_move((32, 5, 3), (1, -64, -640), (1, 64, 640), 2000, 4000, 0, 0)
    for mode in MODES:
        assert ML.describe([m], ML.FAKE, 8, mode, cd.DOUBLE)[0]["kind"] == _kinds(mode)[0]
        assert code(lambda: ML.describe([with_pitch], ML.FAKE, 8, mode, cd.DOUBLE)) == INTERNAL_ERROR
        assert code(lambda: ML.describe([m], ML.FAKE, 8, mode, cd.DOUBLE, base_addresses=[1 << 44])) == INTERNAL_ERROR
        assert code(lambda: ML.describe([two], ML.FAKE, 8, mode, cd.DOUBLE)) == INTERNAL_ERROR  # two mirrored dims
        assert code(lambda: ML.describe([m], ML.FAKE, 8, mode, cd.FLOAT)) == INVALID_USAGE  # the type's size is not es
        assert code(lambda: ML.describe([m], ML.FAKE, 8, mode, 0)) == INVALID_USAGE  # an addition needs a type
        assert code(lambda: ML.describe([plain], ML.FAKE, 8, mode, cd.DOUBLE)) == INVALID_USAGE  # no dim is named
        assert code(lambda: ML.describe([m, plain], ML.FAKE, 8, mode, cd.DOUBLE)) == INVALID_USAGE
        # a mirrored dim one cell thick still names itself
        thin = _fold_move((32, 1, 3), (1, 64, 640), (1, 64, 640), 1, doff=4000)
        assert ML.describe([thin], ML.FAKE, 8, mode, cd.DOUBLE)[0]["kind"] == _kinds(mode)[0]
    assert code(lambda: ML.describe([m], ML.FAKE, 8, 11, cd.DOUBLE)) == INVALID_USAGE  # no such mode
    # every older mode answers for the same geometry as before
    assert ML.describe([plain], ML.FAKE, 8, cd.MOVES_COPY)[0]["kind"] == 0
    assert ML.describe([plain], ML.FAKE, 8, cd.MOVES_ADD, cd.DOUBLE)[0]["kind"] == 8
    assert ML.describe([m], ML.FAKE, 8, cd.MOVES_REFLECT)[0]["kind"] == 16


def test_arguments_are_checked_in_the_stated_order(capfd):
    from tests import halo_check_order
    halo_check_order.check("fold", capfd)
