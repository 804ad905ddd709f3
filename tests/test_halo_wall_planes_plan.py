"""Wall planes (cudecomp_halo_wall_planes.h: cudecompAmdSetWallPlaneHalos{X,Y,Z}) without a GPU: the plan of every rank against
the wall values' plan (the reflection's where the halo is wider than the wall values accept), the plane operand of every move
against the definition worked out independently in numpy from the pencil info, every refusal in its order of precedence -- through
the stateless planner for every rank and through the C ABI --, the plan cache, which does not see the plane pointers, and the
launches the kernel layer would make for lists of wall-plane moves."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402
from tests import accumulate_bodies as AB  # noqa: E402
from tests import move_lists as ML  # noqa: E402
from tests import wall_planes_bodies as WPB  # noqa: E402

GDIMS = (10, 9, 11)
MEM_ORDER = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
PERMS = list(itertools.permutations((0, 1, 2)))
PENCIL, LOW, HIGH = 0x10000000, 0x20000000, 0x30000000  # fabricated addresses, far apart
K_ROWS_WALL_PLANE, K_GENERIC_WALL_PLANE = 41, 42


def _move_tuple(m):
    return (m.src_buf, m.dst_buf, m.src_off, m.dst_off, tuple(m.extent), tuple(m.ss), tuple(m.ds), m.peer, m.row_pitch)


def _plan(grid, rank, axis, halo, periods, dim, parity, centering, sides, padding=None, dtype=cd.DOUBLE, pencil=PENCIL, low=LOW, high=HIGH):
    return cd.cudecompExtPlanHaloWallPlanes(grid, rank, axis, halo, periods, dim, dtype, parity, centering, sides, pencil, low, high, padding)


# ---- which cells, and which plane entries ------------------------------------------------------------------------------------
def _check_operands(grid, rank, axis, halo, padding, dim, p, ops):
    """for every destination cell of every move: the plane operand addresses the element the definition names -- layer k counted
    from the wall outward along `dim`, the pencil's own indices along the other two dims, in the dense layout of the pencil's shape
    with the extent along `dim` replaced by h -- and never an entry at a padding position"""
    info = cd.cudecompExtPencilInfo(grid, rank, axis, halo, padding)
    shape, order = [int(x) for x in info.shape], [int(x) for x in info.order]
    pad = [int(padding[o]) if padding else 0 for o in order]  # by memory position
    a, h = order.index(dim), int(halo[dim])
    n = shape[a] - pad[a]
    plane_shape, elements = cd.wall_plane_shape(info, dim, halo)
    assert list(plane_shape) == [h if k == a else shape[k] for k in range(3)] and elements == int(info.size) // shape[a] * h
    for i in range(p.n_pre):
        m, o = p.pre[i], ops[i]
        side = m.peer
        assert o.plane == side + 1
        dst = ML.cells(m.extent, m.ds, m.dst_off)
        got = ML.cells(m.extent, o.ps, o.off)
        idx = [dst % shape[0], dst // shape[0] % shape[1], dst // (shape[0] * shape[1])]
        layer = (h - 1 - idx[a]) if side == 0 else (idx[a] - (n - h))
        assert layer.min() == 0 and layer.max() == h - 1
        for k in range(3):
            if k != a:
                assert idx[k].max() < shape[k] - pad[k], "a plane entry at a padding position"
        idx[a] = layer
        want = idx[0] + plane_shape[0] * (idx[1] + plane_shape[1] * idx[2])
        assert np.array_equal(got, want), (rank, axis, dim, side)
        assert got.min() >= 0 and got.max() < elements and np.unique(got).size == got.size
        # signed strides: negative along the mirrored dim of the low side, and only there
        assert [s < 0 for s in o.ps] == [side == 0 and d == dim for d in range(3)]
    for i in range(p.n_pre, 2):
        assert ops[i].plane == 0


GRIDS = ((1, 1), (2, 2))
HALO_SETS = (((1, 1, 1), None), ((2, 1, 3), (1, 2, 0)), ((3, 3, 3), (0, 0, 0)))


@pytest.mark.parametrize("pdims", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_the_moves_are_the_wall_values_and_the_operands_follow_the_definition(pdims):
    """every rank, axis, dim, `sides` and centering of a 1 x 1 and a ragged 2 x 2 grid; the halo sets of the wall values' plan test,
    padding (1, 2, 0) among them; the 1 x 1 grid in all six memory orders"""
    seen = {0: 0, 1: 0, 2: 0}
    for order in (PERMS if pdims == (1, 1) else [None]):
        grid = cd.make_grid_spec(GDIMS, pdims, (order,) * 3 if order else MEM_ORDER)
        for rank, axis, dim, (halo, padding) in itertools.product(range(pdims[0] * pdims[1]), range(3), range(3), HALO_SETS):
            for centering, parity, sides in itertools.product((0, 1), (1, -1), (1, 2, 3)):
                v = [0.0] * 8
                ref, _ = cd.cudecompExtPlanHaloWallValues(grid, rank, axis, halo, (0, 0, 0), dim, cd.DOUBLE, parity, centering, sides,
                                                          v if sides & 1 else None, v if sides & 2 else None, padding)
                p, ops = _plan(grid, rank, axis, halo, (0, 0, 0), dim, parity, centering, sides, padding, low=LOW if sides & 1 else 0,
                               high=HIGH if sides & 2 else 0)
                assert [_move_tuple(p.pre[i]) for i in range(p.n_pre)] == [_move_tuple(ref.pre[i]) for i in range(ref.n_pre)]
                assert (p.kind, p.n_pre, p.n_post, p.face_elements) == (ref.kind, ref.n_pre, 0, ref.face_elements)
                assert list(p.neighbor) == list(ref.neighbor)
                assert p.reserved == (1 << 18) | ((1 << 13) if parity == -1 else 0) | (sides << 16)
                _check_operands(grid, rank, axis, halo, padding, dim, p, ops)
                seen[p.n_pre] += 1
    assert seen[1] and seen[2] and (seen[0] or pdims == (1, 1))


@pytest.mark.parametrize("order", PERMS, ids=["".join(map(str, o)) for o in PERMS])
def test_a_halo_of_nine_layers(order):
    """h = 9 along the 13-cell dim, beyond what the wall values accept: the moves are the reflection's for the sides kept"""
    grid = cd.make_grid_spec((13, 10, 11), (1, 1), (order,) * 3)
    for axis, (halo, padding), centering, sides in itertools.product(range(3), (((9, 1, 1), None), ((9, 0, 2), (1, 2, 0))), (0, 1), (1, 2, 3)):
        ref = cd.cudecompExtPlanHaloReflect(grid, 0, axis, halo, (0, 0, 0), 0, padding, centering, True)
        p, ops = _plan(grid, 0, axis, halo, (0, 0, 0), 0, -1, centering, sides, padding)
        assert ref.n_pre == 2 and [_move_tuple(p.pre[i]) for i in range(p.n_pre)] == [
            _move_tuple(ref.pre[i]) for i in range(2) if sides & (1 << i)]
        _check_operands(grid, 0, axis, halo, padding, 0, p, ops)
        with pytest.raises(cd.CudecompError):
            cd.cudecompExtPlanHaloWallValues(grid, 0, axis, halo, (0, 0, 0), 0, cd.DOUBLE, -1, centering, sides, [0.0] * 9, [0.0] * 9, padding)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _plan_rc(*args, **kwargs):
    try:
        _plan(*args, **kwargs)
    except cd.CudecompError as e:
        return e.code
    return cd.RESULT_SUCCESS


def _message(capfd):
    err = capfd.readouterr().err
    found = re.findall(r"CUDECOMP:ERROR: .*\((.*)\)", err)
    return found[-1] if found else err


SIDES, PLANE_NULL, OVERLAP = ("sides argument must be 1, 2 or 3: the low halo, the high halo or both",
                              "the plane of a side named in sides cannot be null", "a plane named in sides cannot overlap the pencil")
PARITY, CENTERING = "parity argument must be +1 or -1", "centering argument must be 0 or 1"


def test_refusals_on_every_rank(capfd):
    """the stateless planner makes the call's checks in the call's order, on every rank of a 2 x 3 grid -- edge or interior,
    periodic dim or not: all ranks agree.  The overlap check compares fabricated addresses."""
    grid = cd.make_grid_spec(GDIMS, (2, 3), MEM_ORDER)
    capfd.readouterr()
    interior = 0
    for rank, axis, dim, periods in itertools.product(range(6), range(3), range(3), ((0, 0, 0), (1, 1, 1))):
        halo = (1, 2, 1)
        args = (grid, rank, axis, halo, periods, dim)
        ok, _ = _plan(*args, 1, 0, 3)
        interior += ok.kind == 0 and not periods[dim]
        for sides in (0, 4, -1):
            assert _plan_rc(*args, 1, 0, sides) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
        assert _plan_rc(*args, 1, 0, 3, low=0) == cd.RESULT_INVALID_USAGE and _message(capfd) == PLANE_NULL
        assert _plan_rc(*args, 1, 0, 2, high=0) == cd.RESULT_INVALID_USAGE and _message(capfd) == PLANE_NULL
        assert _plan_rc(*args, 1, 0, 1, high=0) == cd.RESULT_SUCCESS and _plan_rc(*args, -1, 1, 2, low=0) == cd.RESULT_SUCCESS
        # the order: parity, centering, sides, NULL, overlap -- a tuple that breaks several at once gets the earliest message
        assert _plan_rc(*args, 0, 2, 0, low=0, high=PENCIL) == cd.RESULT_INVALID_USAGE and _message(capfd) == PARITY
        assert _plan_rc(*args, 1, 2, 0, low=0, high=PENCIL) == cd.RESULT_INVALID_USAGE and _message(capfd) == CENTERING
        assert _plan_rc(*args, 1, 1, 0, low=0, high=PENCIL) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
        assert _plan_rc(*args, 1, 1, 3, low=0, high=PENCIL) == cd.RESULT_INVALID_USAGE and _message(capfd) == PLANE_NULL
        # overlap: on every rank of a non-periodic dim with a halo, whether or not it owns an edge; a periodic dim checks NULL only
        info = cd.cudecompExtPencilInfo(grid, rank, axis, halo, None)
        a = [int(x) for x in info.order].index(dim)
        pencil_bytes = int(info.size) * 8
        plane_bytes = int(info.size) // int(info.shape[a]) * halo[dim] * 8
        want = cd.RESULT_SUCCESS if periods[dim] else cd.RESULT_INVALID_USAGE
        for kw in (dict(high=PENCIL), dict(low=PENCIL + pencil_bytes - 1), dict(high=PENCIL - plane_bytes + 1), dict(low=PENCIL + 8, high=PENCIL + 16)):
            assert _plan_rc(*args, -1, 0, 3, **kw) == want, (rank, axis, dim, periods, kw)
            assert periods[dim] or _message(capfd) == OVERLAP
        # ... a plane that ends where the pencil begins, or begins where it ends, does not overlap; nor does one `sides` leaves out
        assert _plan_rc(*args, -1, 0, 3, low=PENCIL - plane_bytes, high=PENCIL + pencil_bytes) == cd.RESULT_SUCCESS
        assert _plan_rc(*args, -1, 0, 1, high=PENCIL) == cd.RESULT_SUCCESS and _plan_rc(*args, -1, 0, 2, low=PENCIL) == cd.RESULT_SUCCESS
        # the two sides may name the same array
        assert _plan_rc(*args, -1, 0, 3, low=LOW, high=LOW) == cd.RESULT_SUCCESS
        # h == 0 along the dim: NULL only
        h0 = tuple(0 if d == dim else 1 for d in range(3))
        assert _plan_rc(grid, rank, axis, h0, periods, dim, 1, 0, 3, high=PENCIL) == cd.RESULT_SUCCESS
        assert _plan_rc(grid, rank, axis, h0, periods, dim, 1, 0, 3, high=0) == cd.RESULT_INVALID_USAGE and _message(capfd) == PLANE_NULL
    assert interior > 0
    # no width limit: 9 layers where the wall values stop at 8
    grid = cd.make_grid_spec((64, 40, 40), (2, 1), MEM_ORDER)
    for rank, axis, periods in itertools.product(range(2), range(3), ((0, 0, 0), (1, 1, 1))):
        halo9 = [0, 0, 0]
        halo9[axis] = 9
        assert _plan_rc(grid, rank, axis, halo9, periods, axis, 1, 0, 3, dtype=cd.HALF) == cd.RESULT_SUCCESS
        assert _plan_rc(grid, rank, axis, halo9, periods, axis, 1, 0, 5, low=0, dtype=cd.HALF) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
    # the reflection's last refusal, h + centering > n - 2 h, only for a side that would be written (the wall values' test has the grid)
    grid = cd.make_grid_spec((64, 16, 40), (2, 1), MEM_ORDER)
    halo = (0, 8, 0)
    answers = set()
    for rank, centering in itertools.product(range(2), (0, 1)):
        codes = {sides: _plan_rc(grid, rank, 0, halo, (0, 0, 0), 1, 1, centering, sides) for sides in (1, 2, 3)}
        capfd.readouterr()
        try:
            cd.cudecompExtPlanHaloReflect(grid, rank, 0, halo, (0, 0, 0), 1, None, centering, False)
            reflect = cd.RESULT_SUCCESS
        except cd.CudecompError as e:
            reflect = e.code
        message = _message(capfd)
        own = 1 if rank == 0 else 2
        assert codes[own] == codes[3] == reflect and codes[3 - own] == cd.RESULT_SUCCESS, (rank, centering, codes, reflect)
        if reflect != cd.RESULT_SUCCESS:  # ... and it comes LAST: an overlapping plane is reported first
            assert _plan_rc(grid, rank, 0, halo, (0, 0, 0), 1, 1, centering, 3, high=PENCIL) == cd.RESULT_INVALID_USAGE and _message(capfd) == OVERLAP
            assert _plan_rc(grid, rank, 0, halo, (0, 0, 0), 1, 1, centering, 3) == reflect and _message(capfd) == message
        answers.add(reflect)
    assert answers == {cd.RESULT_SUCCESS, cd.RESULT_INVALID_USAGE}


@pytest.fixture(scope="module")
def descriptor():
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((40, 6, 12), (1, 1)))
    yield h, gd
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def _call(h, gd, axis, ptr, parity, centering, sides, low, high, halo=(1, 1, 1), dim=0, periods=(False, False, False), dtype=cd.DOUBLE):
    fn = getattr(cd.lib(), cd.AMD_WALL_PLANES_SYMBOLS[axis])
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    return fn(h, gd, ptr, dtype, parity, centering, sides, low, high, hh, (C.c_bool * 3)(*periods), dim, None, None)


def _reflect(h, gd, axis, ptr, parity, centering, halo=(1, 1, 1), dim=0, periods=(False, False, False), dtype=cd.DOUBLE):
    fn = getattr(cd.lib(), "cudecompAmdReflectHalos" + "XYZ"[axis])
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    return fn(h, gd, ptr, dtype, parity, centering, hh, (C.c_bool * 3)(*periods), dim, None, None)


def test_refusals_through_the_c_abi(descriptor, capfd):
    """all found on the host, before anything is launched (the pointers are not device memory): what the reflection refuses first, in
    its order and with its words, then sides, NULL planes, the overlap.  Tuples with cells to write are shown on the stateless planner
    above: through the C ABI they would go on to the device."""
    h, gd = descriptor
    fake, lo, hi = PENCIL, LOW, HIGH
    capfd.readouterr()
    for axis in range(3):
        # what the reflection refuses, refused the same way whatever the new arguments are
        for kwargs in (dict(halo=None), dict(dim=7), dict(dim=-1), dict(halo=(1, 60, 1), dim=1, periods=(True, True, True)), dict(dtype=17)):
            for ptr in (None, fake):
                rc = _reflect(h, gd, axis, ptr, 5, 5, **kwargs)
                message = _message(capfd)
                assert rc != cd.RESULT_SUCCESS
                assert _call(h, gd, axis, ptr, 5, 5, 0, None, ptr, **kwargs) == rc and _message(capfd) == message, (axis, kwargs)
        assert _call(h, gd, axis, None, 1, 0, 3, lo, hi) == cd.RESULT_INVALID_USAGE and _message(capfd) == "input argument cannot be null"
        for periods, halo in (((False,) * 3, (1, 1, 1)), ((True,) * 3, (1, 1, 1)), ((False,) * 3, (0, 1, 1)), ((False,) * 3, (0, 0, 0))):
            kw = dict(halo=halo, periods=periods)
            assert _call(h, gd, axis, fake, 0, 2, 0, None, fake, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == PARITY
            assert _call(h, gd, axis, fake, -1, 2, 0, None, fake, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == CENTERING
            for sides in (0, 4, -3):
                assert _call(h, gd, axis, fake, -1, 1, sides, None, fake, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
            assert _call(h, gd, axis, fake, -1, 1, 3, fake, None, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == PLANE_NULL
            assert _call(h, gd, axis, fake, 1, 0, 1, None, hi, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == PLANE_NULL
        # the overlap, where the dim has ghost cells a wall could own: the plane on the pencil, and one byte into either end
        info = cd.cudecompGetPencilInfo(h, gd, axis, (1, 1, 1))
        pencil_bytes = int(info.size) * 8
        plane_bytes = int(info.size) // int(info.shape[[int(x) for x in info.order].index(0)]) * 8
        for low, high in ((fake, hi), (lo, fake + pencil_bytes - 1), (fake - plane_bytes + 1, hi)):
            assert _call(h, gd, axis, fake, -1, 1, 3, low, high) == cd.RESULT_INVALID_USAGE and _message(capfd) == OVERLAP
        # nothing to write (periodic dim, no halo along the dim, no halo at all): the call succeeds, also with the other plane NULL --
        # and the planes are checked for NULL only: one that lies on the pencil passes
        for kw in (dict(periods=(True,) * 3), dict(halo=(0, 1, 1)), dict(halo=(0, 0, 0))):
            assert _call(h, gd, axis, fake, 1, 0, 1, lo, None, **kw) == cd.RESULT_SUCCESS
            assert _call(h, gd, axis, fake, -1, 1, 2, None, hi, **kw) == cd.RESULT_SUCCESS
            assert _call(h, gd, axis, fake, -1, 1, 3, fake, fake, **kw) == cd.RESULT_SUCCESS
        # no width limit: 9 layers on a periodic dim succeed
        assert _call(h, gd, axis, fake, 1, 0, 3, lo, hi, halo=(9, 1, 1), periods=(True,) * 3) == cd.RESULT_SUCCESS
        assert _call(h, gd, axis, fake, 1, 0, 3, None, hi, halo=(9, 1, 1)) == cd.RESULT_INVALID_USAGE and _message(capfd) == PLANE_NULL
        # the mirror that reaches beyond the interior comes last: dim 1 has 6 cells, h = 6 with centering 1 leaves the sources no room
        assert _reflect(h, gd, axis, fake, 1, 1, halo=(1, 6, 1), dim=1) == cd.RESULT_INVALID_USAGE
        message = _message(capfd)
        assert _call(h, gd, axis, fake, 1, 1, 3, lo, hi, halo=(1, 6, 1), dim=1) == cd.RESULT_INVALID_USAGE and _message(capfd) == message
        assert _call(h, gd, axis, fake, 1, 1, 0, lo, hi, halo=(1, 6, 1), dim=1) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
        assert _call(h, gd, axis, fake, 1, 1, 3, lo, fake, halo=(1, 6, 1), dim=1) == cd.RESULT_INVALID_USAGE and _message(capfd) == OVERLAP


def test_calls_that_differ_only_in_plane_pointers_share_one_plan(descriptor):
    """on a periodic dim the call has nothing to launch, and its plan is cached all the same: other plane pointers add none, other
    sides, another parity and another centering add one each"""
    h, gd = descriptor
    L = cd.lib()

    def plans():
        n = C.c_int64(-1)
        assert L.cudecompExtHaloPlanCount(h, gd, C.byref(n)) == cd.RESULT_SUCCESS
        return n.value

    per, fake = (True, True, True), PENCIL
    before = plans()
    assert _call(h, gd, 0, fake, -1, 0, 3, LOW, HIGH, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 1
    assert _call(h, gd, 0, fake, -1, 0, 3, HIGH + 64, LOW + 8, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert _call(h, gd, 0, fake, -1, 0, 3, LOW, LOW, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 1
    assert _call(h, gd, 0, fake, -1, 0, 1, LOW, None, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 2
    assert _call(h, gd, 0, fake, 1, 0, 3, LOW, HIGH, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert _call(h, gd, 0, fake, 1, 1, 3, LOW, HIGH, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 4
    # ... and the wall values with the same arguments have a plan of their own
    v = (C.c_double * 2)(0.0, 0.0)
    fn = getattr(L, cd.AMD_WALL_VALUES_SYMBOLS[0])
    assert fn(h, gd, fake, cd.DOUBLE, -1, 0, 3, v, v, (C.c_int32 * 3)(2, 1, 1), (C.c_bool * 3)(*per), 0, None, None) == cd.RESULT_SUCCESS
    assert plans() == before + 5


# ---- launch descriptions -----------------------------------------------------------------------------------------------------
_plane_move = WPB.plane_move


def _describe(pairs, es, dtype, addresses=ML.FAKE, negate=False, flags=0):
    return cd.cudecompExtDescribeMoves([m for m, _ in pairs], addresses, es, cd.MOVES_WALL_PLANE_NEGATE if negate else cd.MOVES_WALL_PLANE,
                                       dtype, flags, planes=[o for _, o in pairs])


def test_eight_siblings_share_one_interleaved_launch():
    targets = [1, 300, 2, 99, 5, 150, 17, 40]
    pairs, at = [], 0
    for i, t in enumerate(targets):  # rows of 32 fp64: 16 lanes per row, 64 rows per workgroup
        extent, mirrored = ((32, 64 * (t // 3), 3), 2) if t % 3 == 0 else ((32, 8 if t % 8 == 0 else 2, t), 1)
        ss = (1, 34, 34 * extent[1] + 2)
        span = ML.span(extent, ss)
        pairs.append(_plane_move(extent, ss, mirrored, at, at + span + 6, i & 1, poff=at))
        at += 2 * span + 16
    (l,) = _describe(pairs, 8, cd.DOUBLE)
    assert (l["kind"], l["cls"], l["n"], l["interleave"], l["vec"]) == (K_ROWS_WALL_PLANE, 0, 8, 1, 16), l
    assert l["blocks"] == 8 * 300 and l["index"] == list(range(8)), l
    assert [b - a for a, b in zip(l["first_block"], l["first_block"][1:])] == targets, l
    # a ninth sibling opens a second launch; a forced element-wise run is one launch of the other kind
    two = _describe(pairs + [_plane_move((32, 2, 7), (1, 34, 70), 1, at, at + 600, 0, poff=at)], 8, cd.DOUBLE)
    assert [(l["kind"], l["n"]) for l in two] == [(K_ROWS_WALL_PLANE, 8), (K_ROWS_WALL_PLANE, 1)]
    (l,) = _describe(pairs, 8, cd.DOUBLE, negate=True, flags=1)
    assert (l["kind"], l["cls"], l["n"], l["interleave"], l["vec"]) == (K_GENERIC_WALL_PLANE, 2, 8, 1, 8), l


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_the_lane_width_follows_all_three_operands(dtype):
    """pencil cells 16-byte aligned with 16-byte rows and pitches: 16-byte lanes -- until only the PLANE breaks the alignment: its
    base one element further, or (2-byte types) its row pitch at 2 mod 4; then the widest lane that still divides everything"""
    es = AB.element_bytes(dtype)
    per16 = 16 // es
    extent, ss = (4 * per16, 5, 3), (1, 6 * per16, 40 * per16)
    span = ML.span(extent, ss)

    def vec(poff=0, ps=None, soff=0, doff=None, mirrored=1, side=1):
        doff = span + 4 * per16 if doff is None else doff
        (l,) = _describe([_plane_move(extent, ss, mirrored, soff, doff, side, ps, poff)], es, dtype)
        assert l["kind"] == K_ROWS_WALL_PLANE, l
        return l["vec"]

    def widest(*byte_counts):
        vb = 16
        while vb > es and any(b % vb for b in byte_counts):
            vb //= 2
        return vb

    for mirrored, side in itertools.product((1, 2), (0, 1)):
        assert vec(mirrored=mirrored, side=side) == 16
        assert vec(poff=1, mirrored=mirrored, side=side) == widest(es)                # the plane's base at + es
        assert vec(poff=2, mirrored=mirrored, side=side) == widest(2 * es)
        assert vec(ps=(1, ss[1] + 1, ss[2]), mirrored=mirrored, side=side) == widest((ss[1] + 1) * es)  # the plane's row pitch
        assert vec(ps=(1, ss[1], ss[2] + 1), mirrored=mirrored, side=side) == widest((ss[2] + 1) * es)  # the plane's plane pitch
        assert vec(ps=(1, ss[1] + per16, ss[2] + 3 * per16), mirrored=mirrored, side=side) == 16     # another pitch, still aligned
        # ... as the pencil's own base does
        assert vec(soff=1, mirrored=mirrored, side=side) == widest(es) and vec(doff=span + 4 * per16 + 1, mirrored=mirrored, side=side) == widest(es)
    if es == 2:  # the 2-byte rule at 2 mod 4 applies to the plane as well
        assert vec(poff=1) == 2 and vec(ps=(1, ss[1] + 1, ss[2])) == 2 and vec(poff=2) == 4
    # rows merge into longer ones only if they are contiguous in source, destination AND plane
    dense = (1, extent[0], extent[0] * extent[1] + 8)
    m, o = _plane_move(extent, dense, 2, 0, 3 * dense[2], 1)
    (l,) = cd.cudecompExtDescribeMoves([m], ML.FAKE, es, cd.MOVES_WALL_PLANE, dtype, planes=[o])
    assert l["first_block"][1] == 1  # 5 rows of 64 bytes fused into one of 320: 20 lanes, one workgroup covers the three planes' rows
    fused_blocks = l["blocks"]
    m, o = _plane_move(extent, dense, 2, 0, 3 * dense[2], 1, ps=(1, extent[0] + per16, dense[2] + 5 * per16))
    (l,) = cd.cudecompExtDescribeMoves([m], ML.FAKE, es, cd.MOVES_WALL_PLANE, dtype, planes=[o])
    assert (l["kind"], l["vec"]) == (K_ROWS_WALL_PLANE, 16) and l["blocks"] == 3 and fused_blocks == 1


def test_moves_the_kernels_do_not_serve_are_refused_before_any_launch(capfd):
    """a wall-plane move without a mirrored dim, outside buffer 0 or without a plane named in `peer` is INVALID_USAGE (found when the
    list is read); a remote destination is refused by the classifier as the other local families refuse it, INTERNAL_ERROR"""
    m, o = _plane_move((8, 2, 2), (1, 8, 16), 1, 0, 64, 1)
    plain = cd.make_move((8, 2, 2), (1, 8, 16), (1, 8, 16), 0, 64, 0, 0)
    plain.peer = 1
    elsewhere = cd.make_move((8, 2, 2), (1, -8, 16), (1, 8, 16), 8, 64, 0, 1)
    elsewhere.peer = 1
    unnamed = cd.make_move((8, 2, 2), (1, -8, 16), (1, 8, 16), 8, 64, 0, 0)  # (make_move leaves peer at -1)
    for moves, kw, code in (([plain], {}, cd.RESULT_INVALID_USAGE), ([elsewhere], {}, cd.RESULT_INVALID_USAGE),
                            ([unnamed], {}, cd.RESULT_INVALID_USAGE), ([m], dict(dst_base_addresses=[1 << 44]), cd.RESULT_INTERNAL_ERROR)):
        with pytest.raises(cd.CudecompError) as e:
            cd.cudecompExtDescribeMoves(moves, ML.FAKE, 8, cd.MOVES_WALL_PLANE, cd.DOUBLE, planes=[o], **kw)
        assert e.value.code == code, (e.value.code, code)
    (l,) = cd.cudecompExtDescribeMoves([m], ML.FAKE, 8, cd.MOVES_WALL_PLANE, cd.DOUBLE, planes=[o])  # (the move itself is served)
    assert l["kind"] == K_ROWS_WALL_PLANE
    capfd.readouterr()
