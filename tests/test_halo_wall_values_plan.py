"""Wall values (cudecomp_halo_wall_values.h: cudecompAmdSetWallHalos{X,Y,Z}) without a GPU: the plan of every rank against the
reflection's plan restricted to `sides`, the addend table against a restatement of the conversion in exact rational arithmetic,
every refusal in its order of precedence -- through the stateless planner for every rank and through the C ABI -- and the plan
cache, which does not see the addends."""
import ctypes as C
import fractions
import itertools
import math
import os
import re
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402
from tests import accumulate_bodies as AB  # noqa: E402

GDIMS = (10, 9, 11)
GRIDS = ((1, 1), (2, 2), (2, 3))
MEM_ORDER = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
FORMAT = {"fp16": (5, 10), "bf16": (8, 7)}  # (exponent bits, stored significand bits)


def _spec(pdims):
    return cd.make_grid_spec(GDIMS, pdims, MEM_ORDER)


def _move_tuple(m):
    return (m.src_buf, m.dst_buf, m.src_off, m.dst_off, tuple(m.extent), tuple(m.ss), tuple(m.ds), m.peer, m.row_pitch)


# ---- which cells -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdims", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_the_moves_are_the_reflections_for_the_sides_kept(pdims):
    """every rank, axis, dim, centering, parity and sides: the moves are those of cudecompExtPlanHaloReflect whose side is named,
    field by field (so: the same cells, the same mirror), each naming its side; the plan says `local` exactly when a move is left"""
    grid = _spec(pdims)
    seen_nothing, seen_one, seen_two, seen_interior = 0, 0, 0, 0
    for rank, axis, dim, periods in itertools.product(range(pdims[0] * pdims[1]), range(3), range(3), ((0, 0, 0), (0, 1, 0))):
        halo = (1, 1, 1)
        for centering, parity in itertools.product((0, 1), (1, -1)):
            ref = cd.cudecompExtPlanHaloReflect(grid, rank, axis, halo, periods, dim, None, centering, parity == -1)
            assert all(ref.pre[i].peer in (0, 1) for i in range(ref.n_pre))
            for sides in (1, 2, 3):
                low, high = [0.5] * halo[dim], [1.5] * halo[dim]
                p, table = cd.cudecompExtPlanHaloWallValues(grid, rank, axis, halo, periods, dim, cd.DOUBLE, parity, centering, sides,
                                                            low if sides & 1 else None, high if sides & 2 else None)
                kept = [_move_tuple(ref.pre[i]) for i in range(ref.n_pre) if sides & (1 << ref.pre[i].peer)]
                assert [_move_tuple(p.pre[i]) for i in range(p.n_pre)] == kept, (rank, axis, dim, periods, centering, parity, sides)
                assert p.kind == (1 if kept else 0) and p.n_post == 0
                assert list(p.neighbor) == list(ref.neighbor) and p.face_elements == (ref.face_elements if kept else 0)
                assert p.reserved == (1 << 15) | ((1 << 13) if parity == -1 else 0) | (sides << 16)
                for side in (0, 1):  # the table holds the addends of the sides named, whether or not this rank writes them
                    want = np.zeros((cd.MAX_WALL_HALO, 16), dtype=np.uint8)
                    if sides & (1 << side):
                        want[:halo[dim]] = np.frombuffer(struct.pack("<d", (0.5, 1.5)[side]) * 2, dtype=np.uint8)
                    assert np.array_equal(table[side], want)
                seen_nothing += not kept
                seen_one += len(kept) == 1
                seen_two += len(kept) == 2
            seen_interior += ref.neighbor[0] >= 0 and ref.neighbor[1] >= 0 and not periods[dim]
    assert seen_nothing and seen_one and (seen_two or pdims != (1, 1))
    assert seen_interior or pdims != (2, 3)  # (2 x 3: ranks with a neighbour on both sides of a non-periodic dim)


def test_wider_halos_and_padding_on_one_rank():
    grid = _spec((1, 1))
    for axis, dim, (halo, padding), centering, sides in itertools.product(range(3), range(3), (((2, 1, 3), (1, 2, 0)), ((3, 3, 3), (0, 0, 0))),
                                                                         (0, 1), (1, 2, 3)):
        ref = cd.cudecompExtPlanHaloReflect(grid, 0, axis, halo, (0, 0, 0), dim, padding, centering, True)
        p, _ = cd.cudecompExtPlanHaloWallValues(grid, 0, axis, halo, (0, 0, 0), dim, cd.FLOAT, -1, centering, sides, [0.0] * 3, [0.0] * 3,
                                                padding)
        assert ref.n_pre == 2 and [_move_tuple(p.pre[i]) for i in range(p.n_pre)] == [
            _move_tuple(ref.pre[i]) for i in range(2) if sides & (1 << i)]


# ---- the conversion ----------------------------------------------------------------------------------------------------------
def narrow(x, ebits, mbits):
    """the bit pattern of the double `x` rounded ONCE, to nearest even, to the 16-bit format with `ebits` exponent and `mbits`
    stored significand bits -- in exact rational arithmetic; overflow gives infinity"""
    sign = (struct.unpack("<Q", struct.pack("<d", x))[0] >> 63) << (ebits + mbits)
    inf, bias = ((1 << ebits) - 1) << mbits, (1 << (ebits - 1)) - 1
    if x != x:
        return None  # (a NaN: the pattern is unspecified)
    if math.isinf(x):
        return sign | inf
    f = abs(fractions.Fraction(x))
    if f == 0:
        return sign
    e = f.numerator.bit_length() - f.denominator.bit_length()
    if fractions.Fraction(2) ** e > f:
        e -= 1
    assert fractions.Fraction(2) ** e <= f < fractions.Fraction(2) ** (e + 1)
    e = max(e, 1 - bias)  # (subnormals share the exponent of the smallest normal)
    q = f / fractions.Fraction(2) ** (e - mbits)  # the significand in units of its last place
    n = q.numerator // q.denominator
    r = q - n
    if r > fractions.Fraction(1, 2) or (r == fractions.Fraction(1, 2) and n & 1):
        n += 1
    bits = ((e + bias - 1) << mbits) + n  # (a normal's n holds the implicit bit; a carry moves into the exponent)
    return sign | min(bits, inf)


def element_bytes_of(dtype, reals):
    """the element of `dtype` whose reals are the doubles `reals`, converted as the contract says; None where a real is a NaN"""
    kind = AB.kind_of(dtype)
    out = b""
    for x in reals:
        if kind == "fp64":
            out += struct.pack("<d", x)
        elif kind == "fp32":
            with np.errstate(over="ignore"):
                out += np.float64(x).astype(np.float32).tobytes()
        else:
            bits = narrow(x, *FORMAT[kind])
            if bits is None:
                return None
            out += struct.pack("<H", bits)
    return out


# a double just above the tie between two neighbouring narrow values, which fp32 rounds ONTO the tie: through fp32 the result is the
# even neighbour below, directly it is the neighbour above
TIE_FP16 = 1.0 + 2.0 ** -11 + 2.0 ** -30
TIE_BF16 = 1.0 + 2.0 ** -8 + 2.0 ** -40
VALUES = [TIE_FP16, -TIE_FP16, TIE_BF16, -TIE_BF16, 0.1, -3.75, 65519.99, 65520.0, -1e6, 1e39, 3.5e38, -1e300, 5.9e-8, 2.9e-8, 2.99e-8,
          -6.1e-5, 1e-40, 4.6e-41, -1e-46, 0.0, -0.0, float("inf"), 1.7976931348623157e308, 2.0 ** -24 + 2.0 ** -60, 2.0 ** -25]


def test_the_two_routes_differ_where_the_test_says_so():
    """so that the table test below cannot pass with a conversion that goes through fp32"""
    direct, through = np.float64(TIE_FP16).astype(np.float16), np.float64(TIE_FP16).astype(np.float32).astype(np.float16)
    assert direct.view(np.uint16) == 0x3C01 and through.view(np.uint16) == 0x3C00
    assert narrow(TIE_FP16, 5, 10) == 0x3C01 and narrow(float(np.float32(TIE_FP16)), 5, 10) == 0x3C00
    assert narrow(TIE_BF16, 8, 7) == 0x3F81 and narrow(float(np.float32(TIE_BF16)), 8, 7) == 0x3F80
    # the restatement against numpy's own double -> binary16 conversion, which rounds once
    with np.errstate(over="ignore"):
        for x in VALUES:
            assert narrow(x, 5, 10) == int(np.float64(x).astype(np.float16).view(np.uint16)), x
    assert narrow(1e39, 8, 7) == 0x7F80 and narrow(-1e300, 5, 10) == 0xFC00 and narrow(65520.0, 5, 10) == 0x7C00 and narrow(65519.99, 5, 10) == 0x7BFF


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_the_addend_table(dtype):
    """all seven types; ties that fp32 would round the other way, overflow to infinity, subnormal results, both zeros; the low side
    reversed, the high side as given; entries beyond h and the row of a side not named are zero bytes"""
    grid = _spec((1, 1))
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    rng = np.random.default_rng(5)
    for h, first in ((3, 0), (3, 6), (2, 12), (1, 16), (3, 17), (3, 19)):
        halo = (h, 1, 1)
        low = VALUES[first:first + h * nc] if first + h * nc <= len(VALUES) else list(rng.standard_normal(h * nc))
        low = (low + list(rng.standard_normal(h * nc)))[:h * nc]
        high = list(rng.standard_normal(h * nc) * 1e3)
        high[0] = VALUES[(first + 5) % len(VALUES)]
        for sides in (1, 2, 3):
            _, table = cd.cudecompExtPlanHaloWallValues(grid, 0, 0, halo, (0, 0, 0), 0, dtype, -1, 0, sides, low if sides & 1 else None,
                                                        high if sides & 2 else None)
            want = np.zeros((2, cd.MAX_WALL_HALO, 16), dtype=np.uint8)
            for side, values in ((0, low), (1, high)):
                if not sides & (1 << side):
                    continue
                for k in range(h):
                    j = h - 1 - k if side == 0 else k  # (destination index inside the slab)
                    want[side, j] = np.frombuffer(element_bytes_of(dtype, values[k * nc:(k + 1) * nc]) * (16 // es), dtype=np.uint8)
            assert np.array_equal(table, want), (AB.NAMES[dtype], h, first, sides)
    # h = 8: the whole row; distinct layers, so a reversal that is off by one shows
    halo, values = (8, 1, 1), [float(k + 1) + 0.5 * c for k in range(8) for c in range(nc)]
    _, table = cd.cudecompExtPlanHaloWallValues(_spec((1, 1)), 0, 1, (1, 1, 8), (0, 0, 0), 2, dtype, 1, 0, 3, values, values)
    for k in range(8):
        elem = np.frombuffer(element_bytes_of(dtype, values[k * nc:(k + 1) * nc]) * (16 // es), dtype=np.uint8)
        assert np.array_equal(table[0, 7 - k], elem) and np.array_equal(table[1, k], elem)
    assert halo[0] == cd.MAX_WALL_HALO
    # a NaN addend is accepted and stays a NaN of the type
    _, table = cd.cudecompExtPlanHaloWallValues(grid, 0, 0, (1, 1, 1), (0, 0, 0), 0, dtype, 1, 0, 2, None, [float("nan")] * nc)
    kind = AB.kind_of(dtype)
    reals = table[1, 0, :AB.real_bytes(dtype)].copy().view(AB.FORMATS[kind][0])
    assert AB.classes(kind, reals)["nan"].all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _plan_rc(grid, rank, axis, halo, periods, dim, dtype, parity, centering, sides, low, high, padding=None):
    try:
        cd.cudecompExtPlanHaloWallValues(grid, rank, axis, halo, periods, dim, dtype, parity, centering, sides, low, high, padding)
    except cd.CudecompError as e:
        return e.code
    return cd.RESULT_SUCCESS


def _message(capfd):
    err = capfd.readouterr().err
    found = re.findall(r"CUDECOMP:ERROR: .*\((.*)\)", err)
    return found[-1] if found else err


SIDES, VALUES_NULL, TOO_WIDE = ("sides argument must be 1, 2 or 3: the low halo, the high halo or both", "the value array of a side named in sides cannot be null",
                                "halo_extents[dim] is wider than CUDECOMP_AMD_MAX_WALL_HALO")


def test_refusals_on_every_rank(capfd):
    """the stateless planner makes the call's checks in the call's order, on every rank of a 2 x 3 grid -- edge or interior,
    periodic dim or not: all ranks agree"""
    grid = _spec((2, 3))
    v = [0.0] * 16
    capfd.readouterr()
    interior = 0
    for rank, axis, dim, periods in itertools.product(range(6), range(3), range(3), ((0, 0, 0), (1, 1, 1))):
        args = (grid, rank, axis, (1, 1, 1), periods, dim, cd.FLOAT)
        ok, _ = cd.cudecompExtPlanHaloWallValues(*args, 1, 0, 3, v, v)
        interior += ok.kind == 0 and not periods[dim]
        for sides in (0, 4, -1):
            assert _plan_rc(*args, 1, 0, sides, v, v) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
        assert _plan_rc(*args, 1, 0, 3, None, v) == cd.RESULT_INVALID_USAGE and _message(capfd) == VALUES_NULL
        assert _plan_rc(*args, 1, 0, 2, v, None) == cd.RESULT_INVALID_USAGE and _message(capfd) == VALUES_NULL
        assert _plan_rc(*args, 1, 0, 1, v, None) == cd.RESULT_SUCCESS and _plan_rc(*args, -1, 1, 2, None, v) == cd.RESULT_SUCCESS
        # the order: parity, centering, sides, arrays, width -- a tuple that breaks two at once gets the earlier message
        assert _plan_rc(*args, 0, 2, 0, None, None) == cd.RESULT_INVALID_USAGE and _message(capfd) == "parity argument must be +1 or -1"
        assert _plan_rc(*args, 1, 2, 0, None, None) == cd.RESULT_INVALID_USAGE and _message(capfd) == "centering argument must be 0 or 1"
        assert _plan_rc(*args, 1, 1, 0, None, None) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
    assert interior > 0
    # width, on a grid whose pencils hold a halo of 9: one rank alone along dim 0, two along the others
    grid = cd.make_grid_spec((64, 40, 40), (2, 1), MEM_ORDER)
    for rank, axis, periods in itertools.product(range(2), range(3), ((0, 0, 0), (1, 1, 1))):
        dim = axis  # (never distributed: the pencil's own axis)
        halo9, halo8 = [0, 0, 0], [0, 0, 0]
        halo9[dim], halo8[dim] = 9, 8
        args = (grid, rank, axis)
        assert _plan_rc(*args, halo8, periods, dim, cd.HALF, 1, 0, 3, v, v) == cd.RESULT_SUCCESS
        assert _plan_rc(*args, halo9, periods, dim, cd.HALF, 1, 0, 3, v, v) == cd.RESULT_NOT_SUPPORTED and _message(capfd) == TOO_WIDE
        assert _plan_rc(*args, halo9, periods, dim, cd.HALF, 1, 0, 3, v, None) == cd.RESULT_INVALID_USAGE and _message(capfd) == VALUES_NULL
        assert _plan_rc(*args, halo9, periods, dim, cd.HALF, 1, 0, 5, v, None) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
    # the reflection's last refusal, h + centering > n - 2 h, only for a side that would be written: dim 1 of the X pencil is cut in
    # two halves of 8 interior cells, so h = 8 fits with centering 0 and not with centering 1 -- whatever the reflection answers
    # for a rank is the answer for the sides that name the edge this rank owns, and the other side alone succeeds
    grid = cd.make_grid_spec((64, 16, 40), (2, 1), MEM_ORDER)
    halo = (0, 8, 0)
    answers = set()
    for rank, centering in itertools.product(range(2), (0, 1)):
        codes = {}
        for sides in (1, 2, 3):
            codes[sides] = _plan_rc(grid, rank, 0, halo, (0, 0, 0), 1, cd.DOUBLE, 1, centering, sides, v, v)
            capfd.readouterr()
        try:
            cd.cudecompExtPlanHaloReflect(grid, rank, 0, halo, (0, 0, 0), 1, None, centering, False)
            reflect = cd.RESULT_SUCCESS
        except cd.CudecompError as e:
            reflect = e.code
        capfd.readouterr()
        own = 1 if rank == 0 else 2  # (rank 0 owns the low edge of dim 1, rank 1 the high edge)
        assert codes[own] == codes[3] == reflect and codes[3 - own] == cd.RESULT_SUCCESS, (rank, centering, codes, reflect)
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
    fn = getattr(cd.lib(), cd.AMD_WALL_VALUES_SYMBOLS[axis])
    f64 = lambda a: None if a is None else (C.c_double * max(1, len(a)))(*a)
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    return fn(h, gd, ptr, dtype, parity, centering, sides, f64(low), f64(high), hh, (C.c_bool * 3)(*periods), dim, None, None)


def _reflect(h, gd, axis, ptr, parity, centering, halo=(1, 1, 1), dim=0, periods=(False, False, False), dtype=cd.DOUBLE):
    fn = getattr(cd.lib(), "cudecompAmdReflectHalos" + "XYZ"[axis])
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    return fn(h, gd, ptr, dtype, parity, centering, hh, (C.c_bool * 3)(*periods), dim, None, None)


def test_refusals_through_the_c_abi(descriptor, capfd):
    """all found on the host, before anything is launched (the pointer is not device memory): what the reflection refuses first, in
    its order and with its words, then sides, arrays, width.  Tuples with cells to write are shown on the stateless planner above:
    through the C ABI they would go on to the device."""
    h, gd = descriptor
    fake, v = 0x10000, [0.0] * 16
    capfd.readouterr()
    for axis in range(3):
        # what the reflection refuses, refused the same way whatever the new arguments are
        for kwargs in (dict(halo=None), dict(dim=7), dict(dim=-1), dict(halo=(1, 60, 1), dim=1, periods=(True, True, True)), dict(dtype=17)):
            for ptr in (None, fake):
                rc = _reflect(h, gd, axis, ptr, 5, 5, **kwargs)
                message = _message(capfd)
                assert rc != cd.RESULT_SUCCESS
                assert _call(h, gd, axis, ptr, 5, 5, 0, None, None, **kwargs) == rc and _message(capfd) == message, (axis, kwargs)
        assert _call(h, gd, axis, None, 1, 0, 3, v, v) == cd.RESULT_INVALID_USAGE and _message(capfd) == "input argument cannot be null"
        for periods, halo in (((False,) * 3, (1, 1, 1)), ((True,) * 3, (1, 1, 1)), ((False,) * 3, (0, 1, 1)), ((False,) * 3, (0, 0, 0))):
            kw = dict(halo=halo, periods=periods)
            assert _call(h, gd, axis, fake, 0, 2, 0, None, None, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == "parity argument must be +1 or -1"
            assert _call(h, gd, axis, fake, -1, 2, 0, None, None, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == "centering argument must be 0 or 1"
            for sides in (0, 4, -3):
                assert _call(h, gd, axis, fake, -1, 1, sides, None, None, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES
            assert _call(h, gd, axis, fake, -1, 1, 3, v, None, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == VALUES_NULL
            assert _call(h, gd, axis, fake, 1, 0, 1, None, v, **kw) == cd.RESULT_INVALID_USAGE and _message(capfd) == VALUES_NULL
        # nothing to write (periodic dim, no halo along the dim, no halo at all): the call succeeds, also with the other array NULL
        for kw in (dict(periods=(True,) * 3), dict(halo=(0, 1, 1)), dict(halo=(0, 0, 0))):
            assert _call(h, gd, axis, fake, 1, 0, 1, v, None, **kw) == cd.RESULT_SUCCESS
            assert _call(h, gd, axis, fake, -1, 1, 2, None, v, **kw) == cd.RESULT_SUCCESS
            assert _call(h, gd, axis, fake, -1, 1, 3, v, v, **kw) == cd.RESULT_SUCCESS
        # width: 8 is accepted, 9 is not -- on a periodic dim too; an array that is missing is reported first
        per = (True,) * 3
        assert _call(h, gd, axis, fake, 1, 0, 3, v, v, halo=(8, 1, 1), periods=per) == cd.RESULT_SUCCESS
        assert _call(h, gd, axis, fake, 1, 0, 3, v, v, halo=(9, 1, 1), periods=per) == cd.RESULT_NOT_SUPPORTED and _message(capfd) == TOO_WIDE
        assert _call(h, gd, axis, fake, 1, 0, 3, v, v, halo=(9, 1, 1)) == cd.RESULT_NOT_SUPPORTED and _message(capfd) == TOO_WIDE
        assert _call(h, gd, axis, fake, 1, 0, 3, None, v, halo=(9, 1, 1)) == cd.RESULT_INVALID_USAGE and _message(capfd) == VALUES_NULL
        # the mirror that reaches beyond the interior comes last: dim 1 has 6 cells, h = 6 with centering 1 leaves the sources no room
        assert _reflect(h, gd, axis, fake, 1, 1, halo=(1, 6, 1), dim=1) == cd.RESULT_INVALID_USAGE
        message = _message(capfd)
        assert _call(h, gd, axis, fake, 1, 1, 3, v, v, halo=(1, 6, 1), dim=1) == cd.RESULT_INVALID_USAGE and _message(capfd) == message
        assert _call(h, gd, axis, fake, 1, 1, 0, v, v, halo=(1, 6, 1), dim=1) == cd.RESULT_INVALID_USAGE and _message(capfd) == SIDES


def test_calls_that_differ_only_in_addends_share_one_plan(descriptor):
    """on a periodic dim the call has nothing to launch, and its plan is cached all the same: a second set of addends adds none, other
    sides, another parity and another centering add one each"""
    h, gd = descriptor
    L = cd.lib()

    def plans():
        n = C.c_int64(-1)
        assert L.cudecompExtHaloPlanCount(h, gd, C.byref(n)) == cd.RESULT_SUCCESS
        return n.value

    per, fake = (True, True, True), 0x10000
    before = plans()
    assert _call(h, gd, 0, fake, -1, 0, 3, [1.0, 2.0], [3.0, 4.0], halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 1
    assert _call(h, gd, 0, fake, -1, 0, 3, [-7.5, 1e30], [0.0, float("nan")], halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 1
    assert _call(h, gd, 0, fake, -1, 0, 1, [1.0, 2.0], None, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 2
    assert _call(h, gd, 0, fake, 1, 0, 3, [1.0, 2.0], [3.0, 4.0], halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert _call(h, gd, 0, fake, 1, 1, 3, [1.0, 2.0], [3.0, 4.0], halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 4
    # ... and the reflection with the same arguments has a plan of its own
    assert _reflect(h, gd, 0, fake, -1, 0, halo=(2, 1, 1), periods=per) == cd.RESULT_SUCCESS
    assert plans() == before + 5
