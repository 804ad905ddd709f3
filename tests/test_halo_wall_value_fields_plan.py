"""Multi-field wall values (cudecomp_halo_wall_value_fields.h: cudecompAmdSetWallFieldHalos{X,Y,Z}) without a GPU: the C interface
(symbols, prototypes against the ctypes argtypes), every refusal through the C ABI in its order of precedence, calls with nothing
to write, the plan of every rank against the single call's moves, the plan cache, and the launches of the wall field-move kernels
(cudecompExtDescribeWallFieldMoves): the launch rule and the compact addend table against the conversion restated in exact rational
arithmetic (tests/test_halo_wall_values_plan.py)."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402
from tests import accumulate_bodies as AB  # noqa: E402
from tests.test_halo_wall_fields_plan import _prototypes  # noqa: E402
from tests.test_halo_wall_values_plan import (GRIDS, SIDES, TIE_BF16, TIE_FP16, TOO_WIDE, VALUES, VALUES_NULL, _message, _move_tuple,  # noqa: E402
                                              _spec, element_bytes_of)

HEADER = "cudecomp_halo_wall_value_fields.h"
NAMES = ["cudecompAmdSetWallFieldHalos" + a for a in "XYZ"]
EXT = ["cudecompExtRunWallFieldMoves", "cudecompExtDescribeWallFieldMoves", "cudecompExtPlanHaloWallValueFields"]
K_ROWS_WALL, K_GENERIC_WALL, K_ROWS_FIELDS_WALL, K_GENERIC_FIELDS_WALL = 37, 38, 39, 40
TABLE = 2048


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_three_symbols_are_declared_and_exported():
    assert cd.AMD_WALL_VALUE_FIELDS_SYMBOLS == NAMES and cd.MAX_WALL_VALUE_FIELDS == 32 and cd.WALL_FIELD_TABLE_BYTES == TABLE
    assert sorted(_prototypes(HEADER)) == sorted(NAMES)
    L = cd.lib()
    for name in NAMES + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert re.search(r"#define\s+CUDECOMP_AMD_MAX_WALL_VALUE_FIELDS\s+32\b", text)
    assert "one centering per call" in text.lower() and "one `sides` per call" in text.lower()
    single = open(os.path.join(ROOT, "include", "cudecomp_halo_wall_values.h")).read()
    assert HEADER in single and "a multi-field form" not in single.split("Out of scope")[1]


def test_prototypes_agree_with_the_argtypes():
    """the single call's prototype with (inputs, n_fields) in the place of `input` and `parities` in the place of `parity`: as many
    parameters as argtypes, pointers at the same positions, everything else a 32-bit integer on both sides"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos, singles = _prototypes(HEADER), _prototypes("cudecomp_halo_wall_values.h")
    for name in NAMES:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 15, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        single = singles[name.replace("FieldHalos", "Halos")]
        assert params[2:4] == ["void* const inputs[]", "int32_t n_fields"] and single[2] == "void* input"
        assert params[5] == "const int32_t parities[]" and single[4] == "int32_t parity"
        assert params[:2] + params[4:5] + params[6:] == single[:2] + single[3:4] + single[5:]
    ext = _prototypes("cudecomp_ext.h")
    for name in EXT:
        assert len(getattr(L, name).argtypes) == len(ext[name]), name


@pytest.mark.parametrize("language", ["c11", "c++17"])
def test_header_compiles(language):
    """alone, and before and after the other extension headers, -Wall -Wextra -Werror"""
    cc = "gcc" if language == "c11" else "g++"
    if shutil.which(cc) is None:
        pytest.skip("no " + cc)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = [cc, "-std=" + language, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include"), "-x", "c" if language == "c11" else "c++", "-"]
    others = ["cudecomp_amd.h", "cudecomp_amd_fill.h", "cudecomp_amd_reflect.h", "cudecomp_halo_fold.h", "cudecomp_halo_fields.h",
              "cudecomp_transpose_fields.h", "cudecomp_halo_accumulate_fields.h", "cudecomp_halo_wall_fields.h", "cudecomp_halo_wall_values.h"]
    uses = ("int main(void) {\n  void* f[1] = {0};\n  const int32_t par[1] = {1}, h[3] = {0, 0, 0};\n  const double v[1] = {0.5};\n"
            "  return (int)cudecompAmdSetWallFieldHalosX(0, 0, f, 1, CUDECOMP_DOUBLE, par, 0, 3, v, v, h, 0, 0, 0, 0) +\n"
            "         (int)cudecompAmdSetWallFieldHalosZ(0, 0, f, 1, CUDECOMP_DOUBLE, par, 1, 1, v, 0, h, 0, 0, 0, 0) + "
            "(CUDECOMP_AMD_MAX_WALL_VALUE_FIELDS != 32) + (CUDECOMP_AMD_MAX_WALL_HALO != 8);\n}\n")
    for order in ([HEADER], [HEADER] + others, others + [HEADER]):
        res = subprocess.run(base, input="".join('#include "%s"\n' % h for h in order) + uses, capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (order, res.stderr[-3000:])


# ---- refusals through the C ABI ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def descriptor():
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((40, 6, 12), (1, 1)))
    yield h, gd
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


FAKE = [0x10000 + 0x1000 * f for f in range(40)]


def _call(h, gd, axis, ptrs, parities, centering, sides, low, high, halo=(1, 1, 1), dim=0, periods=(False, False, False), dtype=cd.DOUBLE,
          n_fields=None):
    fn = getattr(cd.lib(), NAMES[axis])
    f64 = lambda a: None if a is None else (C.c_double * max(1, len(a)))(*a)
    arr = None if ptrs is None else (C.c_void_p * max(1, len(ptrs)))(*ptrs)
    par = None if parities is None else (C.c_int32 * max(1, len(parities)))(*parities)
    n = n_fields if n_fields is not None else (len(ptrs) if ptrs is not None else len(parities or []))
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    return fn(h, gd, arr, n, dtype, par, centering, sides, f64(low), f64(high), hh, (C.c_bool * 3)(*periods), dim, None, None)


def _single(h, gd, axis, ptr, parity, centering, sides, low, high, halo=(1, 1, 1), dim=0, periods=(False, False, False), dtype=cd.DOUBLE):
    fn = getattr(cd.lib(), cd.AMD_WALL_VALUES_SYMBOLS[axis])
    f64 = lambda a: None if a is None else (C.c_double * max(1, len(a)))(*a)
    hh = None if halo is None else (C.c_int32 * 3)(*halo)
    return fn(h, gd, ptr, dtype, parity, centering, sides, f64(low), f64(high), hh, (C.c_bool * 3)(*periods), dim, None, None)


def test_refusals_through_the_c_abi(descriptor, capfd):
    """all found on the host, before anything is launched (the pointers are no device memory): what the single call refuses first,
    with its words; the lists where the single call checks `input`; the parities where it checks `parity`; then centering, sides,
    arrays, width, the mirror's reach -- also on a periodic dim and with h == 0, where there is nothing to write"""
    h, gd = descriptor
    v = [0.0] * (16 * 40)
    bad, invalid = cd.RESULT_INVALID_USAGE, cd.RESULT_INVALID_USAGE
    capfd.readouterr()
    for axis, n in itertools.product(range(3), (1, 3, 32)):
        ptrs, par = FAKE[:n], [1, -1, 1][:n] if n <= 3 else [(-1) ** f for f in range(n)]
        # what the single call refuses before it looks at `input`, refused the same way whatever the new arguments are
        for kwargs in (dict(halo=None), dict(dtype=17)):
            rc = _single(h, gd, axis, FAKE[0], 5, 5, 0, None, None, **kwargs)
            message = _message(capfd)
            assert rc != cd.RESULT_SUCCESS
            assert _call(h, gd, axis, None, None, 5, 0, None, None, n_fields=77, **kwargs) == rc and _message(capfd) == message, (axis, kwargs)
        # ... and a tuple the single call refuses at its parity is refused there with the parities' entries, whatever else is wrong
        kwargs = dict(halo=(1, 60, 1), dim=1, periods=(True, True, True))
        rc = _single(h, gd, axis, FAKE[0], 5, 5, 0, None, None, **kwargs)
        message = _message(capfd)
        assert rc != cd.RESULT_SUCCESS
        assert _call(h, gd, axis, ptrs, [5] * n, 5, 0, None, None, **kwargs) == rc and _message(capfd) == message, (axis, kwargs)
        # the lists, in their order
        assert _call(h, gd, axis, None, par, 0, 3, v, v, n_fields=n) == bad and _message(capfd) == "inputs argument cannot be null"
        for count in (0, -1, 33):
            assert _call(h, gd, axis, FAKE, None, 5, 0, None, None, n_fields=count) == bad and _message(capfd) == "n_fields argument out of range"
        if n > 1:
            holes = list(ptrs)
            holes[n - 1] = None
            assert _call(h, gd, axis, holes, None, 5, 0, None, None) == bad and _message(capfd) == "inputs argument cannot hold a null entry"
            twice = list(ptrs)
            twice[n - 1] = twice[0]
            assert _call(h, gd, axis, twice, None, 5, 0, None, None) == bad and _message(capfd) == "inputs argument cannot hold the same field twice"
        else:
            assert _call(h, gd, axis, [None], None, 5, 0, None, None) == bad and _message(capfd) == "inputs argument cannot hold a null entry"
        assert _call(h, gd, axis, ptrs, None, 5, 0, None, None, dim=7) == bad and _message(capfd) == "parities argument cannot be null"
        # dim comes where the single call has it: after the lists, before the parities' entries
        rc = _single(h, gd, axis, FAKE[0], 5, 5, 0, None, None, dim=7)
        message = _message(capfd)
        wrong = list(par)
        wrong[n - 1] = 0
        assert _call(h, gd, axis, ptrs, wrong, 5, 0, None, None, dim=7) == rc and _message(capfd) == message
        for periods, halo in (((False,) * 3, (1, 1, 1)), ((True,) * 3, (1, 1, 1)), ((False,) * 3, (0, 1, 1)), ((False,) * 3, (0, 0, 0))):
            kw = dict(halo=halo, periods=periods)
            for at in {0, n - 1}:
                wrong = list(par)
                wrong[at] = 2
                assert _call(h, gd, axis, ptrs, wrong, 2, 0, None, None, **kw) == invalid and _message(capfd) == "parity argument must be +1 or -1"
            assert _call(h, gd, axis, ptrs, par, 2, 0, None, None, **kw) == invalid and _message(capfd) == "centering argument must be 0 or 1"
            for sides in (0, 4, -3):
                assert _call(h, gd, axis, ptrs, par, 1, sides, None, None, **kw) == invalid and _message(capfd) == SIDES
            assert _call(h, gd, axis, ptrs, par, 1, 3, v, None, **kw) == invalid and _message(capfd) == VALUES_NULL
            assert _call(h, gd, axis, ptrs, par, 0, 1, None, v, **kw) == invalid and _message(capfd) == VALUES_NULL
        # nothing to write (periodic dim, no halo along the dim, no halo at all): the call succeeds, launches nothing, needs no device
        for kw in (dict(periods=(True,) * 3), dict(halo=(0, 1, 1)), dict(halo=(0, 0, 0))):
            assert _call(h, gd, axis, ptrs, par, 0, 1, v, None, **kw) == cd.RESULT_SUCCESS
            assert _call(h, gd, axis, ptrs, par, 1, 2, None, v, **kw) == cd.RESULT_SUCCESS
            assert _call(h, gd, axis, ptrs, par, 1, 3, v, v, **kw) == cd.RESULT_SUCCESS
        # width: 8 is accepted, 9 is not -- on a periodic dim too; an array that is missing is reported first
        per = (True,) * 3
        assert _call(h, gd, axis, ptrs, par, 0, 3, v, v, halo=(8, 1, 1), periods=per) == cd.RESULT_SUCCESS
        assert _call(h, gd, axis, ptrs, par, 0, 3, v, v, halo=(9, 1, 1), periods=per) == cd.RESULT_NOT_SUPPORTED and _message(capfd) == TOO_WIDE
        assert _call(h, gd, axis, ptrs, par, 0, 3, v, v, halo=(9, 1, 1)) == cd.RESULT_NOT_SUPPORTED and _message(capfd) == TOO_WIDE
        assert _call(h, gd, axis, ptrs, par, 0, 3, None, v, halo=(9, 1, 1)) == invalid and _message(capfd) == VALUES_NULL
        # the mirror that reaches beyond the interior comes last: dim 1 has 6 cells, h = 6 with centering 1 leaves the sources no room
        assert _single(h, gd, axis, FAKE[0], 1, 1, 3, v, v, halo=(1, 6, 1), dim=1) == invalid
        message = _message(capfd)
        assert _call(h, gd, axis, ptrs, par, 1, 3, v, v, halo=(1, 6, 1), dim=1) == invalid and _message(capfd) == message
        assert _call(h, gd, axis, ptrs, par, 1, 0, v, v, halo=(1, 6, 1), dim=1) == invalid and _message(capfd) == SIDES


def test_ranks_away_from_the_edge_make_the_checks_and_launch_nothing():
    """the stateless planner on every rank of a 2 x 3 grid: all ranks agree on sides and width, and a rank with neighbours on both
    sides of a non-periodic dim has a plan without moves"""
    grid = _spec((2, 3))
    idle = 0
    for rank, axis, dim, periods in itertools.product(range(6), range(3), range(3), ((0, 0, 0), (1, 1, 1))):
        p = cd.cudecompExtPlanHaloWallValueFields(grid, rank, axis, (1, 1, 1), periods, dim, 0, 3, 5)
        idle += p.n_pre == 0 and not periods[dim]
        assert p.n_pre == 0 or not periods[dim]
        for args, code in (((2, 3, 5), cd.RESULT_INVALID_USAGE), ((0, 0, 5), cd.RESULT_INVALID_USAGE), ((0, 4, 5), cd.RESULT_INVALID_USAGE),
                           ((0, 3, 0), cd.RESULT_INVALID_USAGE), ((0, 3, 33), cd.RESULT_INVALID_USAGE)):
            with pytest.raises(cd.CudecompError) as e:
                cd.cudecompExtPlanHaloWallValueFields(grid, rank, axis, (1, 1, 1), periods, dim, *args)
            assert e.value.code == code, (rank, axis, dim, args)
    assert idle > 0
    grid = cd.make_grid_spec((64, 40, 40), (2, 1), ((0, 1, 2), (1, 2, 0), (2, 0, 1)))
    for rank, axis, periods in itertools.product(range(2), range(3), ((0, 0, 0), (1, 1, 1))):
        halo = [0, 0, 0]
        halo[axis] = 9
        with pytest.raises(cd.CudecompError) as e:
            cd.cudecompExtPlanHaloWallValueFields(grid, rank, axis, halo, periods, axis, 0, 3, 2)
        assert e.value.code == cd.RESULT_NOT_SUPPORTED


# ---- the plan ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdims", GRIDS, ids=["%dx%d" % g for g in GRIDS])
def test_the_moves_are_the_single_calls(pdims):
    """every rank, axis, dim, period mix, centering and sides, 2 and 32 fields: the moves are those of cudecompExtPlanHaloWallValues
    (with parity +1: the plan carries no sign), each naming its side"""
    grid = _spec(pdims)
    with_moves = 0
    for rank, axis, dim, periods in itertools.product(range(pdims[0] * pdims[1]), range(3), range(3), ((0, 0, 0), (0, 1, 0))):
        for halo, padding in (((1, 1, 1), None), ((2, 1, 3), (1, 2, 0))):
            for centering, sides, n in itertools.product((0, 1), (1, 2, 3), (2, 32)):
                v = [0.5] * halo[dim]
                try:
                    single, _ = cd.cudecompExtPlanHaloWallValues(grid, rank, axis, halo, periods, dim, cd.DOUBLE, 1, centering, sides, v, v, padding)
                except cd.CudecompError as e:
                    with pytest.raises(cd.CudecompError) as mine:
                        cd.cudecompExtPlanHaloWallValueFields(grid, rank, axis, halo, periods, dim, centering, sides, n, padding)
                    assert mine.value.code == e.code
                    continue
                p = cd.cudecompExtPlanHaloWallValueFields(grid, rank, axis, halo, periods, dim, centering, sides, n, padding)
                assert [_move_tuple(p.pre[i]) for i in range(p.n_pre)] == [_move_tuple(single.pre[i]) for i in range(single.n_pre)]
                assert (p.kind, p.n_post, p.face_elements, list(p.neighbor)) == (single.kind, 0, single.face_elements, list(single.neighbor))
                assert p.reserved == single.reserved == (1 << 15) | (sides << 16)
                with_moves += p.n_pre > 0
    assert with_moves > 0


def test_calls_that_differ_only_in_parities_or_addends_share_one_plan(descriptor):
    """on a periodic dim the call has nothing to launch, and its plan is cached all the same"""
    h, gd = descriptor
    L = cd.lib()

    def plans():
        n = C.c_int64(-1)
        assert L.cudecompExtHaloPlanCount(h, gd, C.byref(n)) == cd.RESULT_SUCCESS
        return n.value

    per, kw = (True, True, True), dict(halo=(2, 1, 1), periods=(True, True, True))
    before = plans()
    assert _call(h, gd, 0, FAKE[:3], [1, -1, 1], 0, 3, [1.0] * 6, [2.0] * 6, **kw) == cd.RESULT_SUCCESS
    assert plans() == before + 1
    assert _call(h, gd, 0, FAKE[:3], [-1, -1, -1], 0, 3, [1.0] * 6, [2.0] * 6, **kw) == cd.RESULT_SUCCESS
    assert _call(h, gd, 0, FAKE[:3], [1, 1, 1], 0, 3, [-7.5, 1e30] * 3, [0.0, float("nan")] * 3, **kw) == cd.RESULT_SUCCESS
    assert _call(h, gd, 0, FAKE[3:6], [1, 1, -1], 0, 3, [3.0] * 6, [4.0] * 6, **kw) == cd.RESULT_SUCCESS
    assert plans() == before + 1
    assert _call(h, gd, 0, FAKE[:3], [1, -1, 1], 0, 1, [1.0] * 6, None, **kw) == cd.RESULT_SUCCESS  # other sides
    assert _call(h, gd, 0, FAKE[:3], [1, -1, 1], 1, 3, [1.0] * 6, [2.0] * 6, **kw) == cd.RESULT_SUCCESS  # another centering
    assert _call(h, gd, 0, FAKE[:4], [1, -1, 1, 1], 0, 3, [1.0] * 8, [2.0] * 8, **kw) == cd.RESULT_SUCCESS  # another count
    assert plans() == before + 4
    # one field is the single call: parities[0] = -1 and +1 are its two plans, which the single call then finds
    assert _call(h, gd, 0, FAKE[:1], [-1], 0, 3, [1.0] * 2, [2.0] * 2, **kw) == cd.RESULT_SUCCESS
    assert _call(h, gd, 0, FAKE[:1], [1], 0, 3, [1.0] * 2, [2.0] * 2, **kw) == cd.RESULT_SUCCESS
    assert plans() == before + 6
    assert _single(h, gd, 0, FAKE[0], -1, 0, 3, [1.0] * 2, [2.0] * 2, **kw) == cd.RESULT_SUCCESS
    assert _single(h, gd, 0, FAKE[0], 1, 0, 3, [1.0] * 2, [2.0] * 2, **kw) == cd.RESULT_SUCCESS
    assert plans() == before + 6 and per == kw["periods"]


# ---- launches and the compact table -----------------------------------------------------------------------------------------------
def _moves(h, sides, length=16, rows=5, mirrored=1):
    """the wall-moves of `sides` on a small block: h layers along dim `mirrored`, rows of `length` elements"""
    extent = [length, rows, 3]
    extent[mirrored] = h
    strides = (1, length + 2, (length + 2) * extent[1] + 4)
    span = sum((e - 1) * s for e, s in zip(extent, strides)) + 1
    out = []
    for side in (0, 1):
        if not sides & (1 << side):
            continue
        signed = list(strides)
        signed[mirrored] = -strides[mirrored]
        m = cd.make_move(extent, signed, strides, 2 * side * (span + 2) + (h - 1) * strides[mirrored], (2 * side + 1) * (span + 2), 0, 0)
        m.peer = side
        out.append(m)
    return out, 4 * (span + 2)


def _raw_addends(dtype, values):
    """values[f][side][k] = nc doubles -> the bytes cudecompExtDescribeWallFieldMoves takes, converted by the exact restatement"""
    es = AB.element_bytes(dtype)
    raw = bytearray(len(values) * 2 * cd.MAX_WALL_HALO * es)
    for f, per_field in enumerate(values):
        for side in (0, 1):
            for k, reals in enumerate(per_field[side]):
                at = ((f * 2 + side) * cd.MAX_WALL_HALO + k) * es
                raw[at:at + es] = element_bytes_of(dtype, reals)
    return bytes(raw)


def _want_table(dtype, values, moves, first, count, h):
    es = AB.element_bytes(dtype)
    want = np.zeros(TABLE, dtype=np.uint8)
    for i, m in enumerate(moves):
        for f in range(count):
            for j in range(h):
                k = h - 1 - j if m.peer == 0 else j  # (the low side reversed: destination order)
                at = ((i * count + f) * h + j) * es
                want[at:at + es] = np.frombuffer(element_bytes_of(dtype, values[first + f][m.peer][k]), dtype=np.uint8)
    return want


def _describe(dtype, n_fields, h, sides, values=None, fields_neg=0, force=0, **geometry):
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    moves, cells = _moves(h, sides, **geometry)
    if values is None:
        values = [[[[float(1 + f) + 0.25 * side + 0.5 * k + 0.125 * c for c in range(nc)] for k in range(h)] for side in (0, 1)]
                  for f in range(n_fields)]
    fields = [0x7f0000000000 + f * (cells * es + 256) for f in range(n_fields)]
    launches = cd.cudecompExtDescribeWallFieldMoves(moves, fields, dtype, _raw_addends(dtype, values), fields_neg, force)
    return launches, moves, values


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_the_compact_table(dtype):
    """all seven types: ties that fp32 would round the other way, overflow to infinity, subnormal results and both zeros as addends
    of distinct fields, sides and layers; the low side reversed, the high side as given; the rest of the table zero bytes"""
    nc = AB.TYPES[dtype][1]
    finite = [x for x in VALUES if x == x] + [TIE_FP16, TIE_BF16, 65520.0, 1e39, -1e300]
    for h, sides, n_fields in ((3, 3, 5), (1, 1, 2), (2, 2, 9), (8, 3, 3), (3, 1, 32)):
        pool = itertools.cycle(finite)
        values = [[[[next(pool) for _ in range(nc)] for _ in range(h)] for _ in (0, 1)] for _ in range(n_fields)]
        launches, moves, _ = _describe(dtype, n_fields, h, sides, values)
        assert sum(l["fields"] for l in launches) == n_fields
        for l in launches:
            want = _want_table(dtype, values, moves, l["first_field"], l["fields"], h)
            assert np.array_equal(l["table"], want), (AB.NAMES[dtype], h, sides, n_fields, l["first_field"],
                                                      np.nonzero(l["table"] != want)[0][:8])
            assert l["kind"] == K_ROWS_FIELDS_WALL


def test_the_table_rounds_once():
    """fp16 and bf16: the double just above a tie lands on the neighbour above (through fp32 it would land below); 65520 overflows"""
    for dtype, tie, up in ((cd.HALF, TIE_FP16, 0x3C01), (cd.BFLOAT16, TIE_BF16, 0x3F81)):
        values = [[[[tie], [-tie]], [[65520.0 if dtype == cd.HALF else 3.4e38], [1.0]]], [[[1.0], [2.0]], [[-1e39], [tie]]]]
        # the harness takes raw elements: convert with the library's own rule through the stateless planner of the single call ...
        grid = _spec((1, 1))
        raw = bytearray(2 * 2 * cd.MAX_WALL_HALO * 2)
        for f in range(2):
            _, table = cd.cudecompExtPlanHaloWallValues(grid, 0, 0, (2, 1, 1), (0, 0, 0), 0, dtype, 1, 0, 3, [x[0] for x in values[f][0]],
                                                        [x[0] for x in values[f][1]])
            for side in (0, 1):
                for k in range(2):
                    j = 1 - k if side == 0 else k
                    at = ((f * 2 + side) * cd.MAX_WALL_HALO + k) * 2
                    raw[at:at + 2] = bytes(table[side, j, :2])
        moves, cells = _moves(2, 3)
        (l,) = cd.cudecompExtDescribeWallFieldMoves(moves, [0x10000, 0x10000 + 4 * cells], dtype, bytes(raw))
        # ... and the table holds what exact rational rounding of the doubles gives
        assert np.array_equal(l["table"], _want_table(dtype, values, moves, 0, 2, 2))
        t = l["table"].view(np.uint16)
        assert t[1] == up and t[0] == (up | 0x8000)  # field 0, low side reversed: layer 1 (-tie) first
        assert t[4] == (0x7C00 if dtype == cd.HALF else 0x7F80)  # move 1 (high side), field 0, layer 0: infinity


LAUNCH_RULE = [  # dtype, fields, h, sides -> F, launches
    (cd.DOUBLE, 32, 2, 3, 32, 1), (cd.DOUBLE, 32, 1, 3, 32, 1), (cd.DOUBLE_COMPLEX, 32, 8, 3, 8, 4), (cd.DOUBLE_COMPLEX, 32, 8, 1, 16, 2),
    (cd.DOUBLE_COMPLEX, 32, 8, 2, 16, 2), (cd.DOUBLE, 32, 8, 3, 16, 2), (cd.DOUBLE, 32, 8, 1, 32, 1), (cd.DOUBLE, 32, 3, 3, 32, 1),
    (cd.DOUBLE_COMPLEX, 19, 8, 3, 8, 3), (cd.DOUBLE_COMPLEX, 9, 8, 3, 8, 2), (cd.DOUBLE_COMPLEX, 8, 8, 3, 8, 1), (cd.FLOAT_COMPLEX, 21, 7, 3, 18, 2),
    (cd.DOUBLE_COMPLEX, 32, 3, 3, 21, 2), (cd.HALF, 32, 8, 3, 32, 1), (cd.DOUBLE_COMPLEX, 2, 8, 3, 8, 1), (cd.DOUBLE_COMPLEX, 32, 5, 3, 12, 3)]


@pytest.mark.parametrize("dtype,n_fields,h,sides,per_launch,count", LAUNCH_RULE)
def test_the_launch_rule(dtype, n_fields, h, sides, per_launch, count):
    """F = min(32, 2048 / (S h es)) consecutive fields per launch, ceil(n_fields / F) launches in field order; one side only takes
    twice as many fields per launch; a count that is no multiple of F leaves a shorter last launch"""
    es = AB.element_bytes(dtype)
    s = bin(sides).count("1")
    assert per_launch == min(32, TABLE // (s * h * es)) and count == -(-n_fields // per_launch)
    mask = 0x96C3A55A & ((1 << n_fields) - 1)
    launches, moves, values = _describe(dtype, n_fields, h, sides, fields_neg=mask)
    assert len(launches) == count
    first = 0
    for l in launches:
        assert l["first_field"] == first and l["fields"] == min(per_launch, n_fields - first), launches
        assert l["kind"] == K_ROWS_FIELDS_WALL and l["access"] == 0 and l["vec"] == 16
        assert l["blocks"] == l["fields"] * l["blocks_per_field"] and l["blocks_per_field"] >= s
        assert np.array_equal(l["table"], _want_table(dtype, values, moves, first, l["fields"], h))
        first += l["fields"]
    assert first == n_fields


def test_one_field_is_the_single_call_and_force_picks_the_kernel():
    for dtype, force, sides in itertools.product((cd.DOUBLE, cd.HALF_COMPLEX), (0, 1, 2), (1, 3)):
        launches, moves, values = _describe(dtype, 1, 3, sides, force=force)
        assert [l["kind"] for l in launches] == [K_GENERIC_WALL if force & 1 else K_ROWS_WALL]
        assert (launches[0]["first_field"], launches[0]["fields"]) == (0, 1)
        assert np.array_equal(launches[0]["table"], _want_table(dtype, values, moves, 0, 1, 3))
        (l,) = _describe(dtype, 2, 3, sides, force=force)[0]
        assert l["kind"] == (K_GENERIC_FIELDS_WALL if force & 1 else K_ROWS_FIELDS_WALL) and l["access"] == (1 if force == 2 else 0)
    # the mirrored dim as the fastest one: element-wise by itself
    (l,) = _describe(cd.FLOAT, 3, 4, 3, mirrored=0, length=4)[0]
    assert l["kind"] == K_GENERIC_FIELDS_WALL
    # 2-byte elements: one field at 2 mod 4 narrows the lanes of its launch
    moves, cells = _moves(2, 3)
    raw = bytes(3 * 2 * cd.MAX_WALL_HALO * 2)
    assert cd.cudecompExtDescribeWallFieldMoves(moves, [0x10000, 0x20000, 0x30000], cd.HALF, raw)[0]["vec"] == 16
    assert cd.cudecompExtDescribeWallFieldMoves(moves, [0x10000, 0x20002, 0x30000], cd.HALF, raw)[0]["vec"] == 2


def test_the_harness_refuses_what_it_cannot_run():
    moves, cells = _moves(2, 3)
    raw = bytes(2 * 2 * cd.MAX_WALL_HALO * 8)
    fields = [0x10000, 0x20000]
    with pytest.raises(cd.CudecompError) as e:
        cd.cudecompExtDescribeWallFieldMoves(moves, fields, cd.DOUBLE, raw, fields_neg=4)
    assert e.value.code == cd.RESULT_INVALID_USAGE
    moves[0].peer = 2
    with pytest.raises(cd.CudecompError) as e:
        cd.cudecompExtDescribeWallFieldMoves(moves, fields, cd.DOUBLE, raw)
    assert e.value.code == cd.RESULT_INVALID_USAGE
    wide, _ = _moves(9, 1)
    with pytest.raises(cd.CudecompError) as e:
        cd.cudecompExtDescribeWallFieldMoves(wide, fields, cd.DOUBLE, raw)
    assert e.value.code == cd.RESULT_INVALID_USAGE
    plain = cd.make_move((4, 2, 2), (1, 6, 20), (1, 6, 20), 0, 100, 0, 0)
    with pytest.raises(cd.CudecompError) as e:
        cd.cudecompExtDescribeWallFieldMoves([plain], fields, cd.DOUBLE, raw)
    assert e.value.code == cd.RESULT_INVALID_USAGE
