"""Multi-field halo updates (cudecomp_halo_fields.h: cudecompAmdUpdateFieldHalos{X,Y,Z}) without a GPU: the C interface (symbols,
prototypes against the ctypes argtypes, the header as C11 and C++17), the refusals through the C ABI, the properties of the
stateless plan (cudecompExtPlanHaloFields) against the single-field plan over random decompositions, the plan executed with numpy
and a real exchange over gloo on four ranks, and the classifier of the field-move kernels (cudecompExtDescribeFieldMoves)."""
import ctypes as C
import itertools
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402
from tests.mp import run_ranks  # noqa: E402
from tests.test_plan_sim import _cells, decompositions, small3  # noqa: E402

HEADER = "cudecomp_halo_fields.h"
NAMES = ["cudecompAmdUpdateFieldHalos" + a for a in "XYZ"]
EXT = ["cudecompExtPlanHaloFields", "cudecompExtRunFieldMoves", "cudecompExtDescribeFieldMoves", "cudecompExtDataLaunchCount"]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def _prototypes(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_three_symbols_are_declared_and_exported():
    assert cd.AMD_FIELDS_SYMBOLS == NAMES and cd.MAX_HALO_FIELDS == 32
    assert sorted(_prototypes(HEADER)) == sorted(NAMES)
    L = cd.lib()
    for name in NAMES + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp.h"' in text and re.search(r"#define\s+CUDECOMP_AMD_MAX_HALO_FIELDS\s+32\b", text)
    # the header's name keeps it out of the family tests/test_abi.py counts, and the package's table of that family is as it was
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS
    assert not any("Field" in n for names in cd.AMD_HEADER_SYMBOLS.values() for n in names)


def test_prototypes_agree_with_the_argtypes():
    """the update's prototype with (inputs, n_fields) in the place of `input`: as many parameters as argtypes, pointers at the
    same positions, everything else a 32-bit integer on both sides"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    update = _prototypes("cudecomp.h")
    for name in NAMES:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 11, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 4, 6, 7, 9, 10]
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        assert params[2:4] == ["void* const inputs[]", "int32_t n_fields"]
        assert params[:2] + params[4:] == update[name.replace("AmdUpdateFieldHalos", "UpdateHalos")][:2] + \
            update[name.replace("AmdUpdateFieldHalos", "UpdateHalos")][3:]


@pytest.mark.parametrize("language", ["c11", "c++17"])
def test_header_compiles(language):
    """tests/native/halo_fields_header.c: alone and after the other extension headers (two orders), -Wall -Wextra -Werror, every
    function assigned to a hand-written prototype -- and the compile line does notice a prototype that differs"""
    cc = "gcc" if language == "c11" else "g++"
    if shutil.which(cc) is None:
        pytest.skip("no " + cc)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = [cc, "-std=" + language, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")] + (["-x", "c++"] if language != "c11" else [])
    source = os.path.join(ROOT, "tests", "native", "halo_fields_header.c")
    others = ["cudecomp_amd.h", "cudecomp_amd_fill.h", "cudecomp_amd_accumulate_clear.h", "cudecomp_amd_reflect.h", "cudecomp_halo_fold.h"]
    for order in (None, others, others[::-1]):
        defs = [] if order is None else ['-DBEFORE%d="%s"' % (i + 1, h) for i, h in enumerate(order)]
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (order, res.stderr[-3000:])
    # ... and before them
    res = subprocess.run(base + ["-x", "c" if language == "c11" else "c++", "-"], capture_output=True, text=True,
                         input='#include "%s"\n' % HEADER + "".join('#include "%s"\n' % h for h in others) + "int main(void) { return 0; }\n")
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]
    text = open(source).read()
    broken = text.replace("void* const inputs[], int32_t n_fields", "void* inputs, int32_t n_fields")
    assert broken != text
    res = subprocess.run(base + ["-x", "c" if language == "c11" else "c++", "-"], input=broken, capture_output=True, text=True)
    assert res.returncode != 0 and ("incompatible" in res.stderr or "invalid conversion" in res.stderr), res.stderr[-3000:]


# ---- refusals through the C ABI ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def descriptor():
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((12, 10, 8), (1, 1)))
    yield h, gd
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def _call(h, gd, axis, ptrs, n, halo=(1, 1, 1), dim=0, work=0x1000):
    fn = getattr(cd.lib(), NAMES[axis])
    arr = None if ptrs is None else (C.c_void_p * max(1, len(ptrs)))(*ptrs)
    return fn(h, gd, arr, n, work, cd.DOUBLE, (C.c_int32 * 3)(*halo), (C.c_bool * 3)(True, True, True), dim, None, None)


def test_refusals(descriptor, capfd):
    """all found on the host, before anything is launched (the pointers are not device memory, and there is no device here):
    INVALID_USAGE with the update's message format"""
    h, gd = descriptor
    fake = [0x10000 * (i + 1) for i in range(33)]
    cases = [("inputs argument cannot be null", None, 3), ("n_fields argument out of range", fake[:3], 0),
             ("n_fields argument out of range", fake[:3], -1), ("n_fields argument out of range", fake, 33),
             ("inputs argument cannot hold a null entry", [fake[0], None, fake[2]], 3),
             ("inputs argument cannot hold the same field twice", [fake[0], fake[1], fake[0]], 3)]
    capfd.readouterr()
    for axis in range(3):
        for message, ptrs, n in cases:
            assert _call(h, gd, axis, ptrs, n) == cd.RESULT_INVALID_USAGE, (axis, message)
            err = capfd.readouterr().err
            assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(%s\)" % re.escape(message), err), (message, err)
        # the update says the same kind of thing about its `input`
        fn = getattr(cd.lib(), "cudecompUpdateHalos" + "XYZ"[axis])
        assert fn(h, gd, None, 0x1000, cd.DOUBLE, (C.c_int32 * 3)(1, 1, 1), None, 0, None, None) == cd.RESULT_INVALID_USAGE
        assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(input argument cannot be null\)", capfd.readouterr().err)
        # the list is checked where the update checks `input`: after halo_extents, before work and dim
        assert _call(h, gd, axis, None, 3, halo=(0, 0, 0)) == cd.RESULT_SUCCESS
        assert _call(h, gd, axis, None, 3, work=None, dim=7) == cd.RESULT_INVALID_USAGE
        assert "inputs argument cannot be null" in capfd.readouterr().err
        assert _call(h, gd, axis, fake[:3], 3, work=None) == cd.RESULT_INVALID_USAGE
        assert "work argument cannot be null" in capfd.readouterr().err
        assert _call(h, gd, axis, fake[:3], 3, dim=3) == cd.RESULT_INVALID_USAGE
        assert "dim argument out of range" in capfd.readouterr().err
        # 32 fields, nothing to do along this dim: succeeds without a device
        assert _call(h, gd, axis, fake[:32], 32, halo=(1, 0, 1), dim=1) == cd.RESULT_SUCCESS
        assert capfd.readouterr().err == ""


# ---- plan properties ---------------------------------------------------------------------------------------------------------
def _plans(spec, nranks, axis, halo, periods, dim, padding, n, force_packed):
    return [cd.cudecompExtPlanHaloFields(spec, r, axis, halo, periods, dim, padding, n, force_packed) for r in range(nranks)]


@settings(max_examples=150, deadline=None, suppress_health_check=list(HealthCheck))
@given(d=decompositions(), axis=st.integers(0, 2), dim=st.integers(0, 2), halo=small3,
       periods=st.tuples(st.booleans(), st.booleans(), st.booleans()), padding=small3, force_packed=st.booleans())
def test_fields_plans_random_decompositions(d, axis, dim, halo, periods, padding, force_packed):
    spec = cd.make_grid_spec(d["gdims"], d["pdims"], d["mem_order"], d["gdims_dist"], d["col_major"])
    nranks = d["pdims"][0] * d["pdims"][1]
    try:
        singles = [cd.cudecompExtPlanHalo(spec, r, axis, halo, periods, dim, padding, True) for r in range(nranks)]
    except cd.CudecompError as e:  # the refusals are the update's
        for n in (1, 2, 32):
            with pytest.raises(cd.CudecompError) as info:
                _plans(spec, nranks, axis, halo, periods, dim, padding, n, True)
            assert info.value.code == e.code
        return
    plain = [cd.cudecompExtPlanHalo(spec, r, axis, halo, periods, dim, padding, force_packed) for r in range(nranks)]
    for n in (1, 2, 3, 9, 32):
        plans = _plans(spec, nranks, axis, halo, periods, dim, padding, n, force_packed)
        for r, fp in enumerate(plans):
            sp = plain[r] if n == 1 else singles[r]  # one field: the single plan with the caller's force_packed, unchanged
            ws = cd.cudecompExtWorkspaceSizes(spec, r, axis, halo)[1]
            assert (fp.kind, list(fp.neighbor), fp.comm_axis, fp.n_fields) == (sp.kind, list(sp.neighbor), sp.comm_axis, n)
            assert n == 1 or fp.kind != 3
            assert (fp.n_pre, fp.n_post) == (sp.n_pre, sp.n_post) and (fp.kind == 0 or fp.face_elements == sp.face_elements)
            if fp.kind in (0, 3):
                continue
            face = fp.face_elements
            if fp.kind == 1:  # the two wrap copies, pencil to pencil: the single plan's moves
                for i in range(fp.n_pre):
                    assert bytes(fp.pre[i]) == bytes(sp.pre[i])
                continue
            # packed: per field, the pencil cells read and written are exactly those of the single plan
            A = fp.slot_elements
            assert A % 64 == 0 and n * face <= A < n * face + 64 and 4 * A <= max(n * ws, 1)
            assert list(fp.send_off) == [0, A] and list(fp.recv_off) == [2 * A, 3 * A]
            taken = np.zeros(4 * A, dtype=np.int32)
            for i in range(fp.n_pre):
                a, b = fp.pre[i], sp.pre[i]
                assert (a.src_buf, a.dst_buf, a.peer, a.row_pitch) == (0, 2, b.peer, 0)
                assert np.array_equal(_cells(a, "src_off", "ss"), _cells(b, "src_off", "ss"))
                piece = _cells(a, "dst_off", "ds")
                assert np.array_equal(np.sort(piece), fp.send_off[a.peer] + np.arange(face))  # field 0's piece: dense, at the slot's start
                for f in range(n):
                    taken[piece + f * face] += 1
            for i in range(fp.n_post):
                a, b = fp.post[i], sp.post[i]
                assert (a.src_buf, a.dst_buf, a.peer, a.row_pitch) == (2, 0, b.peer, 0)
                assert np.array_equal(_cells(a, "dst_off", "ds"), _cells(b, "dst_off", "ds"))
                piece = _cells(a, "src_off", "ss")
                assert np.array_equal(np.sort(piece), fp.recv_off[a.peer] + np.arange(face))
                # ... in the order the sender packed it: the same dense strides on both ends
                assert list(a.ss) == list(sp.post[i].ss) and list(a.extent) == list(sp.post[i].extent)
                for f in range(n):
                    taken[piece + f * face] += 1
            assert taken.max() <= 1  # the pieces of different fields and sides are disjoint, all below n x the workspace size
            # a rank and both its neighbours agree on the slot size and the offsets (what the one-sided transport relies on)
            for i in range(2):
                nb = fp.neighbor[i]
                if nb < 0:
                    continue
                q = plans[nb]
                assert q.kind == 2 and q.neighbor[1 - i] == r and q.face_elements == face and q.slot_elements == A
                assert list(q.send_off) == list(fp.send_off) and list(q.recv_off) == list(fp.recv_off)


def test_n_fields_below_one_is_refused():
    spec = cd.make_grid_spec((8, 8, 8), (1, 1), ((0, 1, 2),) * 3)
    for n in (0, -1):
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtPlanHaloFields(spec, 0, 0, (1, 1, 1), (1, 1, 1), 0, None, n)
        assert info.value.code == cd.RESULT_INVALID_USAGE


# ---- plan execution over gloo --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdims", [(2, 2), (1, 4)], ids=lambda p: "P%dx%d" % p)
def test_fields_plan_over_gloo(pdims):
    args = {"gdims": (13, 10, 11), "pdims": pdims, "halos": [(1, 1, 1), (2, 1, 3)], "padding": (0, 1, 0),
            "periods": [(1, 1, 1), (1, 0, 1)], "n_fields": [1, 2, 3, 9]}
    for failures in run_ranks(4, "tests.fields_bodies", "plan_fields_gloo", args):
        assert failures == []


# ---- classifier ----------------------------------------------------------------------------------------------------------------
def _describe(extent, ss, ds, bases, es, work=1 << 30, stride=None, force=0, src_buf=0, dst_buf=2, n_moves=1):
    face = int(np.prod(extent))
    moves = [cd.make_move(extent, ss, ds, src_off=0, dst_off=i * 4 * face * len(bases), src_buf=src_buf, dst_buf=dst_buf) for i in range(n_moves)]
    return cd.cudecompExtDescribeFieldMoves(moves, bases, work, face if stride is None else stride, es, force)


def test_two_byte_lanes_follow_every_field():
    extent, ss, ds = (64, 5, 3), (1, 66, 66 * 5 + 6), (1, 64, 320)
    aligned = [1 << 20, 2 << 20, 3 << 20]
    d = _describe(extent, ss, ds, aligned, 2)
    assert (d["kind"], d["vec"], d["access"]) == (22, 16, 0)
    for odd in range(3):  # ONE of three bases at 2 mod 4: the whole launch on 2-byte lanes
        bases = list(aligned)
        bases[odd] += 2
        d = _describe(extent, ss, ds, bases, 2)
        assert (d["kind"], d["vec"]) == (22, 2), (odd, d)
        assert _describe(extent, ss, ds, bases, 4)["vec"] == 16  # (wider elements need only their own alignment)
    # an odd workspace step between the fields' pieces does the same
    assert _describe(extent, ss, ds, aligned, 2, stride=961)["vec"] == 2
    # total workgroups = n_fields x the per-field count, for one and two sides
    for n_moves, n in itertools.product((1, 2), (1, 2, 3, 9, 32)):
        d = _describe(extent, ss, ds, [(i + 1) << 20 for i in range(n)], 2, n_moves=n_moves)
        one = _describe(extent, ss, ds, [1 << 20], 2)
        assert d["blocks_per_field"] == n_moves * one["blocks"] and d["blocks"] == n * d["blocks_per_field"], (n_moves, n, d)


def test_faces_one_element_thick_take_the_element_wise_kernel():
    for es, (h, d_) in itertools.product((2, 4, 8, 16), ((9, 7), (300, 1), (1, 40))):
        d = _describe((1, h, d_), (1, 13, 13 * (h + 2)), (1, 1, h), [1 << 20, 2 << 20, 3 << 20], es)
        assert (d["kind"], d["vec"], d["access"]) == (23, es, 0), (es, h, d_, d)
        assert d["blocks"] == 3 * d["blocks_per_field"]
    # forced
    assert _describe((64, 5, 3), (1, 66, 400), (1, 64, 320), [1 << 20, 2 << 20], 8, force=1)["kind"] == 23
    # nothing to launch
    assert _describe((0, 5, 3), (1, 66, 400), (1, 64, 320), [1 << 20, 2 << 20], 8)["kind"] == -1


def test_access_mode_by_the_size_of_one_field_move():
    """cached below 32 MiB PER FIELD MOVE, non-temporal from there -- whatever the number of fields; the element-wise kernel
    always cached"""
    bases = [(i + 1) << 32 for i in range(9)]
    for es in (2, 4, 8, 16):
        n = (32 << 20) // es
        for extent, ss, ds in (((n, 1, 1), (1, 0, 0), (1, 0, 0)), ((n // 4096, 4096, 1), (1, n // 4096 + 8, 0), (1, n // 4096, 0))):
            d = _describe(extent, ss, ds, bases, es, work=1 << 40)
            assert (d["kind"], d["access"]) == (22, 1), (es, extent, d)
            assert _describe(extent, ss, ds, bases, es, work=1 << 40, force=4)["access"] == 0
            assert _describe(extent, ss, ds, bases, es, work=1 << 40, force=1)["access"] == 0
        d = _describe((n - 1, 1, 1), (1, 0, 0), (1, 0, 0), bases, es, work=1 << 40)
        assert (d["kind"], d["access"]) == (22, 0), (es, d)
        assert _describe((n - 1, 1, 1), (1, 0, 0), (1, 0, 0), bases, es, work=1 << 40, force=2)["access"] == 1


def test_moves_that_are_no_plain_copies_are_internal_errors():
    m = cd.make_move((8, 4, 2), (1, 8, 32), (1, 8, 32), src_buf=0, dst_buf=2, row_pitch=8)
    with pytest.raises(cd.CudecompError) as info:
        cd.cudecompExtDescribeFieldMoves([m], [1 << 20, 2 << 20], 1 << 30, 64, 8)
    assert info.value.code == cd.RESULT_INTERNAL_ERROR
    m = cd.make_move((8, 4, 2), (1, 8, 32), (1, 8, 32), src_buf=0, dst_buf=2)
    with pytest.raises(cd.CudecompError) as info:  # a workspace end without a workspace
        cd.cudecompExtDescribeFieldMoves([m], [1 << 20, 2 << 20], 0, 64, 8)
    assert info.value.code == cd.RESULT_INTERNAL_ERROR
    for n in (0, 33):
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtDescribeFieldMoves([m], [1 << 20] * n, 1 << 30, 64, 8)
        assert info.value.code == cd.RESULT_INVALID_USAGE


def test_the_documents_name_the_kernels_and_say_what_is_unmeasured():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`rows_fields_kernel<VB,STREAM>`" in design and "`generic_fields_kernel<ES>`" in design
    para = [p for p in design.split("\n\n") if "Field-moves" in p]
    assert para and any("unmeasured" in p or "not measured" in p or "nobody has measured" in p.lower() for p in para)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "cudecompAmdUpdateFieldHalos" in integration and "Not covered" in integration


# ---- the launch of two sides that DIFFER, pinned -------------------------------------------------------------------------------
PINS = os.path.join(ROOT, "tests", "golden", "field_launch_pins.json")
PENCIL = (1, 66, 66 * 11 + 6)  # strides of the sides inside a field's pencil
ROW, SHORT, THIN, NONE = (64, 5, 3), (6, 5, 3), (1, 9, 7), (0, 5, 3)


def _pairs(es):
    """(name, [(extent, pencil strides, pencil offset) per side]): what the cases above never give one launch"""
    big = ((32 << 20) // es, 1, 1)
    return [("lanes differ", [(ROW, PENCIL, 0), (SHORT, PENCIL, 4000)]), ("lanes differ, narrow first", [(SHORT, PENCIL, 0), (ROW, PENCIL, 4000)]),
            ("rows with a thin face", [(ROW, PENCIL, 0), (THIN, PENCIL, 4000)]), ("thin faces", [(THIN, PENCIL, 0), ((1, 40, 1), PENCIL, 4000)]),
            ("one side at an odd offset", [(ROW, PENCIL, 0), (ROW, PENCIL, 4001)]), ("one side empty", [(NONE, PENCIL, 0), (ROW, PENCIL, 4000)]),
            ("both sides empty", [(NONE, PENCIL, 0), (NONE, PENCIL, 4000)]), ("large with small", [(ROW, PENCIL, 0), (big, (1, 0, 0), 4000)]),
            ("just below large with small", [((big[0] - 1, 1, 1), (1, 0, 0), 0), (ROW, PENCIL, 1 << 26)]),
            ("one workgroup per plane", [((2, 3, 1 << 25), (1, 5, 17), 0), ((2, 3, 1 << 25), (1, 5, 17), 1 << 30)])]


def _pin_cases():
    """element size x side pair x direction x force, the field count and the workspace stride (the faces' size, or the next odd
    number above it) drawn with a fixed seed: 480 cases"""
    rng = np.random.RandomState(2223)
    for es, direction, force in itertools.product((2, 4, 8, 16), ("field to work", "work to field", "field to field"), (0, 1, 2, 4)):
        for name, sides in _pairs(es):
            n, odd = (2, 3, 32)[rng.randint(3)], int(rng.randint(2))
            faces = [int(np.prod(extent)) for extent, _, _ in sides]
            stride = max(faces) if not odd else max(faces) + 1 + max(faces) % 2
            moves = []
            for s, (extent, strides, off) in enumerate(sides):
                dense, slot = (1, extent[0], extent[0] * extent[1]), s * (n * stride + 6)
                if direction == "field to work":
                    moves.append(cd.make_move(extent, strides, dense, src_off=off, dst_off=slot, src_buf=0, dst_buf=2))
                elif direction == "work to field":
                    moves.append(cd.make_move(extent, dense, strides, src_off=slot, dst_off=off, src_buf=2, dst_buf=0))
                else:
                    moves.append(cd.make_move(extent, strides, strides, src_off=off, dst_off=off + 2000, src_buf=0, dst_buf=1))
            key = "es %d, %s, %s, force %d, %d fields, stride %d" % (es, name, direction, force, n, stride)
            yield key, moves, [(f + 1) << 36 for f in range(n)], stride, es, force


def field_launches():
    table = {}
    for key, moves, bases, stride, es, force in _pin_cases():
        try:
            d = cd.cudecompExtDescribeFieldMoves(moves, bases, 1 << 44, stride, es, force)
            table[key] = [d[k] for k in ("kind", "vec", "access", "blocks_per_field", "blocks")]
        except cd.CudecompError as e:
            table[key] = {"error": e.code}
    return table


def test_launches_of_differing_sides_are_the_pinned_ones():
    """tests/golden/field_launch_pins.json: [kind, lane bytes, access, workgroups per field, workgroups] (or the error code) of the
    ONE launch cudecompExtDescribeFieldMoves answers for two sides that differ in lane width, in kernel, in alignment, in size, or
    of which one or both are empty.  Recorded from the two-sided planner this path had before it moved onto the list planner; a
    mismatch is a finding about the planner's one-choice mode, not a reason to regenerate (python tests/test_halo_fields_plan.py
    --regen rewrites the file from whatever library is built)."""
    with open(PINS) as f:
        pinned = json.load(f)
    now = field_launches()
    assert sorted(now) == sorted(pinned) and len(now) == 480
    diffs = ["%s: pinned %s, now %s" % (k, pinned[k], now[k]) for k in sorted(now) if now[k] != pinned[k]]
    assert not diffs, "field launches differ from tests/golden/field_launch_pins.json:\n" + "\n".join(diffs[:40])
    # a few readable facts of the table
    rows = {k: v for k, v in pinned.items() if ", force 0," in k or ", force 4," in k}
    assert all(v[:2] == [22, 8] for k, v in rows.items() if "es 4, lanes differ" in k)
    assert all(v[:3] == [23, 8, 0] for k, v in rows.items() if "es 8, rows with a thin face" in k)
    assert all(v[:2] == [22, 2] for k, v in rows.items() if "es 2, one side at an odd offset" in k)
    assert all(v[0] == -1 for k, v in pinned.items() if "both sides empty" in k)
    assert all(v[2] == (0 if ", force 4," in k else 1) for k, v in rows.items() if ", large with small" in k)
    assert all(v == {"error": cd.RESULT_NOT_SUPPORTED} for k, v in rows.items() if "one workgroup per plane" in k and "32 fields" in k)
    assert all(v[4] == v[3] * 3 == 3 << 26 for k, v in rows.items() if "one workgroup per plane" in k and " 3 fields" in k)


if __name__ == "__main__" and "--regen" in sys.argv:
    with open(PINS, "w") as f:
        table = field_launches()
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)) + "\n}\n")
    print("wrote", PINS)


def test_arguments_are_checked_in_the_stated_order(capfd):
    from tests import halo_check_order
    halo_check_order.check("fields", capfd)
