"""Multi-field halo accumulation (cudecomp_halo_accumulate_fields.h: cudecompAmdAccumulateFieldHalos{X,Y,Z}) without a GPU: the C
interface (symbols, prototypes against the ctypes argtypes, the header as C11 and C++17), the refusals through the C ABI, the
properties of the stateless plan (cudecompExtPlanHaloAccumulateFields) against the single accumulation plans over random
decompositions, the plan executed with numpy and a real exchange over gloo on four ranks, and the classifier of the adding and
taking field-move kernels (cudecompExtDescribeFieldMovesOp)."""
import ctypes as C
import itertools
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

HEADER = "cudecomp_halo_accumulate_fields.h"
NAMES = ["cudecompAmdAccumulateFieldHalos" + a for a in "XYZ"]
EXT = ["cudecompExtPlanHaloAccumulateFields", "cudecompExtRunFieldMovesOp", "cudecompExtDescribeFieldMovesOp"]
COPY, ADD, TAKE, ADD_TAKE = cd.MOVES_COPY, cd.MOVES_ADD, cd.MOVES_TAKE, cd.MOVES_ADD_TAKE
ARITH = {cd.HALF: "_Float16", cd.HALF_COMPLEX: "_Float16", cd.BFLOAT16: "__bf16", cd.FLOAT: "float", cd.FLOAT_COMPLEX: "float",
         cd.DOUBLE: "double", cd.DOUBLE_COMPLEX: "double"}
ES = {cd.HALF: 2, cd.BFLOAT16: 2, cd.HALF_COMPLEX: 4, cd.FLOAT: 4, cd.FLOAT_COMPLEX: 8, cd.DOUBLE: 8, cd.DOUBLE_COMPLEX: 16}
NC = {cd.HALF: 1, cd.BFLOAT16: 1, cd.HALF_COMPLEX: 2, cd.FLOAT: 1, cd.FLOAT_COMPLEX: 2, cd.DOUBLE: 1, cd.DOUBLE_COMPLEX: 2}


def spell(d, es, dtype):
    """the template spelling of what cudecompExtDescribeFieldMovesOp answers (csrc/kernels.cc spellKernelName)"""
    k = d["kind"]
    if k in (25, 29):
        return "rows_fields_accumulate_kernel<%s,%d,%d,%s>" % (ARITH[dtype], d["vec"], d["access"], "true" if k == 29 else "false")
    if k in (26, 30):
        return "generic_fields_accumulate_kernel<%s,%d,%s>" % (ARITH[dtype], NC[dtype], "true" if k == 30 else "false")
    if k == 27:
        return "rows_fields_take_kernel<%d,%d>" % (d["vec"], d["access"])
    if k == 28:
        return "generic_fields_take_kernel<%d>" % es
    return "rows_fields_kernel<%d,%d>" % (d["vec"], d["access"]) if k == 22 else "generic_fields_kernel<%d>" % es


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def _prototypes(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_three_symbols_are_declared_and_exported():
    assert cd.AMD_ACCUMULATE_FIELDS_SYMBOLS == NAMES and cd.MAX_HALO_ACCUMULATE_FIELDS == 32
    assert sorted(_prototypes(HEADER)) == sorted(NAMES)
    L = cd.lib()
    for name in NAMES + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp.h"' in text and re.search(r"#define\s+CUDECOMP_AMD_MAX_HALO_ACCUMULATE_FIELDS\s+32\b", text)
    # the header's name keeps it out of the family tests/test_abi.py counts, and the package's table of that family is as it was
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS
    assert not any("Field" in n for names in cd.AMD_HEADER_SYMBOLS.values() for n in names)
    # the multi-field update keeps its own list
    assert cd.AMD_FIELDS_SYMBOLS == ["cudecompAmdUpdateFieldHalos" + a for a in "XYZ"]


def test_prototypes_agree_with_the_argtypes():
    """the multi-field update's prototype with `clear` before the stream: as many parameters as argtypes, pointers at the same
    positions, everything else a 32-bit integer on both sides"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    update = _prototypes("cudecomp_halo_fields.h")
    for name in NAMES:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 12, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 4, 6, 7, 9, 11]
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        assert params[10] == "int32_t clear"
        assert params[:10] + params[11:] == update[name.replace("AccumulateFieldHalos", "UpdateFieldHalos")]
    ext = _prototypes("cudecomp_ext.h")
    for new, old in (("cudecompExtRunFieldMovesOp", "cudecompExtRunFieldMoves"), ("cudecompExtDescribeFieldMovesOp", "cudecompExtDescribeFieldMoves")):
        assert ext[new][:8] + ext[new][10:] == ext[old] and ext[new][8:10] == ["int32_t mode", "cudecompDataType_t dtype"]
        assert len(getattr(L, new).argtypes) == len(ext[new])


@pytest.mark.parametrize("language", ["c11", "c++17"])
def test_header_compiles(language):
    """tests/native/halo_accumulate_fields_header.c: alone and after the other extension headers (two orders), -Wall -Wextra
    -Werror, every function assigned to a hand-written prototype -- and the compile line does notice a prototype that differs"""
    cc = "gcc" if language == "c11" else "g++"
    if shutil.which(cc) is None:
        pytest.skip("no " + cc)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = [cc, "-std=" + language, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")] + (["-x", "c++"] if language != "c11" else [])
    source = os.path.join(ROOT, "tests", "native", "halo_accumulate_fields_header.c")
    others = ["cudecomp_amd.h", "cudecomp_amd_fill.h", "cudecomp_amd_accumulate_clear.h", "cudecomp_amd_reflect.h", "cudecomp_halo_fold.h",
              "cudecomp_halo_fields.h", "cudecomp_transpose_fields.h"]
    for order in (None, others, others[::-1]):
        defs = [] if order is None else ['-DBEFORE%d="%s"' % (i + 1, h) for i, h in enumerate(order)]
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (order, res.stderr[-3000:])
    # ... and before them
    res = subprocess.run(base + ["-x", "c" if language == "c11" else "c++", "-"], capture_output=True, text=True,
                         input='#include "%s"\n' % HEADER + "".join('#include "%s"\n' % h for h in others) + "int main(void) { return 0; }\n")
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]
    text = open(source).read()
    broken = text.replace("int32_t clear, hipStream_t stream", "hipStream_t stream, int32_t clear")
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


def _call(h, gd, axis, ptrs, n, halo=(1, 1, 1), dim=0, work=0x1000, clear=0, periods=(True, True, True)):
    fn = getattr(cd.lib(), NAMES[axis])
    arr = None if ptrs is None else (C.c_void_p * max(1, len(ptrs)))(*ptrs)
    return fn(h, gd, arr, n, work, cd.DOUBLE, (C.c_int32 * 3)(*halo), (C.c_bool * 3)(*periods), dim, None, clear, None)


def test_refusals(descriptor, capfd):
    """all found on the host, before anything is launched (the pointers are not device memory, and there is no device here):
    INVALID_USAGE with the accumulation's message format"""
    h, gd = descriptor
    fake = [0x10000 * (i + 1) for i in range(33)]
    cases = [("inputs argument cannot be null", None, 3), ("n_fields argument out of range", fake[:3], 0),
             ("n_fields argument out of range", fake[:3], -1), ("n_fields argument out of range", fake, 33),
             ("inputs argument cannot hold a null entry", [fake[0], None, fake[2]], 3),
             ("inputs argument cannot hold the same field twice", [fake[0], fake[1], fake[0]], 3)]
    capfd.readouterr()
    for axis in range(3):
        for (message, ptrs, n), clear in itertools.product(cases, (0, 1)):
            assert _call(h, gd, axis, ptrs, n, clear=clear) == cd.RESULT_INVALID_USAGE, (axis, message)
            err = capfd.readouterr().err
            assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(%s\)" % re.escape(message), err), (message, err)
        # the accumulation says the same kind of thing about its `input`
        fn = getattr(cd.lib(), "cudecompAmdAccumulateHalos" + "XYZ"[axis])
        assert fn(h, gd, None, 0x1000, cd.DOUBLE, (C.c_int32 * 3)(1, 1, 1), None, 0, None, None) == cd.RESULT_INVALID_USAGE
        assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(input argument cannot be null\)", capfd.readouterr().err)
        # any other value of clear, also when there is nothing to do
        for clear, halo in itertools.product((2, -1, 256), ((1, 1, 1), (0, 0, 0))):
            assert _call(h, gd, axis, fake[:3], 3, halo=halo, clear=clear) == cd.RESULT_INVALID_USAGE
            assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(clear argument must be 0 or 1\)", capfd.readouterr().err)
        # the list is checked where the accumulation checks `input`: after halo_extents, before work and dim
        assert _call(h, gd, axis, None, 3, halo=(0, 0, 0)) == cd.RESULT_SUCCESS
        assert _call(h, gd, axis, None, 3, work=None, dim=7) == cd.RESULT_INVALID_USAGE
        assert "inputs argument cannot be null" in capfd.readouterr().err
        assert _call(h, gd, axis, fake[:3], 3, work=None) == cd.RESULT_INVALID_USAGE
        assert "work argument cannot be null" in capfd.readouterr().err
        assert _call(h, gd, axis, fake[:3], 3, dim=3) == cd.RESULT_INVALID_USAGE
        assert "dim argument out of range" in capfd.readouterr().err
        # 32 fields, nothing to do along this dim: succeeds without a device
        for clear in (0, 1):
            assert _call(h, gd, axis, fake[:32], 32, halo=(1, 0, 1), dim=1, clear=clear) == cd.RESULT_SUCCESS
            assert capfd.readouterr().err == ""
        # wide halos are refused as the accumulation refuses them, for one field and for several (extents 12, 10, 8)
        single = getattr(cd.lib(), "cudecompAmdAccumulateHalos" + "XYZ"[axis])
        rc = single(h, gd, fake[0], 0x1000, cd.DOUBLE, (C.c_int32 * 3)(1, 1, 9), (C.c_bool * 3)(True, True, True), 2, None, None)
        message = re.search(r"CUDECOMP:ERROR: .*\((.*)\)", capfd.readouterr().err).group(1)
        assert rc == cd.RESULT_INVALID_USAGE and "halo wider" in message
        for n in (1, 3):
            assert _call(h, gd, axis, fake[:n], n, halo=(1, 1, 9), dim=2) == rc
            assert message in capfd.readouterr().err


def test_empty_pencils_are_refused_as_the_accumulation_refuses_them(capfd):
    spec = cd.make_grid_spec((2, 8, 8), (4, 1), ((0, 1, 2),) * 3)
    for planner, more in ((cd.cudecompExtPlanHaloAccumulate, ()), (cd.cudecompExtPlanHaloAccumulateFields, (None, 3, True))):
        with pytest.raises(cd.CudecompError) as info:
            planner(spec, 0, 1, (1, 1, 1), (1, 1, 1), 0, *more)
        assert info.value.code == cd.RESULT_NOT_SUPPORTED
    capfd.readouterr()


# ---- plan properties ---------------------------------------------------------------------------------------------------------
def _plans(spec, nranks, axis, halo, periods, dim, padding, n, clear):
    return [cd.cudecompExtPlanHaloAccumulateFields(spec, r, axis, halo, periods, dim, padding, n, clear) for r in range(nranks)]


def test_plans_random_decompositions():
    """for every rank of random decompositions: the moves of the single accumulation plan with the workspace offsets re-laid, equal
    `ordered`, add and take flags, slots disjoint and within n x the queried size, both ends of every exchange agreeing; a draw the
    single planner refuses is refused identically.  At least half of the draws must be accepted."""
    counts = {"drawn": 0, "accepted": 0}

    @settings(max_examples=150, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
    @given(d=decompositions(), axis=st.integers(0, 2), dim=st.integers(0, 2), halo=small3,
           periods=st.tuples(st.booleans(), st.booleans(), st.booleans()), padding=small3, clear=st.booleans())
    def check(d, axis, dim, halo, periods, padding, clear):
        counts["drawn"] += 1
        spec = cd.make_grid_spec(d["gdims"], d["pdims"], d["mem_order"], d["gdims_dist"], d["col_major"])
        nranks = d["pdims"][0] * d["pdims"][1]
        single_planner = cd.cudecompExtPlanHaloAccumulateClear if clear else cd.cudecompExtPlanHaloAccumulate
        refusals = []
        for r in range(nranks):  # (a wide halo concerns some ranks only: rank by rank)
            try:
                single_planner(spec, r, axis, halo, periods, dim, padding, True)
                refusals.append(0)
            except cd.CudecompError as e:
                refusals.append(e.code)
            for n in (1, 2, 32):
                try:
                    cd.cudecompExtPlanHaloAccumulateFields(spec, r, axis, halo, periods, dim, padding, n, clear)
                    code = 0
                except cd.CudecompError as e:
                    code = e.code
                assert code == refusals[r], (r, n, code, refusals[r])
        if any(refusals):
            return
        counts["accepted"] += 1
        singles = [single_planner(spec, r, axis, halo, periods, dim, padding, True) for r in range(nranks)]
        for n in (1, 2, 3, 9, 32):
            plans = _plans(spec, nranks, axis, halo, periods, dim, padding, n, clear)
            for r, fp in enumerate(plans):
                sp = singles[r]
                ws = cd.cudecompExtWorkspaceSizes(spec, r, axis, halo)[1]
                assert (fp.kind, list(fp.neighbor), fp.comm_axis, fp.n_fields) == (sp.kind, list(sp.neighbor), sp.comm_axis, n)
                assert fp.kind in (0, 1, 2) and fp.reserved == sp.reserved  # accumulate, ordered, add and take bits
                assert (fp.n_pre, fp.n_post) == (sp.n_pre, sp.n_post) and (fp.kind == 0 or fp.face_elements == sp.face_elements)
                if fp.kind == 0:
                    continue
                assert fp.reserved & 1 and bool(fp.reserved & 512) == clear
                face = fp.face_elements
                if fp.kind == 1 or n == 1:  # pencil to pencil, or one field: the single plan's moves and offsets, unchanged
                    for i in range(fp.n_pre):
                        assert bytes(fp.pre[i]) == bytes(sp.pre[i])
                    for i in range(fp.n_post):
                        assert bytes(fp.post[i]) == bytes(sp.post[i])
                    assert list(fp.send_off) == list(sp.send_off) and list(fp.recv_off) == list(sp.recv_off)
                    if fp.kind == 1:
                        assert fp.reserved // 16 & 3 == 3 and (fp.reserved // 1024 & 3) == (3 if clear else 0)
                    continue
                A = fp.slot_elements
                assert A % 64 == 0 and n * face <= A < n * face + 64 and 4 * A <= max(n * ws, 1)
                assert list(fp.send_off) == [0, A] and list(fp.recv_off) == [2 * A, 3 * A]
                taken = np.zeros(4 * A, dtype=np.int32)
                for i in range(fp.n_pre):
                    a, b = fp.pre[i], sp.pre[i]
                    assert (a.src_buf, a.dst_buf, a.peer, a.row_pitch) == (0, 2, b.peer, 0)
                    assert np.array_equal(_cells(a, "src_off", "ss"), _cells(b, "src_off", "ss"))
                    assert list(a.ds) == list(b.ds) and list(a.extent) == list(b.extent)
                    piece = _cells(a, "dst_off", "ds")
                    assert np.array_equal(np.sort(piece), fp.send_off[a.peer] + np.arange(face))
                    for f in range(n):
                        taken[piece + f * face] += 1
                for i in range(fp.n_post):
                    a, b = fp.post[i], sp.post[i]
                    assert (a.src_buf, a.dst_buf, a.peer, a.row_pitch) == (2, 0, b.peer, 0)
                    assert np.array_equal(_cells(a, "dst_off", "ds"), _cells(b, "dst_off", "ds"))
                    assert list(a.ss) == list(b.ss) and list(a.extent) == list(b.extent)
                    piece = _cells(a, "src_off", "ss")
                    assert np.array_equal(np.sort(piece), fp.recv_off[a.peer] + np.arange(face))
                    for f in range(n):
                        taken[piece + f * face] += 1
                assert taken.max() <= 1  # the pieces of different fields and sides are disjoint, all below n x the workspace size
                for i in range(2):  # both ends of every exchange agree on sizes and offsets
                    nb = fp.neighbor[i]
                    if nb < 0:
                        continue
                    q = plans[nb]
                    assert q.kind == 2 and q.neighbor[1 - i] == r and q.face_elements == face and q.slot_elements == A
                    assert list(q.send_off) == list(fp.send_off) and list(q.recv_off) == list(fp.recv_off)

    check()
    assert counts["drawn"] >= 100 and 2 * counts["accepted"] >= counts["drawn"], counts


def test_bad_counts_and_clear_are_refused_by_the_planner():
    spec = cd.make_grid_spec((8, 8, 8), (1, 1), ((0, 1, 2),) * 3)
    for n, clear in ((0, 0), (-1, 1), (3, 2), (3, -1)):
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtPlanHaloAccumulateFields(spec, 0, 0, (1, 1, 1), (1, 1, 1), 0, None, n, clear)
        assert info.value.code == cd.RESULT_INVALID_USAGE
    # the plan of a self-exchanging rank is packed, an ordinary one self-periodic; halo 3 <= interior 5 < 2 * 3: ordered
    spec = cd.make_grid_spec((5, 8, 8), (1, 1), ((0, 1, 2),) * 3)
    a = cd.cudecompExtPlanHaloAccumulateFields(spec, 0, 0, (3, 1, 1), (1, 1, 1), 0, None, 3, True)
    b = cd.cudecompExtPlanHaloAccumulateFields(spec, 0, 0, (3, 1, 1), (1, 1, 1), 0, None, 3, True, self_exchange=True)
    assert (a.kind, b.kind) == (1, 2) and a.reserved & 2 and b.reserved & 2


# ---- plan execution over gloo --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pdims", [(2, 2), (1, 4)], ids=lambda p: "P%dx%d" % p)
def test_plan_over_gloo(pdims):
    args = {"gdims": (13, 10, 11), "pdims": pdims, "halos": [(1, 1, 1), (2, 1, 3)], "padding": (0, 1, 0),
            "periods": [(1, 1, 1), (1, 0, 1)], "n_fields": [1, 2, 3, 9]}
    for failures in run_ranks(4, "tests.accumulate_fields_bodies", "plan_gloo", args):
        assert failures == []


# ---- classifier ----------------------------------------------------------------------------------------------------------------
OPS = {"add work to field": (ADD, 2, 0), "add field to field": (ADD, 0, 1), "take field to work": (TAKE, 0, 2),
       "add-take field to field": (ADD_TAKE, 0, 1)}
KINDS = {ADD: (25, 26), TAKE: (27, 28), ADD_TAKE: (29, 30), COPY: (22, 23)}


def _describe(extent, pencil, bases, dtype, op, work=1 << 30, stride=None, force=0, n_moves=1):
    mode, src_buf, dst_buf = OPS[op]
    face = int(np.prod(extent))
    dense = (1, extent[0], extent[0] * extent[1])
    ss, ds = (dense if src_buf == 2 else pencil), (dense if dst_buf == 2 else pencil)
    moves = [cd.make_move(extent, ss, ds, src_off=i * 4 * face * len(bases) if src_buf == 2 else 8 * i * face,
                          dst_off=i * 4 * face * len(bases) if dst_buf == 2 else (8 * i + 4) * face, src_buf=src_buf, dst_buf=dst_buf)
             for i in range(n_moves)]
    return cd.cudecompExtDescribeFieldMovesOp(moves, bases, work, face if stride is None else stride, ES[dtype], mode, dtype, force)


def test_kinds_and_names():
    L = cd.lib()
    L.cudecompExtLastKernelName.restype = C.c_char_p
    extent, pencil = (64, 5, 3), (1, 66, 66 * 5 + 6)
    bases = [1 << 20, 2 << 20, 3 << 20]
    for dtype, (op, (mode, _, _)) in itertools.product(ES, OPS.items()):
        d = _describe(extent, pencil, bases, dtype, op)
        assert (d["kind"], d["vec"], d["access"]) == (KINDS[mode][0], 16, 0), (dtype, op, d)
        assert d["blocks"] == 3 * d["blocks_per_field"]
        assert spell(d, ES[dtype], dtype).startswith("rows_fields_take_kernel<16,0>" if mode == TAKE else
                                                     "rows_fields_accumulate_kernel<%s,16,0," % ARITH[dtype])
        d = _describe(extent, pencil, bases, dtype, op, force=1)
        assert (d["kind"], d["vec"], d["access"]) == (KINDS[mode][1], ES[dtype], 0), (dtype, op, d)
        # the copy through the new entry is the copy of the old one
        m = cd.make_move(extent, pencil, (1, 64, 320), src_buf=0, dst_buf=2)
        assert cd.cudecompExtDescribeFieldMovesOp([m], bases, 1 << 30, 960, ES[dtype], COPY, dtype) == \
            cd.cudecompExtDescribeFieldMoves([m], bases, 1 << 30, 960, ES[dtype])
    # nothing to launch
    assert _describe((0, 5, 3), pencil, bases, cd.DOUBLE, "add field to field")["kind"] == -1


def test_lanes_follow_every_field():
    extent, pencil = (64, 5, 3), (1, 66, 66 * 5 + 6)
    aligned = [1 << 20, 2 << 20, 3 << 20]
    for op, (mode, _, _) in OPS.items():
        for dtype in (cd.HALF, cd.BFLOAT16):
            assert _describe(extent, pencil, aligned, dtype, op)["vec"] == 16
            for odd in range(3):  # ONE of three bases at 2 mod 4: the whole launch on 2-byte lanes
                bases = list(aligned)
                bases[odd] += 2
                d = _describe(extent, pencil, bases, dtype, op)
                assert (d["kind"], d["vec"]) == (KINDS[mode][0], 2), (op, odd, d)
                assert _describe(extent, pencil, bases, cd.HALF_COMPLEX, op)["vec"] == 16  # (wider elements: their own alignment)
            if "work" in op:  # an odd workspace step between the fields' pieces does the same, and an odd workspace
                assert _describe(extent, pencil, aligned, dtype, op, stride=961)["vec"] == 2
                assert _describe(extent, pencil, aligned, dtype, op, work=(1 << 30) + 2)["vec"] == 2
        # the row length decides the rest: the widest lanes that divide it, never narrower than one element
        for dtype, length in itertools.product(ES, (1, 2, 3, 4, 6, 8)):
            pitch = 2 * length + 2  # (even strides: 2-byte elements stay dword-aligned from row to row)
            d = _describe((length, 5, 3), (1, pitch, pitch * 5 + 2), aligned, dtype, "add field to field")
            want = 16
            while want > ES[dtype] and (length * ES[dtype]) % want:
                want //= 2
            assert (d["kind"], d["vec"]) == ((25, want) if length > 1 else (26, ES[dtype])), (dtype, length, d)
        # total workgroups = n_fields x the per-field count, for one and two sides
        for n_moves, n in itertools.product((1, 2), (1, 2, 3, 9, 32)):
            d = _describe(extent, pencil, [(i + 1) << 20 for i in range(n)], cd.DOUBLE, op, n_moves=n_moves)
            one = _describe(extent, pencil, [1 << 20], cd.DOUBLE, op)
            assert d["blocks_per_field"] == n_moves * one["blocks"] and d["blocks"] == n * d["blocks_per_field"], (n_moves, n, d)


def test_thin_faces_take_the_element_wise_kinds():
    for dtype, (h, d_), (op, (mode, _, _)) in itertools.product(ES, ((9, 7), (300, 1), (1, 40)), OPS.items()):
        d = _describe((1, h, d_), (1, 13, 13 * (h + 2)), [1 << 20, 2 << 20, 3 << 20], dtype, op)
        assert (d["kind"], d["vec"], d["access"]) == (KINDS[mode][1], ES[dtype], 0), (dtype, h, d_, op, d)
        assert d["blocks"] == 3 * d["blocks_per_field"]
    # rows beside a thin face: one choice, the element-wise kernel
    moves = [cd.make_move((64, 5, 3), (1, 66, 400), (1, 66, 400), 0, 2000, 0, 1), cd.make_move((1, 9, 7), (1, 13, 150), (1, 13, 150), 4000, 6000, 0, 1)]
    d = cd.cudecompExtDescribeFieldMovesOp(moves, [1 << 20, 2 << 20], 0, 0, 8, ADD, cd.DOUBLE)
    assert (d["kind"], d["vec"]) == (26, 8)


def test_access_mode_by_the_size_of_one_field_move():
    """cached below 32 MiB PER FIELD MOVE, non-temporal source loads (take: zero stores too) from there -- whatever the number of
    fields; the element-wise kernels always cached"""
    bases = [(i + 1) << 36 for i in range(9)]
    for dtype, (op, (mode, _, _)) in itertools.product((cd.HALF, cd.FLOAT, cd.DOUBLE, cd.DOUBLE_COMPLEX), OPS.items()):
        n = (32 << 20) // ES[dtype]
        d = _describe((n, 1, 1), (1, 0, 0), bases, dtype, op, work=1 << 44)
        assert (d["kind"], d["access"]) == (KINDS[mode][0], 1), (dtype, op, d)
        assert spell(d, ES[dtype], dtype).split(",")[-1 if mode == TAKE else -2].rstrip(">") == "1"
        assert _describe((n, 1, 1), (1, 0, 0), bases, dtype, op, work=1 << 44, force=4)["access"] == 0
        assert _describe((n, 1, 1), (1, 0, 0), bases, dtype, op, work=1 << 44, force=1)["access"] == 0
        d = _describe((n - 1, 1, 1), (1, 0, 0), bases, dtype, op, work=1 << 44)
        assert (d["kind"], d["access"]) == (KINDS[mode][0], 0), (dtype, op, d)
        assert _describe((n - 1, 1, 1), (1, 0, 0), bases, dtype, op, work=1 << 44, force=2)["access"] == 1


def test_refused_forms_are_internal_errors():
    bases = [1 << 20, 2 << 20]
    geometry = ((8, 4, 2), (1, 8, 32), (1, 8, 32))

    def refused(code, moves, mode, dtype, es=8, work=1 << 30, fields=bases):
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtDescribeFieldMovesOp(moves, fields, work, 64, es, mode, dtype)
        assert info.value.code == code, (info.value.code, code)

    to_work = cd.make_move(*geometry, src_buf=0, dst_buf=2)
    from_work = cd.make_move(*geometry, src_buf=2, dst_buf=0)
    for mode in (ADD, ADD_TAKE):
        refused(cd.RESULT_INTERNAL_ERROR, [to_work], mode, cd.DOUBLE)  # an add whose destination is the workspace
    for mode in (TAKE, ADD_TAKE):
        refused(cd.RESULT_INTERNAL_ERROR, [from_work], mode, cd.DOUBLE)  # a take whose source is the workspace
    for mode in (COPY, ADD, TAKE, ADD_TAKE):  # dst_row_pitch; a workspace end without a workspace
        refused(cd.RESULT_INTERNAL_ERROR, [cd.make_move(*geometry, src_buf=0, dst_buf=1, row_pitch=8)], mode, cd.DOUBLE)
    refused(cd.RESULT_INTERNAL_ERROR, [from_work], ADD, cd.DOUBLE, work=0)
    refused(cd.RESULT_INTERNAL_ERROR, [to_work], TAKE, cd.DOUBLE, work=0)
    # fill, the mirror copies and the folds have no field form; neither has an add whose type does not fit the element size
    for mode in (cd.MOVES_FILL, cd.MOVES_REFLECT, cd.MOVES_REFLECT_NEGATE, cd.MOVES_FOLD, cd.MOVES_FOLD_NEGATE, cd.MOVES_FOLD_TAKE,
                 cd.MOVES_FOLD_NEGATE_TAKE, 11, -1):
        refused(cd.RESULT_INVALID_USAGE, [from_work], mode, cd.DOUBLE)
    refused(cd.RESULT_INVALID_USAGE, [from_work], ADD, cd.FLOAT)
    for n in (0, 33):
        refused(cd.RESULT_INVALID_USAGE, [from_work], ADD, cd.DOUBLE, fields=[1 << 20] * n)
    # the existing pair has no way to ask for an operation, and refuses what it refused
    ext = _prototypes("cudecomp_ext.h")
    assert not any("mode" in p or "dtype" in p for name in ("cudecompExtRunFieldMoves", "cudecompExtDescribeFieldMoves") for p in ext[name])
    with pytest.raises(cd.CudecompError) as info:
        cd.cudecompExtDescribeFieldMoves([cd.make_move(*geometry, src_buf=0, dst_buf=2, row_pitch=8)], bases, 1 << 30, 64, 8)
    assert info.value.code == cd.RESULT_INTERNAL_ERROR


def test_the_code_object_is_the_seventeenth_and_small():
    from tests.test_abi import _code_objects
    sizes = _code_objects(os.path.join(ROOT, "cudecomp_amd", "lib", "libcudecomp.so"))
    assert len(sizes) == 17 and max(sizes) < 400_000, sizes
    makefile = open(os.path.join(ROOT, "cudecomp_amd", "Makefile")).read()
    assert "csrc/kernels_field_accumulate.hip" in makefile


def test_the_documents_name_the_kernels_and_say_what_is_unmeasured():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel in ("`rows_fields_accumulate_kernel<T,VB,STREAM,TAKE>`", "`rows_fields_take_kernel<VB,STREAM>`",
                   "`generic_fields_accumulate_kernel<T,NC,TAKE>`", "`generic_fields_take_kernel<ES>`"):
        assert kernel in design, kernel
    para = [p for p in design.split("\n\n") if "rows_fields_accumulate_kernel" in p]
    assert para and any("unmeasured" in p or "not measured" in p or "nobody has measured" in p.lower() for p in para)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = integration[integration.index("cudecompAmdAccumulateFieldHalos"):]
    assert "Not covered" in section
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "cudecomp_halo_accumulate_fields.h" in readme and "kernels_field_accumulate.hip" in readme


def test_arguments_are_checked_in_the_stated_order(capfd):
    from tests import halo_check_order
    halo_check_order.check("accumulate_fields", capfd)
