"""Multi-field transposes (cudecomp_transpose_fields.h: cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX}) without a GPU: the C
interface (symbols, prototypes against the ctypes argtypes, the header as C11 and C++17), the refusals through the C ABI, the
properties of the stateless plan (cudecompExtPlanTransposeFields) against the single plan over random decompositions, the plans
executed with numpy and a real exchange over gloo on four ranks, and the launch planning of the field-move kernels
(cudecompExtDescribeFieldMoveList)."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import cudecomp_amd as cd
from tests.mp import run_ranks
from tests.test_plan_sim import _cells, decompositions, small3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cudecomp_transpose_fields.h"
NAMES = ["cudecompAmdTransposeFields" + op for op in cd.OPS]
EXT = ["cudecompExtPlanTransposeFields", "cudecompExtRunFieldMoveList", "cudecompExtDescribeFieldMoveList"]
K_TRANSPOSE, K_ROWS, K_GENERIC = 24, 22, 23


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def _prototypes(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_four_symbols_are_declared_and_exported():
    assert cd.TRANSPOSE_FIELDS_SYMBOLS == NAMES and cd.MAX_TRANSPOSE_FIELDS == 32
    assert sorted(_prototypes(HEADER)) == sorted(NAMES)
    L = cd.lib()
    for name in NAMES + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert re.findall(r'#include\s+"([^"]+)"', text) == ["cudecomp.h"]
    assert re.search(r"#define\s+CUDECOMP_AMD_MAX_TRANSPOSE_FIELDS\s+32\b", text)
    # the header's name keeps it out of the family tests/test_abi.py counts, and the package's table of that family is as it was
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS
    assert not any("TransposeFields" in n for names in cd.AMD_HEADER_SYMBOLS.values() for n in names)


def test_prototypes_agree_with_the_argtypes():
    """the transpose's prototype with (inputs, outputs, n_fields) in the place of (input, output): as many parameters as argtypes,
    pointers at the same positions, everything else a 32-bit integer on both sides"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    single = _prototypes("cudecomp.h")
    for name in NAMES:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 12, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if not ptr] == [4, 6]
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        assert params[2:5] == ["void* const inputs[]", "void* const outputs[]", "int32_t n_fields"]
        one = single[name.replace("AmdTransposeFields", "Transpose")]
        assert params[:2] + params[5:] == one[:2] + one[4:]


@pytest.mark.parametrize("language", ["c11", "c++17"])
def test_header_compiles(language):
    """tests/native/transpose_fields_header.c: alone and after the other extension headers (two orders), -Wall -Wextra -Werror,
    every function assigned to a hand-written prototype -- and the compile line does notice a prototype that differs"""
    cc = "gcc" if language == "c11" else "g++"
    if shutil.which(cc) is None:
        pytest.skip("no " + cc)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = [cc, "-std=" + language, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")] + (["-x", "c++"] if language != "c11" else [])
    source = os.path.join(ROOT, "tests", "native", "transpose_fields_header.c")
    others = ["cudecomp_amd.h", "cudecomp_amd_fill.h", "cudecomp_amd_accumulate_clear.h", "cudecomp_amd_reflect.h", "cudecomp_halo_fold.h",
              "cudecomp_halo_fields.h"]
    for order in (None, others, others[::-1]):
        defs = [] if order is None else ['-DBEFORE%d="%s"' % (i + 1, h) for i, h in enumerate(order)]
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (order, res.stderr[-3000:])
    # ... and before them
    res = subprocess.run(base + ["-x", "c" if language == "c11" else "c++", "-"], capture_output=True, text=True,
                         input='#include "%s"\n' % HEADER + "".join('#include "%s"\n' % h for h in others) + "int main(void) { return 0; }\n")
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]
    text = open(source).read()
    broken = text.replace("void* const outputs[],", "void* outputs,")
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


def _call(h, gd, op, ins, outs, n, work=0x1000, dtype=cd.DOUBLE):
    fn = getattr(cd.lib(), "cudecompAmdTransposeFields" + op)
    tab = [None if p is None else (C.c_void_p * max(1, len(p)))(*p) for p in (ins, outs)]
    return fn(h, gd, tab[0], tab[1], n, work, dtype, None, None, None, None, None)


def test_refusals(descriptor, capfd):
    """all found on the host, before anything is launched (the pointers are not device memory, and there is no device here):
    INVALID_USAGE with the transpose's message format, and the count of data-movement launches unchanged"""
    h, gd = descriptor
    a = [0x100000 * (i + 1) for i in range(33)]
    b = [0x100000 * (i + 101) for i in range(33)]
    cases = [("inputs argument cannot be null", None, b[:3], 3), ("outputs argument cannot be null", a[:3], None, 3),
             ("n_fields argument out of range", a[:3], b[:3], 0), ("n_fields argument out of range", a[:3], b[:3], -1),
             ("n_fields argument out of range", a, b, 33),
             ("inputs argument cannot hold a null entry", [a[0], None, a[2]], b[:3], 3),
             ("outputs argument cannot hold a null entry", a[:3], [b[0], b[1], None], 3),
             ("inputs argument cannot hold the same field twice", [a[0], a[1], a[0]], b[:3], 3),
             ("outputs argument cannot hold the same field twice", a[:3], [b[0], b[1], b[1]], 3),
             ("an input field cannot be the output of another field", a[:3], [b[0], a[0], b[2]], 3),
             ("fields must be all in place or all out of place", a[:3], [a[0], b[1], b[2]], 3),
             ("fields must be all in place or all out of place", a[:3], [b[0], a[1], a[2]], 3),
             ("work argument cannot be null", a[:3], b[:3], 3)]
    capfd.readouterr()
    for op in cd.OPS:
        for message, ins, outs, n in cases:
            before = cd.cudecompExtDataLaunchCount()
            rc = _call(h, gd, op, ins, outs, n, work=None if message.startswith("work") else 0x1000)
            assert rc == cd.RESULT_INVALID_USAGE, (op, message)
            assert cd.cudecompExtDataLaunchCount() == before
            err = capfd.readouterr().err
            assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(%s\)" % re.escape(message), err), (message, err)
        # the single transpose says the same kind of thing about its `input`, and the lists are checked where it checks them:
        # after the data type, before work
        fn = getattr(cd.lib(), "cudecompTranspose" + op)
        assert fn(h, gd, None, 0x2000, 0x1000, cd.DOUBLE, None, None, None, None, None) == cd.RESULT_INVALID_USAGE
        assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(input argument cannot be null\)", capfd.readouterr().err)
        assert _call(h, gd, op, None, b[:3], 3, work=None) == cd.RESULT_INVALID_USAGE
        assert "inputs argument cannot be null" in capfd.readouterr().err
        assert _call(h, gd, op, None, None, 3, dtype=77) == cd.RESULT_INVALID_USAGE
        assert "inputs argument" not in capfd.readouterr().err
    # in place, identical layouts (default memory order, no halos): a no-op that needs no device, for 32 fields too
    before = cd.cudecompExtDataLaunchCount()
    assert _call(h, gd, "XToY", a[:32], a[:32], 32) == cd.RESULT_SUCCESS
    assert cd.cudecompExtDataLaunchCount() == before and capfd.readouterr().err == ""


def test_empty_pencils_are_refused_like_the_single_call(capfd):
    spec = cd.make_grid_spec((2, 8, 8), (4, 1), ((0, 1, 2),) * 3)
    codes = []
    for planner, more in ((cd.cudecompExtPlanTranspose, ()), (cd.cudecompExtPlanTransposeFields, (False, False, 0, 3))):
        with pytest.raises(cd.CudecompError) as info:
            planner(spec, 0, "XToY", None, None, None, None, False, *more)
        codes.append(info.value.code)
    assert codes[0] == codes[1] == cd.RESULT_NOT_SUPPORTED
    capfd.readouterr()
    for n in (0, -1):
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtPlanTransposeFields(cd.make_grid_spec((8, 8, 8), (1, 1), ((0, 1, 2),) * 3), 0, "XToY", n_fields=n)
        assert info.value.code == cd.RESULT_INVALID_USAGE


# ---- plan properties ---------------------------------------------------------------------------------------------------------
def _plan_fields(p):
    skip = ("pack", "unpack", "direct")
    return {name: (list(v) if hasattr(v, "__len__") else v) for name, _ in cd.ExtTransposePlan._fields_ if name not in skip
            for v in [getattr(p, name)]}


@settings(max_examples=120, deadline=None, suppress_health_check=list(HealthCheck))
@given(d=decompositions(), op=st.sampled_from(cd.OPS), in_halo=small3, out_halo=small3, in_pad=small3, out_pad=small3,
       inplace=st.booleans(), symmetric=st.booleans(), pipelined=st.booleans())
def test_fields_plans_random_decompositions(d, op, in_halo, out_halo, in_pad, out_pad, inplace, symmetric, pipelined):
    spec = cd.make_grid_spec(d["gdims"], d["pdims"], d["mem_order"], d["gdims_dist"], d["col_major"])
    nranks = d["pdims"][0] * d["pdims"][1]
    hp = (in_halo, out_halo, in_pad, out_pad)
    singles = [cd.cudecompExtPlanTranspose(spec, r, op, *hp, inplace, pipelined, symmetric) for r in range(nranks)]
    # n == 1: buildTransposePlan's plan, unchanged
    for r in range(nranks):
        one, ps, us = cd.cudecompExtPlanTransposeFields(spec, r, op, *hp, inplace, pipelined, symmetric, 0, 1)
        assert bytes(one) == bytes(singles[r]) and not any(ps) and not any(us)
    ws = [cd.cudecompExtWorkspaceSizes(spec, r, 0, (0, 0, 0))[0] for r in range(nranks)]
    # the single plans with both elisions off (never pipelined): what every plan of two fields or more is derived from
    unelided = [cd.cudecompExtPlanTransposeFields(spec, r, op, *hp, inplace, False, symmetric, 0, 1, no_elide=True)[0] for r in range(nranks)]
    axis_in = {"XToY": 0, "YToZ": 1, "ZToY": 2, "YToX": 1}[op]
    interior = [cd.cudecompExtPencilInfo(spec, r, axis_in).size for r in range(nranks)]
    for n in (2, 3, 9):
        plans = [cd.cudecompExtPlanTransposeFields(spec, r, op, *hp, inplace, pipelined, symmetric, 0, n) for r in range(nranks)]
        for r, (fp, ps, us) in enumerate(plans):
            sp = singles[r]
            assert (fp.noop, fp.exchange, fp.comm_axis, fp.nranks, fp.comm_rank) == (sp.noop, sp.exchange, sp.comm_axis, sp.nranks, sp.comm_rank)
            assert list(fp.member_global_rank) == list(sp.member_global_rank) and list(fp.schedule_dst) == list(sp.schedule_dst)
            assert fp.n_direct == 0 and fp.rotate == 0
            moves = [fp.pack[i] for i in range(fp.n_pack)] + [fp.unpack[i] for i in range(fp.n_unpack)]
            assert all(m.row_pitch == 0 for m in moves)
            if fp.noop:
                assert not moves
                continue
            if not fp.exchange:
                # one rank: out of place one move pencil -> pencil, the single plan's; in place through n pieces of the workspace
                if not inplace:
                    assert (fp.n_pack, fp.n_unpack, ps) == (1, 0, [0])
                    a, b = fp.pack[0], sp.pack[0]
                    assert (a.src_buf, a.dst_buf) == (0, 1)
                    assert np.array_equal(_cells(a, "src_off", "ss"), _cells(b, "src_off", "ss"))
                    assert np.array_equal(_cells(a, "dst_off", "ds"), _cells(b, "dst_off", "ds"))
                else:
                    assert (fp.n_pack, fp.n_unpack) == (1, 1) and ps == us
                    a, b = fp.pack[0], fp.unpack[0]
                    piece = np.sort(_cells(a, "dst_off", "ds"))
                    assert (a.src_buf, a.dst_buf, b.src_buf, b.dst_buf) == (0, 2, 2, 1)
                    assert np.array_equal(piece, np.arange(piece.size)) and ps[0] == piece.size and n * piece.size <= n * ws[r]
                    assert np.array_equal(_cells(a, "dst_off", "ds"), _cells(b, "src_off", "ss"))
                    assert np.array_equal(_cells(a, "src_off", "ss"), _cells(sp.pack[0], "src_off", "ss"))
                    assert np.array_equal(_cells(b, "dst_off", "ds"), _cells(sp.unpack[0], "dst_off", "ds"))
                continue
            # with an exchange: the single plan with both elisions off (its pencil cells are those of ANY single plan: which
            # cells of the input travel to whom does not depend on the staging), re-based as specified
            P = fp.nranks
            assert (fp.send_buf, fp.recv_buf, fp.send_base, fp.n_pack, fp.n_unpack) == (2, 2, 0, P, P)
            # move by move the elision-free single plan's: the same peer, the same pencil cells in the same order, and the
            # workspace end moved from off[d] + x to n * off[d] + x (receive side: behind the new base); the exchange times n
            nb = unelided[r]
            assert (nb.send_buf, nb.recv_buf, nb.send_base, nb.n_pack, nb.n_unpack, nb.exchange) == (2, 2, 0, P, P, 1)
            for i in range(P):
                a, b = fp.pack[i], nb.pack[i]
                d_ = b.peer
                assert a.peer == d_ and list(a.extent) == list(b.extent) and list(a.ss) == list(b.ss) and list(a.ds) == list(b.ds)
                assert (a.src_buf, a.src_off) == (b.src_buf, b.src_off) and a.dst_off - n * nb.send_off[d_] == b.dst_off - nb.send_off[d_] == 0
                assert ps[i] == nb.send_cnt[d_]
                a, b = fp.unpack[i], nb.unpack[i]
                s_ = b.peer
                assert a.peer == s_ and list(a.extent) == list(b.extent) and list(a.ss) == list(b.ss) and list(a.ds) == list(b.ds)
                assert (a.dst_buf, a.dst_off) == (b.dst_buf, b.dst_off)
                assert a.src_off - fp.recv_base - n * nb.recv_off[s_] == b.src_off - nb.recv_base - nb.recv_off[s_] == 0
                assert us[i] == nb.recv_cnt[s_]
                for name in ("send_cnt", "send_off", "recv_cnt", "recv_off", "remote_recv_off"):
                    assert getattr(fp, name)[i] == n * getattr(nb, name)[i], name
            # the receive base: n x the unaligned base (one-sided: the largest input pencil of the decomposition, else my own), aligned once
            up = lambda v: -(-v // 64) * 64
            if not symmetric:
                assert nb.recv_base == up(interior[r]) and fp.recv_base == up(n * interior[r])
            else:  # (the planner's own upper bound x of any input pencil: only up(x) = the single base is visible here)
                assert max(interior) <= nb.recv_base and fp.recv_base % 64 == 0
                assert up(n * max(nb.recv_base - 63, max(interior))) <= fp.recv_base <= n * nb.recv_base
            # ... and where the caller's own single plan does not elide either, the elision-free plan IS that plan
            if sp.send_buf == 2 and sp.recv_buf == 2 and not pipelined:
                for i in range(P):
                    assert bytes(nb.pack[i])[:-4] == bytes(sp.pack[i])[:-4] and bytes(nb.unpack[i])[:-4] == bytes(sp.unpack[i])[:-4]
            assert fp.recv_base % 64 == 0
            total = fp.recv_base + sum(fp.recv_cnt[:P])
            assert total <= n * ws[r], (total, n, ws[r])
            send_taken = np.zeros(sum(fp.send_cnt[:P]), dtype=np.int32)
            recv_taken = np.zeros(total, dtype=np.int32)
            in_cells, out_cells = [], []
            for i in range(P):
                m, d_ = fp.pack[i], fp.pack[i].peer
                assert (m.src_buf, m.dst_buf) == (0, 2) and fp.send_cnt[d_] == n * ps[i]
                piece = _cells(m, "dst_off", "ds")
                assert np.array_equal(np.sort(piece), fp.send_off[d_] + np.arange(ps[i]))  # field 0's piece: dense, at the chunk's start
                for f in range(n):
                    send_taken[piece + f * ps[i]] += 1
                in_cells.append(_cells(m, "src_off", "ss"))
                m, s = fp.unpack[i], fp.unpack[i].peer
                assert (m.src_buf, m.dst_buf) == (2, 1) and fp.recv_cnt[s] == n * us[i]
                piece = _cells(m, "src_off", "ss")
                assert np.array_equal(np.sort(piece), fp.recv_base + fp.recv_off[s] + np.arange(us[i]))
                for f in range(n):
                    recv_taken[piece + f * us[i]] += 1
                out_cells.append(_cells(m, "dst_off", "ds"))
            # the pieces of all (peer, field) pairs tile the send area, and the receive area behind its base, without overlap
            assert (send_taken == 1).all() and (recv_taken[fp.recv_base:] == 1).all() and not recv_taken[:fp.recv_base].any()
            assert fp.recv_base >= send_taken.size
            # exactly the interior cells: every input interior cell is packed once, every output interior cell unpacked once
            ai, ao = {"XToY": (0, 1), "YToZ": (1, 2), "ZToY": (2, 1), "YToX": (1, 0)}[op]
            for cells_, axis, halo, pad in ((in_cells, ai, in_halo, in_pad), (out_cells, ao, out_halo, out_pad)):
                info = cd.cudecompExtPencilInfo(spec, r, axis, halo, pad)
                bare = cd.cudecompExtPencilInfo(spec, r, axis)
                allc = np.concatenate(cells_)
                assert allc.size == np.unique(allc).size == bare.size and allc.min() >= 0 and allc.max() < info.size
            # sender and receiver agree on every piece's length and position
            for di in range(P):
                q, qps, qus = plans[fp.member_global_rank[di]]
                assert q.recv_cnt[fp.comm_rank] == fp.send_cnt[di]
                if symmetric:  # one-sided: the receive base is the same number everywhere, the slot offset the receiver's
                    assert fp.remote_recv_off[di] == q.recv_off[fp.comm_rank] and q.recv_base == fp.recv_base
                mine = [i for i in range(P) if fp.pack[i].peer == di][0]
                theirs = [i for i in range(P) if q.unpack[i].peer == fp.comm_rank][0]
                assert ps[mine] == qus[theirs]
                # ... and on the order inside a piece: the same dense wire strides over the same extents
                a, b = fp.pack[mine], q.unpack[theirs]
                assert list(a.extent) == list(b.extent) and list(a.ds) == list(b.ss)
            # the scaled exchange is the elision-free single plan's: counts and offsets are multiples of n
            for i in range(P):
                for arr in (fp.send_cnt, fp.send_off, fp.recv_cnt, fp.recv_off, fp.remote_recv_off):
                    assert arr[i] % n == 0


# ---- plan execution over gloo --------------------------------------------------------------------------------------------------
def test_fields_plan_over_gloo():
    """4 ranks (2 x 2), ragged (10, 9, 11), a full X->Y->Z->Y->X cycle of 3 fields against the single plans"""
    zero = [(0, 0, 0)] * 3
    halos, pads = [(1, 1, 2), (2, 1, 1), (1, 2, 1)], [(1, 0, 0), (0, 1, 0), (0, 0, 2)]
    cases = [(zero, zero, False, False), (zero, zero, True, True), (halos, pads, False, True), (halos, pads, True, False)]
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "n_fields": 3, "cases": cases}
    for failures in run_ranks(4, "tests.transpose_fields_bodies", "plan_fields_gloo", args):
        assert failures == []


# ---- launch planning -----------------------------------------------------------------------------------------------------------
def _describe(geometries, n_fields, es, force=0, bases=None, work=1 << 40, steps=None):
    """geometries: (extent, ss, ds, src_buf, dst_buf); every move at offset 0 of its ends (nothing runs: overlap is no concern)"""
    moves = [cd.make_move(e, ss, ds, src_buf=sb, dst_buf=db) for e, ss, ds, sb, db in geometries]
    ins = bases or [(i + 1) << 32 for i in range(n_fields)]
    outs = [x + (1 << 30) for x in ins]
    return cd.cudecompExtDescribeFieldMoveList(moves, steps or [1 << 20] * len(moves), ins, outs, work, es, force)


ROWS = ((64, 5, 3), (1, 66, 336), (1, 68, 346))
TRANS = ((72, 40, 3), (1, 74, 74 * 40 + 6), (44, 1, 44 * 72 + 10))
THIN = ((1, 9, 7), (1, 13, 200), (1, 13, 200))


def test_kernel_by_geometry():
    for es in (2, 4, 8, 16):
        d = _describe([ROWS + (0, 2)], 3, es)
        assert [(x["kind"], x["vec"], x["access"]) for x in d] == [(K_ROWS, 16, 0)]
        d = _describe([TRANS + (0, 2)], 3, es)
        vw = 16 // es
        tile = {2: (128, 128), 4: (64, 128), 8: (64, 64), 16: (32, 32)}[es]
        assert [(x["kind"], x["vec"], x["ti"], x["tj"], x["guard"], x["access"]) for x in d] == [(K_TRANSPOSE, vw) + tile + (1, 0)]
        assert d[0]["blocks_per_field"] == -(-72 // tile[0]) * -(-40 // tile[1]) * 3 and d[0]["blocks"] == 3 * d[0]["blocks_per_field"]
        d = _describe([THIN + (0, 1)], 3, es)
        assert [(x["kind"], x["vec"], x["access"]) for x in d] == [(K_GENERIC, es, 0)]
        # extents below 4, and the forced case: element-wise
        assert _describe([((3, 40, 2), (1, 8, 400), (44, 1, 200), 0, 1)], 2, es)[0]["kind"] == K_GENERIC
        assert [x["kind"] for x in _describe([TRANS + (0, 2), ROWS + (2, 1)], 2, es, force=1)] == [K_GENERIC]
        # odd extents: element-wise lanes in the narrower tile
        d = _describe([((69, 37, 2), (1, 71, 71 * 37 + 6), (41, 1, 41 * 69 + 10), 0, 1)], 2, es)
        assert (d[0]["kind"], d[0]["vec"], d[0]["ti"], d[0]["tj"], d[0]["guard"]) == (K_TRANSPOSE, 1, 32 if es == 16 else 64, 32 if es == 16 else 64, 1)
        # whole tiles: the unguarded form
        whole = (tile[0], 2 * tile[1], 2)
        d = _describe([(whole, (1, whole[0] + 8, (whole[0] + 8) * whole[1]), (whole[1] + 8, 1, (whole[1] + 8) * whole[0]), 0, 2)], 2, es)
        assert (d[0]["kind"], d[0]["vec"], d[0]["guard"]) == (K_TRANSPOSE, vw, 0)
        # nothing to launch
        assert _describe([((0, 5, 3), (1, 66, 400), (1, 64, 320), 0, 1)], 2, es) == []


def test_two_byte_lanes_narrow_when_any_field_sits_at_two_mod_four():
    aligned = [(i + 1) << 32 for i in range(3)]
    assert _describe([TRANS + (0, 1)], 3, 2, bases=aligned)[0]["vec"] == 8
    assert _describe([ROWS + (0, 1)], 3, 2, bases=aligned)[0]["vec"] == 16
    for odd in range(3):  # ONE of three inputs at 2 mod 4: the move on 2-byte lanes
        bases = list(aligned)
        bases[odd] += 2
        d = _describe([TRANS + (0, 1)], 3, 2, bases=bases)[0]
        assert (d["kind"], d["vec"], d["ti"], d["tj"]) == (K_TRANSPOSE, 1, 64, 64), (odd, d)
        assert _describe([ROWS + (0, 1)], 3, 2, bases=bases)[0]["vec"] == 2
        assert _describe([TRANS + (0, 1)], 3, 4, bases=bases)[0]["vec"] == 4  # (wider elements need only their own alignment)
    # the workspace at 2 mod 4, or an odd step between the fields' pieces, does the same -- for the moves that touch the workspace
    d = _describe([TRANS + (0, 2), TRANS + (0, 1)], 3, 2, bases=aligned, work=(1 << 40) + 2)
    assert [(x["vec"], x["index"]) for x in d] == [(1, [0]), (8, [1])]
    d = _describe([TRANS + (0, 2), TRANS + (0, 1)], 3, 2, bases=aligned, steps=[(1 << 20) + 1, 0])
    assert [(x["vec"], x["index"]) for x in d] == [(1, [0]), (8, [1])]
    # an odd stride does it whatever the addresses
    assert _describe([((72, 40, 3), (1, 75, 75 * 40 + 6), (44, 1, 44 * 72 + 10), 0, 1)], 3, 2, bases=aligned)[0]["vec"] == 1


def test_nine_moves_give_two_launches_and_the_list_does_not_depend_on_the_number_of_fields():
    nine = [TRANS + ((0, 2, 0)[i % 3], (2, 1, 1)[i % 3]) for i in range(9)]
    mixed = [TRANS + (0, 2), ROWS + (0, 1), THIN + (2, 1), TRANS + (0, 1), ROWS + (0, 2)]
    want = None
    for n in (1, 2, 3, 9, 32):
        d = _describe(nine, n, 8)
        assert [x["index"] for x in d] == [list(range(8)), [8]]
        assert all(x["blocks"] == n * x["blocks_per_field"] for x in d)
        d = _describe(mixed, n, 8)
        shape = [(x["kind"], x["vec"], x["ti"], x["tj"], x["access"], x["guard"], x["index"], x["blocks_per_field"]) for x in d]
        assert [(s[0], s[6]) for s in shape] == [(K_TRANSPOSE, [0, 3]), (K_ROWS, [1, 4]), (K_GENERIC, [2])]
        want = want or shape
        assert shape == want


def test_access_mode_by_the_size_of_one_field_move():
    """cached below 32 MiB PER FIELD MOVE, non-temporal from there -- whatever the number of fields; the element-wise kernel
    always cached"""
    for es in (2, 4, 8, 16):
        n = (32 << 20) // es
        side = 1 << ((n.bit_length() - 1) // 2)
        big = ((side, n // side, 1), (1, side + 8, 0), (n // side + 8, 1, 0))
        for nf in (2, 9):
            assert [(x["kind"], x["access"]) for x in _describe([big + (0, 1)], nf, es)] == [(K_TRANSPOSE, 2)]
            assert _describe([big + (0, 1)], nf, es, force=4)[0]["access"] == 0
            assert _describe([big + (0, 1)], nf, es, force=1)[0]["access"] == 0
            rows = ((n, 1, 1), (1, 0, 0), (1, 0, 0))
            assert [(x["kind"], x["access"]) for x in _describe([rows + (0, 1)], nf, es)] == [(K_ROWS, 1)]
            small = ((n - 1, 1, 1), (1, 0, 0), (1, 0, 0))
            assert _describe([small + (0, 1)], nf, es)[0]["access"] == 0
            assert _describe([small + (0, 1)], nf, es, force=2)[0]["access"] == 1
        assert _describe([TRANS + (0, 1)], 2, es, force=2)[0]["access"] == 2


def test_moves_that_are_no_plain_copies_are_internal_errors():
    m = cd.make_move((8, 4, 2), (1, 8, 32), (1, 8, 32), src_buf=0, dst_buf=2, row_pitch=8)
    ins = [1 << 32, 2 << 32]
    with pytest.raises(cd.CudecompError) as info:
        cd.cudecompExtDescribeFieldMoveList([m], [64], ins, ins, 1 << 40, 8)
    assert info.value.code == cd.RESULT_INTERNAL_ERROR
    m = cd.make_move((8, 4, 2), (1, 8, 32), (1, 8, 32), src_buf=0, dst_buf=2)
    with pytest.raises(cd.CudecompError) as info:  # a workspace end without a workspace
        cd.cudecompExtDescribeFieldMoveList([m], [64], ins, ins, 0, 8)
    assert info.value.code == cd.RESULT_INTERNAL_ERROR
    m = cd.make_move((8, 4, 2), (1, 8, 32), (1, 8, 32), src_buf=0, dst_buf=1)
    with pytest.raises(cd.CudecompError) as info:  # an output end without outputs
        cd.cudecompExtDescribeFieldMoveList([m], None, ins, None, 0, 8)
    assert info.value.code == cd.RESULT_INTERNAL_ERROR
    for n in (0, 33):
        with pytest.raises(cd.CudecompError) as info:
            cd.cudecompExtDescribeFieldMoveList([m], None, [1 << 32] * n, [1 << 33] * n, 0, 8)
        assert info.value.code == cd.RESULT_INVALID_USAGE
    # more than 2^31 - 1 workgroups: not supported
    huge = cd.make_move((64 * 40000, 64 * 40000, 2), (1, 1 << 22, 1 << 44), (1 << 22, 1, 1 << 44), src_buf=0, dst_buf=1)
    with pytest.raises(cd.CudecompError) as info:
        cd.cudecompExtDescribeFieldMoveList([huge], None, ins, [x + (1 << 50) for x in ins], 0, 8)
    assert info.value.code == cd.RESULT_NOT_SUPPORTED


def test_the_documents_carry_the_contract_and_say_what_is_unmeasured():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name in ("`transpose_fields_kernel<ES,VW,TI,TJ,STREAM,GUARD>`", "`rows_fields_kernel<VB,STREAM>`", "`generic_fields_kernel<ES>`"):
        assert name in design, name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = integration[integration.index("## 14."):]
    assert "cudecompAmdTransposeFields" in section and "Not covered" in section
    for words in ("pipelined, staged or direct", "fallback to single calls", "performance report", "autotuner", "multi-GPU"):
        assert words in section, words
    assert "NOT MEASURED" in design or os.path.exists(os.path.join(ROOT, "profiles", "transpose_fields_bench.json"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "cudecomp_transpose_fields.h" in readme and "kernels_field_transpose.hip" in readme
