"""cudecomp_interior_profile.h (cudecompAmdProfileInterior{X,Y,Z}, cudecompAmdProfileInteriorWorkspaceBytes) as a C interface: the
four symbols are declared, exported and listed; the header's parameters agree with the ctypes argtypes every Python test calls
through; the header compiles as C11 under -Wall -Wextra -Werror in either include order; and the entry points refuse their arguments
in the order the header states, each with its CUDECOMP:ERROR message.  No GPU needed: every refusal is made on the host before
anything is launched."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cudecomp_amd as cd
from tests.test_interior_reduce_abi import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cudecomp_interior_profile.h"
EXT = ["cudecompExtProfile3D", "cudecompExtDescribeProfile3D"]


def test_the_four_symbols_are_declared_exported_and_listed():
    assert cd.INTERIOR_PROFILE_SYMBOLS == ["cudecompAmdProfileInteriorWorkspaceBytes"] + ["cudecompAmdProfileInterior" + a for a in "XYZ"]
    assert sorted(_prototypes(HEADER)) == sorted(cd.INTERIOR_PROFILE_SYMBOLS)
    L = cd.lib()
    for name in cd.INTERIOR_PROFILE_SYMBOLS + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp_interior_reduce.h"' in text and "#define CUDECOMP_AMD" not in text  # (the scalar call's macros are reused)
    for word in ("cross-rank combine", "weights", "modulus-based", "2-D result", "performance report", "autotuner", "managed memory"):
        assert word in " ".join(text.split("Out of scope")[1].split()), word
    assert "MPI_Allreduce" in text and "results + 2 * lo[dim]" in text  # the recipe
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "cd.INTERIOR_PROFILE_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_prototypes_agree_with_the_argtypes():
    """as many parameters in the header as in the argtypes, the pointers at the same positions, ld a 64-bit integer, everything else
    a 32-bit one"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    for name in cd.INTERIOR_PROFILE_SYMBOLS[1:]:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 14, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 3, 7, 9, 11, 12, 13]
        assert params[2:10] == ["const void* const a[]", "const void* const b[]", "int32_t n_fields", "int32_t op", "int32_t dim",
                                "double* results", "int64_t ld", "void* work"]
        assert argtypes[8] is C.c_int64 and argtypes[7]._type_ is C.c_double
        assert all(t is C.c_int32 for i, (t, ptr) in enumerate(zip(argtypes, in_python)) if not ptr and i != 8), (name, argtypes)
    assert protos["cudecompAmdProfileInteriorWorkspaceBytes"] == ["int32_t n_fields", "int64_t length", "int64_t* bytes"]
    ws = L.cudecompAmdProfileInteriorWorkspaceBytes.argtypes
    assert ws[0] is C.c_int32 and ws[1] is C.c_int64 and ws[2]._type_ is C.c_int64
    ext = _prototypes("cudecomp_ext.h")
    for name in EXT:
        assert len(getattr(L, name).argtypes) == len(ext[name]), name


def test_header_compiles_as_c11():
    """tests/native/interior_profile_header_c11.c: alone, after and before the other extension headers -- and the compile line does
    notice a prototype that differs"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")]
    source = os.path.join(ROOT, "tests", "native", "interior_profile_header_c11.c")
    for defs in ([], ["-DOTHERS_FIRST"], ["-DOTHERS_LAST"], ["-DOTHERS_FIRST", "-DOTHERS_LAST"]):
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (defs, res.stderr[-3000:])
    res = subprocess.run(base + ["-DLD_TYPE=double*", source], capture_output=True, text=True)
    assert res.returncode != 0 and "incompatible" in res.stderr, res.stderr[-3000:]


def test_the_workspace_function_refuses_bad_arguments(capfd):
    L = cd.lib()
    out = C.c_int64(-1)
    capfd.readouterr()
    for n in (0, -1, 33):
        assert L.cudecompAmdProfileInteriorWorkspaceBytes(n, 8, C.byref(out)) == cd.RESULT_INVALID_USAGE
        assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(n_fields argument out of range\)", capfd.readouterr().err)
    assert L.cudecompAmdProfileInteriorWorkspaceBytes(1, -1, C.byref(out)) == cd.RESULT_INVALID_USAGE
    assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(length argument cannot be negative\)", capfd.readouterr().err)
    assert L.cudecompAmdProfileInteriorWorkspaceBytes(1, 8, None) == cd.RESULT_INVALID_USAGE
    assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(bytes argument cannot be null\)", capfd.readouterr().err)
    assert out.value == -1


# argument -> (wrong value, message); the ladder below is the order of the checks
_i3 = C.c_int32 * 3
_FIELDS = (C.c_void_p * 2)(0x10000, 0x20000)
_HOLE = (C.c_void_p * 2)(0x10000, None)
_RESULTS = C.cast(C.c_void_p(0x30000), C.POINTER(C.c_double))
_ODD = C.cast(C.c_void_p(0x30004), C.POINTER(C.c_double))
LADDER = [
    ("handle", None, "invalid handle"),
    ("gd", None, "invalid grid descriptor"),
    ("dtype", 99, "unknown data type"),
    ("halo", None, "halo_extents argument cannot be null"),
    ("halo", _i3(1, -1, 1), "halo_extents values must be non-negative"),
    ("pad", _i3(0, 0, -2), "padding values must be non-negative"),
    ("n_fields", 0, "n_fields argument out of range"),
    ("n_fields", 33, "n_fields argument out of range"),
    ("op", 3, "op argument out of range"),
    ("op", -1, "op argument out of range"),
    ("dim", 3, "dim argument out of range"),
    ("dim", -1, "dim argument out of range"),
    ("a", None, "a argument cannot be null"),
    ("a", _HOLE, "a argument cannot hold a null entry"),
    ("b", None, "b argument cannot be null for a dot product"),
    ("b", _HOLE, "b argument cannot hold a null entry"),
    ("results", None, "results argument cannot be null"),
    ("results", _ODD, "results argument must be 8-byte aligned"),
    ("ld", 1, "ld argument is smaller than the interior extent along dim"),
    ("work", None, "work argument cannot be null"),
    ("work", 0x40004, "work argument must be 8-byte aligned"),
]
ORDER = "handle gd a b n_fields op dim results ld work dtype halo pad stream".split()


@pytest.mark.parametrize("axis", range(3))
def test_arguments_are_refused_in_the_stated_order(axis, capfd):
    """every argument wrong at once: the call is refused for the first check of the header's list; with that argument put right,
    for the second; and so on.  No pointer is device memory -- nothing is ever launched -- and no GPU is needed."""
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((12, 10, 9), (1, 1)))
    fn = getattr(cd.lib(), "cudecompAmdProfileInterior" + "XYZ"[axis])
    right = {"handle": h, "gd": gd, "dtype": cd.FLOAT, "halo": _i3(1, 1, 1), "pad": _i3(0, 1, 0), "n_fields": 2, "op": cd.REDUCE_DOT,
             "dim": 1, "a": _FIELDS, "b": _FIELDS, "results": _RESULTS, "ld": 64, "work": 0x40000, "stream": None}
    capfd.readouterr()
    for step, (name, wrong, message) in enumerate(LADDER):
        args = dict(right)
        for later, value, _ in reversed(LADDER[step:]):  # everything from this check on is wrong; the first wrong value of each wins
            args[later] = value
        args[name] = wrong
        assert fn(*[args[k] for k in ORDER]) == cd.RESULT_INVALID_USAGE, message
        err = capfd.readouterr().err
        assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(%s\)" % re.escape(message), err), (message, err)
    # `b` is not looked at for the other two operations
    for op in (cd.REDUCE_SUM, cd.REDUCE_MAX_ABS):
        args = dict(right, op=op, b=None, results=None)
        assert fn(*[args[k] for k in ORDER]) == cd.RESULT_INVALID_USAGE
        assert "results argument cannot be null" in capfd.readouterr().err
    # ld equal to the interior extent passes that check: the next one is reached
    p = cd.cudecompGetPencilInfo(h, gd, axis, (1, 1, 1), (0, 1, 0))
    pos = [int(x) for x in p.order].index(1)
    L = int(p.shape[pos]) - 2 - 1
    for ld, message in ((L - 1, "ld argument is smaller"), (L, "work argument cannot be null")):
        args = dict(right, ld=ld, work=None)
        assert fn(*[args[k] for k in ORDER]) == cd.RESULT_INVALID_USAGE
        assert message in capfd.readouterr().err, (ld, message)
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)
