"""cudecomp_interior_reduce.h (cudecompAmdReduceInterior{X,Y,Z}, cudecompAmdReduceInteriorWorkspaceBytes) as a C interface: the four
symbols are declared, exported and listed; the header's parameters agree with the ctypes argtypes every Python test calls through; the
header compiles as C11 under -Wall -Wextra -Werror in either include order; the operation macros are the values the package uses; the
workspace size is monotone in the number of fields and at most 1 MiB; and the entry points refuse their arguments in the order the
header states, each with its CUDECOMP:ERROR message.  No GPU needed: every refusal is made on the host before anything is launched."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cudecomp_amd as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cudecomp_interior_reduce.h"
EXT = ["cudecompExtReduce3D", "cudecompExtDescribeReduce3D"]


def _prototypes(header):
    """{function: [parameter text, ...]} of the cudecompResult_t functions a header declares"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_four_symbols_are_declared_exported_and_listed():
    assert cd.INTERIOR_REDUCE_SYMBOLS == ["cudecompAmdReduceInteriorWorkspaceBytes"] + ["cudecompAmdReduceInterior" + a for a in "XYZ"]
    assert sorted(_prototypes(HEADER)) == sorted(cd.INTERIOR_REDUCE_SYMBOLS)
    L = cd.lib()
    for name in cd.INTERIOR_REDUCE_SYMBOLS + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    # the header's name keeps it out of the family tests/test_abi.py counts, and the package's table of that family is as it was
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS
    assert not any("Reduce" in n for names in cd.AMD_HEADER_SYMBOLS.values() for n in names)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp_amd.h"' in text
    for word in ("cross-rank combine", "weighted or masked", "modulus-based", "single-launch", "performance report", "autotuner",
                 "managed memory"):
        assert word in " ".join(text.split("Out of scope")[1].split()), word
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc


def test_prototypes_agree_with_the_argtypes():
    """as many parameters in the header as in the argtypes, the pointers at the same positions, everything else a 32-bit integer"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    for name in cd.INTERIOR_REDUCE_SYMBOLS[1:]:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 12, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 3, 6, 7, 9, 10, 11]
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        assert params[2:8] == ["const void* const a[]", "const void* const b[]", "int32_t n_fields", "int32_t op", "double* results",
                               "void* work"]
        assert argtypes[6]._type_ is C.c_double
    assert protos["cudecompAmdReduceInteriorWorkspaceBytes"] == ["int32_t n_fields", "int64_t* bytes"]
    ws = L.cudecompAmdReduceInteriorWorkspaceBytes.argtypes
    assert ws[0] is C.c_int32 and ws[1]._type_ is C.c_int64
    ext = _prototypes("cudecomp_ext.h")
    for name in EXT:
        assert len(getattr(L, name).argtypes) == len(ext[name]), name


def test_header_compiles_as_c11():
    """tests/native/interior_reduce_header_c11.c: alone, after and before the other extension headers -- and the compile line does
    notice a prototype that differs"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")]
    source = os.path.join(ROOT, "tests", "native", "interior_reduce_header_c11.c")
    for defs in ([], ["-DOTHERS_FIRST"], ["-DOTHERS_LAST"], ["-DOTHERS_FIRST", "-DOTHERS_LAST"]):
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (defs, res.stderr[-3000:])
    res = subprocess.run(base + ["-DRESULTS_TYPE=float*", source], capture_output=True, text=True)
    assert res.returncode != 0 and "incompatible" in res.stderr, res.stderr[-3000:]


def test_the_macros_are_the_values_the_package_uses():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    macros = dict(re.findall(r"#define\s+(CUDECOMP_AMD_\w+)\s+(\d+)", text))
    assert macros == {"CUDECOMP_AMD_MAX_REDUCE_FIELDS": "32", "CUDECOMP_AMD_REDUCE_SUM": "0", "CUDECOMP_AMD_REDUCE_DOT": "1",
                      "CUDECOMP_AMD_REDUCE_MAX_ABS": "2"}
    assert (cd.MAX_REDUCE_FIELDS, cd.REDUCE_SUM, cd.REDUCE_DOT, cd.REDUCE_MAX_ABS) == (32, 0, 1, 2)


def test_the_workspace_is_monotone_and_at_most_one_mebibyte(capfd):
    sizes = [cd.cudecompAmdReduceInteriorWorkspaceBytes(n) for n in range(1, 33)]
    assert all(b > a for a, b in zip(sizes, sizes[1:])) and sizes[0] >= 16 and sizes[-1] <= 1 << 20
    # one pair of doubles per stage-one workgroup: the cap on workgroups per field is what the size stands for
    assert sizes == [n * cd.REDUCE_MAX_BLOCKS * 16 for n in range(1, 33)]
    L = cd.lib()
    out = C.c_int64(-1)
    capfd.readouterr()
    for n in (0, -1, 33):
        assert L.cudecompAmdReduceInteriorWorkspaceBytes(n, C.byref(out)) == cd.RESULT_INVALID_USAGE
        assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(n_fields argument out of range\)", capfd.readouterr().err)
    assert L.cudecompAmdReduceInteriorWorkspaceBytes(1, None) == cd.RESULT_INVALID_USAGE
    assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(bytes argument cannot be null\)", capfd.readouterr().err)
    assert out.value == -1


# argument -> (wrong value, right value, message); the ladder below is the order of the checks
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
    ("a", None, "a argument cannot be null"),
    ("a", _HOLE, "a argument cannot hold a null entry"),
    ("b", None, "b argument cannot be null for a dot product"),
    ("b", _HOLE, "b argument cannot hold a null entry"),
    ("results", None, "results argument cannot be null"),
    ("results", _ODD, "results argument must be 8-byte aligned"),
    ("work", None, "work argument cannot be null"),
    ("work", 0x40004, "work argument must be 8-byte aligned"),
]
ORDER = "handle gd a b n_fields op results work dtype halo pad stream".split()


@pytest.mark.parametrize("axis", range(3))
def test_arguments_are_refused_in_the_stated_order(axis, capfd):
    """every argument wrong at once: the call is refused for the first check of the header's list; with that argument put right,
    for the second; and so on.  No pointer is device memory -- nothing is ever launched -- and no GPU is needed."""
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((12, 10, 9), (1, 1)))
    fn = getattr(cd.lib(), "cudecompAmdReduceInterior" + "XYZ"[axis])
    right = {"handle": h, "gd": gd, "dtype": cd.FLOAT, "halo": _i3(1, 1, 1), "pad": _i3(0, 1, 0), "n_fields": 2, "op": cd.REDUCE_DOT,
             "a": _FIELDS, "b": _FIELDS, "results": _RESULTS, "work": 0x40000, "stream": None}
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
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)
