"""cudecomp_interior_planes.h (cudecompAmdApplyPlanesInterior{X,Y,Z}) as a C interface: the three symbols are declared, exported and
listed; the header's parameters agree with the ctypes argtypes every Python test calls through; the header compiles as C11 under
-Wall -Wextra -Werror in either include order; and the entry points refuse their arguments in the order the header states, each with
its CUDECOMP:ERROR message.  No GPU needed: every refusal is made on the host before anything is launched, and the calls that are
accepted are made in a child process that sees no device, so they end at the library's request for one."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cudecomp_amd as cd
from tests.test_interior_reduce_abi import _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cudecomp_interior_planes.h"
EXT = ["cudecompExtPlanes3D", "cudecompExtDescribePlanes3D"]


def test_the_three_symbols_are_declared_exported_and_listed():
    assert cd.INTERIOR_PLANES_SYMBOLS == ["cudecompAmdApplyPlanesInterior" + a for a in "XYZ"]
    assert sorted(_prototypes(HEADER)) == sorted(cd.INTERIOR_PLANES_SYMBOLS)
    assert (cd.PLANES_ADD, cd.PLANES_MUL) == (0, 1)
    L = cd.lib()
    for name in cd.INTERIOR_PLANES_SYMBOLS + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp_interior_profile.h"' in text
    assert "#define CUDECOMP_AMD_PLANES_ADD 0" in text and "#define CUDECOMP_AMD_PLANES_MUL 1" in text
    for word in ("two coefficient arrays", "out-of-place", "2-D coefficient", "managed memory", "performance report", "autotuner"):
        assert word in " ".join(text.split("Out of scope")[1].split()), word
    assert "coef + 2 * lo[dim]" in text  # the recipe across ranks
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "cd.INTERIOR_PLANES_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def test_prototypes_agree_with_the_argtypes():
    """as many parameters in the header as in the argtypes, the pointers at the same positions, ld a 64-bit integer, scale a double,
    everything else a 32-bit integer"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    for name in cd.INTERIOR_PLANES_SYMBOLS:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 13, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 6, 10, 11, 12]
        assert params[2:9] == ["void* const fields[]", "int32_t n_fields", "int32_t op", "int32_t dim", "const double* coef", "int64_t ld",
                               "double scale"]
        assert argtypes[7] is C.c_int64 and argtypes[8] is C.c_double and argtypes[6]._type_ is C.c_double
        assert all(t is C.c_int32 for i, (t, ptr) in enumerate(zip(argtypes, in_python)) if not ptr and i not in (7, 8)), (name, argtypes)
    ext = _prototypes("cudecomp_ext.h")
    for name in EXT:
        assert len(getattr(L, name).argtypes) == len(ext[name]), name


def test_header_compiles_as_c11():
    """tests/native/interior_planes_header_c11.c: alone, after and before the other extension headers -- and the compile line does
    notice a prototype that differs"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")]
    source = os.path.join(ROOT, "tests", "native", "interior_planes_header_c11.c")
    for defs in ([], ["-DOTHERS_FIRST"], ["-DOTHERS_LAST"], ["-DOTHERS_FIRST", "-DOTHERS_LAST"]):
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (defs, res.stderr[-3000:])
    res = subprocess.run(base + ["-DSCALE_TYPE=double*", source], capture_output=True, text=True)
    assert res.returncode != 0 and "incompatible" in res.stderr, res.stderr[-3000:]


# argument -> (wrong value, message); the ladder below is the order of the checks
_i3 = C.c_int32 * 3
_FIELDS = (C.c_void_p * 3)(0x10000, 0x20000, 0x30000)
_HOLE = (C.c_void_p * 3)(0x10000, None, 0x10000)  # (the null entry is found before the pair of equal ones)
_TWICE = (C.c_void_p * 3)(0x10000, 0x20000, 0x10000)
_COEF = C.cast(C.c_void_p(0x40000), C.POINTER(C.c_double))
_ODD = C.cast(C.c_void_p(0x40004), C.POINTER(C.c_double))
LADDER = [
    ("handle", None, "invalid handle"),
    ("gd", None, "invalid grid descriptor"),
    ("dtype", 99, "unknown data type"),
    ("halo", None, "halo_extents argument cannot be null"),
    ("halo", _i3(1, -1, 1), "halo_extents values must be non-negative"),
    ("pad", _i3(0, 0, -2), "padding values must be non-negative"),
    ("n_fields", 0, "n_fields argument out of range"),
    ("n_fields", 33, "n_fields argument out of range"),
    ("op", 2, "op argument out of range"),
    ("op", -1, "op argument out of range"),
    ("dim", 3, "dim argument out of range"),
    ("dim", -1, "dim argument out of range"),
    ("fields", None, "fields argument cannot be null"),
    ("fields", _HOLE, "fields argument cannot hold a null entry"),
    ("fields", _TWICE, "fields argument cannot hold the same field twice"),
    ("coef", None, "coef argument cannot be null"),
    ("coef", _ODD, "coef argument must be 8-byte aligned"),
    ("ld", 1, "ld argument is neither 0 nor at least the interior extent along dim"),
]
ORDER = "handle gd fields n_fields op dim coef ld scale dtype halo pad stream".split()


@pytest.mark.parametrize("axis", range(3))
def test_arguments_are_refused_in_the_stated_order(axis, capfd):
    """every argument wrong at once: the call is refused for the first check of the header's list; with that argument put right,
    for the second; and so on.  No pointer is device memory -- nothing is ever launched -- and no GPU is needed."""
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((12, 10, 9), (1, 1)))
    fn = getattr(cd.lib(), "cudecompAmdApplyPlanesInterior" + "XYZ"[axis])
    right = {"handle": h, "gd": gd, "dtype": cd.FLOAT, "halo": _i3(1, 1, 1), "pad": _i3(0, 1, 0), "n_fields": 3, "op": cd.PLANES_MUL,
             "dim": 1, "fields": _FIELDS, "coef": _COEF, "ld": 64, "scale": 1.0, "stream": None}
    capfd.readouterr()
    for step, (name, wrong, message) in enumerate(LADDER):
        args = dict(right)
        for later, value, _ in reversed(LADDER[step:]):  # everything from this check on is wrong; the first wrong value of each wins
            args[later] = value
        args[name] = wrong
        assert fn(*[args[k] for k in ORDER]) == cd.RESULT_INVALID_USAGE, message
        err = capfd.readouterr().err
        assert re.search(r"CUDECOMP:ERROR: .*Invalid usage\. \(%s\)" % re.escape(message), err), (message, err)
    # 0 < ld < L is refused for every such ld, whatever else is right
    p = cd.cudecompGetPencilInfo(h, gd, axis, (1, 1, 1), (0, 1, 0))
    pos = [int(x) for x in p.order].index(1)
    L = int(p.shape[pos]) - 2 - 1
    assert L > 2
    for ld in range(1, L):
        args = dict(right, ld=ld)
        assert fn(*[args[k] for k in ORDER]) == cd.RESULT_INVALID_USAGE
        assert "ld argument is neither 0 nor at least" in capfd.readouterr().err, ld
    assert fn(*[dict(right, ld=-1)[k] for k in ORDER]) == cd.RESULT_INVALID_USAGE
    capfd.readouterr()
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


_ACCEPTED = r"""
import ctypes as C
import sys
import cudecomp_amd as cd
i3 = C.c_int32 * 3
fields = (C.c_void_p * 3)(0x10000, 0x20000, 0x30000)
coef = C.cast(C.c_void_p(0x40000), C.POINTER(C.c_double))
h = cd.cudecompInit()
gd = cd.cudecompGridDescCreate(h, cd.make_config((12, 10, 9), (1, 1)))
out = []
for axis in range(3):
    fn = getattr(cd.lib(), "cudecompAmdApplyPlanesInterior" + "XYZ"[axis])
    for ld in (0, 10, 11, 1 << 40, 1, 9, -1):  # the interior extent along dim 1 is 10: the cells the rank owns
        out.append((axis, ld, fn(h, gd, fields, 3, cd.PLANES_ADD, 1, coef, ld, -0.5, cd.DOUBLE, i3(1, 1, 1), i3(0, 1, 0), None)))
print(out)
"""


def test_ld_zero_and_ld_of_the_extent_are_accepted():
    """in a child process that sees no device: a call whose arguments are all accepted gets as far as asking for the device and
    returns CUDA_ERROR -- ld == 0 (all fields share row 0), ld == L, ld > L -- while 0 < ld < L and a negative ld are INVALID_USAGE.
    (With a device the accepted calls would launch on pointers that are no device memory.)"""
    import sys
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", _ACCEPTED], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert res.returncode == 0, res.stderr[-3000:]
    got = eval(res.stdout.strip().splitlines()[-1])
    want = [(axis, ld, cd.RESULT_CUDA_ERROR if ld in (0, 10, 11, 1 << 40) else cd.RESULT_INVALID_USAGE)
            for axis in range(3) for ld in (0, 10, 11, 1 << 40, 1, 9, -1)]
    assert got == want, (got, res.stderr[-2000:])
    assert res.stderr.count("no usable HIP device") == 12 and res.stderr.count("ld argument is neither 0 nor at least") == 9, res.stderr[-3000:]
