"""cudecomp_halo_wall_planes.h (cudecompAmdSetWallPlaneHalos{X,Y,Z}) as a C interface: the three symbols are exported, the header's
parameters agree with the ctypes argtypes every Python test calls through, the header compiles as C11 under -Wall -Wextra -Werror
in either include order with cudecomp_halo_wall_values.h, and the documents name the call and spell its two kernels the way the
library names them.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import cudecomp_amd as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cudecomp_halo_wall_planes.h"
EXT = ["cudecompExtPlanHaloWallPlanes", "cudecompExtWallPlane3D"]


def _prototypes(header):
    """{function: [parameter text, ...]} of the cudecompResult_t functions a header declares"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_three_symbols_are_declared_and_exported():
    assert cd.AMD_WALL_PLANES_SYMBOLS == ["cudecompAmdSetWallPlaneHalos" + a for a in "XYZ"]
    assert sorted(_prototypes(HEADER)) == sorted(cd.AMD_WALL_PLANES_SYMBOLS)
    L = cd.lib()
    for name in cd.AMD_WALL_PLANES_SYMBOLS + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp_amd.h"' in text
    for word in ("several fields", "adjoint", "performance report", "autotuner"):  # the header's own out-of-scope list
        assert word in text.split("Out of scope")[1], word
    # the header's name keeps it out of the family tests/test_abi.py counts, and the package's table of that family is as it was
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS
    assert not any("Wall" in n for names in cd.AMD_HEADER_SYMBOLS.values() for n in names)
    assert (cd.MOVES_WALL_PLANE, cd.MOVES_WALL_PLANE_NEGATE) == (13, 14)
    # the wall values' header points here instead of declaring the plane out of scope
    values = open(os.path.join(ROOT, "include", "cudecomp_halo_wall_values.h")).read()
    assert HEADER in values and "a plane of values); halos wider" not in values


def test_prototypes_agree_with_the_argtypes():
    """as many parameters in the header as in the argtypes, the pointers at the same positions, everything else a 32-bit integer on
    both sides; the wall values' prototype with two `const void*` in the place of the arrays of doubles"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    values = _prototypes("cudecomp_halo_wall_values.h")
    for name in cd.AMD_WALL_PLANES_SYMBOLS:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 14, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 7, 8, 9, 10, 12, 13]
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        assert params[6:9] == ["int32_t sides", "const void* planes_low", "const void* planes_high"]
        assert argtypes[7] is C.c_void_p and argtypes[8] is C.c_void_p
        twin = values[name.replace("SetWallPlaneHalos", "SetWallHalos")]
        assert params[:7] + params[9:] == twin[:7] + twin[9:]
    ext = _prototypes("cudecomp_ext.h")
    for name in EXT:
        assert len(getattr(L, name).argtypes) == len(ext[name]), name
    assert C.sizeof(cd.ExtPlaneOperand) == 40


def test_header_compiles_as_c11():
    """tests/native/wall_planes_header_c11.c: alone, after and before cudecomp_halo_wall_values.h and its neighbours -- and the
    compile line does notice a prototype that differs"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")]
    source = os.path.join(ROOT, "tests", "native", "wall_planes_header_c11.c")
    for defs in ([], ["-DVALUES_FIRST"], ["-DVALUES_LAST"], ["-DVALUES_FIRST", "-DVALUES_LAST"]):
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (defs, res.stderr[-3000:])
    res = subprocess.run(base + ["-DPLANE_TYPE=const double*", source], capture_output=True, text=True)
    assert res.returncode != 0 and "incompatible" in res.stderr, res.stderr[-3000:]


def test_the_documents_name_the_call_and_its_kernels():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`rows_wall_plane_kernel<T,VB,STREAM,NEG>`" in text and "`generic_wall_plane_kernel<T,ES,NEG>`" in text
    para = [p for p in text.split("\n\n") if "Wall-plane moves" in p]
    assert para and any("the access-mode rule is the reflection's and unmeasured for these kernels" in " ".join(p.split()) for p in para)
    for doc in ("README.md", "INTEGRATION.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc


def test_the_new_kinds_are_appended():
    """41 and 42, behind the pinned kinds: a wall-plane move alone is described as one of them, rows or element-wise"""
    m = cd.make_move((16, 4, 3), (1, 16, -64), (1, 16, 64), 128, 1024, 0, 0)
    m.peer = 1
    planes = [(0, (1, 16, 64))]
    (l,) = cd.cudecompExtDescribeMoves([m], (1 << 32, 1 << 36, 1 << 40), 8, cd.MOVES_WALL_PLANE, cd.DOUBLE, planes=planes)
    assert (l["kind"], l["cls"], l["vec"], l["arith"]) == (41, 0, 16, 4), l
    (l,) = cd.cudecompExtDescribeMoves([m], (1 << 32, 1 << 36, 1 << 40), 8, cd.MOVES_WALL_PLANE_NEGATE, cd.DOUBLE, flags=1, planes=planes)
    assert (l["kind"], l["cls"], l["vec"]) == (42, 2, 8), l
