"""cudecomp_halo_wall_values.h (cudecompAmdSetWallHalos{X,Y,Z}) as a C interface: the three symbols are exported, the header's
parameters agree with the ctypes argtypes every Python test calls through, the header compiles as C11 under -Wall -Wextra -Werror
alone and around the other extension headers, and the design document spells the two kernels the way the library names them.  No
GPU needed."""
import ctypes as C
import os
import re
import subprocess

import cudecomp_amd as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cudecomp_halo_wall_values.h"
EXT = ["cudecompExtPlanHaloWallValues", "cudecompExtWall3D"]


def _prototypes(header):
    """{function: [parameter text, ...]} of the cudecompResult_t functions a header declares"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_three_symbols_are_declared_and_exported():
    assert cd.AMD_WALL_VALUES_SYMBOLS == ["cudecompAmdSetWallHalos" + a for a in "XYZ"] and cd.MAX_WALL_HALO == 8
    assert sorted(_prototypes(HEADER)) == sorted(cd.AMD_WALL_VALUES_SYMBOLS)
    L = cd.lib()
    for name in cd.AMD_WALL_VALUES_SYMBOLS + EXT:
        assert hasattr(L, name), name
    assert set(EXT) <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp_amd.h"' in text and re.search(r"#define\s+CUDECOMP_AMD_MAX_WALL_HALO\s+8\b", text)
    # the header's name keeps it out of the family tests/test_abi.py counts, and the package's table of that family is as it was
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS
    assert not any("Wall" in n for names in cd.AMD_HEADER_SYMBOLS.values() for n in names)
    assert (cd.MOVES_WALL, cd.MOVES_WALL_NEGATE) == (11, 12)


def test_prototypes_agree_with_the_argtypes():
    """as many parameters in the header as in the argtypes, the pointers -- arrays, the buffer, and the handle, descriptor and
    stream, which are pointers in C -- at the same positions, everything else a 32-bit integer on both sides; the reflection's
    prototype with `sides` and the two arrays of doubles after `centering`"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    reflect = _prototypes("cudecomp_amd_reflect.h")
    for name in cd.AMD_WALL_VALUES_SYMBOLS:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 14, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 7, 8, 9, 10, 12, 13]
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        assert params[6:9] == ["int32_t sides", "const double values_low[]", "const double values_high[]"]
        assert argtypes[7]._type_ is C.c_double and argtypes[8]._type_ is C.c_double
        assert params[:6] + params[9:] == reflect[name.replace("SetWallHalos", "ReflectHalos")]
    ext = _prototypes("cudecomp_ext.h")
    for name in EXT:
        assert len(getattr(L, name).argtypes) == len(ext[name]), name


def test_header_compiles_as_c11():
    """tests/native/wall_values_header_c11.c: alone, after and before the other extension headers -- and the compile line does
    notice a prototype that differs"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")]
    source = os.path.join(ROOT, "tests", "native", "wall_values_header_c11.c")
    for defs in ([], ["-DOTHERS_FIRST"], ["-DOTHERS_LAST"], ["-DOTHERS_FIRST", "-DOTHERS_LAST"]):
        res = subprocess.run(base + defs + [source], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), (defs, res.stderr[-3000:])
    res = subprocess.run(base + ["-DSIDES_TYPE=const int32_t*", source], capture_output=True, text=True)
    assert res.returncode != 0 and "incompatible" in res.stderr, res.stderr[-3000:]


def test_the_documents_name_the_call_and_its_kernels():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`rows_wall_kernel<T,VB,STREAM,NEG>`" in text and "`generic_wall_kernel<T,ES,NEG>`" in text
    para = [p for p in text.split("\n\n") if "Wall-moves" in p]
    assert para and any("unmeasured" in p or "not measured" in p for p in para)
    for doc in ("README.md", "INTEGRATION.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
