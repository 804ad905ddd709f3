"""cudecomp_halo_fold.h (cudecompAmdFoldHalos{X,Y,Z}) as a C interface: the three symbols are exported, the header's parameters
agree with the ctypes argtypes every Python test calls through, the header compiles as C11 under -Wall -Wextra -Werror, and the
design document spells the two kernels the way the library names them.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import cudecomp_amd as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "cudecomp_halo_fold.h"


def _prototypes(header):
    """{function: [parameter text, ...]} of the cudecompResult_t functions a header declares"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return {name: [" ".join(a.split()) for a in args.split(",")]
            for name, args in re.findall(r"cudecompResult_t\s+(cudecomp\w+)\s*\(([^)]*)\)\s*;", src)}


def test_the_three_symbols_are_declared_and_exported():
    assert cd.AMD_FOLD_SYMBOLS == ["cudecompAmdFoldHalos" + a for a in "XYZ"]
    assert sorted(_prototypes(HEADER)) == sorted(cd.AMD_FOLD_SYMBOLS)
    L = cd.lib()
    for name in cd.AMD_FOLD_SYMBOLS + ["cudecompExtPlanHaloFold", "cudecompExtFold3D"]:
        assert hasattr(L, name), name
    assert {"cudecompExtPlanHaloFold", "cudecompExtFold3D"} <= set(cd.EXT_SYMBOLS) & set(_prototypes("cudecomp_ext.h"))
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "cudecomp_amd.h"' in text
    # the header's name keeps it out of the family tests/test_abi.py counts, and the package's table of that family is as it was
    assert not HEADER.startswith("cudecomp_amd") and HEADER not in cd.AMD_HEADER_SYMBOLS
    assert not any("Fold" in n for names in cd.AMD_HEADER_SYMBOLS.values() for n in names)
    assert (cd.MOVES_FOLD, cd.MOVES_FOLD_NEGATE, cd.MOVES_FOLD_TAKE, cd.MOVES_FOLD_NEGATE_TAKE) == (7, 8, 9, 10)


def test_prototypes_agree_with_the_argtypes():
    """as many parameters in the header as in the argtypes, the pointers -- arrays, the buffer, and the handle, descriptor and
    stream, which are pointers in C -- at the same positions, everything else a 32-bit integer on both sides; `clear` follows
    `centering`"""
    L = cd.lib()
    opaque = ("cudecompHandle_t", "cudecompGridDesc_t", "hipStream_t")
    protos = _prototypes(HEADER)
    for name in cd.AMD_FOLD_SYMBOLS:
        params, argtypes = protos[name], getattr(L, name).argtypes
        assert len(params) == len(argtypes) == 12, (name, params)
        in_header = ["*" in p or "[" in p or p.split()[0] in opaque for p in params]
        in_python = [t is C.c_void_p or t is C.c_char_p or hasattr(t, "contents") for t in argtypes]
        assert in_header == in_python, (name, params, argtypes)
        assert [i for i, ptr in enumerate(in_header) if ptr] == [0, 1, 2, 7, 8, 10, 11]
        assert all(p.split()[0] in ("int32_t", "cudecompDataType_t") for p, ptr in zip(params, in_header) if not ptr), (name, params)
        assert all(t is C.c_int32 for t, ptr in zip(argtypes, in_python) if not ptr), (name, argtypes)
        assert [p.split()[-1] for p in params[3:7]] == ["dtype", "parity", "centering", "clear"]
    # the reflection's prototype with `clear` taken out
    reflect = _prototypes("cudecomp_amd_reflect.h")
    for name in cd.AMD_FOLD_SYMBOLS:
        assert [p for p in protos[name] if p != "int32_t clear"] == reflect[name.replace("Fold", "Reflect")]


def test_header_compiles_as_c11(tmp_path):
    """alone, before and after the other extension headers, with every function assigned to a pointer of the prototype written
    out by hand -- and the compile line does notice a prototype that differs"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    base = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
            "-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(rocm, "include")]
    proto = ("cudecompResult_t (*%s)(cudecompHandle_t, cudecompGridDesc_t, void*, cudecompDataType_t, int32_t, int32_t, int32_t,\n"
             "    const int32_t[], const bool[], int32_t, const int32_t[], hipStream_t) = %s;\n")
    body = "".join(proto % ("p" + a, "cudecompAmdFoldHalos" + a) for a in "XYZ") + "int main(void) { return pX == pY && pY == pZ; }\n"
    others = ['#include "cudecomp_amd_fill.h"\n#include "cudecomp_amd_reflect.h"\n', ""]
    for before, after in ((others[1], others[1]), (others[0], others[1]), (others[1], others[0])):
        src = tmp_path / "fold_header.c"
        src.write_text(before + '#include "%s"\n' % HEADER + after + '#include "%s"\n' % HEADER + body)
        res = subprocess.run(base + [str(src)], capture_output=True, text=True)
        assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]
    src.write_text('#include "%s"\n' % HEADER + body.replace("int32_t, int32_t, int32_t,\n", "int32_t, int32_t, const int32_t*,\n"))
    res = subprocess.run(base + [str(src)], capture_output=True, text=True)
    assert res.returncode != 0 and "incompatible" in res.stderr, res.stderr[-3000:]


def test_the_design_document_spells_the_kernels():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "`rows_fold_kernel<T,VB,STREAM,TAKE>`" in text and "`generic_fold_kernel<T,NC,TAKE>`" in text
    # ... and says that the access-mode rule is unmeasured for them
    para = [p for p in text.split("\n\n") if "Fold-moves" in p]
    assert para and any("unmeasured" in p or "not measured" in p or "nobody has measured" in p.lower() for p in para)
