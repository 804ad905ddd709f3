"""2-byte element types of cudecomp_amd.h (fp16, bf16) and complex-fp16, without a GPU: the API accepts them and nothing
else new, the header stands alone and is clean under UBSan's enum check, the kernel layer's choices for 2-byte moves are the
intended ones (16-byte lanes only at dword-aligned addresses, never the window / lines / row-lines / shifted / dense kernels),
and the planner's transposes carry a uint16 payload over gloo on 4 ranks."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cudecomp_amd as cd
from tests import half_bodies as HB
from tests.mp import run_ranks
from tests.test_kernel_choice_pins import _halos, _transposes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cudecomp_amd.h")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CFLAGS = ["-I" + os.path.join(ROOT, "include"), "-isystem", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__"]


def test_sizes_of_the_new_types_and_invalid_values():
    assert cd.cudecompGetDataTypeSize(cd.HALF) == 2
    assert cd.cudecompGetDataTypeSize(cd.BFLOAT16) == 2
    assert cd.cudecompGetDataTypeSize(cd.HALF_COMPLEX) == 4
    n = C.c_int64()
    for bad in (0, 4, -5, 999):
        assert cd.lib().cudecompGetDataTypeSize(bad, C.byref(n)) == cd.RESULT_INVALID_USAGE, bad


def test_header_constants_match_the_python_mirror():
    text = open(HEADER).read()
    found = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+CUDECOMP_AMD_(\w+)\s+\(\(cudecompDataType_t\)(-?\d+)\)", text)}
    assert found == {"HALF": cd.HALF, "BFLOAT16": cd.BFLOAT16, "HALF_COMPLEX": cd.HALF_COMPLEX}


@pytest.mark.parametrize("lang", ["c99", "c++17"])
def test_header_compiles_standalone(tmp_path, lang):
    src = tmp_path / ("t.c" if lang == "c99" else "t.cc")
    src.write_text('#include "cudecomp_amd.h"\nint main(void) { cudecompDataType_t t = CUDECOMP_AMD_HALF; return (int)t - 1; }\n')
    cc = ["gcc", "-std=c99"] if lang == "c99" else ["g++", "-std=c++17"]
    r = subprocess.run(cc + ["-Wall", "-Werror", "-pedantic-errors", "-fsyntax-only"] + CFLAGS + [str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_constants_in_enum_variables_are_clean_under_ubsan(tmp_path):
    src = tmp_path / "enum_check.cc"
    src.write_text(r'''#include <cstdio>
#include "cudecomp_amd.h"
int main() {
  volatile cudecompDataType_t t[3] = {CUDECOMP_AMD_HALF, CUDECOMP_AMD_BFLOAT16, CUDECOMP_AMD_HALF_COMPLEX};
  int sum = 0;
  for (int i = 0; i < 3; ++i) {
    cudecompDataType_t v = t[i];  // a load through the enum type: what -fsanitize=enum checks
    sum += (int)v;
  }
  std::printf("%d\n", sum);
  return sum == 6 ? 0 : 1;
}
''')
    exe = tmp_path / "enum_check"
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-fsanitize=enum", "-fno-sanitize-recover=all"] + CFLAGS +
                       [str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "6" and "runtime error" not in r.stderr, (r.stdout, r.stderr)


# ---- classifier choices (cudecompExtDescribeMove; entries as in tests/test_kernel_choice_pins.py:
# [class, variant, tile_i, tile_j, p0 (run), p1 (walk bits), access mode]) ----------------------------------------------------
def test_fp16_8gib_cycle_takes_16_byte_lanes():
    n = (2048, 2048, 1024)
    contiguous = _transposes(n, (1, 1), (1, 1, 1), 2)
    # forward hops: 128 x 128 tiles, 16-byte lanes, the run walk over far-strided destinations; inverse hops j first
    assert contiguous["XToY"]["pack"] == [[1, 8, 128, 128, 1024, 3, 2]]
    assert contiguous["YToZ"]["pack"] == [[1, 8, 128, 128, 1024, 3, 2]]
    assert contiguous["ZToY"]["pack"] == [[1, 8, 128, 128, 0, 3, 2]]
    assert contiguous["YToX"]["pack"] == [[1, 8, 128, 128, 0, 3, 2]]
    default = _transposes(n, (1, 1), (0, 0, 0), 2)
    assert all(v["pack"] == [[0, 16, 0, 0, 8, 0, 2]] for v in default.values()), default   # 16-byte rows
    in_place = _transposes(n, (1, 1), (1, 1, 1), 2, inplace=True)
    assert all(v["pack"][0][:4] == [1, 8, 128, 128] and v["unpack"] == [[0, 16, 0, 0, 8, 0, 2]] for v in in_place.values())


def _describe(src, dst, es, extent, ss, ds, flags=0, row_pitch=0):
    return cd.cudecompExtDescribeMove(src, dst, es, extent, ss, ds, flags=flags, row_pitch=row_pitch)


BASE_S, BASE_D = 1 << 32, 1 << 36


def test_2_byte_moves_at_2_mod_4_never_take_4_byte_or_wider_accesses():
    cases = []
    for so, do in ((1, 0), (0, 1), (3, 5), (0, 0)):
        for ext, ss, ds in (((64, 64, 4), (1, 64, 4096), (64, 1, 4096)),        # transposition, dense rows
                            ((64, 64, 4), (1, 66, 66 * 66), (66, 1, 66 * 64)),   # halo-1 pencils: rows at 2 mod 4
                            ((66, 64, 4), (1, 66, 66 * 64), (1, 66, 66 * 64)),  # row copies
                            ((64, 64, 4), (1, 65, 65 * 64), (1, 64, 4096)),      # odd source pitch
                            ((128, 8, 2), (1, 128, 1024), (1, 131, 8 * 131))):   # odd destination pitch
            cases.append((so, do, ext, ss, ds))
    for so, do, ext, ss, ds in cases:
        d = _describe(BASE_S + 2 * so, BASE_D + 2 * do, 2, ext, ss, ds)
        odd = (so | do) & 1 or any(s != 1 and s % 2 for s in ss + ds)   # some row or base at 2 mod 4 bytes
        width = d["variant"] if d["cls"] == 0 else (2 * d["variant"] if d["cls"] == 1 else 2)
        if odd:
            assert width == 2, (so, do, ext, ss, ds, d)
        assert d["cls"] != 0 or d["tile_i"] == 0, d   # rows: the plain kernel only


def test_2_byte_moves_never_take_the_excluded_kernels():
    # the same large move onto destination rows off the 64-byte grid: 4-byte elements take the window kernel (streaming
    # whole-unit stores, j first), 2-byte elements the plain tiled kernel (cached stores, i first)
    ext, ss, ds = (512, 512, 64), (1, 520, 520 * 512), (514, 1, 514 * 512)   # (32 MiB and more: streaming access)
    w4 = _describe(BASE_S, BASE_D + 4, 4, ext, ss, ds)
    assert w4["cls"] == 1 and w4["access"] == 4 and w4["walk"] & 2
    w2 = _describe(BASE_S, BASE_D + 4, 2, ext, ss, ds)
    assert w2 == dict(w2, cls=1, variant=8, tile_i=128, tile_j=128, access=0) and not w2["walk"] & (2 | 8 | 16), w2
    # flag 4 (window kernel whenever the destination is misaligned) does not apply to 2-byte elements either
    assert _describe(BASE_S, BASE_D + 4, 2, ext, ss, ds, flags=4) == w2
    # whole interior rows of halo-carrying pencils (the planner's row pitch): lines / row-lines for 4 bytes, not for 2
    for es in (4, 2):
        fwd = _transposes((512, 512, 256), (1, 1), (1, 1, 1), es, halo=(1, 1, 1))
        walks = [m[5] for v in fwd.values() for m in v["pack"] + v["unpack"]]
        assert any(w & (8 | 16) for w in walks) == (es == 4), (es, walks)
    # row copies onto halo rows: shifted / dense kernels for 4 bytes, the plain one for 2
    for es in (4, 2):
        d = _transposes((512, 512, 256), (1, 1), (0, 0, 0), es, halo=(1, 1, 1))
        kinds = {m[2] for v in d.values() for m in v["pack"] + v["unpack"] if m[0] == 0}
        assert (kinds == {0}) == (es == 2), (es, kinds)
    faces = _halos((256, 256, 128), (2, 2), (0, 0, 0), 2, (3, 3, 3))
    assert all(m[0] != 0 or m[2] == 0 for v in faces.values() for m in v), faces


def test_uint16_plans_over_gloo_four_ranks():
    backends = [cd.TRANSPOSE_COMM_NCCL, cd.TRANSPOSE_COMM_MPI_P2P]
    for pdims, ac in (((2, 2), (0, 0, 0)), ((1, 4), (1, 1, 1))):
        args = {"gdims": (13, 10, 11), "pdims": pdims, "ac": ac, "backends": backends,
                "halos": [(1, 1, 1), (0, 0, 0), (2, 1, 3)], "pads": [(0, 1, 0), (1, 1, 1), (0, 0, 0)]}
        for failures in run_ranks(4, "tests.half_bodies", "plan_transpose_gloo", args):
            assert failures == []
