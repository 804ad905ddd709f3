"""Multi-field halo accumulation (cudecomp_halo_accumulate_fields.h: cudecompAmdAccumulateFieldHalos{X,Y,Z}) as a C / C++ and as a
Fortran solver call it: tests/native/halo_accumulate_fields_test.cpp includes the header and calls every entry point through its
prototype there, tests/fortran/halo_accumulate_fields_test.f90 goes through the wrappers of module `cudecomp`; both compare whole
pencils, byte for byte, with the single calls the header names as the definition (no tolerance: the payloads are small integers).
Everything else in the suite reaches these functions through ctypes argtypes written by hand.

The case lists are those of tests/test_gpu_native_halo_fields.py (the 16 x 20 x 18 grid of tests/halo_ops_cases.py with its three
(halo, periods, padding) sets, every axis, both layouts; `--fields N` cycling through 2, 3, 9, 1, 4) with `--clear` alternating.
The programs are built on demand by tests/native/accumulate_fields.mk and fortran/Makefile."""
import os
import shutil
import subprocess
import tempfile
import time

import pytest

from tests.mp import ROOT, run_binary_ranks
from tests.test_gpu_native import NATIVE, _run_side_by_side
from tests.test_gpu_native_halo_fields import COUNTS, Forms, four_rank_lines, single_rank_lines

pytestmark = pytest.mark.gpu
FORTRAN_BUILD = os.path.join(ROOT, "fortran", "build")
WRAPPERS = ["cudecompAmdAccumulateFieldHalos" + a for a in "XYZ"]


def _binary(name):
    path = os.path.join(NATIVE, "build", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", NATIVE, "-f", "accumulate_fields.mk", "build/" + name], check=True, capture_output=True)
    return path


def _fortran_binary():
    path = os.path.join(FORTRAN_BUILD, "fortran", "halo_accumulate_fields_test_R64")
    if not os.path.exists(path):
        if shutil.which("amdflang") is None:
            pytest.skip("amdflang not installed")
        subprocess.run(["make", "-C", os.path.join(ROOT, "cudecomp_amd")], check=True, capture_output=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "fortran"), "all", "accumulate_fields_test"], check=True, capture_output=True)
    return path


def _with_clear(lines):
    """--clear 0, 1, 1, 0, ...: period 4 against the field counts' period 5, so every count meets both"""
    return [l + " --clear %d" % (1 if i % 4 in (1, 2) else 0) for i, l in enumerate(lines)]


def test_the_lists_reach_every_count_with_both_values_of_clear():
    lines = _with_clear(single_rank_lines(Forms()))
    for n in COUNTS:
        assert {l.rsplit(" ", 1)[1] for l in lines if " --fields %d " % n in l + " "} == {"0", "1"}, n
    assert any("--nullpad" in l for l in lines) and any("--nullpad" not in l for l in lines)


@pytest.mark.parametrize("dtype", ["R32", "R64", "C64", "H16"])
def test_native_single_rank(dtype):
    _run_side_by_side([("halo_accumulate_fields_test_" + dtype, 1, _with_clear(single_rank_lines(Forms())), None)], path_of=_binary)


def test_native_four_ranks():
    """four ranks sharing the GPU, R64, over process grids 2 x 2, 1 x 4 and 4 x 1: one exchange per direction carries every field"""
    _run_side_by_side([("halo_accumulate_fields_test_R64", 4, _with_clear(four_rank_lines(Forms())), None)], path_of=_binary)


def _shifted_case_file(base):
    good = [l for l in _with_clear(single_rank_lines(Forms(base=base))) if "--hpx 1 --hpy 1 --hpz 1" in l][:3]
    f = tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False)
    f.write("\n".join([good[0], good[1] + " --self-check-shift-dim", good[2]]) + "\n")
    f.close()
    return f.name


def test_native_comparison_can_fail():
    """--self-check-shift-dim: the second of three cases calls along (dim + 1) % 3 while the single calls run along dim; it must
    report FAILED and end the list there, within seconds"""
    name = _shifted_case_file(0)
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_binary("halo_accumulate_fields_test_R64"), "--testfile", name], 120,
                             {"CUDECOMP_TEST_STOP_AT_FIRST_FAILURE": "1", "CUDECOMP_TEST_VERDICT_TIMEOUT": "60"})
    finally:
        os.unlink(name)
    text = str(e.value)
    assert "Stopping at the first failing case (2 of 3 run)" in text and " FAILED" in text, text[-2000:]
    assert "differ after the accumulation along dim" in text, text[-2000:]
    assert time.time() - t0 < 30


# ---- the Fortran twin ------------------------------------------------------------------------------------------------------
def _run_fortran(nranks, lines):
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        logs = run_binary_ranks(nranks, [_fortran_binary(), "--testfile", f.name], timeout=900)
    finally:
        os.unlink(f.name)
    out = logs[0]
    ok = out.count(" PASSED") == len(lines) and " FAILED" not in out and "Passed all tests." in out
    assert ok, "\n".join("===== rank %d =====\n%s" % (r, text[-3000:]) for r, text in enumerate(logs))
    return sorted(line.split()[1] for line in out.splitlines() if line.startswith("WRAPPER "))


def test_fortran_single_rank():
    lines = _with_clear(single_rank_lines(Forms(base=1)))
    assert any("--stream" in l for l in lines) and any("--stream" not in l for l in lines)
    assert _run_fortran(1, lines) == WRAPPERS


def test_fortran_four_ranks():
    assert _run_fortran(4, _with_clear(four_rank_lines(Forms(base=1)))) == WRAPPERS


def test_fortran_comparison_can_fail():
    name = _shifted_case_file(1)
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_fortran_binary(), "--testfile", name], 120)
    finally:
        os.unlink(name)
    text = str(e.value)
    assert text.count(" PASSED") == 1 and text.count(" FAILED") == 1 and "Failed 1/3 tests." in text, text[-2000:]
    assert "differ after the accumulation along dim" in text, text[-2000:]
    assert time.time() - t0 < 30
