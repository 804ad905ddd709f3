"""Multi-field halo updates (cudecomp_halo_fields.h: cudecompAmdUpdateFieldHalos{X,Y,Z}) as a C / C++ solver calls them:
tests/native/halo_fields_test.cpp includes the header and calls every entry point through its prototype there, and compares whole
pencils, byte for byte, with closed forms built from the header's text (no tolerance: the payloads are small integers).  Everything
else in the suite reaches these functions through ctypes argtypes written by hand.

The case lists: the 16 x 20 x 18 grid of tests/halo_ops_cases.py (ragged slabs on 1 x 4 and 4 x 1) with its three (halo, periods,
padding) sets, every axis, both layouts; `--fields N` cycles through 2, 3, 9, 1, 4.  The program is built on demand by
tests/native/fields.mk."""
import itertools
import os
import shutil
import subprocess
import tempfile
import time

import pytest

from tests.halo_ops_cases import GRID, SETS
from tests.mp import ROOT, run_binary_ranks
from tests.test_gpu_native import NATIVE, _run_side_by_side

pytestmark = pytest.mark.gpu
FORTRAN_BUILD = os.path.join(ROOT, "fortran", "build")
COUNTS = (2, 3, 9, 1, 4)


def _binary(name):
    path = os.path.join(NATIVE, "build", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", NATIVE, "-f", "fields.mk", "build/" + name], check=True, capture_output=True)
    return path


def _fortran_binary():
    path = os.path.join(FORTRAN_BUILD, "fortran", "halo_fields_test_R64")
    if not os.path.exists(path):
        if shutil.which("amdflang") is None:
            pytest.skip("amdflang not installed")
        subprocess.run(["make", "-C", os.path.join(ROOT, "cudecomp_amd")], check=True, capture_output=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "fortran"), "all", "fields_test"], check=True, capture_output=True)
    return path


class Forms:
    """what varies from case to case beside the geometry: the number of fields, padding = NULL every other time it is zero, and for
    the Fortran twin (base 1: one-based --ax) `stream` present two times in three"""

    def __init__(self, base=0):
        self.n, self.nullpad, self.base, self.stream = 0, 0, base, 0

    def line(self, pdims, backend, ax, ac, halo, per, pad, grid=GRID, more=""):
        text = "--pr %d --pc %d %s --backend %d --ax %d --ac %d --hex %d --hey %d --hez %d --hpx %d --hpy %d --hpz %d " \
               "--pdx %d --pdy %d --pdz %d" % (tuple(pdims) + (grid, backend, ax + self.base, ac) + tuple(halo) + tuple(per) + tuple(pad))
        text += " --fields %d" % COUNTS[self.n % len(COUNTS)]
        self.n += 1
        if not any(pad):
            self.nullpad += 1
            if self.nullpad % 2 == 0:
                text += " --nullpad"
        if self.base:
            self.stream += 1
            if self.stream % 3 != 1:
                text += " --stream"
        return text + more


def single_rank_lines(forms, more=""):
    return [forms.line((1, 1), 3, ax, ac, h, per, pad, more=more) for ax, ac, (h, per, pad) in itertools.product((0, 1, 2), (0, 1), SETS)]


def four_rank_lines(forms):
    return [forms.line(pdims, 1, ax, (i + ax) % 2, h, per, pad)
            for pdims in ((2, 2), (1, 4), (4, 1)) for i, (ax, (h, per, pad)) in enumerate(itertools.product((0, 1, 2), SETS))]


def test_the_lists_reach_every_count_and_form():
    lines = single_rank_lines(Forms())
    assert all(any(" --fields %d" % n in l + " " for l in lines) for n in COUNTS)
    assert any("--nullpad" in l for l in lines) and any("--nullpad" not in l for l in lines)
    assert any("--hpx 0 --hpy 0 --hpz 0" in l for l in lines) and any("--hpx 1 --hpy 1 --hpz 1" in l for l in lines)


@pytest.mark.parametrize("dtype", ["R32", "R64", "C64", "H16"])
def test_native_halo_fields_single_rank(dtype):
    _run_side_by_side([("halo_fields_test_" + dtype, 1, single_rank_lines(Forms()), None)], path_of=_binary)


def test_native_halo_fields_four_ranks():
    """four ranks sharing the GPU, R64, over process grids 2 x 2, 1 x 4 and 4 x 1: one exchange per direction carries every field"""
    _run_side_by_side([("halo_fields_test_R64", 4, four_rank_lines(Forms()), None)], path_of=_binary)


def test_native_halo_fields_comparison_can_fail():
    """--self-check-shift-dim: the second of three cases calls along (dim + 1) % 3 while expecting dim; it must report FAILED and end
    the list there, within seconds"""
    good = [l for l in single_rank_lines(Forms()) if "--hpx 1 --hpy 1 --hpz 1" in l][:3]
    lines = [good[0], good[1] + " --self-check-shift-dim", good[2]]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_binary("halo_fields_test_R64"), "--testfile", f.name], 120,
                             {"CUDECOMP_TEST_STOP_AT_FIRST_FAILURE": "1", "CUDECOMP_TEST_VERDICT_TIMEOUT": "60"})
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert "Stopping at the first failing case (2 of 3 run)" in text and " FAILED" in text, text[-2000:]
    assert "differ after the update along dim" in text, text[-2000:]
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


def test_fortran_halo_fields_single_rank():
    lines = single_rank_lines(Forms(base=1))
    assert any("--stream" in l for l in lines) and any("--stream" not in l for l in lines)
    assert _run_fortran(1, lines) == ["cudecompAmdUpdateFieldHalos" + a for a in "XYZ"]


def test_fortran_halo_fields_four_ranks():
    assert _run_fortran(4, four_rank_lines(Forms(base=1))) == ["cudecompAmdUpdateFieldHalos" + a for a in "XYZ"]


def test_fortran_halo_fields_comparison_can_fail():
    good = [l for l in single_rank_lines(Forms(base=1)) if "--hpx 1 --hpy 1 --hpz 1" in l][:3]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join([good[0], good[1] + " --self-check-shift-dim", good[2]]) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_fortran_binary(), "--testfile", f.name], 120)
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert text.count(" PASSED") == 1 and text.count(" FAILED") == 1 and "Failed 1/3 tests." in text, text[-2000:]
    assert "differ after the update along dim" in text, text[-2000:]
    assert time.time() - t0 < 30
