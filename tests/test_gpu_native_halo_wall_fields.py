"""Multi-field wall halos (cudecomp_halo_wall_fields.h: cudecompAmdReflectFieldHalos{X,Y,Z}, cudecompAmdFoldFieldHalos{X,Y,Z}) as a
C / C++ and as a Fortran solver call them: tests/native/halo_wall_fields_test.cpp includes the header and calls every entry point
through its prototype there, tests/fortran/halo_wall_fields_test.f90 goes through the six wrappers of module `cudecomp`; both compare
whole pencils of every field, byte for byte, with the header's formulas applied on the host (no tolerance: the payloads are small
integers without a zero).  Everything else in the suite reaches these functions through ctypes argtypes written
by hand.

The case lists: the 16 x 20 x 18 grid of tests/halo_ops_cases.py with its two (halo, periods, padding) sets that have walls and one
more without padding, every
axis, both layouts, on one rank and on four ranks as 1 x 4 and 4 x 1 (ragged slabs; every case accepted: h + centering <= the
narrowest slab of 4 cells); the parities come from the command line and cycle through five lists of 1, 2, 3, 4 and 9 fields, the
operation through reflect / fold / fold that clears, the centering through 0 / 1.  The C++ program is built on demand by
tests/native/wall_fields.mk, the Fortran one by the wall_fields_test target of fortran/Makefile."""
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
WRAPPERS = sorted("cudecompAmd%sFieldHalos%s" % (k, a) for k in ("Reflect", "Fold") for a in "XYZ")
# the sets with a non-periodic dim, and walls along dims 0 and 2 without padding (the form that may pass padding = NULL)
WALLS = [s for s in SETS if not all(s[1])] + [((1, 1, 1), (0, 1, 0), (0, 0, 0))]
PARITIES = ["-1 +1 -1", "+1 -1", "-1", "-1 -1 +1 +1", "+1 -1 -1 +1 -1 +1 +1 -1 -1"]
FORMS = [("reflect", 0, 0), ("fold", 0, 0), ("fold", 1, 1), ("reflect", 1, 0), ("fold", 1, 0), ("fold", 0, 1)]  # (op, centering, clear)


def _binary(name):
    path = os.path.join(NATIVE, "build", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", NATIVE, "-f", "wall_fields.mk", "build/" + name], check=True, capture_output=True)
    return path


def _fortran_binary():
    path = os.path.join(FORTRAN_BUILD, "fortran", "halo_wall_fields_test_R64")
    if not os.path.exists(path):
        if shutil.which("amdflang") is None:
            pytest.skip("amdflang not installed")
        subprocess.run(["make", "-C", os.path.join(ROOT, "cudecomp_amd")], check=True, capture_output=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "fortran"), "all", "wall_fields_test"], check=True, capture_output=True)
    return path


class Forms:
    """what varies from case to case beside the geometry: the operation with its centering and clear, the list of parities,
    padding = NULL every other time the padding is zero, and for the Fortran twin (base 1) `stream` present two times in three"""

    def __init__(self, base=0):
        self.base, self.n, self.nullpad, self.stream = base, 0, 0, 0

    def line(self, pdims, backend, ax, ac, halo, per, pad, more=""):
        text = "--pr %d --pc %d %s --backend %d --ax %d --ac %d --hex %d --hey %d --hez %d --hpx %d --hpy %d --hpz %d " \
               "--pdx %d --pdy %d --pdz %d" % (tuple(pdims) + (GRID, backend, ax + self.base, ac) + tuple(halo) + tuple(per) + tuple(pad))
        op, centering, clear = FORMS[self.n % len(FORMS)]
        text += " --op %s --centering %d --clear %d --parities %s" % (op, centering, clear, PARITIES[self.n % len(PARITIES)])
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


def single_rank_lines(forms):
    return [forms.line((1, 1), 3, ax, ac, h, per, pad) for _, ax, ac, (h, per, pad) in itertools.product(range(3), (0, 1, 2), (0, 1), WALLS)]


def four_rank_lines(forms):
    return [forms.line(pdims, 1, ax, (i + ax) % 2, h, per, pad)
            for pdims in ((1, 4), (4, 1)) for i, (ax, (h, per, pad)) in enumerate(itertools.product((0, 1, 2), WALLS + WALLS[::-1]))]


def test_the_lists_reach_every_form_with_every_list_of_parities():
    lines = single_rank_lines(Forms())
    assert len(WALLS) == 3 and len(lines) == 54
    for (op, centering, clear), parities in itertools.product(FORMS, PARITIES):  # (6 and 5 are coprime: 30 pairs in 54 lines)
        assert any("--op %s --centering %d --clear %d --parities %s" % (op, centering, clear, parities) in l + " " for l in lines)
    assert any("--nullpad" in l for l in lines) and any("--nullpad" not in l for l in lines)
    four = four_rank_lines(Forms())
    assert any("--pr 1 --pc 4" in l for l in four) and any("--pr 4 --pc 1" in l for l in four)


@pytest.mark.parametrize("dtype", ["R32", "R64", "C64", "H16"])
def test_native_single_rank(dtype):
    _run_side_by_side([("halo_wall_fields_test_" + dtype, 1, single_rank_lines(Forms()), None)], path_of=_binary)


def test_native_four_ranks():
    """four ranks sharing the GPU, R64, process grids 1 x 4 and 4 x 1: every rank serves the sides on which cudecompGetShiftedRank
    names no neighbour, and only those"""
    _run_side_by_side([("halo_wall_fields_test_R64", 4, four_rank_lines(Forms()), None)], path_of=_binary)


def test_native_comparison_can_fail():
    """--self-check-shift-dim: the second of three cases calls along (dim + 1) % 3 while expecting dim; it must report FAILED and end
    the list there, within seconds"""
    good = [l for l in single_rank_lines(Forms()) if "--hpx 0 --hpy 0 --hpz 0" in l][:3]
    lines = [good[0], good[1] + " --self-check-shift-dim", good[2]]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_binary("halo_wall_fields_test_R64"), "--testfile", f.name], 120,
                             {"CUDECOMP_TEST_STOP_AT_FIRST_FAILURE": "1", "CUDECOMP_TEST_VERDICT_TIMEOUT": "60"})
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert "Stopping at the first failing case (2 of 3 run)" in text and " FAILED" in text, text[-2000:]
    assert "differ after the" in text, text[-2000:]
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
    lines = single_rank_lines(Forms(base=1))
    assert any("--stream" in l for l in lines) and any("--stream" not in l for l in lines)
    assert _run_fortran(1, lines) == WRAPPERS


def test_fortran_four_ranks():
    assert _run_fortran(4, four_rank_lines(Forms(base=1))) == WRAPPERS


def test_fortran_comparison_can_fail():
    good = [l for l in single_rank_lines(Forms(base=1)) if "--hpx 0 --hpy 0 --hpz 0" in l][:3]
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
    assert "differ after the call along dim" in text, text[-2000:]
    assert time.time() - t0 < 30
