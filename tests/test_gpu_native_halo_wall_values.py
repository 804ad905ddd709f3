"""Wall values (cudecomp_halo_wall_values.h: cudecompAmdSetWallHalos{X,Y,Z}) as a C / C++ and as a Fortran solver call them:
tests/native/halo_wall_values_test.cpp includes the header and calls every entry point through its prototype there,
tests/fortran/halo_wall_values_test.f90 goes through the three wrappers of module `cudecomp`; both compare the whole pencil, byte for
byte, after every call with the header's definition applied on the host (no tolerance: payload and addends are small integers, every
sum exact in fp16 and wider, no addend zero).  Everything else in the suite reaches these functions through ctypes argtypes written
by hand; nothing else runs the Fortran wrappers, which turn two optional assumed-size arrays into pointers, count `dim` from one and
pass 2 h interleaved doubles for the complex types.

The case lists: the 16 x 20 x 18 grid of tests/halo_ops_cases.py with its two (halo, periods, padding) sets that have walls, one
more without padding (the form that may leave `padding` out) and one with three ghost layers per side, every axis, both layouts, on
one rank and on four ranks as 1 x 4 and 4 x 1 (ragged slabs; every case accepted: h + centering <= the narrowest slab of 4 cells).
From case to case parity x centering cycle through the four mirrors, --sides through 3, 1, 2 and --unnamed (what is passed for the
side --sides leaves out) through null and garbage.  The value arrays are temporaries that hold NaNs as soon as the call has returned.
The C++ program is built on demand by tests/native/wall_values.mk, the Fortran one by the wall_values_test target of
fortran/Makefile."""
import itertools
import os
import shutil
import subprocess
import tempfile
import time

import pytest

from tests.halo_ops_cases import GRID, MIRRORS, SETS
from tests.mp import ROOT, run_binary_ranks
from tests.test_gpu_native import NATIVE, _run_side_by_side

pytestmark = pytest.mark.gpu
FORTRAN_BUILD = os.path.join(ROOT, "fortran", "build")
WRAPPERS = ["cudecompAmdSetWallHalos" + a for a in "XYZ"]
WIDE = ((3, 2, 3), (0, 0, 0), (1, 0, 2))  # three layers per side; h + centering = 4 fits the 4-cell slabs of the four-rank grids
# the sets with a non-periodic dim, walls along dims 0 and 2 without padding (the form that may pass padding = NULL), the wide one
WALLS = [s for s in SETS if not all(s[1])] + [((1, 1, 1), (0, 1, 0), (0, 0, 0)), WIDE]
SIDES = (3, 1, 2)
UNNAMED = ("null", "garbage")


class Forms:
    """what varies from case to case beside the geometry: the mirror (n mod 4), the sides (n mod 3), what the unnamed side is given
    (n / 4 mod 2: 24 combinations in 24 consecutive cases), padding = NULL every other time the padding is zero, and for the
    Fortran twin (base 1) `stream` present two times in three"""

    def __init__(self, base=0):
        self.base, self.n, self.nullpad, self.stream = base, 0, 0, 0

    def line(self, pdims, backend, ax, ac, halo, per, pad, more=""):
        text = "--pr %d --pc %d %s --backend %d --ax %d --ac %d --hex %d --hey %d --hez %d --hpx %d --hpy %d --hpz %d " \
               "--pdx %d --pdy %d --pdz %d" % (tuple(pdims) + (GRID, backend, ax + self.base, ac) + tuple(halo) + tuple(per) + tuple(pad))
        text += " --parity %+d --centering %d" % MIRRORS[self.n % 4]
        text += " --sides %d --unnamed %s" % (SIDES[self.n % 3], UNNAMED[(self.n // 4) % 2])
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
    """two passes over axis x layout x set (24 geometries); the second pass meets the 24 combinations five places further on"""
    lines = []
    for again in range(2):
        forms.n += 5 * again
        lines += [forms.line((1, 1), 3, ax, ac, h, per, pad) for ax, ac, (h, per, pad) in itertools.product((0, 1, 2), (0, 1), WALLS)]
    return lines


def four_rank_lines(forms):
    return [forms.line(pdims, 1, ax, (i + ax) % 2, h, per, pad)
            for pdims in ((1, 4), (4, 1)) for i, (ax, (h, per, pad)) in enumerate(itertools.product((0, 1, 2), WALLS + WALLS[::-1]))]


def refusal_lines(forms):
    """(lines, how many of them are refusals): every refusal happens on the host before any launch, the program checks the result
    code and that the pencil stays byte-identical, and a valid case follows each of them"""
    b = forms.base
    head = "--pr 1 --pc 1 %s --backend 3 --ac 0 --hex 1 --hey 2 --hez 1 --hpx 0 --hpy 0 --hpz 0 --pdx 0 --pdy 1 --pdz 0 " \
           "--parity -1 --centering 0" % GRID
    refused = ["--ax %d --dim %d --sides 0 --expect-refusal invalid %s" % (0 + b, 1 + b, head),
               "--ax %d --dim %d --sides 4 --expect-refusal invalid %s" % (1 + b, 0 + b, head),
               # a named side without its array; the other side's garbage is no substitute
               "--ax %d --dim %d --sides 1 --named-null --unnamed garbage --expect-refusal invalid %s" % (2 + b, 1 + b, head),
               "--ax %d --dim %d --sides 2 --named-null --unnamed garbage --expect-refusal invalid %s" % (0 + b, 2 + b, head),
               "--ax %d --dim %d --sides 3 --named-null --expect-refusal invalid %s" % (1 + b, 1 + b, head),
               # nine layers on a 32-cell dim: the mirror itself would fit (9 + 0 <= 32), the table of addends holds eight
               "--ax %d --dim %d --sides 3 --expect-refusal unsupported %s" % (2 + b, 0 + b, head.replace("--gx 16", "--gx 32").replace("--hex 1", "--hex 9"))]
    valid = single_rank_lines(forms)
    lines = []
    for i, r in enumerate(refused):
        lines += [r, valid[(7 * i) % len(valid)]]
    return lines, len(refused)


def _binary(name):
    path = os.path.join(NATIVE, "build", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", NATIVE, "-f", "wall_values.mk", "build/" + name], check=True, capture_output=True)
    return path


def _fortran_binary(dtype="R64"):
    path = os.path.join(FORTRAN_BUILD, "fortran", "halo_wall_values_test_" + dtype)
    if not os.path.exists(path):
        if shutil.which("amdflang") is None:
            pytest.skip("amdflang not installed")
        subprocess.run(["make", "-C", os.path.join(ROOT, "cudecomp_amd")], check=True, capture_output=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "fortran"), "all", "wall_values_test"], check=True, capture_output=True)
    return path


def test_the_lists_reach_every_mirror_with_every_choice_of_sides():
    lines = single_rank_lines(Forms())
    assert len(WALLS) == 4 and len(lines) == 48
    for (parity, centering), sides, unnamed in itertools.product(MIRRORS, SIDES, UNNAMED):
        form = "--parity %+d --centering %d --sides %d --unnamed %s" % (parity, centering, sides, unnamed)
        assert any(form in l + " " for l in lines) and any(form in l + " " for l in single_rank_lines(Forms(base=1)))
    zero_pad = [l for l in lines if "--pdx 0 --pdy 0 --pdz 0" in l]
    assert any("--nullpad" in l for l in zero_pad) and any("--nullpad" not in l for l in zero_pad)
    assert all("--nullpad" not in l for l in lines if l not in zero_pad)
    four = four_rank_lines(Forms())
    assert any("--pr 1 --pc 4" in l for l in four) and any("--pr 4 --pc 1" in l for l in four)
    for some in (lines, four):  # three layers per side: where a reversed layer order shows best
        assert any("--hex 3 " in l for l in some)
    refusals, refused = refusal_lines(Forms())
    assert refused == 6 and len(refusals) == 12 and all(("--expect-refusal" in l) == (i % 2 == 0) for i, l in enumerate(refusals))
    assert sum("--expect-refusal unsupported" in l and "--gx 32" in l and "--hex 9" in l for l in refusals) == 1


@pytest.mark.parametrize("dtype", ["R32", "R64", "C64", "H16"])
def test_native_single_rank(dtype):
    _run_side_by_side([("halo_wall_values_test_" + dtype, 1, single_rank_lines(Forms()), None)], path_of=_binary)


def test_native_four_ranks():
    """four ranks sharing the GPU, R64, process grids 1 x 4 and 4 x 1: every rank serves the named sides on which
    cudecompGetShiftedRank names no neighbour, and only those"""
    _run_side_by_side([("halo_wall_values_test_R64", 4, four_rank_lines(Forms()), None)], path_of=_binary)


def test_native_refusals():
    lines, refused = refusal_lines(Forms())
    _run_side_by_side([("halo_wall_values_test_R64", 1, lines, None)], path_of=_binary)


def _self_check_lines(forms, option):
    """three cases of the wide set (h = 3, 2, 3, walls everywhere), the second with the self-check option"""
    good = [l for l in single_rank_lines(forms) if "--hex 3 --hey 2 --hez 3" in l][:3]
    assert len(good) == 3
    return [good[0], good[1] + " " + option, good[2]]


@pytest.mark.parametrize("option", ["--self-check-reverse-layers", "--self-check-swap-sides"])
def test_native_comparison_can_fail(option):
    """the second of three cases expects a[h-1-k] where the header says a[k], or the two arrays exchanged; it must report FAILED and
    end the list there, within seconds"""
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(_self_check_lines(Forms(), option)) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_binary("halo_wall_values_test_R64"), "--testfile", f.name], 120,
                             {"CUDECOMP_TEST_STOP_AT_FIRST_FAILURE": "1", "CUDECOMP_TEST_VERDICT_TIMEOUT": "60"})
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert "Stopping at the first failing case (2 of 3 run)" in text, text[-2000:]
    assert text.count(" PASSED") == 1 and text.count(" FAILED") == 1, text[-2000:]
    assert "differ after the wall values along dim" in text and "went unnoticed" not in text, text[-2000:]
    assert time.time() - t0 < 30


# ---- the Fortran twin ------------------------------------------------------------------------------------------------------
def _run_fortran(nranks, lines, dtype="R64"):
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    try:
        logs = run_binary_ranks(nranks, [_fortran_binary(dtype), "--testfile", f.name], timeout=900)
    finally:
        os.unlink(f.name)
    out = logs[0]
    ok = out.count(" PASSED") == len(lines) and " FAILED" not in out and "Passed all tests." in out
    assert ok, "\n".join("===== rank %d =====\n%s" % (r, text[-3000:]) for r, text in enumerate(logs))
    return sorted(line.split()[1] for line in out.splitlines() if line.startswith("WRAPPER "))


@pytest.mark.parametrize("dtype", ["R64", "C64"])
def test_fortran_single_rank(dtype):
    """C64: a Fortran caller's 2 h doubles per side, re and im interleaved"""
    lines = single_rank_lines(Forms(base=1))
    assert any("--stream" in l for l in lines) and any("--stream" not in l for l in lines)
    assert _run_fortran(1, lines, dtype) == WRAPPERS


def test_fortran_four_ranks():
    assert _run_fortran(4, four_rank_lines(Forms(base=1))) == WRAPPERS


def test_fortran_refusals():
    """a named side whose array is ABSENT reaches the library as NULL"""
    lines, refused = refusal_lines(Forms(base=1))
    assert _run_fortran(1, lines) == WRAPPERS


@pytest.mark.parametrize("option", ["--self-check-reverse-layers", "--self-check-swap-sides"])
def test_fortran_comparison_can_fail(option):
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(_self_check_lines(Forms(base=1), option)) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_fortran_binary(), "--testfile", f.name], 120)
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert text.count(" PASSED") == 1 and text.count(" FAILED") == 1 and "Failed 1/3 tests." in text, text[-2000:]
    assert "differ after the call along dim" in text and "went unnoticed" not in text, text[-2000:]
    assert time.time() - t0 < 30
