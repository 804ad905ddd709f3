"""Halo folding (cudecomp_halo_fold.h: cudecompAmdFoldHalos{X,Y,Z}) as a C / C++ and as a Fortran solver call it:
tests/native/halo_fold_test.cpp includes the header and calls every entry point through its prototype there,
tests/fortran/halo_fold_test.f90 calls the three wrappers of module `cudecomp`; both compare the whole pencil, byte for byte, with
closed forms built from the header's text (no tolerance: the payloads are small integers).  Everything else in the suite reaches
these functions through ctypes argtypes written by hand.

The case lists: the 16 x 20 x 18 grid of tests/halo_ops_cases.py (ragged slabs on 1 x 4 and 4 x 1), every case accepted by the
library (h + centering <= the narrowest slab of 4 cells); a refused case in a positive list fails the list.  The C++ program is
built on demand by tests/native/fold.mk, the Fortran one by the fold_test target of fortran/Makefile."""
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
MIRRORS = [(1, 0, 0), (-1, 0, 1), (1, 1, 1), (-1, 1, 0), (-1, 0, 0), (1, 0, 1), (-1, 1, 1), (1, 1, 0)]  # (parity, centering, clear)


def _binary(name):
    path = os.path.join(NATIVE, "build", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", NATIVE, "-f", "fold.mk", "build/" + name], check=True, capture_output=True)
    return path


def _fortran_binary(dtype):
    path = os.path.join(FORTRAN_BUILD, "fortran", "halo_fold_test_" + dtype)
    if not os.path.exists(path):
        if shutil.which("amdflang") is None:
            pytest.skip("amdflang not installed")
        subprocess.run(["make", "-C", os.path.join(ROOT, "cudecomp_amd")], check=True, capture_output=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "fortran"), "all", "fold_test"], check=True, capture_output=True)
    return path


class Forms:
    """what varies from case to case beside the geometry: the eight (parity, centering, clear) in turn, padding = NULL every other
    time the padding is zero, and for the Fortran twin (base 1) `stream` present two times in three"""

    def __init__(self, base=0):
        self.base, self.n, self.nullpad, self.stream = base, 0, 0, 0

    def line(self, pdims, backend, ax, ac, halo, per, pad, grid=GRID, more=""):
        text = "--pr %d --pc %d %s --backend %d --ax %d --ac %d --hex %d --hey %d --hez %d --hpx %d --hpy %d --hpz %d " \
               "--pdx %d --pdy %d --pdz %d" % (tuple(pdims) + (grid, backend, ax + self.base, ac) + tuple(halo) + tuple(per) + tuple(pad))
        text += " --parity %+d --centering %d --clear %d" % MIRRORS[self.n % 8]
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


# beside the sets of tests/halo_ops_cases.py: walls on every dim with a halo of 2 and padding
WALLS = SETS + [((2, 2, 2), (0, 0, 0), (1, 0, 2))]


def single_rank_lines(forms, more=""):
    return [forms.line((1, 1), 3, ax, ac, h, per, pad, more=more) for ax, ac, (h, per, pad) in itertools.product((0, 1, 2), (0, 1), WALLS)]


def mem_order_lines(forms):
    """the six memory orders of the tested pencil on 12 x 14 x 10, walls along dims 1 and 2"""
    return [forms.line((1, 1), 3, ax, 0, (1, 2, 1), (1, 0, 0), (0, 1, 0), grid="--gx 12 --gy 14 --gz 10",
                       more=" --mem_order %d %d %d" % tuple(x + forms.base for x in perm))
            for ax, perm in itertools.product((0, 1, 2), itertools.permutations((0, 1, 2)))]


def four_rank_lines(forms):
    return [forms.line(pdims, 1, ax, (i + ax) % 2, h, per, pad)
            for pdims in ((2, 2), (1, 4), (4, 1)) for i, (ax, (h, per, pad)) in enumerate(itertools.product((0, 1, 2), SETS[1:]))]


def refusal_lines(forms):
    """(lines, how many of them are refusals): every refusal is CUDECOMP_RESULT_INVALID_USAGE on the host before any launch, the
    pencil stays byte-identical, and a valid case follows each of them"""
    b = forms.base
    head = "--pr 1 --pc 1 %s --backend 3 --ac 0 --hpx 0 --hpy 1 --hpz 1 --pdx 0 --pdy 1 --pdz 0 --expect-refusal" % GRID
    refused = ["--ax %d --dim %d --parity 1 --centering 0 --clear 0 %s" % (0 + b, 3 + b, head),
               "--ax %d --dim %d --parity 0 --centering 0 --clear 0 %s" % (1 + b, 0 + b, head),
               "--ax %d --dim %d --parity -1 --centering 2 --clear 1 %s" % (2 + b, 0 + b, head),
               "--ax %d --dim %d --parity 1 --centering 1 --clear 2 %s" % (0 + b, 0 + b, head),
               "--ax %d --dim %d --parity -1 --centering 0 --clear -1 --hex 0 %s" % (1 + b, 0 + b, head),
               # the mirror reaches beyond the interior along the wall dim: 3 + 1 > 3
               "--ax %d --dim %d --parity 1 --centering 1 --clear 0 --hex 3 %s" % (0 + b, 0 + b, head.replace("--gx 16", "--gx 3"))]
    valid = single_rank_lines(forms)
    lines = []
    for i, r in enumerate(refused):
        lines += [r, valid[(5 * i) % len(valid)]]
    return lines, len(refused)


def test_the_lists_reach_walls_and_every_form():
    lines = single_rank_lines(Forms()) + mem_order_lines(Forms())
    assert any("--hpx 0 --hpy 0 --hpz 0" in l for l in lines) and any("--hpx 1 --hpy 0 --hpz 1" in l for l in lines)
    assert {(p, c, k) for p, c, k in MIRRORS} == set(itertools.product((1, -1), (0, 1), (0, 1)))
    assert all(any("--parity %+d --centering %d --clear %d" % m in l for l in lines) for m in MIRRORS)
    assert any("--nullpad" in l for l in lines) and any("--nullpad" not in l for l in lines)
    fl = single_rank_lines(Forms(base=1))
    assert any("--stream" in l for l in fl) and any("--stream" not in l for l in fl)


@pytest.mark.parametrize("dtype", ["R32", "R64", "C64", "H16"])
def test_native_halo_fold_single_rank(dtype):
    forms = Forms()
    lines = single_rank_lines(forms)
    if dtype == "R64":
        lines += mem_order_lines(forms)
    if dtype == "H16":  # CUDECOMP_AMD_BFLOAT16 and CUDECOMP_AMD_HALF_COMPLEX as cudecomp_amd.h defines them, chosen at run time
        lines += [l + " --dtype " + sel for sel in ("bf16", "half_complex") for l in single_rank_lines(forms)[3::4]]
    _run_side_by_side([("halo_fold_test_" + dtype, 1, lines, None)], path_of=_binary)


def test_native_halo_fold_four_ranks():
    """four ranks sharing the GPU, R64, over process grids 2 x 2, 1 x 4 and 4 x 1: every rank folds the sides on which
    cudecompGetShiftedRank names no neighbour, and only those"""
    _run_side_by_side([("halo_fold_test_R64", 4, four_rank_lines(Forms()), None)], path_of=_binary)


def test_native_halo_fold_refusals():
    lines, refused = refusal_lines(Forms())
    assert refused == 6 and len(lines) == 12
    _run_side_by_side([("halo_fold_test_R64", 1, lines, None)], path_of=_binary)


def test_native_halo_fold_comparison_can_fail():
    """--self-check-shift-dim: the second of three cases calls along (dim + 1) % 3 while expecting dim; it must report FAILED and end
    the list there, within seconds"""
    good = [l for l in single_rank_lines(Forms()) if "--hpx 0 --hpy 0 --hpz 0" in l][:3]
    lines = [good[0], good[1] + " --self-check-shift-dim", good[2]]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_binary("halo_fold_test_R64"), "--testfile", f.name], 120,
                             {"CUDECOMP_TEST_STOP_AT_FIRST_FAILURE": "1", "CUDECOMP_TEST_VERDICT_TIMEOUT": "60"})
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert "Stopping at the first failing case (2 of 3 run)" in text and " FAILED" in text, text[-2000:]
    assert "elements differ after fold along dim" in text, text[-2000:]
    assert time.time() - t0 < 30


# ---- the Fortran twin ------------------------------------------------------------------------------------------------------
def _run_fortran(dtype, nranks, lines):
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


@pytest.mark.parametrize("dtype", ["R32", "R64", "C64"])
def test_fortran_halo_fold_single_rank(dtype):
    forms = Forms(base=1)
    lines = single_rank_lines(forms)
    if dtype == "R64":
        lines += mem_order_lines(forms)
    assert _run_fortran(dtype, 1, lines) == ["cudecompAmdFoldHalos" + a for a in "XYZ"]


def test_fortran_halo_fold_four_ranks():
    assert _run_fortran("R64", 4, four_rank_lines(Forms(base=1))) == ["cudecompAmdFoldHalos" + a for a in "XYZ"]


def test_fortran_halo_fold_refusals():
    lines, refused = refusal_lines(Forms(base=1))
    assert refused == 6
    _run_fortran("R64", 1, lines)


def test_fortran_halo_fold_comparison_can_fail():
    good = [l for l in single_rank_lines(Forms(base=1)) if "--hpx 0 --hpy 0 --hpz 0" in l][:3]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join([good[0], good[1] + " --self-check-shift-dim", good[2]]) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_fortran_binary("R64"), "--testfile", f.name], 120)
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert text.count(" PASSED") == 1 and text.count(" FAILED") == 1 and "Failed 1/3 tests." in text, text[-2000:]
    assert "words differ after fold along dim" in text, text[-2000:]
    assert time.time() - t0 < 30
