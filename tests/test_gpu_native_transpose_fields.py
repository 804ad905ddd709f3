"""Multi-field transposes (cudecomp_transpose_fields.h: cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX}) as a C / C++ and a Fortran
solver call them: tests/native/transpose_fields_test.cpp includes the header and calls every entry point through its prototype
there; tests/fortran/transpose_fields_test.f90 goes through the wrappers of module `cudecomp`.  Each runs the cycle X -> Y -> Z ->
Y -> X of --fields N pencils next to N single cudecompTranspose* calls per hop on a second copy and compares every buffer of both
copies byte for byte after every hop.  Everything else in the suite reaches these functions through ctypes argtypes written by
hand.  The programs are built by tests/native/transpose_fields.mk and fortran/Makefile (transpose_fields_test)."""
import itertools
import os
import shutil
import subprocess
import tempfile
import time

import pytest

from tests.mp import ROOT, run_binary_ranks
from tests.test_gpu_native import NATIVE, _run_side_by_side

pytestmark = pytest.mark.gpu
FORTRAN_BUILD = os.path.join(ROOT, "fortran", "build")
GRID = "--gx 10 --gy 9 --gz 11"
HALOS = [((0, 0, 0), (0, 0, 0)), ((1, 2, 1), (0, 0, 0)), ((2, 1, 1), (1, 0, 2))]
NAMES = ["cudecompAmdTransposeFields" + op for op in ("XToY", "YToX", "YToZ", "ZToY")]


def _binary(name):
    path = os.path.join(NATIVE, "build", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", NATIVE, "-f", "transpose_fields.mk", "build/" + name], check=True, capture_output=True)
    return path


def _fortran_binary():
    path = os.path.join(FORTRAN_BUILD, "fortran", "transpose_fields_test_R64")
    if not os.path.exists(path):
        if shutil.which("amdflang") is None:
            pytest.skip("amdflang not installed")
        subprocess.run(["make", "-C", os.path.join(ROOT, "cudecomp_amd")], check=True, capture_output=True)
        subprocess.run(["make", "-C", os.path.join(ROOT, "fortran"), "all", "transpose_fields_test"], check=True, capture_output=True)
    return path


def lines(pdims_list, backend, fortran=False, n_fields=3):
    """process grids x layouts x (halos, padding) x out of place / in place; NULL halos and padding every other time they are
    zero; for the Fortran twin `stream` present two times in three"""
    out = []
    for i, (pdims, ac, (halo, pad), inplace) in enumerate(itertools.product(pdims_list, (0, 1), HALOS, (False, True))):
        text = "--pr %d --pc %d %s --backend %d --ac %d --hex %d --hey %d --hez %d --pdx %d --pdy %d --pdz %d --fields %d" % (
            tuple(pdims) + (GRID, backend, ac) + tuple(halo) + tuple(pad) + (n_fields,))
        if inplace:
            text += " --inplace"
        if not any(halo) and not any(pad) and i % 2 == 0:
            text += " --nullhalo"
        if fortran and i % 3 != 0:
            text += " --stream"
        out.append(text)
    return out


@pytest.mark.parametrize("dtype", ["R32", "R64", "C64", "H16"])
def test_native_transpose_fields_single_rank(dtype):
    _run_side_by_side([("transpose_fields_test_" + dtype, 1, lines([(1, 1)], 1), None)], path_of=_binary)


def test_native_transpose_fields_four_ranks():
    """four ranks sharing the GPU, R64, over process grids 2 x 2, 1 x 4 and 4 x 1, ragged (10, 9, 11): one message per peer
    carries every field; MPI_P2P and NVSHMEM enums (the one-sided transport)"""
    _run_side_by_side([("transpose_fields_test_R64", 4, lines([(2, 2), (1, 4), (4, 1)], 1), None),
                       ("transpose_fields_test_R64", 4, lines([(2, 2)], 6), None)], path_of=_binary)


def test_native_transpose_fields_comparison_can_fail():
    """--self-check-swap-fields: the second of three cases hands the call its outputs in reversed order; it must report FAILED
    and end the list there, within seconds"""
    good = [l for l in lines([(1, 1)], 1) if "--inplace" not in l][:3]
    cases = [good[0], good[1] + " --self-check-swap-fields", good[2]]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(cases) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_binary("transpose_fields_test_R64"), "--testfile", f.name], 120,
                             {"CUDECOMP_TEST_STOP_AT_FIRST_FAILURE": "1", "CUDECOMP_TEST_VERDICT_TIMEOUT": "60"})
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert "Stopping at the first failing case (2 of 3 run)" in text and " FAILED" in text, text[-2000:]
    assert "differ from the single call" in text, text[-2000:]
    assert time.time() - t0 < 30


# ---- the Fortran twin ------------------------------------------------------------------------------------------------------
def _run_fortran(nranks, cases):
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(cases) + "\n")
    try:
        logs = run_binary_ranks(nranks, [_fortran_binary(), "--testfile", f.name], timeout=900)
    finally:
        os.unlink(f.name)
    out = logs[0]
    ok = out.count(" PASSED") == len(cases) and " FAILED" not in out and "Passed all tests." in out
    assert ok, "\n".join("===== rank %d =====\n%s" % (r, text[-3000:]) for r, text in enumerate(logs))
    return sorted(line.split()[1] for line in out.splitlines() if line.startswith("WRAPPER "))


def test_fortran_transpose_fields_single_rank():
    cases = lines([(1, 1)], 1, fortran=True)
    assert any("--stream" in l for l in cases) and any("--stream" not in l for l in cases)
    assert any("--nullhalo" in l for l in cases) and any("--inplace" in l for l in cases)
    assert _run_fortran(1, cases) == NAMES


def test_fortran_transpose_fields_four_ranks():
    assert _run_fortran(4, lines([(2, 2), (1, 4)], 1, fortran=True)) == NAMES


def test_fortran_transpose_fields_comparison_can_fail():
    good = [l for l in lines([(1, 1)], 1, fortran=True) if "--inplace" not in l][:3]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join([good[0], good[1] + " --self-check-swap-fields", good[2]]) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_fortran_binary(), "--testfile", f.name], 120)
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert text.count(" PASSED") == 1 and text.count(" FAILED") == 1 and "Failed 1/3 tests." in text, text[-2000:]
    assert "differ from the single call" in text, text[-2000:]
    assert time.time() - t0 < 30
