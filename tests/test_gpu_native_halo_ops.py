"""The halo extensions -- cudecompAmdAccumulateHalos, cudecompAmdFillHalos, cudecompAmdAccumulateAndClearHalos and
cudecompAmdReflectHalos {X,Y,Z} -- as a C / C++ solver calls them: tests/native/halo_ops_test.cpp includes the four cudecomp_amd*.h
headers, calls every entry point through its prototype there and compares the whole pencil, byte for byte, with closed forms built
from the headers' text (no tolerance: the payloads are small integers).  Everything else in the suite reaches these functions
through ctypes argtypes written by hand.

The case lists: the 16 x 20 x 18 grid of tests/test_gpu_native.py::_halo_lines (ragged slabs on 1 x 4 and 4 x 1), every case
accepted by the library (h + centering <= the narrowest slab of 4 cells, halos no wider than a slab); a refused case in a positive
list fails the list."""
import itertools
import os
import tempfile
import time

import pytest

from tests.halo_ops_cases import COMMUNICATING, OPS, SETS, Forms, four_rank_lines, mem_order_lines, refusal_lines, single_rank_lines
from tests.mp import run_binary_ranks
from tests.test_gpu_native import SHIM, _binary, _run, _run_side_by_side

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["R32", "R64", "C32", "C64", "H16"])
def test_native_halo_ops_single_rank(dtype):
    forms = Forms()
    lines = single_rank_lines(forms)
    if dtype == "R64":
        lines += mem_order_lines(forms)
    _run("halo_ops_test_" + dtype, 1, lines)


def test_native_halo_ops_bfloat16_and_half_complex_macros():
    """CUDECOMP_AMD_BFLOAT16 and CUDECOMP_AMD_HALF_COMPLEX as cudecomp_amd.h defines them, chosen at run time.  Fill and reflection are
    pure bit movement; the two accumulations are there because only arithmetic tells bfloat16 from binary16 (both have two bytes):
    bfloat16 1 + 1 added as binary16 patterns is not bfloat16 2."""
    forms = Forms()
    lines = []
    for sel in ("bf16", "half_complex"):
        lines += [forms.line(op, (1, 1), 3, ax, ax % 2, h, per, pad, more=" --dtype " + sel)
                  for op, ax, (h, per, pad) in itertools.product(OPS, (0, 1, 2), SETS[1:])]
    _run("halo_ops_test_H16", 1, lines)


def test_native_halo_ops_four_ranks():
    """Four ranks sharing the GPU, R64: the communicating operations over process grids 2 x 2, 1 x 4, 4 x 1 and halo backends 1 (MPI),
    2 (MPI blocking), 4 (NVSHMEM); fill and reflection, which do not communicate, over one backend.  Two independent lists side by side."""
    grids = [(2, 2), (1, 4), (4, 1)]
    a = four_rank_lines(Forms(), grids, [1, 2, 4], ["accumulate"]) + four_rank_lines(Forms(), grids, [1], ["fill"])
    b = four_rank_lines(Forms(), grids, [1, 2, 4], ["accumulate_clear"]) + four_rank_lines(Forms(), grids, [4], ["reflect"])
    _run_side_by_side([("halo_ops_test_R64", 4, a, None), ("halo_ops_test_R64", 4, b, None)])


def test_native_halo_ops_four_ranks_rccl_code_path():
    if not os.path.exists(SHIM):
        pytest.skip("tests/shim/libfake_rccl.so not built")
    lines = four_rank_lines(Forms(), [(2, 2), (4, 1)], [3], COMMUNICATING)
    _run("halo_ops_test_R64", 4, lines, {"LD_PRELOAD": SHIM})


def test_native_halo_ops_refusals():
    lines, refused = refusal_lines(Forms())
    assert refused == 9 and len(lines) == 18
    _run("halo_ops_test_R64", 1, lines)


def test_native_halo_ops_comparison_can_fail():
    """--self-check-shift-dim: the second of three cases calls along (dim + 1) % 3 while expecting dim; it must report FAILED and end
    the list there, within seconds."""
    good = single_rank_lines(Forms(), ops=("accumulate",))[:3]
    lines = [good[0], good[1] + " --self-check-shift-dim", good[2]]
    with tempfile.NamedTemporaryFile("w", suffix="_cases.txt", delete=False) as f:
        f.write("\n".join(lines) + "\n")
    t0 = time.time()
    try:
        with pytest.raises(AssertionError) as e:
            run_binary_ranks(1, [_binary("halo_ops_test_R64"), "--testfile", f.name], 120,
                             {"CUDECOMP_TEST_STOP_AT_FIRST_FAILURE": "1", "CUDECOMP_TEST_VERDICT_TIMEOUT": "60"})
    finally:
        os.unlink(f.name)
    text = str(e.value)
    assert "Stopping at the first failing case (2 of 3 run)" in text and " FAILED" in text, text[-2000:]
    assert "elements differ after accumulate along dim" in text, text[-2000:]
    assert time.time() - t0 < 30
