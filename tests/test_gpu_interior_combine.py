"""Interior combinations (cudecomp_interior_combine.h: cudecompAmdCombineInterior{X,Y,Z}) on the GPU: the two kernels box by box
inside position-dependent bytes over every row length, pitch and phase of the 16-byte grid, rows longer than a tile column, a cut row,
more rows than a tile, the four operations; ghost cells and padding of x and y that keep distinct NaN payloads bit for bit; single-rank
pencils of every axis, memory order, halo width, padding and data type; several fields against their single-field calls, with a pair
of coefficients each and with the shared pair, in one launch; the coefficients' product, quotient and conversion straight from the
double; IEEE edge values and a case that tells fused from separately rounded arithmetic; one CG step without a host read; four ranks
on a ragged 2 x 2 grid against a closed form, and a rank that owns nothing; capture into a hipGraph whose ratio changes between
replays; asynchrony.  Every comparison is bit for bit against numpy in the stated arithmetic (tests/interior_combine_bodies.py).  Every
body runs on launched ranks."""
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

BODIES = "tests.interior_combine_bodies"


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity(dtype):
    assert run_ranks(1, BODIES, "kernel_parity", {"dtype": dtype}, timeout=300)[0] == []


def test_ghost_cells_and_padding_keep_their_bytes_and_influence_nothing():
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "halo": (2, 1, 3), "padding": (1, 2, 0)}
    assert run_ranks(1, BODIES, "ghosts_keep_their_bytes", args, timeout=300)[0] == []


def test_single_rank_sweep():
    args = {"shapes": [(13, 10, 11), (5, 6, 7)], "orders": [(0, 1, 2), (1, 2, 0)], "halos": [(0, 0, 0), (1, 1, 1), (2, 1, 3)],
            "paddings": [(0, 0, 0), (1, 2, 0)]}
    assert run_ranks(1, BODIES, "single_rank_sweep", args, timeout=300)[0] == []


def test_a_field_of_a_multi_field_call_equals_its_single_field_call_in_one_launch():
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "halo": (1, 2, 1), "padding": (0, 1, 0)}
    assert run_ranks(1, BODIES, "multi_field", args, timeout=300)[0] == []


def test_the_coefficient_is_a_product_then_a_quotient_rounded_once_directly_from_the_double():
    """1 + 2^-11 + 2^-30 gives 1 + 2^-10 in fp16 and 1 + 2^-8 + 2^-30 gives 1 + 2^-7 in bf16 (through fp32 both give 1.0); 1 / 3 and
    (0.1 * 3) / 0.3 held to numpy's fp64 product and quotient rounded once; overflow, subnormals, -0.0, a zero and a NaN denominator"""
    assert run_ranks(1, BODIES, "coefficient_conversion", {}, timeout=300)[0] == []


def test_ieee_edge_values_and_no_fused_multiply_add():
    assert run_ranks(1, BODIES, "edge_values", {}, timeout=300)[0] == []


def test_one_cg_step_without_a_host_read():
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "halo": (1, 2, 1), "padding": (0, 1, 0)}
    assert run_ranks(1, BODIES, "cg_step", args, timeout=300)[0] == []


def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (10, 9, 11): every owned cell equals 2 x - y of two closed forms, ghost bytes are unchanged, for every axis"""
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "halos": [(1, 1, 1), (2, 0, 3)]}
    per_rank = run_ranks(4, BODIES, "ranks_sweep", args, timeout=300, fresh=False)
    for failures, cases in per_rank:
        assert failures == []
        assert len(cases) == 3 * 2 and all(cells > 0 and launches == 1 for cells, launches in cases.values())
    for key in per_rank[0][1]:
        assert sum(r[1][key][0] for r in per_rank) == 10 * 9 * 11, key  # the interiors partition the grid


def test_an_empty_interior_makes_no_launch_and_changes_nothing():
    """a 1 x 4 grid over 3 cells: the last rank's pencils of axes 0 and 1 have no interior"""
    args = {"gdims": (8, 6, 3), "pdims": (1, 4), "halo_backend": cd.HALO_COMM_MPI, "halos": [(1, 1, 1)], "dtype": cd.DOUBLE}
    per_rank = run_ranks(4, BODIES, "ranks_sweep", args, timeout=300, fresh=False)
    for failures, _ in per_rank:
        assert failures == []
    empty = [key for key, (cells, launches) in per_rank[3][1].items() if cells == 0]
    assert len(empty) >= 2, per_rank[3][1]
    assert all(per_rank[3][1][key][1] == 0 for key in empty), per_rank[3][1]


def test_a_replayed_graph_equals_an_eager_call_and_picks_up_a_new_ratio():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "padding": (0, 1, 0)},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ((1, 2, 0),) * 3, "axis": 1, "halo": (2, 1, 2),
                  "dtype": cd.FLOAT_COMPLEX}):
        assert run_ranks(1, BODIES, "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1)}
    res = run_ranks(1, BODIES, "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["host_ms"] < 0.25 * res["total_ms"], res
