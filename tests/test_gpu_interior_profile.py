"""Interior profiles (cudecomp_interior_profile.h: cudecompAmdProfileInterior{X,Y,Z}) on the GPU: the three stage-one kernels box by
box inside NaN poison over every row length, pitch and phase of the 16-byte grid with the kept dim at each of the three memory
positions; more entries than workgroups in flight, more parts than the final stage has lanes per entry and a kept extent of 1 against
the scalar reduction; ld > L; ghost cells and padding that never reach a result; single-rank pencils of every axis, memory order,
halo width, padding, dim and data type, whose profiles add up to the scalar cudecompAmdReduceInterior result; several fields against
their single-field calls; accuracy per entry against an exactly rounded reference, held to the derived bound; IEEE edge values; an
empty interior; four ranks on a ragged 2 x 2 grid whose profiles, placed at lo[dim] of a zeroed global array, add up to a closed
form; capture into a hipGraph; asynchrony.  Integer data wherever the comparison is bit for bit.  Every body runs on launched ranks."""
import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import interior_profile_bodies as PB
from tests import interior_reduce_bodies as RB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

BODIES = "tests.interior_profile_bodies"


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity(dtype):
    assert run_ranks(1, BODIES, "kernel_parity", {"dtype": dtype}, timeout=300)[0] == []


def test_sizes_at_which_the_kernels_take_another_path_and_ld_beyond_the_profile():
    assert run_ranks(1, BODIES, "sizes", {}, timeout=300)[0] == []


def test_ghost_cells_and_padding_never_reach_a_result():
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "halo": (2, 1, 3), "padding": (1, 2, 0)}
    assert run_ranks(1, BODIES, "ghost_independence", args, timeout=300)[0] == []


def test_single_rank_sweep():
    args = {"shapes": [(13, 10, 11), (5, 6, 7)], "orders": [(0, 1, 2), (1, 2, 0)], "halos": [(0, 0, 0), (1, 1, 1), (2, 1, 3)],
            "paddings": [(0, 0, 0), (1, 2, 0)]}
    assert run_ranks(1, BODIES, "single_rank_sweep", args, timeout=300)[0] == []


def test_a_field_of_a_multi_field_call_equals_its_single_field_call():
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "halo": (1, 2, 1), "padding": (0, 1, 0)}
    assert run_ranks(1, BODIES, "multi_field", args, timeout=300)[0] == []


def test_accuracy_within_the_derived_bound():
    """per entry |got - exact| <= n_k * 2^-53 * sum |term|, n_k the cells of the plane: the derivation of
    tests/test_gpu_interior_reduce.py::test_accuracy_within_the_derived_bound, applied to one plane"""
    res = run_ranks(1, BODIES, "accuracy", {"gdims": (50, 48, 44), "pdims": (1, 1), "halo": (1, 1, 1)}, timeout=300)[0]
    print("\n".join(res["figures"]))
    assert res["failures"] == [], res


def test_edge_values():
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "halo": (1, 0, 2), "padding": (0, 1, 0)}
    assert run_ranks(1, BODIES, "edge_values", args, timeout=300)[0] == []


def _combine(per_rank, gdims):
    """the ranks' global arrays of every case against the closed form over the whole grid: sums add up, maxima are the maximum"""
    wa, wb = RB.closed_form(gdims)
    checked = 0
    for key in per_rank[0][1]:
        op, dim = (int(x) for x in key.split()[-2:])
        dtype = per_rank[0][1][key][1]
        nc = AB.TYPES[dtype][1]
        ia, ib = np.stack([wa, wb] if nc == 2 else [wa], axis=-1), np.stack([wb, wa] if nc == 2 else [wb], axis=-1)
        want = np.stack([PB.profile_reference(op, ia, ib, 2 - dim), PB.profile_reference(op, ib, ia, 2 - dim)])  # (numpy axes z, y, x)
        owners = [r for r in per_rank if r[1][key][2] > 0]  # (a rank with L == 0 wrote nothing: its array is all sentinel)
        parts = np.array([r[1][key][0] for r in owners])
        got = parts.max(axis=0) if op == cd.REDUCE_MAX_ABS else parts.sum(axis=0)  # (integers: exact in any order)
        assert RB.same_bits(got + 0.0, want), (key, got.tolist(), want.tolist())
        assert sum(r[1][key][3] for r in per_rank) == int(np.prod(gdims)), key  # the interiors partition the grid
        checked += 1
    return checked


def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (10, 9, 11): every rank places its profiles at lo[dim] of a zeroed global array with ld = the global extent;
    the four arrays added (max for MAX_ABS) equal the closed form over the whole grid exactly, for every axis and dim"""
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "halos": [(1, 1, 1), (2, 0, 3)]}
    per_rank = run_ranks(4, BODIES, "ranks_sweep", args, timeout=300, fresh=False)
    for failures, _ in per_rank:
        assert failures == []
    assert _combine(per_rank, args["gdims"]) == 3 * 2 * 3 * 3


def test_an_empty_interior():
    """a 1 x 4 grid over 3 cells: the last rank's pencils of axes 0 and 1 have no interior.  Where its L is 0 nothing is written (the
    sentinel stays); where L > 0 and another extent is 0, zeros are written (both checked on the rank)."""
    args = {"gdims": (8, 6, 3), "pdims": (1, 4), "halo_backend": cd.HALO_COMM_MPI, "halos": [(1, 1, 1)], "dtype": cd.DOUBLE}
    per_rank = run_ranks(4, BODIES, "ranks_sweep", args, timeout=300, fresh=False)
    for failures, _ in per_rank:
        assert failures == []
    cases = per_rank[3][1]
    nothing = [key for key, (got, _, L, cells) in cases.items() if L == 0]
    zeros = [key for key, (got, _, L, cells) in cases.items() if L > 0 and cells == 0]
    assert len(nothing) >= 3 and len(zeros) >= 3, cases
    for key in nothing:
        assert (np.array(cases[key][0]) == -777.0).all(), (key, cases[key])
    for key in zeros:
        assert RB.same_bits(cases[key][0], np.zeros_like(cases[key][0])), (key, cases[key])
    assert _combine(per_rank, args["gdims"]) == 3 * 1 * 3 * 3


def test_a_replayed_graph_equals_an_eager_call():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "padding": (0, 1, 0)},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ((1, 2, 0),) * 3, "axis": 1, "halo": (2, 1, 2),
                  "dtype": cd.FLOAT_COMPLEX, "op": cd.REDUCE_SUM}):
        assert run_ranks(1, BODIES, "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1)}
    res = run_ranks(1, BODIES, "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["host_ms"] < 0.25 * res["total_ms"], res
