"""Every instantiation of the LDS-tiled single-field copy kernels -- transpose_kernel (30), transpose_window_kernel (15),
transpose_lines_kernel (10), transpose_rowlines_kernel (10) -- and of the remote-store forms of the row and element-wise copies
(rows_kernel<VB,3>, rows_shifted_kernel<VB,3>, generic_kernel<ES,true>: 11), launched by name through cudecompExtRunMoves with
the recipes of tests/tiled_instantiations.py (shapes and their reasons are there; tests/test_tiled_instantiation_table.py checks
the table without a GPU).  The remote-store policy (STREAM 3: write-through stores in inline assembly) runs on local memory: a
list with destination bases is a list of one-sided sends, whatever memory the bases name.

Every recipe runs three launches -- the wide move alone, the small move alone, both as one list (with bases ONE interleaved
launch whose filler workgroups pass through locate()) -- and the tiled kernels the wide move twice more, the tile walk forced i
first and j first.  After every launch EVERY byte of every buffer -- the source, the destination or the per-move base buffers,
the cells between the moves, the gap cells the lines kernels read back and rewrite, 256 poison bytes on both sides of each --
is compared with numpy applying oracle.move3d_reference one move at a time (tests/move_lists.run_list), bit for bit: pure data
movement, tolerance 0.  cudecompExtLastKernelName() must equal the recipe's literal name and the launch count 1.  Payloads are
seeded random bytes; the largest buffer is below 4 MiB."""
import pytest

import cudecomp_amd as cd
from tests import move_lists as ML
from tests import tiled_instantiations as T

pytestmark = pytest.mark.gpu


def run(recipe, which, extra, seed, reference_moves=None):
    moves = recipe.moves(which)
    try:
        want = ML.run_list(moves, recipe.es, cd.MOVES_COPY, flags=recipe.flags | extra, bases=recipe.bases, seed=seed,
                           reference_moves=reference_moves)
    except AssertionError as e:  # (say which instantiation it was)
        raise AssertionError((recipe.name, which, extra) + e.args) from None
    name = cd.cudecompExtLastKernelName()
    assert len(want) == 1 and name == recipe.name, (recipe.name, which, extra, name, want)
    return name


@pytest.mark.parametrize("family,es", T.GROUPS, ids=["%s-%d" % g for g in T.GROUPS])
def test_every_instantiation(family, es):
    seen = set()
    for n, recipe in enumerate(T.recipes(family, es)):
        for k, (which, extra) in enumerate(T.launches_of(recipe)):
            seen.add(run(recipe, which, extra, 1000 * es + 10 * n + k))
    assert seen == set(T.INVENTORY[(family, es)]), sorted(set(T.INVENTORY[(family, es)]) ^ seen)


@pytest.mark.parametrize("family,es,name", [("transpose", 2, "transpose_kernel<2,8,128,128,0,true>"),
                                            ("window", 8, "transpose_window_kernel<8,2,64,64,4>"),
                                            ("remote", 8, "rows_shifted_kernel<16,3>")], ids=("plain", "window", "remote"))
def test_the_comparison_can_fail(family, es, name):
    """the numpy side alone moves one lane vector less along the destination rows: the GPU launch stays the valid move, and the
    bytes of that vector must show as differences"""
    (recipe,) = [r for r in T.recipes(family, es) if r.name == name]
    lane = recipe.name.split("<")[1].split(",")
    lane = int(lane[1]) if family != "remote" else int(lane[0]) // es  # elements per lane
    moves = recipe.moves("wide")
    (m,) = moves
    along = 1 if family != "remote" else 0  # the destination's unit-stride dim
    extent = [int(e) for e in m.extent]
    extent[along] -= lane
    short = cd.make_move(extent, tuple(m.ss), tuple(m.ds), m.src_off, m.dst_off, m.src_buf, m.dst_buf, m.row_pitch)
    with pytest.raises(AssertionError, match="bytes differ"):
        run(recipe, "wide", 0, 7, reference_moves=[short])
    assert cd.cudecompExtLastKernelName() == name
    run(recipe, "wide", 0, 7)
