"""The host rule of csrc/kernels.cc residencyPadBytes as a table, through cudecompExtDescribeResidency (no GPU, no memory): the
dynamic LDS each launch of a list asks for.  Only large far-strided streaming transposes get a pad -- the forward hops of the
bench cycle (fp64, 64 x 64 tile, EVERY move of the launch on the run walk over tiles), its inverse hops (64 x 128 tile) and the
forward hops of the complex128 cycle (32 x 32 tile, run walk) -- and the pads are the ones DESIGN.md section 4 gives with their
measurements; everything else launches with none."""
import pytest

import cudecomp_amd as cd
from tests import move_lists as ML
from tests.test_kernel_choice_pins import BASE, _orders

FORWARD_PAD, INVERSE_PAD, FORWARD_PAD_16 = 16 << 10, 32 << 10, 23 << 10  # bytes: DESIGN.md section 4 "Tiles and walks", profiles/transpose_residency.json
STREAMING = 2
ADDRESSES = [BASE[0], BASE[1], BASE[2]]


def planned(gdims, ac, es, halo=None, inplace=False):
    """{op: pack moves} of a one-rank cycle, as the stateless planner gives them"""
    g = cd.make_grid_spec(gdims, (1, 1), _orders(ac))
    out = {}
    for op in cd.OPS:
        p = cd.cudecompExtPlanTranspose(g, 0, op, halo, halo, None, None, inplace)
        out[op] = list(p.pack)[:p.n_pack] + list(p.unpack)[:p.n_unpack]
    return out


def pads(moves, es, flags=0):
    launches = ML.describe(moves, ADDRESSES, es, flags=flags)
    got = cd.cudecompExtDescribeResidency(moves, ADDRESSES, es, flags)
    assert len(got) == len(launches)
    return got, launches


def test_bench_cycle_hops():
    hops = planned((1024, 1024, 1024), (1, 1, 1), 8)
    for op, want, tile_j in (("XToY", FORWARD_PAD, 64), ("YToZ", FORWARD_PAD, 64), ("ZToY", INVERSE_PAD, 128), ("YToX", INVERSE_PAD, 128)):
        got, (l,) = pads(hops[op], 8)
        assert (ML.KINDS[l["kind"]], l["vec"], l["tile_i"], l["tile_j"], l["access"]) == ("transpose", 2, 64, tile_j, 2), (op, l)
        assert got == [want], op


def test_other_element_sizes_of_the_cycle():
    """fp32: every hop as before; complex128: the forward hops (32 x 32 tile) padded, the inverse hops (32 x 64) as before"""
    for gdims, es in (((2048, 1024, 1024), 4), ((1024, 1024, 512), 16)):
        for op, moves in planned(gdims, (1, 1, 1), es).items():
            got, (l,) = pads(moves, es)
            assert ML.KINDS[l["kind"]] == "transpose" and l["access"] == 2, (es, op, l)
            forward_16 = es == 16 and op in ("XToY", "YToZ")
            assert (l["tile_i"], l["tile_j"]) == ((32, 32) if forward_16 else (32, 64) if es == 16 else (64, 128)), (es, op, l)
            assert got == [FORWARD_PAD_16 if forward_16 else 0], (es, op, l)


FORWARD = ((64, 1024, 64), (1, 64, 64 * 1024), (1024 * 64, 1, 1024))    # run of 512 tiles along j
SMALL = ((64, 64, 3), (1, 64, 4096), (64, 1, 4096))                     # same kernel choice when streaming is forced, no run
PLANES = ((64, 192, 32), (1, 64, 64 * 192), (256 * 32, 1, 256))         # destination planes a padded pitch apart: runs over PLANES


def listed(*shapes):
    p = ML.Packer(gap=0, align=256)
    for extent, ss, ds in shapes:
        p.add(extent, ss, ds)
    return p.moves


def test_the_rule_looks_at_every_move_of_the_launch():
    d = cd.cudecompExtDescribeMove(BASE[0], BASE[1], 8, *FORWARD, STREAMING)
    assert (d["run"], d["walk"], d["access"]) == (512, 3, 2), d
    assert pads(listed(FORWARD), 8, STREAMING)[0] == [FORWARD_PAD]
    assert pads(listed(FORWARD, FORWARD), 8, STREAMING)[0] == [FORWARD_PAD]
    for mixed in ((FORWARD, SMALL), (SMALL, FORWARD), (FORWARD, SMALL, FORWARD)):  # one launch, one of its moves without a run
        got, (l,) = pads(listed(*mixed), 8, STREAMING)
        assert l["n"] == len(mixed) and got == [0], mixed
    d = cd.cudecompExtDescribeMove(BASE[0], BASE[1], 8, *PLANES, STREAMING)
    assert d["run"] > 1 and d["walk"] & 4, d  # runs over batch planes: not the measured case
    assert pads(listed(PLANES), 8, STREAMING)[0] == [0]
    assert pads(listed(FORWARD, PLANES), 8, STREAMING)[0] == [0]


def test_cached_moves_launch_without_a_pad():
    assert pads(listed(SMALL), 8)[0] == [0]
    got, (l,) = pads(listed(((64, 256, 16), (1, 64, 64 * 256), (256 * 16, 1, 256))), 8)  # the forward geometry, below the streaming size
    assert l["access"] == 0 and got == [0]
    got, (l,) = pads(listed(((64, 256, 33), (1, 64 * 33, 64), (256, 1, 64 * 256))), 8)  # the inverse geometry, cached: 64 x 64 tile
    assert (l["access"], l["tile_j"]) == (0, 64) and got == [0]


def test_window_lines_row_lines_and_row_copies_launch_without_a_pad():
    seen = set()
    for gdims, ac, halo in (((1024, 1024, 1024), (1, 1, 1), (1, 1, 1)), ((1024, 1024, 1024), (0, 0, 0), (1, 1, 1)),
                            ((2048, 1024, 256), (1, 1, 1), (2, 2, 2)), ((1024, 1024, 1024), (0, 0, 0), None)):
        for op, moves in planned(gdims, ac, 8, halo).items():
            got, launches = pads(moves, 8)
            assert got == [0] * len(launches), (gdims, ac, halo, op)
            seen |= {ML.KINDS[l["kind"]] for l in launches}
    assert {"transpose_lines", "transpose_rowlines", "rows_dense", "rows"} <= seen, seen
    # the window kernel: a streaming transpose onto rows off the 64-byte grid that says nothing about whole rows
    got, (l,) = pads([cd.make_move((1024, 1024, 8), (1, 1024, 1 << 20), (1026, 1, 1026 * 1024), 0, 1)], 8, STREAMING)
    assert ML.KINDS[l["kind"]] == "transpose_window" and got == [0], l


def test_refusals():
    with pytest.raises(cd.CudecompError) as e:
        cd.cudecompExtDescribeResidency(listed(SMALL), ADDRESSES, 3)
    assert e.value.code == cd.RESULT_INVALID_USAGE
    assert cd.cudecompExtDescribeResidency([], ADDRESSES, 8) == []
