"""The table of tests/tiled_instantiations.py, checked without a GPU: every recipe is described by cudecompExtDescribeMoves at
stand-in addresses (no launch) -- each move alone and the two-move list -- and must spell exactly its literal name; the shapes
must be those at which the kernel's branches are live (an interior tile and an edge tile, an XCD walk with a permuted part and a
tail, filler workgroups in the interleaved list).  tests/test_gpu_tiled_kernel_instantiations.py runs the same recipes."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402
from tests import move_lists as ML  # noqa: E402
from tests import tiled_instantiations as T  # noqa: E402

BASES = [(1 << 44) + (i << 32) for i in range(2)]  # 256-byte aligned stand-ins for the per-move destination buffers


def describe(recipe, which, extra=0):
    moves = recipe.moves(which)
    return moves, ML.describe(moves, ML.FAKE, recipe.es, cd.MOVES_COPY, 0, recipe.flags | extra, BASES[:len(moves)] if recipe.bases else None)


def test_inventory_counts():
    names = [n for g in T.GROUPS for n in T.INVENTORY[g]]
    assert len(names) == 76 and len(set(names)) == 76
    for family, count in T.COUNTS.items():
        assert sum(len(T.INVENTORY[g]) for g in T.GROUPS if g[0] == family) == count, family
    remote = [n for n in names if n.startswith(("rows_", "generic_")) or ",3>" in n or ",3,t" in n or ",3,f" in n]
    assert len(remote) == 11 + 5 + 7
    assert T.UNREACHABLE == {}


def test_every_name_has_one_recipe():
    got = [r.name for g in T.GROUPS for r in T.recipes(*g)]
    assert sorted(got) == sorted(n for g in T.GROUPS for n in T.INVENTORY[g])
    for g in T.GROUPS:
        assert [r.name for r in T.recipes(*g)] == T.INVENTORY[g], g
        assert all((r.family, r.es) == g for r in T.recipes(*g))


@pytest.mark.parametrize("family,es", T.GROUPS, ids=["%s-%d" % g for g in T.GROUPS])
def test_recipes_choose_their_kernels(family, es):
    for r in T.recipes(family, es):
        blocks = {}
        for which, extra in T.launches_of(r):
            moves, ls = describe(r, which, extra)
            what = (r.name, which, extra, ls)
            assert len(ls) == 1 and T.spell(ls[0]) == r.name, what
            l = ls[0]
            assert l["n"] == len(moves) and l["elements"] == sum(m.extent[0] * m.extent[1] * m.extent[2] for m in moves), what
            if which != "both":
                assert blocks.setdefault(which, l["blocks"]) == l["blocks"], what  # (the forced walks change no count)
                continue
            counts = [l["first_block"][i + 1] - l["first_block"][i] for i in range(2)]
            assert counts == [blocks["wide"], blocks["small"]] and counts[0] != counts[1], what
            if r.bases:  # one interleaved launch: the narrower move's surplus workgroups are fillers that locate() turns away
                assert l["interleave"] == 1 and l["blocks"] == 2 * max(counts) > sum(counts), what
            else:
                assert l["interleave"] == 0 and l["blocks"] == sum(counts), what
        # the XCD walk of the wide move: a permuted part (8 * per workgroups, per >= 1) and a tail
        assert blocks["wide"] >= 9 and blocks["wide"] % 8 != 0, (r.name, blocks)
        if family in T.TILED:
            inside, ending, total = r.tiles(r.wide)
            assert total == blocks["wide"] and inside >= 1 and ending >= 1, (r.name, inside, ending, total, blocks)
            inside, ending, total = r.tiles(r.small)
            assert total == blocks["small"] and inside == 0, (r.name, inside, ending, total, blocks)  # one tile row that ends inside the move
        for geo in (r.wide, r.small):  # every buffer stays under 4 MiB
            assert max(ML.span(geo[0], geo[1]), ML.span(geo[0], geo[2]) + r.doff) * es * 2 < 4 << 20, r.name


def test_plain_tiles_meet_all_four_edges():
    """the wide move of a plain transposition: exactly one interior tile per plane, and one tile that ends inside the move along
    i, one along j, one along both"""
    for g in T.GROUPS:
        for r in T.recipes(*g):
            if r.family != "transpose":
                continue
            (ei, ej, ek), (ti, tj) = r.wide[0], r.tile
            kinds = sorted(((bi + 1) * ti <= ei, (bj + 1) * tj <= ej) for bi in range(-(-ei // ti)) for bj in range(-(-ej // tj)))
            assert kinds == [(False, False), (False, True), (True, False), (True, True)] and ek == 3, (r.name, kinds)
            assert r.small[0][0] < ti and r.small[0][2] == 2, r.name


def test_window_recipes_have_both_edge_windows_and_rows_at_several_phases():
    for g in T.GROUPS:
        for r in T.recipes(*g):
            if r.family != "window":
                continue
            (ei, ej, _), _, ds, _ = r.wide
            u, tj = 64 // r.es, r.tile[1]
            jb = [b * tj - (u - 1) for b in range(-(-(ej + u - 1) // tj))]
            assert jb[0] < 0 and any(j >= 0 and j + tj + u - 1 <= ej for j in jb) and jb[-1] + tj + u - 1 > ej, (r.name, jb)
            assert (ds[0] * r.es) % 64 != 0 and (r.doff * r.es) % 64 != 0, r.name
            assert len({(r.doff + i * ds[0]) % u for i in range(ei)}) == u, r.name  # every phase of the unit
