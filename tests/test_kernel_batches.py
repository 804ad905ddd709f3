"""WHICH launches the kernel layer makes for a LIST of moves (csrc/kernels.cc planLaunches, the host step in front of every
launch), through cudecompExtDescribeMoves -- no GPU, no memory: the split at 8 moves, that every non-empty move lands in exactly
one launch and empty ones in none, the regrouping by kernel choice in the order of first appearance, the interleave rule (several
moves that are no local transposes: workgroup b serves move b % n, the launch padded to widest * n workgroups), the limits at
2^31 - 1 workgroups, and a property sweep over random lists.  tests/test_gpu_kernel_batches.py runs such lists on the GPU and
requires the launch counts this entry predicts."""
import itertools
import math
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402
from tests import move_lists as ML  # noqa: E402

SRC, DST, WORK = 1 << 32, 1 << 36, 1 << 40  # line-aligned "addresses" of buffers 0, 1, 2
ADDR = (SRC, DST, WORK)
LIMIT = 0x7fffffff


def row_move(i, w=64, h=7, d=3, **kw):
    """rows of w elements, region i of the destination"""
    return cd.make_move((w, h, d), (1, w + 16, (w + 16) * (h + 2)), (1, w, w * (h + 1)), src_off=i << 20, dst_off=i << 20, **kw)


def transpose_move(i, ei=70, ej=66, ek=5):
    return cd.make_move((ei, ej, ek), (1, ei, ei * ej), (ej, 1, ei * ej), src_off=i << 20, dst_off=i << 20)


def gather_move(i):
    """1-element rows gathered with a stride: the element-wise kernel"""
    return cd.make_move((1, 50, 20), (1, 64, 64 * 52), (1, 1, 50), src_off=i << 20, dst_off=i << 20)


def empty_move(i, dim):
    m = row_move(i)
    m.extent[dim] = 0
    return m


def served(launches):
    return [i for l in launches for i in l["index"]]


def check_shape(launches):
    """what holds for every launch: its moves' workgroups are consecutive ranges, and the interleave rule for its block count"""
    for l in launches:
        fb = l["first_block"]
        assert 1 <= l["n"] <= 8 and len(fb) == l["n"] + 1 and fb[0] == 0 and len(l["index"]) == l["n"]
        counts = [b - a for a, b in zip(fb, fb[1:])]
        assert min(counts) >= 1
        if l["interleave"]:
            assert l["n"] > 1 and l["blocks"] == max(counts) * l["n"]
        else:
            assert l["blocks"] == fb[-1]
        assert l["blocks"] <= LIMIT


@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 16, 17, 25])
@pytest.mark.parametrize("kind", ["rows", "transpose", "generic"])
def test_split_at_eight(n, kind):
    make = {"rows": row_move, "transpose": transpose_move, "generic": gather_move}[kind]
    launches = ML.describe([make(i) for i in range(n)], ADDR, 8)
    check_shape(launches)
    assert len(launches) == math.ceil(n / 8)
    assert [l["n"] for l in launches] == [8] * (n // 8) + ([n % 8] if n % 8 else [])
    assert served(launches) == list(range(n))  # in list order, each once
    assert {ML.KINDS[l["kind"]] for l in launches} == {kind}


@pytest.mark.parametrize("mode,dtype", [(cd.MOVES_COPY, 0), (cd.MOVES_ADD, cd.DOUBLE), (cd.MOVES_FILL, 0)], ids=["copy", "add", "fill"])
def test_every_move_in_exactly_one_launch_and_empty_moves_in_none(mode, dtype):
    # empty moves (one zero extent) at the head, in the middle and at the tail of an 11-move list
    moves = [empty_move(0, 0)] + [row_move(i) for i in range(1, 5)] + [empty_move(5, 1), empty_move(6, 2)] + \
            [row_move(i) for i in range(7, 10)] + [empty_move(10, 2)]
    launches = ML.describe(moves, ADDR, 8, mode, dtype)
    check_shape(launches)
    assert sorted(served(launches)) == [1, 2, 3, 4, 7, 8, 9]
    assert len(launches) == 1 and launches[0]["elements"] == 7 * 64 * 7 * 3
    # ... and 9 non-empty ones around them: the ninth starts a launch of its own
    moves += [row_move(i) for i in range(11, 13)]
    launches = ML.describe(moves, ADDR, 8, mode, dtype)
    assert [l["index"] for l in launches] == [[1, 2, 3, 4, 7, 8, 9, 11], [12]]
    # nothing but empty moves, and no moves at all: no launch
    assert ML.describe([empty_move(i, i % 3) for i in range(5)], ADDR, 8, mode, dtype) == []
    assert ML.describe([], ADDR, 8, mode, dtype) == []


def test_regrouping_by_choice_keeps_the_order_of_first_appearance():
    # rows (16-byte lanes) / transpose / generic / rows with 8-byte lanes (odd row length), three times over
    kinds = [lambda i: row_move(i), transpose_move, gather_move, lambda i: row_move(i, w=63)]
    moves = [kinds[i % 4](i) for i in range(12)]
    launches = ML.describe(moves, ADDR, 8)
    check_shape(launches)
    assert [(ML.KINDS[l["kind"]], l["vec"]) for l in launches] == [("rows", 16), ("transpose", 2), ("generic", 8), ("rows", 8)]
    assert [l["index"] for l in launches] == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]]
    assert [l["cls"] for l in launches] == [0, 1, 2, 0]
    # a group of more than eight is cut where the ninth of ITS choice comes, wherever that is in the list
    moves = [kinds[i % 2](i) for i in range(22)]  # 11 row moves and 11 transposes alternating
    launches = ML.describe(moves, ADDR, 8)
    assert [l["index"] for l in launches] == [list(range(0, 16, 2)), list(range(1, 16, 2)), [16, 18, 20], [17, 19, 21]]


def test_interleave_rule():
    rows = [row_move(i, h=7 + 40 * i) for i in range(3)]  # 3, 6 and 9 workgroups
    tr = [transpose_move(i, ek=1 + i) for i in range(3)]   # 4, 8 and 12 tiles
    (l,) = ML.describe(rows, ADDR, 8)
    counts = [b - a for a, b in zip(l["first_block"], l["first_block"][1:])]
    assert len(set(counts)) == 3 and l["interleave"] == 1 and l["blocks"] == max(counts) * 3
    (l,) = ML.describe(rows[:1], ADDR, 8)   # one move: nothing to interleave
    assert l["interleave"] == 0 and l["blocks"] == l["first_block"][1]
    (l,) = ML.describe(tr, ADDR, 8)         # local transposes keep their tile walk: one range of workgroups per move
    assert ML.KINDS[l["kind"]] == "transpose" and l["interleave"] == 0 and l["blocks"] == l["first_block"][3] and l["access"] == 0
    assert [b - a for a, b in zip(l["first_block"], l["first_block"][1:])] == [4, 8, 12]
    bases = [DST + (i << 30) for i in range(3)]
    (l,) = ML.describe(tr, ADDR, 8, base_addresses=bases)  # destination bases: interleaved, with the stores of a peer's memory
    assert ML.KINDS[l["kind"]] == "transpose" and l["interleave"] == 1 and l["blocks"] == 12 * 3 and l["access"] == 3
    (l,) = ML.describe(tr[:1], ADDR, 8, base_addresses=bases[:1])
    assert l["interleave"] == 0 and l["access"] == 3
    for mode, dtype, kinds in ((cd.MOVES_ADD, cd.FLOAT_COMPLEX, ("rows_add", "generic_add")), (cd.MOVES_FILL, 0, ("rows_fill", "generic_fill"))):
        for flags, kind in zip((0, 1), kinds):
            (l,) = ML.describe(rows, ADDR, 8, mode, dtype, flags)
            assert ML.KINDS[l["kind"]] == kind and l["interleave"] == 1 and l["n"] == 3
            check_shape([l])


def test_additions_and_fills_refuse_destination_bases():
    rows = [row_move(i) for i in range(2)]
    for mode, dtype in ((cd.MOVES_ADD, cd.DOUBLE), (cd.MOVES_FILL, 0)):
        with pytest.raises(cd.CudecompError) as e:
            ML.describe(rows, ADDR, 8, mode, dtype, base_addresses=[DST, DST + (1 << 30)])
        assert e.value.code == cd.RESULT_INTERNAL_ERROR


def tall_rows(i, blocks):
    """a row move of `blocks` workgroups, on paper: 4096-byte rows of fp32 (256 lanes of 16 bytes), 4 rows per workgroup; padded
    rows, so that they stay rows (contiguous ones would be fused into one)"""
    m = cd.make_move((1024, 4 * blocks, 1), (1, 1040, 0), (1, 1040, 0), src_off=i << 44, dst_off=i << 44)
    (l,) = ML.describe([m], ADDR, 4)
    assert l["blocks"] == blocks and ML.KINDS[l["kind"]] == "rows"
    return m


def test_limits_at_two_to_the_31_workgroups():
    """described only: nothing of these sizes is allocated or launched"""
    g, s = 1 << 30, 2048  # (s: the smallest of these moves that streams, 32 MiB, as the large ones do -- one kernel choice for all)
    # the third move would take the sum past 2^31 - 1: the launch is cut before it and it starts the next one
    launches = ML.describe([tall_rows(0, g), tall_rows(1, g - 3000), tall_rows(2, 3000), tall_rows(3, s)], ADDR, 4)
    assert len({(l["kind"], l["vec"], l["access"]) for l in launches}) == 1
    assert [l["index"] for l in launches] == [[0, 1], [2, 3]]
    assert launches[0]["first_block"] == [0, g, 2 * g - 3000]
    # ... whose widest * n is past the limit: no interleaving, the moves' workgroups one range after the other
    assert launches[0]["interleave"] == 0 and launches[0]["blocks"] == 2 * g - 3000
    assert launches[1]["interleave"] == 1 and launches[1]["blocks"] == 6000
    check_shape(launches)
    (l,) = ML.describe([tall_rows(0, g), tall_rows(1, g - 3000), tall_rows(2, 2999)], ADDR, 4)  # the control: exactly 2^31 - 1 fits
    assert l["index"] == [0, 1, 2] and l["blocks"] == LIMIT and l["interleave"] == 0
    # the sum fits, widest * n does not
    (l,) = ML.describe([tall_rows(0, g + 1), tall_rows(1, s)], ADDR, 4)
    assert l["interleave"] == 0 and l["blocks"] == g + 1 + s and l["first_block"] == [0, g + 1, g + 1 + s]
    (l,) = ML.describe([tall_rows(0, g - 1), tall_rows(1, s)], ADDR, 4)  # ... and the largest that is still interleaved
    assert l["interleave"] == 1 and l["blocks"] == 2 * g - 2
    # exactly the limit in one move is a launch; one workgroup more is refused
    (l,) = ML.describe([tall_rows(0, LIMIT)], ADDR, 4)
    assert l["blocks"] == LIMIT
    too_large = cd.make_move((1024, 4 * (LIMIT + 1), 1), (1, 1040, 0), (1, 1040, 0))
    for moves in ([too_large], [tall_rows(1, s), too_large]):
        with pytest.raises(cd.CudecompError) as e:
            ML.describe(moves, ADDR, 4)
        assert e.value.code == cd.RESULT_NOT_SUPPORTED


CHOICE = ("cls", "variant", "tile_i", "tile_j", "access")  # of a cudecompExtDescribeMove record: WHAT runs (the rest is the walk)


def test_random_lists_property_sweep():
    """random lists of up to 30 moves drawn from the strategy of the single-move sweep, some of them empty: the launches
    partition the non-empty moves, none holds more than 8, and all moves of a launch have the same single-move description"""
    from hypothesis import HealthCheck, given, settings
    from hypothesis import strategies as st

    one = st.fixed_dictionaries(dict(ML.shape_strategies(st), empty=st.sampled_from([-1] * 7 + [0, 1, 2])))

    # flags both entries read alike: 2 streaming access, 4 shifted / window kernels whatever the size, 64 / 128 the walk order
    @settings(max_examples=300, deadline=None, suppress_health_check=list(HealthCheck))
    @given(es=st.sampled_from([2, 4, 8, 16]), flags=st.sampled_from([0, 0, 2, 4, 6, 64, 128 | 2]), drawn=st.lists(one, min_size=0, max_size=30),
           bases=st.booleans())
    def check(es, flags, drawn, bases):
        p = ML.Packer()
        for d in drawn:
            ext = list(d["ext"])
            if d["empty"] >= 0:
                ext[d["empty"]] = 0
            ss, slen = ML.padded_strides(d["ext"], d["sperm"], d["spad"])
            ds, dlen = ML.padded_strides(d["ext"], d["dperm"], d["dpad"])
            p.add(ext, ss, ds, d["soff"], d["doff"], slen, dlen)
        moves = p.moves
        ML.assert_disjoint_destinations(moves)
        base_addresses = [DST + (i << 28) for i in range(len(moves))] if bases else None
        launches = ML.describe(moves, ADDR, es, flags=flags, base_addresses=base_addresses)
        check_shape(launches)
        live = [i for i, m in enumerate(moves) if 0 not in tuple(m.extent)]
        assert sorted(served(launches)) == live
        opened = [l["index"][0] for l in launches]
        assert opened == sorted(opened)  # a launch is made when the list reaches its first move: the order of first appearance
        for l in launches:
            assert l["index"] == sorted(l["index"])
            assert l["elements"] == sum(moves[i].extent[0] * moves[i].extent[1] * moves[i].extent[2] for i in l["index"])
            if bases:
                assert l["access"] == 3 and l["interleave"] == (1 if l["n"] > 1 else 0)
                continue  # (cudecompExtDescribeMove describes local destinations)
            assert l["interleave"] == (1 if l["n"] > 1 and l["cls"] != 1 else 0)
            records = set()
            for i in l["index"]:
                m = moves[i]
                r = cd.cudecompExtDescribeMove(SRC + m.src_off * es, DST + m.dst_off * es, es, tuple(m.extent), tuple(m.ss), tuple(m.ds), flags)
                records.add(tuple(r[k] for k in CHOICE))
                assert r["cls"] == l["cls"] and r["access"] == l["access"]
            assert len(records) == 1, (l, records)

    check()


# ---- the workgroup decode restated: what the GPU lists can tell apart ------------------------------------------------------------------
# kernels_dev.h locate() / findMove() and the tile decodes of kernels_rows.hip / kernels_tile.h in numpy, at workgroup granularity:
# which (move, tile i, tile j, plane) every workgroup of a launch serves.  Served correctly, every move gets each of its
# t0 * t1 * planes tiles exactly once and nothing else.  A tile that is never served leaves its cells as they were (random bytes
# on both sides: the comparison sees it); a served tile whose plane index is past the move's planes stores outside the move's
# cells (the tile kernels guard i and j against the extents, none guards the plane) -- into a neighbour's region, the cells
# between the regions or the poison.  The test below plants three decode faults into the restatement and requires that, at the
# lists tests/test_gpu_kernel_batches.py runs, each shows in that way -- and that none can show in a launch of one move, which
# is all the single-move parity tests ever make.
def served_tiles(launch, geometry, tiled, fault=None):
    """{move: [(tile i, tile j, plane)] of every workgroup that stores for it}; geometry[m] = (t0, t1, planes, run, walk)"""
    import numpy as np
    n, fb = launch["n"], launch["first_block"]
    nb = [fb[i + 1] - fb[i] for i in range(n)]
    block = np.arange(launch["blocks"], dtype=np.int64)
    if launch["interleave"]:
        mi, lb = block % n, block // n
        live = lb < np.array(nb)[mi] if fault != "fillers stay" else np.ones(block.size, dtype=bool)
    else:
        mi = np.zeros(block.size, dtype=np.int64)
        for i in range(1, n):
            mi[block >= fb[i]] = i
        lb, live = block - np.array(fb)[mi], np.ones(block.size, dtype=bool)
    out = {}
    for m in range(n):
        t0, t1, planes, run, walk = geometry[m]
        l = lb[(mi == m) & live]
        t0_read = geometry[0][0] if fault == "t0 of move 0" else t0
        if not tiled:  # rows_kernel and its siblings
            bi, rest = l % t0_read, l // t0_read
            bj, k = rest % t1, rest // t1
        else:          # transpose_kernel
            lt = l.copy()
            if walk & 1:
                per = (launch["blocks"] if fault == "per of the launch" else nb[m]) >> 3
                sel = l < (per << 3)
                lt[sel] = (l[sel] & 7) * per + (l[sel] >> 3)
            if walk & 2 and run > 1 and not walk & 4:
                jlo, rest = lt % run, lt // run
                bi, rest = rest % t0_read, rest // t0_read
                bj, k = (rest % (t1 // run)) * run + jlo, rest // (t1 // run)
            elif walk & 2 and run > 1:
                bj, rest = lt % t1, lt // t1
                klo, rest = rest % run, rest // run
                bi, k = rest % t0_read, (rest // t0_read) * run + klo
            elif walk & 2:
                bj, rest = lt % t1, lt // t1
                bi, k = rest % t0_read, rest // t0_read
            else:
                bi, rest = lt % t0_read, lt // t0_read
                bj, k = rest % t1, rest // t1
        stores = (bi < t0) & (bj < t1)  # (the guards against the extents)
        out[m] = sorted(zip(bi[stores].tolist(), bj[stores].tolist(), k[stores].tolist()))
    return out


def shows(launch, geometry, tiled, fault):
    """does the fault leave a tile unserved or store past a move's planes, in this launch?"""
    served = served_tiles(launch, geometry, tiled, fault)
    for m, (t0, t1, planes, _, _) in enumerate(geometry):
        full = sorted((i, j, k) for k in range(planes) for j in range(t1) for i in range(t0))
        inside = sorted(set(t for t in served[m] if t[2] < planes))
        if inside != full or any(t[2] >= planes for t in served[m]):
            return True
    return False


def geometry_of(moves, launch, es, flags):
    g = []
    for slot, i in enumerate(launch["index"]):
        m = moves[i]
        r = cd.cudecompExtDescribeMove(ML.FAKE[0] + m.src_off * es, ML.FAKE[1] + m.dst_off * es, es, tuple(m.extent), tuple(m.ss), tuple(m.ds),
                                       flags, m.row_pitch)
        g.append((r["tiles_i"], r["tiles_j"], r["batch"], r["run"], r["walk"]))
        assert r["tiles_i"] * r["tiles_j"] * r["batch"] == launch["first_block"][slot + 1] - launch["first_block"][slot]
    return g


FAULTS = ("fillers stay", "t0 of move 0", "per of the launch")


def test_planted_decode_faults_show_at_the_lists_the_gpu_tests_run():
    from tests import test_gpu_kernel_batches as GB
    seen = {f: 0 for f in FAULTS}
    # interleaved row copies with unequal workgroup counts, three orders
    for name, es, mode, dtype, flags, kind, vec, rows in GB.UNEQUAL:
        if kind != "rows":
            continue
        moves = GB.unequal_list(es, mode, dtype, flags, kind, vec, rows)
        (l,) = ML.describe(moves, ML.FAKE, es, mode, dtype, flags)
        for order in GB.ORDERS.values():
            ordered = ML.reorder(moves, order(GB.counts_of(l)))
            (lo,) = ML.describe(ordered, ML.FAKE, es, mode, dtype, flags)
            g = geometry_of(ordered, lo, es, flags)
            assert not shows(lo, g, False, None)                  # the restatement itself serves every tile once
            assert shows(lo, g, False, "fillers stay"), name
            seen["fillers stay"] += 1
    # local transposes of 2, 3 and 8 moves
    for es, flags in itertools.product((2, 4, 8, 16), (0, GB.STREAMING, GB.I_FIRST, GB.J_FIRST | GB.STREAMING)):
        hit = {f: 0 for f in FAULTS[1:]}
        for choice, moves in GB.transpose_lists(es, flags, ("transpose",)):
            (l,) = ML.describe(moves, ML.FAKE, es, flags=flags)
            g = geometry_of(moves, l, es, flags)
            assert not shows(l, g, True, None)
            assert not shows(l, g, True, "fillers stay")          # (no fillers in a launch that is not interleaved)
            for f in hit:
                hit[f] += shows(l, g, True, f)
        assert all(hit.values()), (es, flags, hit)                # every parametrised GPU case has a list that tells
        for f in hit:
            seen[f] += hit[f]
    assert all(seen.values()), seen
    # ... and a launch of ONE move cannot tell any of them: what the single-move entries launch
    for make, tiled in ((row_move, False), (transpose_move, True)):
        m = make(0)
        (l,) = ML.describe([m], ADDR, 8)
        g = geometry_of([m], l, 8, 0)
        for f in FAULTS:
            assert served_tiles(l, g, tiled, f) == served_tiles(l, g, tiled, None)
