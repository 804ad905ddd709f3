"""Batched kernel launches on the GPU: LISTS of moves through cudecompExtRunMoves -- the entry to csrc/kernels.cc launchMoves
that takes what the executor's phases and the one-sided transports pass: many moves, and optionally one destination base per
move -- against numpy applying the moves one after the other (oracle.move3d_reference for copies, AB.typed_add for additions,
an assignment for fills).  The single-move parity tests (tests/test_gpu_kernels.py and its siblings) only ever launch a Batch of
one move; these reach what a batch adds: the workgroup -> (move, local workgroup) decode of kernels_dev.h (findMove for local
transposes, block % n and the filler workgroups of interleaved launches), the per-move geometry arrays t0 / t1 / p0 / p1, the
XCD-contiguous tile walk taken from the move's own workgroup count, the split at 8 moves and the regrouping by kernel choice, and
the system-scope stores of destinations given by base pointers.

Every test asserts first that the destination cells of its list are disjoint, compares EVERY byte of every destination buffer
(256 poison bytes on both sides and the cells between the moves included) bit for bit -- additions under the any-NaN rule of
tests/test_gpu_halo_accumulate.py: where the expected real is a NaN the device's must be a NaN -- and requires the launches per
class, the launches in all and the elements per class that cudecompExtDescribeMoves predicts for the same addresses, so the
batch form under test is the one that ran (tests/move_lists.py run_list).  The lists are composed from candidate moves by what
the describe entry says about each (kernel choice, workgroups), never by hand."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import move_lists as ML

pytestmark = pytest.mark.gpu

STREAMING, ALWAYS, NEVER, I_FIRST, J_FIRST = 2, 4, 8, 64, 128  # flags of cudecompExtMove3D / cudecompExtRunMoves (1: element-wise)
WORKGROUPS = [1, 1, 300, 2, 40, 1, 7, 120]  # wanted per move of the unequal lists; what they get comes from the describe entry
ORDERS = {"smallest_first": lambda c: sorted(range(8), key=lambda i: c[i]), "smallest_last": lambda c: sorted(range(8), key=lambda i: -c[i]),
          "shuffled": lambda c: [5, 2, 7, 0, 3, 6, 1, 4]}


@pytest.fixture(scope="module", autouse=True)
def no_rank_pool_beside_this_process():
    """these tests use the GPU from the process that runs them: the rank pool of the multi-rank tests ends first"""
    from tests import mp
    mp.pool_stop()


def counts_of(launch):
    return [b - a for a, b in zip(launch["first_block"], launch["first_block"][1:])]


def test_the_comparison_notices_a_move_that_did_not_land():
    """the harness itself: the device runs three row moves, numpy is told of two -- whichever is left out, the run must fail"""
    p = ML.Packer(gap=2, align=8)
    for i in range(3):
        p.add((64, 7, 3), (1, 80, 720), (1, 64, 512))
    ML.run_list(p.moves, 8)
    for dropped in range(3):
        with pytest.raises(AssertionError, match="bytes differ"):
            ML.run_list(p.moves, 8, reference_moves=[m for i, m in enumerate(p.moves) if i != dropped])


# ---- unequal workgroup counts in one interleaved launch ---------------------------------------------------------------------------
def widths(es, vec):
    """row lengths (elements) whose widest lane is `vec` bytes: an odd number of lanes"""
    return [max(1, vec // es) * k for k in (1, 3, 5, 9, 17, 33, 65, 129, 257)] if vec >= es else []


def _unequal_cases():
    C, A, F = cd.MOVES_COPY, cd.MOVES_ADD, cd.MOVES_FILL
    cases = []
    for es in (2, 4, 8, 16):
        for vec in (16, 8, 4, 2):
            if vec >= es:  # rows_kernel at every lane width the element size has
                cases.append(("rows_kernel_es%d_vec%d" % (es, vec), es, C, 0, 0, "rows", vec, dict(widths=widths(es, vec))))
        cases.append(("generic_kernel_es%d" % es, es, C, 0, 1, "generic", es, dict(widths=[1, 3, 8, 33, 130])))
        cases.append(("rows_fill_kernel_es%d" % es, es, F, 0, 0, "rows_fill", 16, dict(widths=[1, 3, 8, 33, 130, 1031], doff=1)))
        cases.append(("generic_fill_kernel_es%d" % es, es, F, 0, 1, "generic_fill", es, dict(widths=[1, 3, 8, 33, 130])))
    for es in (4, 8, 16):  # destinations off the 64-byte grid, rows of 256 bytes and more (no 2-byte forms of these two)
        w = [k * 16 // es + 64 for k in (4, 5, 9, 17, 33, 65, 129)]
        cases.append(("rows_shifted_kernel_es%d" % es, es, C, 0, ALWAYS, "rows_shifted", 16, dict(widths=w, doff=1)))
        cases.append(("rows_dense_kernel_es%d" % es, es, C, 0, ALWAYS, "rows_dense", 16, dict(widths=w, doff=1, dpad=2, pitch=True)))
    for dtype in (cd.HALF, cd.FLOAT, cd.DOUBLE_COMPLEX):
        es = AB.element_bytes(dtype)
        for vec in (16, 8, 4, 2):
            if vec >= es:
                cases.append(("rows_accumulate_kernel_%s_vec%d" % (AB.NAMES[dtype], vec), es, A, dtype, 0, "rows_add", vec, dict(widths=widths(es, vec))))
        cases.append(("generic_accumulate_kernel_%s" % AB.NAMES[dtype], es, A, dtype, 1, "generic_add", es, dict(widths=[1, 3, 8, 33, 130])))
    return cases


UNEQUAL = _unequal_cases()


def unequal_list(es, mode, dtype, flags, kind, vec, rows):
    """eight moves of ONE kernel choice (`kind` at lane width `vec`) whose workgroup counts are nearest to WORKGROUPS, packed into
    regions that start on 256-element boundaries (each keeps the alignment it was chosen at)"""
    groups = ML.groups_by_choice(ML.row_candidates(es, **rows), es, mode, dtype, flags)
    fitting = [g for c, g in groups.items() if ML.KINDS[c[0]] == kind and c[2] == vec]
    assert fitting, (kind, vec, sorted((ML.KINDS[c[0]], c[2]) for c in groups))
    group = max(fitting, key=lambda g: len({m[0] for m in g}))
    p = ML.Packer(gap=3, align=256)
    for _, _, (extent, ss, ds, soff, doff, pitch) in ML.pick_by_workgroups(group, WORKGROUPS):
        p.add(extent, ss, ds, soff, doff, row_pitch=pitch)
    return p.moves


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name,es,mode,dtype,flags,kind,vec,rows", UNEQUAL, ids=[c[0] for c in UNEQUAL])
def test_unequal_workgroup_counts_in_one_interleaved_launch(name, es, mode, dtype, flags, kind, vec, rows, order):
    """a filler workgroup that does not leave, or a move indexed with another move's geometry, changes a poison byte or a
    neighbour's cells"""
    moves = unequal_list(es, mode, dtype, flags, kind, vec, rows)
    (alone,) = ML.describe(moves, ML.FAKE, es, mode, dtype, flags)
    moves = ML.reorder(moves, ORDERS[order](counts_of(alone)))
    value = np.random.default_rng(es).integers(1, 255, es, dtype=np.uint8).tobytes() if mode == cd.MOVES_FILL else None
    (l,) = ML.run_list(moves, es, mode, dtype, value, flags, seed=len(name))
    counts = counts_of(l)
    assert (ML.KINDS[l["kind"]], l["vec"], l["n"], l["interleave"]) == (kind, vec, 8, 1), l
    assert l["blocks"] == 8 * max(counts) and max(counts) >= 100 * min(counts) and len(set(counts)) >= 5, counts
    if order != "shuffled":
        assert counts == sorted(counts, reverse=order == "smallest_last")


# ---- local transposes: findMove, the tile walk per move ---------------------------------------------------------------------------
SHAPES = [(130, 70, 3), (64, 64, 1), (200, 9, 5), (16, 260, 2)]
DST_ORDERS = [(1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]  # memory position i of the destination holds source dim DST_ORDERS[.][i]


def transpose_candidates(doff=0, pads=((0, 0), (3, 1))):
    """the four shapes and the permutations of their extents, written in every order that makes another dim the destination's
    fastest, dense and with halo-style padding on both sides"""
    seen = set()
    for shape, pad in itertools.product(SHAPES, pads):
        for ext in itertools.permutations(shape):
            for dperm in DST_ORDERS:
                ss, _ = ML.padded_strides(ext, (0, 1, 2), pad)
                ds, _ = ML.padded_strides(ext, dperm, pad)
                if (ext, tuple(ds), pad) not in seen:
                    seen.add((ext, tuple(ds), pad))
                    yield (ext, tuple(ss), tuple(ds), 0, doff, 0)


def spread(group, n):
    """n members of a choice group with workgroup counts that are no multiple of 8, spread over the counts the group has,
    the largest and the smallest among them"""
    odd = sorted((m for m in group if m[0] % 8 != 0), key=lambda m: (m[0], m[1]))
    by_count = {}
    for m in odd:
        by_count.setdefault(m[0], []).append(m)
    keys = sorted(by_count)
    if len(keys) < 2:
        return None
    picked = [by_count[keys[(len(keys) - 1) * i // (n - 1)]] for i in range(n)] if n > 1 else [by_count[keys[0]]]
    out, used = [], {}
    for members in picked:  # the same count twice: its next member (another shape or order)
        k = used.get(id(members), 0)
        used[id(members)] = k + 1
        out.append(members[k % len(members)])
    return out


def transpose_lists(es, flags, kinds, doff=0, sizes=(2, 3, 8)):
    """per kernel choice the candidates fall into (largest groups first), lists of 2, 3 and 8 of its moves"""
    groups = ML.groups_by_choice(transpose_candidates(doff), es, flags=flags)
    out = []
    for choice, group in sorted(groups.items(), key=lambda kv: -len(kv[1])):
        if ML.KINDS[choice[0]] in kinds:
            for n in sizes:
                members = spread(group, n)
                if members is not None:
                    p = ML.Packer(gap=5, align=256)
                    for _, _, (extent, ss, ds, soff, off, pitch) in members:
                        p.add(extent, ss, ds, soff, off, row_pitch=pitch)
                    out.append((choice, p.moves))
    return out


def tiles_of(m, es, flags):
    r = cd.cudecompExtDescribeMove(ML.FAKE[0] + m.src_off * es, ML.FAKE[1] + m.dst_off * es, es, tuple(m.extent), tuple(m.ss), tuple(m.ds), flags)
    return r["tiles_i"], r["tiles_j"], r["batch"]


def run_transpose_lists(es, flags, kinds, doff=0):
    lists = transpose_lists(es, flags, kinds, doff)
    sizes, shapes = set(), set()
    for choice, moves in lists:
        (l,) = ML.run_list(moves, es, flags=flags, seed=len(moves) + es)
        counts = counts_of(l)
        assert ML.choice_of(l) == choice and l["n"] == len(moves) and l["interleave"] == 0 and l["blocks"] == sum(counts), l
        assert all(c % 8 != 0 for c in counts) and len(set(counts)) >= 2, counts  # the remainder of the XCD walk differs per move
        sizes.add(len(moves))
        for m in moves:
            ti, tj, _ = tiles_of(m, es, flags & ~NEVER)
            shapes.add("rows" if ti > tj else ("columns" if tj > ti else "square"))
    assert sizes == {2, 3, 8}, sizes
    assert {"rows", "columns"} <= shapes  # more tile rows than columns and the reverse, so t0 and t1 are told apart
    return lists


@pytest.mark.parametrize("flags", [0, STREAMING, I_FIRST, J_FIRST | STREAMING], ids=["default", "streaming", "i_first", "j_first_streaming"])
@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_local_transpose_batches(es, flags):
    lists = run_transpose_lists(es, flags, ("transpose",))
    assert {c[2] for c, _ in lists} >= ({1, 16 // es} if es < 16 else {1})  # element-wise lanes and 16-byte lanes


@pytest.mark.parametrize("es", [4, 8, 16])
def test_window_transpose_batches_off_the_64_byte_grid(es):
    for doff in (1, 3):
        for choice, moves in run_transpose_lists(es, ALWAYS, ("transpose_window",), doff):
            assert all((m.dst_off * es) % 64 != 0 for m in moves)


@pytest.mark.parametrize("es", [4, 8, 16])
def test_far_strided_run_walk_beside_a_small_move(es):
    """a forward hop of an axis-contiguous cycle (destination rows far apart: the tile walk in runs over batch planes, p0 > 1)
    and a small line-aligned transpose in one launch, in both orders: the run length and the walk bits are per move.  (The moves
    of test_transpose_far_strided_destination_walk are too small for a run of tiles and their planes fuse into the rows, so the
    describe entry reports no runs for them; this one keeps its planes apart.)"""
    ei, ej, ek, pitch = 64, 192, 32, 256  # destination (y, z, x) with the rows of consecutive planes a line-aligned pitch apart
    far = ((ei, ej, ek), (1, ei, ei * ej), (pitch * ek, 1, pitch), 0, 0, 0)
    small = ((64, 64, 3), (1, 64, 4096), (64, 1, 4096), 0, 0, 0)
    lone = cd.cudecompExtDescribeMove(ML.FAKE[0], ML.FAKE[1], es, *far[:3], STREAMING)
    assert lone["run"] > 1 and lone["walk"] & 2, lone
    assert cd.cudecompExtDescribeMove(ML.FAKE[0], ML.FAKE[1], es, *small[:3], STREAMING)["run"] <= 1
    for order in ((far, small), (small, far), (small, far, small)):
        p = ML.Packer(gap=0, align=256)
        for extent, ss, ds, soff, doff, _ in order:
            p.add(extent, ss, ds, soff, doff)
        (l,) = ML.run_list(p.moves, es, flags=STREAMING, seed=es)
        assert ML.KINDS[l["kind"]] == "transpose" and l["n"] == len(order) and l["interleave"] == 0 and l["access"] == 2, l
        assert len(set(counts_of(l))) == 2


# the halo configurations of test_planned_moves_onto_halo_and_padding_pencils (tests/test_gpu_kernels.py)
PLAN_ORDERS = {"default": [(0, 1, 2)] * 3, "contiguous": [(0, 1, 2), (1, 2, 0), (2, 0, 1)]}
PLAN_AXES = {"XToY": (0, 1), "YToZ": (1, 2), "ZToY": (2, 1), "YToX": (1, 0)}
PLAN_SHIFTED = [(2, 1, 1), (1, 2, 1), (1, 1, 2)]
PLAN_CONFIGS = [("contiguous", [(1, 1, 1)] * 3, [(1, 1, 1), None, (1, 1, 1)]), ("default", PLAN_SHIFTED, [None] * 3),
                ("contiguous", PLAN_SHIFTED, [None] * 3)]


LONG_AXIS = {4: 340, 8: 168, 16: 96}  # rows long enough for both whole-line kernels at this element size (two windows and more)


def planned_whole_row_transposes(es):
    """The transposing moves to which the planner gives a row pitch (they write whole interior rows of a halo-carrying pencil),
    over those configurations on one, two and four ranks: of the (64, 60, 68) grid, and -- its rows are too short for the
    whole-line kernels at 4 and 8 bytes per element -- of slim grids with one long axis.  As candidates (extent, ss, ds, source
    offset, destination offset, row pitch), each once."""
    L = LONG_AXIS[es]
    out = set()
    for gdims in [(64, 60, 68), (12, L, 20), (20, L, 12), (L, 20, 12), (12, 20, L)]:
        for (layout, halo, pad), pdims in itertools.product(PLAN_CONFIGS, [(1, 1), (1, 2), (2, 1), (1, 4), (4, 1)]):
            grid = cd.make_grid_spec(gdims, pdims, PLAN_ORDERS[layout])
            for rank, op in itertools.product(range(pdims[0] * pdims[1]), cd.OPS):
                a, b = PLAN_AXES[op]
                plan = cd.cudecompExtPlanTranspose(grid, rank, op, halo[a], halo[b], pad[a], pad[b])
                for m in list(plan.pack)[:plan.n_pack] + list(plan.unpack)[:plan.n_unpack]:
                    if m.row_pitch > 0 and not (m.ss[0] == 1 and m.ds[0] == 1) and 0 not in tuple(m.extent):
                        out.add((tuple(m.extent), tuple(m.ss), tuple(m.ds), m.src_off, m.dst_off, m.row_pitch))
    return sorted(out)


@pytest.mark.parametrize("es", [4, 8, 16])
def test_whole_line_transposes_of_planned_moves_in_batches(es):
    """transpose_lines_kernel / transpose_rowlines_kernel: the planner only ever hands them one move at a time (a transposing move
    that covers whole rows is the single move of its phase), so a batch of them is composed here -- 2, 3 and 8 planned moves of
    one choice, each with the planner's offsets, strides and row pitch inside a region of its own, the window variants switched on
    for these small moves as run_move of tests/test_gpu_kernels.py does"""
    groups = ML.groups_by_choice(planned_whole_row_transposes(es), es, flags=ALWAYS)
    ran = {}
    for choice, group in sorted(groups.items()):
        kind = ML.KINDS[choice[0]]
        for n in (2, 3, 8):
            members = spread(group, n) if kind in ("transpose_lines", "transpose_rowlines") else None
            if members is None:
                continue
            p = ML.Packer(gap=7, align=256)
            for _, _, (extent, ss, ds, soff, doff, pitch) in members:
                p.add(extent, ss, ds, soff, doff, row_pitch=pitch)
            (l,) = ML.run_list(p.moves, es, flags=ALWAYS, seed=n + es)
            assert ML.choice_of(l) == choice and l["n"] == n and l["interleave"] == 0 and len(set(counts_of(l))) >= 2, l
            ran.setdefault(kind, set()).add(n)
    assert ran == {"transpose_lines": {2, 3, 8}, "transpose_rowlines": {2, 3, 8}}, ran


# ---- mixed lists, more than eight moves ---------------------------------------------------------------------------------------------
def kinds_of_four(i, es):
    """rows with 16-byte lanes / a transpose / a gather (element-wise) / rows with narrower lanes, sizes varying with i"""
    k = i // 4
    return [((64 + 16 * k, 7 + 30 * k, 3), (1, 100 + 16 * k, (100 + 16 * k) * (40 + 30 * k)), (1, 64 + 16 * k, (64 + 16 * k) * (8 + 30 * k)), 0, 0, 0),
            ((70 + 64 * k, 66, 2 + k), (1, 70 + 64 * k, (70 + 64 * k) * 66), (66, 1, (70 + 64 * k) * 66), 0, 0, 0),
            ((1, 50 + 7 * k, 20), (1, 64, 64 * (52 + 7 * k)), (1, 1, 50 + 7 * k), 2, 0, 0),
            ((63 + 2 * k, 9 + k, 5), (1, 80, 80 * 20), (1, 75, 75 * 15), 1, 1, 0)][i % 4]


@pytest.mark.parametrize("es", [4, 8, 16])
def test_mixed_list_of_twenty_moves_with_empty_ones(es):
    p = ML.Packer(gap=2, align=1)
    for i in range(20):
        extent, ss, ds, soff, doff, _ = kinds_of_four(i, es)
        if i in (0, 9, 19):  # an empty move at the head, in the middle and at the tail
            extent = tuple(0 if d == i % 3 else e for d, e in enumerate(extent))
        p.add(extent, ss, ds, soff, doff, ML.span(kinds_of_four(i, es)[0], ss), ML.span(kinds_of_four(i, es)[0], ds))
    launches = ML.run_list(p.moves, es, seed=es)
    assert len(launches) >= 4 and {l["cls"] for l in launches} == {0, 1, 2}
    assert sorted(i for l in launches for i in l["index"]) == [i for i in range(20) if i not in (0, 9, 19)]
    assert all(l["interleave"] == (1 if l["n"] > 1 and l["cls"] != 1 else 0) for l in launches)
    ML.run_list(p.moves, es, flags=1, seed=es + 1)  # ... and all of them element-wise: two interleaved launches + one


@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("mode,dtype,es", [(cd.MOVES_COPY, 0, 8), (cd.MOVES_COPY, 0, 2), (cd.MOVES_ADD, cd.FLOAT_COMPLEX, 8),
                                           (cd.MOVES_FILL, 0, 16)], ids=["copy_es8", "copy_es2", "add_complex64", "fill_es16"])
def test_more_than_eight_row_moves(n, mode, dtype, es):
    """every one lands exactly once: a move that is dropped leaves its cells as they were, one that runs twice adds twice"""
    p = ML.Packer(gap=2, align=8)
    for i in range(n):
        w, h = 64 + 16 * (i % 5), 3 + 11 * (i % 4)
        p.add((w, h, 2), (1, w + 16, (w + 16) * (h + 1)), (1, w, w * (h + 2)))
    value = bytes(range(1, es + 1)) if mode == cd.MOVES_FILL else None
    launches = ML.run_list(p.moves, es, mode, dtype, value, seed=n)
    assert [l["n"] for l in launches] == [8] * (n // 8) + [n % 8]
    assert [i for l in launches for i in l["index"]] == list(range(n))
    assert all(l["interleave"] == (1 if l["n"] > 1 else 0) for l in launches)


@pytest.mark.parametrize("es", [2, 8])
def test_nine_transposes(es):
    p = ML.Packer(gap=1, align=256)
    for i in range(9):
        ei, ej, ek = 64 * (1 + i % 3) + 6, 64 * (1 + i % 2) + 2, 1 + i % 4
        p.add((ei, ej, ek), (1, ei, ei * ej), (ej, 1, ei * ej))
    launches = ML.run_list(p.moves, es, seed=es)
    assert [(ML.KINDS[l["kind"]], l["n"], l["interleave"]) for l in launches] == [("transpose", 8, 0), ("transpose", 1, 0)]
    assert [i for l in launches for i in l["index"]] == list(range(9))


# ---- destination bases: the calling form of the one-sided transports, on local memory ----------------------------------------------
# csrc/peer_exchange.cc gives EVERY move of an exchange the receive area (or output pencil) of the member it feeds as its destination
# base, the rank's own slot included (remote_recv[own rank] is its own buffer): a local buffer behind a base pointer is what the
# library itself passes.
@pytest.mark.parametrize("what", ["rows", "generic", "transposes"])
@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_destination_bases(what, es):
    flags = 1 if what == "generic" else 0
    if what == "transposes":
        cands = [(ext, (1, ext[0], ext[0] * ext[1]), (ext[1], 1, ext[0] * ext[1]), 0, off, 0)
                 for ext, off in (((130, 70, 3), 0), ((64, 64, 1), 2), ((200, 9, 5), 0), ((16, 260, 2), 4), ((66, 134, 2), 0), ((8, 8, 40), 6),
                                 ((8, 12, 1), 0), ((6, 5, 1), 2))]
    else:
        cands = [((w, h, d), (1, w + 6, (w + 6) * (h + 1)), (1, w + 2, (w + 2) * (h + 2)), 1, off, 0)
                 for (w, h, d), off in (((64, 7, 3), 0), ((128, 150, 7), 4), ((8, 33, 2), 0), ((520, 70, 3), 8), ((16, 400, 7), 0), ((72, 1, 1), 12))]
    moves = [cd.make_move(ext, ss, ds, soff + 1000 * i, doff) for i, (ext, ss, ds, soff, doff, _) in enumerate(cands)]
    launches = ML.run_list(moves, es, flags=flags, bases=True, seed=es)
    assert all(l["access"] == 3 for l in launches), launches          # the stores of a peer's memory
    assert all(l["interleave"] == 1 for l in launches if l["n"] > 1)  # transposes too
    assert any(l["n"] >= 3 and max(counts_of(l)) >= 8 * min(counts_of(l)) for l in launches), launches  # unequal moves in one launch
    assert {ML.KINDS[l["kind"]] for l in launches} <= {"rows": {"rows", "rows_shifted"}, "generic": {"generic"}, "transposes": {"transpose"}}[what]


@pytest.mark.parametrize("mode,dtype", [(cd.MOVES_ADD, cd.DOUBLE), (cd.MOVES_FILL, 0)], ids=["add", "fill"])
def test_additions_and_fills_with_destination_bases_are_refused_before_any_launch(mode, dtype):
    import torch
    moves = [cd.make_move((64, 7, 3), (1, 80, 720), (1, 64, 512), 1000 * i, 0) for i in range(3)]
    rng = np.random.default_rng(1)
    host = [rng.integers(0, 256, 4096 * 8, dtype=np.uint8) for _ in range(4)]
    dev = [torch.from_numpy(h.copy()).cuda() for h in host]
    with pytest.raises(cd.CudecompError) as e:
        cd.cudecompExtRunMoves(moves, [dev[0].data_ptr(), None, None], 8, mode, dtype, None, 0, [t.data_ptr() for t in dev[1:]],
                               torch.cuda.current_stream().cuda_stream)
    assert e.value.code == cd.RESULT_INTERNAL_ERROR
    torch.cuda.synchronize()
    for t, h in zip(dev, host):
        assert np.array_equal(t.cpu().numpy(), h)


# ---- property sweep -------------------------------------------------------------------------------------------------------------------
def test_random_lists_property_sweep():
    """random lists of 2..12 moves drawn from the strategy of the single-move sweep (any permutations, pads and offsets), packed
    into disjoint regions of one destination buffer: with flag 0 the fast paths in whatever batches the choices give, with flag 1
    all element-wise -- one or two big interleaved launches"""
    from hypothesis import HealthCheck, given, settings
    from hypothesis import strategies as st

    @settings(max_examples=100, deadline=None, suppress_health_check=list(HealthCheck))
    @given(es=st.sampled_from([2, 4, 8, 16]), drawn=st.lists(st.fixed_dictionaries(ML.shape_strategies(st)), min_size=2, max_size=12),
           seed=st.integers(0, 1 << 20))
    def check(es, drawn, seed):
        p = ML.Packer(gap=1, align=1)
        for d in drawn:
            ss, slen = ML.padded_strides(d["ext"], d["sperm"], d["spad"])
            ds, dlen = ML.padded_strides(d["ext"], d["dperm"], d["dpad"])
            p.add(d["ext"], ss, ds, d["soff"], d["doff"], slen, dlen)
        ML.run_list(p.moves, es, flags=0, seed=seed)
        launches = ML.run_list(p.moves, es, flags=1, seed=seed + 1)
        assert [l["n"] for l in launches] == [8] * (len(drawn) // 8) + ([len(drawn) % 8] if len(drawn) % 8 else [])
        assert all(ML.KINDS[l["kind"]] == "generic" and l["interleave"] == (1 if l["n"] > 1 else 0) for l in launches)

    check()
