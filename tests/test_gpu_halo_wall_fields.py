"""Multi-field wall halos (cudecomp_halo_wall_fields.h: cudecompAmdReflectFieldHalos{X,Y,Z}, cudecompAmdFoldFieldHalos{X,Y,Z}) on
the GPU: the mirrored field-move kernels against torch index arithmetic on small integers (every byte of an arena that holds all
fields, with slack around each); single-rank pencils of every axis, memory order, halo width, period mix, padding, dim and centering
against single calls on clones, ordered folds among them; launch counts; the plan cache; update + reflection sequences; the adjoint
identity; four ranks sharing the device; capture into a hipGraph.  Everything is compared byte for byte: no tolerance anywhere."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import wall_fields_bodies as WB
from tests.mp import run_ranks
from tests.test_halo_wall_fields_plan import ES, KINDS, NC, spell

pytestmark = pytest.mark.gpu

SLACK = 256  # bytes between any two fields (and before the first, after the last) that no move may touch
REFLECT, FOLD, FOLD_TAKE = cd.MIRROR_REFLECT, cd.MIRROR_FOLD, cd.MIRROR_FOLD_TAKE
MODES = (REFLECT, FOLD, FOLD_TAKE)
MASKS = ("none", "all", "alternating", "first", "last")


def mask_of(kind, n):
    every = (1 << n) - 1
    return {"none": 0, "all": every, "alternating": 0xAAAAAAAA & every, "first": 1, "last": 1 << (n - 1)}[kind]


def _torch_real(dtype):
    import torch
    return {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32, "fp64": torch.float64}[AB.kind_of(dtype)]


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
def _cells(extent, strides, device):
    import torch
    k = [torch.arange(int(e), dtype=torch.int64, device=device) * int(s) for e, s in zip(extent, strides)]
    return (k[0][:, None, None] + k[1][None, :, None] + k[2][None, None, :]).reshape(-1)


def _span(extent, strides):
    return sum((int(e) - 1) * int(s) for e, s in zip(extent, strides)) + 1


class _Arena:
    """One device buffer that holds every field of a case: integers of [lo, 8] in every real of `dtype`, exact in all seven types,
    sums of two included.  A case copies the pristine values in, runs its launch through cudecompExtRunMirroredFieldMoves and
    compares EVERY byte with what torch index arithmetic on the pristine values gives: dst = s * src or dst = dst + s * src with the
    source running backwards along the mirrored dim, s = -1 for the fields of the mask (times -1 is the flip of the sign bit, of
    zero too), then zero into the source cells."""

    def __init__(self, dtype, nbytes, lo=-8):
        import torch
        self.dtype, self.es, self.nc, self.rb = dtype, ES[dtype], NC[dtype], ES[dtype] // NC[dtype]
        g = torch.Generator(device="cuda")
        g.manual_seed(4321)
        nbytes += -nbytes % 16
        self.init = torch.randint(lo, 9, (nbytes // self.rb,), device="cuda", generator=g).to(_torch_real(dtype))
        self.buf = torch.empty_like(self.init)

    def run(self, extent, strides, mirrored, n_fields, mode, mask, sides, force, offsets):
        """`sides` moves of the geometry (extent, pencil strides) mirrored along dim `mirrored` for n_fields fields whose bases lie
        offsets[f] elements into their regions.  Returns (kernel name, description, source cells as element numbers of the arena)."""
        import torch
        es, nc, rb = self.es, self.nc, self.rb
        dev = self.buf.device
        span = _span(extent, strides)
        part = span + 3 + (span + 3) % 2  # (even: the 2-byte cases decide their alignment by the fields' offsets alone)
        # a field's region: [side 0 source | side 0 destination | side 1 source | side 1 destination], each `part` apart
        region = (max(offsets) + 4 * part) * es + SLACK
        region += -region % 16
        total = SLACK + n_fields * region
        assert total <= self.buf.numel() * rb, (total, self.buf.numel() * rb)
        buf, init = self.buf[:total // rb], self.init[:total // rb]
        self.last_elements = total // es
        buf.copy_(init)
        bases = [SLACK + f * region + offsets[f] * es for f in range(n_fields)]  # bytes from the start of the arena
        expected = init.clone()
        E, I = expected.view(-1, nc), init.view(-1, nc)
        base_el = torch.tensor([b // es for b in bases], dtype=torch.int64, device=dev)[:, None]
        sign = torch.tensor([-1.0 if (mask >> f) & 1 else 1.0 for f in range(n_fields)], device=dev).to(I.dtype)[:, None, None]
        backwards = [-s if d == mirrored else s for d, s in enumerate(strides)]
        first = (int(extent[mirrored]) - 1) * int(strides[mirrored])  # the source cell of index 0 along the mirrored dim
        kd = _cells(extent, strides, dev)[None, :]
        ks = _cells(extent, backwards, dev)[None, :] + first
        moves, sources = [], []
        for s in range(sides):
            src_off, dst_off = (2 * s) * part, (2 * s + 1) * part
            moves.append(cd.make_move(extent, backwards, strides, src_off=src_off + first, dst_off=dst_off, src_buf=0, dst_buf=0))
            src, dst = base_el + src_off + ks, base_el + dst_off + kd
            value = I[src] * sign
            E[dst.reshape(-1)] = (value if mode == REFLECT else I[dst] + value).reshape(-1, nc)
            if mode == FOLD_TAKE:
                E[src.reshape(-1)] = 0
            sources.append(src.reshape(-1))
        ptr = buf.data_ptr()
        assert ptr % 256 == 0
        fields = [ptr + b for b in bases]
        desc = cd.cudecompExtDescribeMirroredFieldMoves(moves, fields, es, mode, self.dtype, mask, force)
        n = cd.cudecompExtRunMirroredFieldMoves(moves, fields, es, mode, self.dtype, mask, force, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        name = cd.cudecompExtLastKernelName()
        what = (self.dtype, extent, strides, mirrored, n_fields, mode, hex(mask), sides, force, offsets, name)
        assert n == 1 and name == spell(desc, es, self.dtype), what + (desc,)
        assert desc["kind"] in KINDS[mode] and desc["blocks"] == n_fields * desc["blocks_per_field"], what + (desc,)
        got, want = buf.view(torch.uint8), expected.view(torch.uint8)
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).reshape(-1)
            raise AssertionError(what + ("%d bytes differ, first at byte %d of the arena (fields begin at %s)" % (bad.numel(), int(bad[0]), bases[:4]),))
        rows = name.startswith("rows_")
        if force & 1:
            assert not rows, what
        elif rows:
            assert desc["access"] == (1 if force & 2 else 0), what + (desc,)
        return name, desc, torch.cat(sources)


LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130, 1025)
COMBINATIONS = list(itertools.product((2, 3, 9, 32), MASKS, MODES, (0, 1, 2), (1, 2)))  # fields x mask x operation x force x sides


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows(dtype):
    """type x row length x row pitch (length + 0, 1, 3) x mirrored extent (1, 2, 3, 5) as the row index and as the plane index: the
    whole cross of geometries, each with three draws (a seeded shuffle, walked round) of field count {2, 3, 9, 32} x mask of signs
    (none, all, alternating, only field 0, only the last field -- field 31 of 32) x operation (reflect, fold, fold with take) x fast
    path / forced element-wise / forced streaming x one / two sides; all 360 combinations must have come up.  Base offsets 0 ..
    16 / es + 1 elements, another one for every field (field f: (f + k) mod (16 / es + 2))."""
    es = ES[dtype]
    arena = _Arena(dtype, SLACK + 32 * ((12 + 4 * (1028 * 5 * 4 + 40)) * es + 2 * SLACK))
    rng = np.random.RandomState(200 + dtype)
    order = rng.permutation(len(COMBINATIONS))
    phases = 16 // es + 2
    seen, lanes, kernels, draw = set(), set(), set(), 0
    for length, extra, thick, where in itertools.product(LENGTHS, (0, 1, 3), (1, 2, 3, 5), (1, 2)):
        pitch = length + extra
        other = 4 if where == 1 else 3  # (the extent of the slow dim that is not mirrored)
        rows, planes = (thick, other) if where == 1 else (other, thick)
        extent, strides = (length, rows, planes), (1, pitch, pitch * rows + 5)  # (planes never continue one another)
        for _ in range(3):
            n, mask_kind, mode, force, sides = COMBINATIONS[order[draw % len(order)]]
            draw += 1
            k = int(rng.randint(phases))
            offsets = [(f + k) % phases for f in range(n)]
            name, desc, _ = arena.run(extent, strides, where, n, mode, mask_of(mask_kind, n), sides, force, offsets)
            seen.add((n, mask_kind, mode, force, sides))
            kernels.add(name.split("<")[0])
            if length >= 2 and not force & 1:
                assert name.startswith("rows_fields_"), (extent, strides, name)
            if name.startswith("rows_"):
                lanes.add(desc["vec"])
                if es == 2:  # consecutive fields sit at consecutive phases: one of them is at 2 mod 4
                    assert desc["vec"] == 2, (extent, strides, offsets, desc)
                if es >= 4 and extra != 0:  # (no fusion of rows: the row length decides)
                    want = 16
                    while want > es and (length * es) % want:
                        want //= 2
                    assert desc["vec"] == want, (extent, strides, desc)
    assert len(seen) == len(COMBINATIONS) == 360, sorted(set(COMBINATIONS) - seen)
    assert lanes == ({2} if es == 2 else {v for v in (4, 8, 16) if v >= es}), lanes
    assert kernels == {"rows_fields_reflect_kernel", "rows_fields_fold_kernel", "generic_fields_reflect_kernel", "generic_fields_fold_kernel"}, kernels


@pytest.mark.parametrize("dtype", [cd.HALF, cd.BFLOAT16], ids=["fp16", "bf16"])
def test_kernel_parity_two_byte_lanes_follow_every_field(dtype):
    """2-byte elements: all bases dword-aligned and even strides -> 16-byte lanes; ONE field of nine at 2 mod 4 -> 2-byte lanes for
    the whole launch; both compared byte for byte"""
    arena = _Arena(dtype, 1 << 22)
    extent, strides = (64, 5, 3), (1, 66, 66 * 5 + 6)
    for mode, where in itertools.product(MODES, (1, 2)):
        name, desc, _ = arena.run(extent, strides, where, 9, mode, 0x155, 2, 0, [0, 2, 4, 6, 8, 0, 2, 4, 6])
        assert (name.startswith("rows_fields_"), desc["vec"]) == (True, 16), (mode, name)
        name, desc, _ = arena.run(extent, strides, where, 9, mode, 0x155, 2, 0, [0, 2, 4, 6, 8, 0, 3, 4, 6])
        assert (name.startswith("rows_fields_"), desc["vec"]) == (True, 2), (mode, name)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_mirrored_dim_fastest(dtype):
    """the mirrored dim as the fastest memory axis: rows of 1 to 5 elements, reversed in themselves, a row pitch apart -- the
    element-wise kernels by themselves, whatever is forced"""
    es = ES[dtype]
    arena = _Arena(dtype, SLACK + 32 * ((12 + 4 * 39200) * es + 2 * SLACK))
    phases = 16 // es + 2
    c = 0
    for thick, (rows, planes), pitch, mode, sides in itertools.product((1, 2, 3, 4, 5), ((9, 7), (37, 3), (1, 40), (300, 1)), (5, 16, 131), MODES, (1, 2)):
        n = (2, 3, 9, 32)[c % 4]
        force = (0, 1, 2)[(c // 4) % 3]
        mask_kind = MASKS[(c // 12) % 5]
        c += 1
        extent, strides = (thick, rows, planes), (1, pitch, pitch * (rows + 3))
        name, _, _ = arena.run(extent, strides, 0, n, mode, mask_of(mask_kind, n), sides, force, [(f + c) % phases for f in range(n)])
        if thick > 1 or rows == 1 or planes == 1 or force & 1:  # (one cell thick has no direction: long enough rows of cells may fuse)
            assert name.startswith("generic_fields_reflect_kernel<" if mode == REFLECT else "generic_fields_fold_kernel<"), (extent, strides, name)


def test_kernel_parity_second_grid_stride_pass():
    """the element-wise kernels launch at most 8192 workgroups of 256 lanes per field: more elements than that take a second pass"""
    cells = 8192 * 256 + 257
    arena = _Arena(cd.HALF, SLACK + 2 * ((8 + 4 * (2 * cells + 8)) * 2 + 2 * SLACK))
    for mode in MODES:
        name, desc, _ = arena.run((cells, 2, 1), (1, cells + 1, 0), 1, 2, mode, 2, 1, 1, [1, 4])
        assert name.startswith("generic_fields_") and desc["blocks_per_field"] == 8192, (name, desc)


@pytest.mark.parametrize("dtype", [cd.HALF, cd.FLOAT, cd.DOUBLE, cd.DOUBLE_COMPLEX], ids=["fp16", "fp32", "fp64", "complex128"])
def test_after_a_fold_with_take_exactly_the_source_cells_are_zero(dtype):
    """a payload without a zero (integers 1 .. 8, every sign kept: mask none, so no sum is zero either): afterwards the zero bytes of
    the arena are exactly the source cells of the moves -- their neighbours in the rows' gaps, between the planes and around the
    fields are not"""
    import torch
    arena = _Arena(dtype, 1 << 22, lo=1)
    for extent, strides, where, force in (((7, 5, 3), (1, 9, 9 * 5 + 5), 1, 0), ((33, 3, 4), (1, 36, 36 * 3 + 5), 2, 2), ((3, 9, 7), (1, 13, 13 * 12), 0, 0),
                                          ((9, 5, 3), (1, 12, 12 * 5 + 7), 1, 1)):
        name, _, sources = arena.run(extent, strides, where, 3, FOLD_TAKE, 0, 2, force, [0, 1, 2])
        used = arena.buf.view(-1, arena.nc)[:arena.last_elements]  # the fields and the slack around them
        zero = torch.zeros(used.shape[0], dtype=torch.bool, device="cuda")
        zero[sources] = True
        is_zero = (used.view(torch.uint8).reshape(used.shape[0], -1) == 0).all(dim=1)
        assert torch.equal(is_zero, zero), (extent, strides, name)
        assert int(zero.sum()) == 2 * 3 * int(np.prod(extent))


# ---- single-rank pencils ---------------------------------------------------------------------------------------------------
GDIMS = (11, 9, 7)
ORDERS = {"default": None, "contiguous": ((0, 1, 2), (1, 2, 0), (2, 0, 1)), "mixed": ((1, 0, 2), (2, 1, 0), (0, 2, 1))}
HALOS = [(1, 1, 1), (2, 0, 3), (3, 2, 1)]
PERIODS = [(1, 1, 1), (1, 0, 1), (0, 0, 0)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
OTHER_TYPES = [t for t in AB.ALL_TYPES if t not in (cd.DOUBLE, cd.HALF)]


def _sweep(args):
    out = WB.wall_sweep(0, 1, args)
    assert out["failures"] == [], out["failures"][:10]
    return out


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("halo", HALOS, ids=["h111", "h203", "h321"])
def test_single_rank_full_cross_fp64_fp16(layout, halo):
    """every axis, dim, period mix, padding, centering 0 and 1, reflection / fold / fold that clears, 2, 3 and 9 fields with mixed
    parities: whole buffers against single calls on clones, refusals against the single call's, launches by the counter"""
    for periods, padding in itertools.product(PERIODS, PADDINGS):
        out = _sweep({"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
                      "dtypes": [cd.DOUBLE, cd.HALF], "n_fields": [2, 3, 9]})
        if periods == (1, 1, 1):
            assert out["launching"] == 0 and out["accepted"] == out["drawn"]
        if periods == (0, 0, 0):
            assert out["launching"] == out["drawn"] * sum(1 for x in halo if x) // 3


@pytest.mark.parametrize("layout", list(ORDERS))
def test_single_rank_at_least_half_of_the_tuples_are_accepted(layout):
    """... so that the sweep cannot pass by refusing (counted over all three halo sets and period mixes of a layout), and at least a
    quarter of them have a wall to write"""
    total = {"drawn": 0, "accepted": 0, "launching": 0}
    for halo, periods in itertools.product(HALOS, PERIODS):
        out = _sweep({"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": (0, 0, 0),
                      "dtypes": [cd.DOUBLE], "n_fields": [3]})
        for k in total:
            total[k] += out[k]
    assert 2 * total["accepted"] >= total["drawn"] and 4 * total["launching"] >= total["drawn"], total


@pytest.mark.parametrize("layout,halo,periods,padding", [("default", (3, 2, 1), (0, 0, 0), (1, 2, 0)), ("contiguous", (1, 1, 1), (1, 0, 1), (0, 0, 0)),
                                                         ("mixed", (2, 0, 3), (0, 0, 0), (1, 2, 0))], ids=["default", "contiguous", "mixed"])
def test_single_rank_other_types(layout, halo, periods, padding):
    out = _sweep({"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
                  "dtypes": OTHER_TYPES, "n_fields": [2, 3, 9]})
    assert out["launching"] > 0


def test_single_rank_refusals_follow_the_single_call():
    """three interior cells under a halo of three: fine with centering 0, beyond the interior with centering 1 -- there the field call
    answers what the single call answers, launches nothing and leaves the fields alone"""
    out = _sweep({"gdims": (11, 9, 3), "pdims": (1, 1), "halo": (1, 1, 3), "periods": (0, 0, 0), "dtypes": [cd.DOUBLE], "n_fields": [2, 9], "dims": [2]})
    assert out["accepted"] * 2 == out["drawn"], out


def test_single_rank_ordered_fold():
    """global extent 3 along the dim, halo 2, no period, one rank: interior 3 >= h + c and n = 7 < 4h + 2c for both centerings -- the
    two sides add onto the same cells: two launches, low side first, and the bits of the single call (the payload's sums round, so
    the order shows)"""
    for layout, dim in itertools.product(ORDERS, range(3)):
        gdims, halo = [9, 8, 7], [1, 1, 1]
        gdims[dim], halo[dim] = 3, 2
        out = _sweep({"gdims": tuple(gdims), "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": tuple(halo), "periods": (0, 0, 0),
                      "padding": (0, 1, 0), "dtypes": [cd.DOUBLE, cd.HALF, cd.BFLOAT16], "n_fields": [2, 9], "dims": [dim]})
        assert out["accepted"] == out["drawn"] and out["ordered"] == 2 * out["drawn"] // 3, out  # (the two folds of every three operations)


def test_one_field_is_the_single_call():
    """n_fields == 1: the single call's kernel name and launch count (the sweep compares both), its bytes, its refusals"""
    out = _sweep({"gdims": GDIMS, "pdims": (1, 1), "halo": (2, 1, 3), "periods": (0, 1, 0), "padding": (0, 1, 0), "dtypes": [cd.DOUBLE, cd.HALF],
                  "n_fields": [1]})
    assert out["launching"] > 0
    for parity in (1, -1):
        out = _sweep({"gdims": GDIMS, "pdims": (1, 1), "halo": (2, 1, 1), "periods": (0, 0, 0), "dtypes": [cd.FLOAT_COMPLEX], "n_fields": [1],
                      "parities": [parity]})
        assert out["launching"] > 0


def test_parities_are_no_part_of_the_cached_plan():
    steps = WB.plan_cache(0, 1, {"gdims": (12, 10, 8), "pdims": (1, 1)})
    #        reflect 3 fields x 3 sign sets; fold clear 1 x 2 sign sets; clear 0; centering 1; 2 fields; 1 field +1; 1 field -1; single -1
    assert steps == [1, 0, 0, 1, 0, 1, 1, 1, 1, 1, 0], steps


@pytest.mark.parametrize("periods", [(0, 0, 0), (0, 1, 0), (1, 0, 1)], ids=["walls", "y_periodic", "y_wall"])
def test_update_then_reflection_fills_every_ghost_cell(periods):
    for axis, layout in ((0, "default"), (1, "contiguous"), (2, "mixed")):
        args = {"gdims": (9, 8, 7), "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": (2, 1, 2), "periods": periods, "axis": axis,
                "parities": [-1, 1, -1, 1]}
        assert WB.sequence(0, 1, args) == []


def test_adjoint_of_the_field_reflection():
    for periods, padding in (((0, 0, 0), (0, 0, 0)), ((0, 1, 0), (1, 0, 2))):
        args = {"gdims": (12, 10, 9), "pdims": (1, 1), "halo": (2, 1, 3), "periods": periods, "padding": padding, "parities": [-1, 1, -1]}
        for lhs, rhs, broken in WB.adjoint(0, 1, args):
            assert lhs == rhs and lhs != 0, (lhs, rhs)
            assert broken != rhs, "flipping one field's parity in the fold alone went unnoticed"


# ---- ranks sharing the GPU -------------------------------------------------------------------------------------------------
def test_four_ranks_ragged_grid_walls_on_every_dim():
    """2 x 2 ranks on 10 x 9 x 11, no period: three fields with parities (-1, +1, -1), both operations against single calls; a rank
    launches exactly where it has a wall side (along the split dims every rank has one, along the third two; the test below has a
    rank without one)"""
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo": (1, 2, 1), "periods": (0, 0, 0), "padding": (1, 0, 2), "dtypes": [cd.DOUBLE, cd.HALF],
            "n_fields": [3], "parities": [-1, 1, -1]}
    for out in run_ranks(4, "tests.wall_fields_bodies", "wall_sweep", args, timeout=300):
        assert out["failures"] == [] and out["accepted"] == out["drawn"] == out["launching"], out
    # ... and with a period along the dims that are split, so that only the third dim has walls
    args.update(periods=(0, 1, 1), axes=[0])
    for out in run_ranks(4, "tests.wall_fields_bodies", "wall_sweep", args, timeout=300):
        assert out["failures"] == [] and 3 * out["launching"] == out["drawn"], out


def test_three_ranks_along_a_walled_dim_the_middle_one_launches_nothing():
    """3 x 1 ranks on 10 x 9 x 11, no period: every pencil axis has one dim split in three, and along it the middle rank has a
    neighbour on both sides -- its field calls succeed, launch nothing and leave every field as it was, while the two edge ranks
    launch along every dim; all against single calls"""
    args = {"gdims": (10, 9, 11), "pdims": (3, 1), "halo": (1, 2, 1), "periods": (0, 0, 0), "padding": (1, 0, 2), "dtypes": [cd.DOUBLE, cd.HALF],
            "n_fields": [3], "parities": [-1, 1, -1]}
    outs = run_ranks(3, "tests.wall_fields_bodies", "wall_sweep", args, timeout=300)
    for out in outs:
        assert out["failures"] == [] and out["accepted"] == out["drawn"] == out["launching"] + out["idle"], out
    assert outs[0]["idle"] == outs[2]["idle"] == 0 and 3 * outs[1]["idle"] == outs[1]["drawn"] > 0, outs


# ---- hipGraph --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clear", [0, 1])
def test_captured_calls_replay_on_refilled_fields(clear):
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (0, 1, 0), "padding": (0, 1, 0), "parities": [-1, 1, -1]},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "axis": 1, "halo": (2, 1, 2), "periods": (0, 0, 0),
                  "dtype": cd.HALF, "centering": 1, "parities": [1, -1]}):
        assert run_ranks(1, "tests.wall_fields_bodies", "graph_replay", dict(args, clear=clear), timeout=300)[0] == []
