"""Halo folding (cudecomp_halo_fold.h: cudecompAmdFoldHalos{X,Y,Z}) on the GPU: the fold kernels move by move with source and
destination in ONE buffer (every byte of it, poison slack on both sides included); lists of fold-moves through the kernel layer's
batching; single-rank pencils of every axis, memory order, halo width, padding, period mix, parity, centering, clear and data type
against the definition of tests/fold_bodies.py; the adjoint identity <S x, y> == <x, S^T y> on one rank and on four; clear = 1
against clear = 0 and a zeroing; the sums against add-moves taken one by one; four ranks sharing the GPU on a ragged 2 x 2 grid;
capture into a hipGraph; asynchrony; refusals.  Everything is compared byte for byte against numpy with the additions of
tests/accumulate_bodies.py: there is no tolerance anywhere.  Buffers start as a poison byte; payloads are finite, with zeros of
both signs and subnormals, without NaN: these tests are about WHERE cells go.  NaNs, infinities, overflow, ties and exact
cancellation through the fold kernels (every lane width, access, parity and TAKE) and through cudecompAmdFoldHalos* on whole pencils
are in tests/test_gpu_halo_edge_arithmetic.py."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fold_bodies as FB
from tests import move_lists as ML
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = FB.SLACK
MODES = {(False, False): cd.MOVES_FOLD, (True, False): cd.MOVES_FOLD_NEGATE, (False, True): cd.MOVES_FOLD_TAKE,
         (True, True): cd.MOVES_FOLD_NEGATE_TAKE}  # (negate, take) -> mode of cudecompExtRunMoves
KIND_OF = {(True, False): FB.K_ROWS_FOLD, (False, False): FB.K_GENERIC_FOLD, (True, True): FB.K_ROWS_FOLD_TAKE,
           (False, True): FB.K_GENERIC_FOLD_TAKE}  # (rows, take) -> kernel kind


def _expect_move(body, dtype, src, dst, negate, take):
    """one fold-move in numpy on `body` (uint8, (cells, element bytes)): cells dst += (flipped) cells src; then src = 0"""
    u, nc = FB.unsigned_of(dtype), AB.TYPES[dtype][1]
    bits = body.reshape(-1).view(u).reshape(-1, nc)
    bits[dst] = FB.fold_add(dtype, bits[dst], bits[src], negate)
    if take:
        bits[src] = 0


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
def _fold(buf, dtype, negate, take, extent, ss, ds, mirrored, soff, doff, force, seed=0):
    """one fold-move through cudecompExtFold3D inside the device buffer `buf`: the source block (strides `ss`, all positive here)
    begins `soff` elements past the slack and is read backwards along dim `mirrored`; the destination block begins at `doff`.  The
    buffer is poisoned, source and destination cells receive finite payloads; afterwards EVERY byte of the buffer -- slack, source
    cells, the cells between rows -- against numpy.  Returns (kernel class, kernel name)."""
    import torch
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    signed = list(ss)
    first = soff + (extent[mirrored] - 1) * ss[mirrored]  # the source cell of index 0 along the mirrored dim
    signed[mirrored] = -ss[mirrored]
    src, dst = ML.cells(extent, signed, first), ML.cells(extent, ds, doff)
    cells = max(int(src.max()), int(dst.max())) + 1
    nbytes = 2 * SLACK + cells * es
    assert nbytes <= buf.numel() and src.min() >= 0
    if src.size <= (1 << 20):
        both = np.concatenate([src, dst])
        assert np.unique(both).size == both.size, "source and destination cells overlap"
    want = np.full(nbytes, FB.POISON, dtype=np.uint8)
    body = want[SLACK:nbytes - SLACK].reshape(-1, es)
    payload = FB.finite_bits(dtype, 2 * src.size, seed).view(np.uint8).reshape(-1, es)
    body[src], body[dst] = payload[:src.size], payload[src.size:]
    view = buf[:nbytes]
    view.copy_(torch.from_numpy(want))
    _expect_move(body, dtype, src, dst, negate, take)
    base = buf.data_ptr() + SLACK
    cls = cd.cudecompExtFold3D(base + first * es, base + doff * es, dtype, negate, take, extent, signed, ds, force,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    got = view.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (AB.NAMES[dtype], negate, take, extent, ss, ds, mirrored, soff, doff, force, cls, name,
                           "%d bytes differ, first at byte %d of the buffer (source at %d, destination at %d)"
                           % (bad.size, bad[0], SLACK + soff * es, SLACK + doff * es))
    return cls, name


def _lane_bytes(es, length, *elements):
    """the VB rule of rows_kernel: the widest of 16, 8, 4, 2 bytes (not below the element) that divides the row; 2-byte elements
    whose bases or strides (`elements`, in elements) sit at 2 mod 4 take 2-byte lanes"""
    vb = 16
    while vb > es and (length * es) % vb:
        vb //= 2
    if es == 2 and any(e % 2 for e in elements):
        vb = 2
    return vb


LENGTHS = (1, 2, 3, 7, 8, 9, 15, 17, 33, 65, 130, 1025)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows(dtype):
    """row length x row pitch (length + 0, 1, 3) x extent along the mirrored dim (1, 2, 3, 5) as the row index and as the plane
    index x base offset (every phase of the 16-byte grid and one past it) x fast path, forced element-wise, forced streaming;
    parity and take alternate with the case number (all four combinations meet every force).  The kernel class and its name on
    every case."""
    import torch
    es = AB.element_bytes(dtype)
    buf = torch.empty(2 * SLACK + 2 * (1028 * 5 * 5 + 64) * es, dtype=torch.uint8, device="cuda")
    n = 0
    for length, extra, m, as_plane in itertools.product(LENGTHS, (0, 1, 3), (1, 2, 3, 5), (False, True)):
        pitch = length + extra
        # (row, strides): the row the lanes see and the strides they step by -- rows that continue one another (pitch == length,
        # three of them below each mirrored plane) are one row; a dim of extent 1 steps nowhere
        if as_plane:
            extent, mirrored = (length, 3, m), 2
            ss = ds = (1, pitch, pitch * 3 + 5)
            row, strides = (3 * length, []) if extra == 0 else (length, [pitch])
            strides += [ss[2]] if m > 1 else []
        else:
            extent, mirrored = (length, m, 3), 1
            ss = ds = (1, pitch, pitch * m + 5)
            row, strides = length, ([pitch] if m > 1 else []) + [ss[2]]
        span = ML.span(extent, ss)
        for offset, force in itertools.product(range(16 // es + 2), (0, 1, 2)):
            negate, take = bool(n & 1), bool(n & 2)  # (period 4 against the force's 3: every pair meets every force)
            n += 1
            soff, doff = offset, offset + span + 3
            cls, name = _fold(buf, dtype, negate, take, extent, ss, ds, mirrored, soff, doff, force, seed=n)
            if force & 1 or row == 1:  # (rows of one element a pitch apart have no contiguous dim: a degenerate shape)
                assert (cls, name) == (2, FB.generic_name(dtype, take)), (extent, ss, offset, force, name)
            else:
                vb = _lane_bytes(es, row, soff, doff, *strides)
                assert (cls, name) == (0, FB.rows_name(dtype, vb, 1 if force & 2 else 0, take)), (extent, ss, offset, force, name)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_mirrored_fastest_dim(dtype):
    """the mirrored dim as the fastest one: rows of 1..5 elements reversed in themselves, a row pitch apart -- the element-wise
    kernel by itself, whatever is forced; one and many rows and planes, every base phase"""
    import torch
    es = AB.element_bytes(dtype)
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    n = 0
    for h, (rows, planes), pitch, offset, force in itertools.product((1, 2, 3, 4, 5), ((1, 1), (9, 7), (300, 1), (1, 40)), (11, 16),
                                                                     range(16 // es + 2), (0, 1, 2)):
        negate, take = bool(n & 1), bool(n & 2)
        n += 1
        extent, ss = (h, rows, planes), (1, pitch, pitch * (rows + 2))
        cls, name = _fold(buf, dtype, negate, take, extent, ss, ss, 0, offset, offset + h, force, seed=n)  # (ghost cells below the interior)
        if h > 1 or rows * planes > 1 or force & 1:  # (h == 1: single cells a pitch apart, the degenerate shape of the copies)
            assert (cls, name) == (2, FB.generic_name(dtype, take)), (extent, ss, offset, force, name)
        else:  # a single cell: a row of one element
            assert (cls, name) == (0, FB.rows_name(dtype, es, 1 if force & 2 else 0, take)), (extent, offset, force, name)


def test_kernel_parity_streaming_by_size_and_second_grid_stride_pass():
    import torch
    buf = torch.empty(2 * SLACK + (64 << 20) + 4096, dtype=torch.uint8, device="cuda")
    # 32 MiB of fp64 in one move, the mirrored dim the plane index: the size rule itself picks the non-temporal instantiation
    extent, ss = (2048, 1024, 2), (1, 2048, 2048 * 1024)
    assert _fold(buf, cd.DOUBLE, True, True, extent, ss, ss, 2, 0, 2 * 2048 * 1024 + 8, 0) == (0, "rows_fold_kernel<double,16,1,true>")
    # ... and 16 MiB the cached one
    extent, ss = (2048, 512, 2), (1, 2048, 2048 * 512)
    assert _fold(buf, cd.DOUBLE, False, False, extent, ss, ss, 2, 0, 2 * 2048 * 512 + 8, 0) == (0, "rows_fold_kernel<double,16,0,false>")
    assert _fold(buf, cd.DOUBLE, True, False, (2047, 512, 2), ss, ss, 1, 0, 2 * 2048 * 512 + 8, 0) == (0, "rows_fold_kernel<double,8,0,false>")
    # the element-wise kernel launches at most 8192 workgroups of 256 lanes: more elements than that take a second pass
    extent, ss = (3, 8192 * 128 + 77, 1), (1, 3, 0)
    assert _fold(buf, cd.HALF, True, True, extent, ss, ss, 0, 5, 3 * (8192 * 128 + 80), 0) == (2, "generic_fold_kernel<_Float16,1,true>")


# ---- lists -----------------------------------------------------------------------------------------------------------------
def _fold_move(extent, ss, ds, mirrored, soff, doff):
    signed = list(ss)
    signed[mirrored] = -ss[mirrored]
    return cd.make_move(extent, signed, ds, soff + (extent[mirrored] - 1) * ss[mirrored], doff, 0, 0)


def _run_fold_list(moves, dtype, negate, take, flags=0):
    """the list through cudecompExtRunMoves (modes 7 ... 10) inside ONE device buffer; every byte of it against numpy applying the
    moves one by one; launches and elements per class against cudecompExtDescribeMoves.  Returns the described launches."""
    import torch
    es = AB.element_bytes(dtype)
    mode = MODES[(negate, take)]
    src = [ML.cells(m.extent, m.ss, m.src_off) for m in moves]
    dst = [ML.cells(m.extent, m.ds, m.dst_off) for m in moves]
    everything = np.concatenate(src + dst)
    assert everything.min() >= 0 and np.unique(everything).size == everything.size, "the cells of the list overlap"
    cells = int(everything.max()) + 1
    want = np.full(2 * SLACK + cells * es, FB.POISON, dtype=np.uint8)
    body = want[SLACK:want.size - SLACK].reshape(-1, es)
    for i, c in enumerate(src + dst):
        body[c] = FB.finite_bits(dtype, c.size, 50 + i).view(np.uint8).reshape(-1, es)
    dev = torch.from_numpy(want.copy()).cuda()
    for s, d in zip(src, dst):
        _expect_move(body, dtype, s, d, negate, take)
    ptrs = [dev.data_ptr() + SLACK, 0, 0]
    described = ML.describe(moves, ptrs, es, mode, dtype, flags)
    launches, elements, total = cd.cudecompExtRunMoves(moves, ptrs, es, mode, dtype, None, flags, None,
                                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = [(l["kind"], l["vec"], l["n"], l["interleave"], l["blocks"]) for l in described]
    assert total == len(described), what
    assert launches == [sum(1 for l in described if l["cls"] == c) for c in range(3)], what
    assert elements == [sum(l["elements"] for l in described if l["cls"] == c) for c in range(3)], what
    bad = np.nonzero(dev.cpu().numpy() != want)[0]
    assert bad.size == 0, ("%d bytes differ, first at byte %d" % (bad.size, bad[0] if bad.size else -1), what)
    return described


@pytest.mark.parametrize("negate,take", list(MODES), ids=["fold", "sign_flip", "take", "sign_flip_take"])
def test_eight_siblings_share_one_interleaved_launch(negate, take):
    """eight moves of one kernel choice with 1 .. 300 workgroups each: one launch, served round robin, padded to 8 x 300"""
    targets = [1, 300, 2, 99, 5, 150, 17, 40]
    moves, at = [], 0
    for i, t in enumerate(targets):  # rows of 32 fp64: 16 lanes per row, 64 rows per workgroup
        planes = 3 if t % 3 == 0 else 1
        rows = 64 * (t // planes) - (5 if t > 1 and planes == 1 else 0)
        extent, mirrored = ((32, rows, planes), 2) if planes > 1 else ((32, rows, 1), 1)
        ss = (1, 34, 34 * rows + 2)
        span = ML.span(extent, ss)
        moves.append(_fold_move(extent, ss, ss, mirrored, at, at + span + 6))
        at += 2 * span + 16
    (l,) = _run_fold_list(moves, cd.DOUBLE, negate, take)
    assert (l["kind"], l["n"], l["interleave"], l["blocks"]) == (KIND_OF[(True, take)], 8, 1, 8 * 300), l
    assert [b - a for a, b in zip(l["first_block"], l["first_block"][1:])] == targets and l["index"] == list(range(8))


@pytest.mark.parametrize("dtype,negate,take", [(cd.HALF, False, True), (cd.BFLOAT16, True, False), (cd.FLOAT_COMPLEX, True, True)],
                         ids=["fp16_take", "bf16_flip", "complex64_flip_take"])
def test_a_mixed_list_of_nine_moves(dtype, negate, take):
    """row moves at several lane widths (2-byte rows at 2 mod 4 among them), the mirrored dim as the row and as the plane index,
    mirrored fastest dims and a single cell: several launches, every byte against numpy applying the moves one by one"""
    es = AB.element_bytes(dtype)
    shapes = [((64, 5, 3), (1, 64, 330), 1, 0), ((64, 5, 3), (1, 64, 330), 2, 0), ((33, 4, 2), (1, 35, 150), 1, 1),
              ((3, 9, 7), (1, 13, 130), 0, 0), ((130, 2, 1), (1, 131, 0), 1, 2), ((1, 1, 1), (1, 1, 1), 0, 3),
              ((8, 37, 2), (1, 8, 300), 2, 0), ((2, 50, 1), (1, 5, 0), 0, 1), ((1025, 3, 2), (1, 1028, 3100), 1, 0)]
    moves, at = [], 0
    for extent, ss, mirrored, phase in shapes:
        span = ML.span(extent, ss)
        at += phase
        moves.append(_fold_move(extent, ss, ss, mirrored, at, at + span + 4))
        at = -(-(at + 2 * span + 8) // 8) * 8  # every move starts from a 16-byte boundary (2-byte elements) plus its phase
    described = _run_fold_list(moves, dtype, negate, take)
    assert len(moves) == 9 and len(described) >= 3
    assert {l["kind"] for l in described} == {KIND_OF[(True, take)], KIND_OF[(False, take)]}
    assert sorted(i for l in described for i in l["index"]) == list(range(9))
    if es == 2:
        assert {l["vec"] for l in described if l["kind"] == KIND_OF[(True, take)]} >= {2, 16}


# ---- the sums are addPayload's: a fold against add-moves taken one by one --------------------------------------------------
@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_one_side_with_parity_plus_one_is_a_list_of_add_moves(dtype):
    """a fold with parity +1 of one side (h = 3 planes of 37 x 5 cells mirrored as the plane index, then as the fastest dim) and
    the same cells added by an add-move list (mode 1), one move per mirrored index: the two device buffers are bit-identical"""
    import torch
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    stream = torch.cuda.current_stream().cuda_stream
    for extent, ss, mirrored in (((37, 5, 3), (1, 40, 240), 2), ((3, 37, 5), (1, 8, 320), 0)):
        h, span = extent[mirrored], ML.span(extent, ss)
        cells = 2 * span + 16
        start = FB.guarded(FB.finite_bits(dtype, cells, 9))
        folded, added = torch.from_numpy(start).cuda(), torch.from_numpy(start).cuda()
        soff, doff = 0, span + 5
        signed = list(ss)
        signed[mirrored] = -ss[mirrored]
        first = soff + (h - 1) * ss[mirrored]
        base = folded.data_ptr() + SLACK
        cd.cudecompExtFold3D(base + first * es, base + doff * es, dtype, False, False, extent, signed, ss, 0, stream)
        slices = []
        for j in range(h):  # destination index j takes source index h - 1 - j
            e = list(extent)
            e[mirrored] = 1
            slices.append(cd.make_move(e, ss, ss, soff + (h - 1 - j) * ss[mirrored], doff + j * ss[mirrored], 0, 0))
        cd.cudecompExtRunMoves(slices, [added.data_ptr() + SLACK, 0, 0], es, cd.MOVES_ADD, dtype, None, 0, None, stream)
        torch.cuda.synchronize()
        a, b = folded.cpu().numpy(), added.cpu().numpy()
        assert np.array_equal(a, b), (AB.NAMES[dtype], extent, FB.first_difference(a, b, es))
        assert not np.array_equal(a, start), "nothing was added"


# ---- single-rank pencils ---------------------------------------------------------------------------------------------------
# 5x4x6 is not among the shapes the halo sets below were first written for: with single-rank pencils of 13x10x11 and 7x6x8 no
# halo of theirs reaches the overlapping-sides range 3h + c <= n < 4h + 2c (n = interior + 2h, so it asks for an interior below
# 2h + 2c: at most 5 cells for h = 2, 7 for h = 3), which only 5x4x6 with halo (2, 1, 2), dim 0, centering 1 does (n = 9 < 10)
SHAPES = {"13x10x11": (13, 10, 11), "7x6x8": (7, 6, 8), "5x4x6": (5, 4, 6)}
HALOS = {"13x10x11": [(1, 1, 1), (2, 1, 3), (3, 3, 3)], "7x6x8": [(1, 1, 1), (2, 1, 2)], "5x4x6": [(1, 1, 1), (2, 1, 2)]}
PERMS = list(itertools.permutations((0, 1, 2)))
PADDINGS = [(0, 0, 0), (1, 2, 0)]
PERIODS = list(itertools.product((0, 1), repeat=3))
MIRRORS = list(itertools.product((1, -1), (0, 1), (0, 1)))  # (parity, centering, clear)


def _pencil_cases(shape):
    cases = []
    for axis, halo, padding, periods, (parity, centering, clear) in itertools.product(range(3), HALOS[shape], PADDINGS, PERIODS, MIRRORS):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering, clear])
    return cases


def _overlapping(shape, cases, order):
    """the (case, dim) pairs whose two sides share destination cells, by the contract's arithmetic -- and the planner agrees"""
    spec = cd.make_grid_spec(SHAPES[shape], (1, 1), (order,) * 3)
    out = 0
    for axis, halo, periods, padding, dtype, parity, centering, clear in cases:
        for dim in range(3):
            h, n = halo[dim], SHAPES[shape][dim] + 2 * halo[dim]
            assert h + centering <= n - 2 * h, "a case of the sweep would be refused"
            overlap = not periods[dim] and n < 4 * h + 2 * centering
            plan = cd.cudecompExtPlanHaloFold(spec, 0, axis, halo, periods, dim, padding, centering, parity < 0, clear)
            assert bool(plan.reserved & FB.ORDERED_MARK) == overlap, (shape, axis, halo, periods, dim, centering)
            out += overlap
    return out


@pytest.mark.parametrize("order", PERMS, ids=["".join(map(str, o)) for o in PERMS])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_rank_pencils(shape, order):
    """every axis, halo set, padding, period mix, parity, centering and clear; the seven data types in turn.  The fold over dims
    2, 1, 0 on a pencil of finite reals: whole pencils against the definition applied dim by dim; the two smaller shapes also
    every dim alone, and there clear = 1 against clear = 0 followed by a zeroing (13x10x11: test_clear_zeroes_... below).  Every case is accepted (a refusal is a failure of the
    sweep), and the overlapping-sides range occurs: in the smallest shape, 96 times per memory order."""
    cases = _pencil_cases(shape)
    assert len(cases) == 3 * len(HALOS[shape]) * 2 * 8 * 8 and len({tuple(c[4:]) for c in cases}) == 56
    overlapping = _overlapping(shape, cases, order)
    assert overlapping == (96 if shape == "5x4x6" else 0)
    args = {"gdims": SHAPES[shape], "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases, "single_dims": shape != "13x10x11"}
    assert FB.fold_sweep(0, 1, args) == []


def test_the_overlapping_sides_range_occurs():
    assert sum(_overlapping(s, _pencil_cases(s), (0, 1, 2)) for s in SHAPES) > 0


def test_clear_zeroes_exactly_the_ghost_cells_that_were_read():
    """clear = 1 equals clear = 0 followed by zero bytes into the ghost slabs of the sides without a neighbour, byte for byte (the
    sweep checks it dim by dim); here by name: after folds along all dims of a pencil with a non-periodic dim 1 (h = 1) and
    periodic dims 0 and 2, the ghost cells of dim 1 are zero, and every cell away from dim 1's two ghost planes and the two
    interior planes they are added to -- the ghost cells of the periodic dims among them -- holds what it held"""
    import torch
    from tests import gpu_bodies as B
    from tests import reflect_bodies as RB
    cases = [[axis, (2, 1, 3), per, (1, 0, 2), AB.ALL_TYPES[i % 7], -1, i % 2, 1]
             for i, (axis, per) in enumerate(itertools.product(range(3), ((0, 0, 0), (1, 0, 1), (0, 1, 0))))]
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "cases": cases, "single_dims": True}
    assert FB.fold_sweep(0, 1, args) == []
    h, gd, g = B._setup(0, 1, args)
    halo, periods = (2, 1, 3), (1, 0, 1)
    p = g.pencil_info(0, 0, halo, (0, 0, 0))
    start = FB.start_pencil(p, cd.DOUBLE, 3)
    dev = torch.from_numpy(FB.guarded(start)).cuda()
    for dim in range(3):
        cd.cudecompFoldHalos(0, h, gd, dev.data_ptr() + SLACK, cd.DOUBLE, 1, 0, 1, halo, periods, dim, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    after = dev.cpu().numpy()[SLACK:-SLACK].view(np.uint64).reshape(-1, 1)
    for which in ("L", "H"):
        assert not np.any(AB.pencil3(p, after)[AB.slab(p, 1, which, 1)])
    ax, n = RB._dim_axis(p, 1)
    away = RB._unpadded(p)
    away[ax] = slice(2, n - 2)
    untouched = np.zeros(int(p.size), dtype=bool)
    AB.pencil3(p, untouched)[tuple(away)] = True
    assert (untouched & ~FB.interior_mask(p)).any() and np.array_equal(after[untouched], start[untouched])
    assert not np.array_equal(after, start)
    cd.cudecompGridDescDestroy(h, gd)


# ---- the adjoint identity --------------------------------------------------------------------------------------------------
def _adjoint_cases(halos, paddings):
    cases = []
    for periods, axis, (halo, padding), (parity, centering) in itertools.product(((0, 0, 0), (1, 0, 1), (0, 1, 0), (1, 1, 1)), range(3),
                                                                                 zip(halos, paddings), itertools.product((1, -1), (0, 1))):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering])
    return cases


def _check_adjoint(per_rank, cases):
    told_apart = 0
    for i, case in enumerate(cases):
        apart = False
        for k in range(2):  # two independent draws of x
            lhs, rhs = sum(r[i][k][0] for r in per_rank), sum(r[i][k][1] for r in per_rank)
            assert lhs == rhs, ("<S x, y> != <x, S^T y>", case, k, lhs, rhs)
            if per_rank[0][i][k][2] is not None:
                apart = apart or sum(r[i][k][2] for r in per_rank) != lhs
            else:
                assert all(case[2]), case
        told_apart += apart
    walls = sum(1 for c in cases if not all(c[2]))
    # with the fold left out of a non-periodic dim the identity does not hold: in every wall case, for one draw of x at least
    assert walls > 0 and told_apart == walls, (told_apart, walls)


def test_adjoint_identity_single_rank():
    """<S x, y> == <x, S^T y> with S = (update, reflection) over dims 0, 1, 2 and S^T = (accumulation, fold) over dims 2, 1, 0,
    in int64 on the host from small integers (exact in every type); and not with the fold left out of one non-periodic dim"""
    cases = _adjoint_cases([(1, 1, 1), (2, 1, 3)], [(0, 0, 0), (1, 0, 2)])
    args = {"gdims": (13, 10, 11), "pdims": (1, 1), "cases": cases}
    _check_adjoint([FB.adjoint(0, 1, args)], cases)


def test_adjoint_identity_four_ranks():
    cases = _adjoint_cases([(1, 2, 1), (2, 1, 2)], [(0, 0, 0), (1, 0, 2)])
    args = {"gdims": (15, 14, 17), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "cases": cases}
    _check_adjoint(run_ranks(4, "tests.fold_bodies", "adjoint", args, timeout=300, fresh=False), cases)


# ---- four ranks sharing the GPU --------------------------------------------------------------------------------------------
def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (15, 14, 17): slabs of 8 + 7, 7 + 7 and 9 + 8 cells, every rank an edge rank.  Non-periodic and mixed
    periods, halos (1, 2, 1) and (2, 1, 2): the fold of every rank -- each side only where the oracle's shifted rank names no
    neighbour -- is the definition on its pencil.  The fold does not communicate."""
    cases = []
    for periods, axis, (halo, padding), (parity, centering, clear) in itertools.product(((0, 0, 0), (1, 0, 1), (0, 1, 0)), range(3),
                                                                                        (((1, 2, 1), (0, 0, 0)), ((2, 1, 2), (1, 0, 2))), MIRRORS):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering, clear])
    args = {"gdims": (15, 14, 17), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "cases": cases, "single_dims": True}
    for failures in run_ranks(4, "tests.fold_bodies", "fold_sweep", args, timeout=300, fresh=False):
        assert failures == []


# ---- hipGraph, asynchrony --------------------------------------------------------------------------------------------------
def test_captured_sequence_replays_on_fresh_data():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 0, 1), "padding": (0, 1, 0), "parity": -1,
                  "centering": 0},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ((1, 2, 0),) * 3, "axis": 1, "halo": (2, 1, 2),
                  "periods": (0, 0, 0), "dtype": cd.HALF_COMPLEX, "parity": 1, "centering": 1}):
        assert run_ranks(1, "tests.fold_bodies", "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three fold calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (0, 0, 0)}
    res = run_ranks(1, "tests.fold_bodies", "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["fold_host_ms"] < 0.25 * res["total_ms"], res


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    FB.check_entry_points()
    L = cd.lib()
    import ctypes as C
    import torch
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    halo = (1, 2, 1)
    for axis, name in enumerate(cd.AMD_FOLD_SYMBOLS):  # with cells to fold and a device: success on a real buffer
        data = torch.zeros(int(cd.cudecompGetPencilInfo(h, gd, axis, halo).size), dtype=torch.float32, device="cuda")
        for dim, (parity, centering, clear) in itertools.product(range(3), ((1, 0, 0), (-1, 1, 1))):
            assert getattr(L, name)(h, gd, data.data_ptr(), cd.FLOAT, parity, centering, clear, i3(*halo), b3(False, False, False), dim,
                                    None, None) == cd.RESULT_SUCCESS
            assert getattr(L, name)(h, gd, data.data_ptr(), cd.FLOAT, parity, centering, 2, i3(*halo), b3(False, False, False), dim,
                                    None, None) == cd.RESULT_INVALID_USAGE
        torch.cuda.synchronize()
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)
