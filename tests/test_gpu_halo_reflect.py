"""Halo reflection (cudecomp_amd_reflect.h: cudecompAmdReflectHalos{X,Y,Z}) on the GPU: the reflect kernels move by move with
source and destination in ONE buffer (every byte of it, poison slack on both sides included); lists of mirror-moves through the
kernel layer's batching; single-rank pencils of every axis, memory order, halo width, padding, period mix, centering, parity and
data type against the two numpy restatements of tests/reflect_bodies.py; four ranks sharing the GPU on a ragged 2 x 2 grid;
update + reflection as complements; capture into a hipGraph; asynchrony.  Everything is compared byte for byte: there is no
tolerance anywhere.  Buffers start as a poison byte that occurs in no payload."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import move_lists as ML
from tests import reflect_bodies as RB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = RB.SLACK
K_ROWS_REFLECT, K_GENERIC_REFLECT = 16, 17
NEG = {False: "false", True: "true"}


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
def _reflect(buf, dtype, negate, extent, ss, ds, mirrored, soff, doff, force, seed=0):
    """one reflect-move through cudecompExtReflect3D inside the device buffer `buf`: the source block (strides `ss`, all positive
    here) begins `soff` elements past the slack and is read backwards along dim `mirrored`; the destination block begins at
    `doff`.  The buffer is poisoned, the source cells receive a payload; afterwards EVERY byte of the buffer -- slack, source
    cells, the cells between rows -- against numpy.  Returns (kernel class, kernel name)."""
    import torch
    es, rb = AB.element_bytes(dtype), AB.real_bytes(dtype)
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
    want = np.full(nbytes, RB.POISON, dtype=np.uint8)
    body = want[SLACK:nbytes - SLACK].reshape(-1, es)
    body[src] = RB.payload(dtype, src.size, seed)
    view = buf[:nbytes]
    view.copy_(torch.from_numpy(want))
    x = body[src].copy()
    if negate:
        RB.flip_signs(x, rb)
    body[dst] = x
    base = buf.data_ptr() + SLACK
    cls = cd.cudecompExtReflect3D(base + first * es, base + doff * es, dtype, negate, extent, signed, ds, force,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    got = view.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (AB.NAMES[dtype], negate, extent, ss, ds, mirrored, soff, doff, force, cls, name,
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
    the sign flip on every second case, with the real type of `dtype`.  The kernel and its name on every case."""
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
            negate = bool(n & 1)
            n += 1
            soff, doff = offset, offset + span + 3
            cls, name = _reflect(buf, dtype, negate, extent, ss, ds, mirrored, soff, doff, force, seed=n)
            if force & 1 or row == 1:  # (rows of one element a pitch apart have no contiguous dim: a degenerate shape)
                assert (cls, name) == (2, "generic_reflect_kernel<%d,%s>" % (es, NEG[negate])), (extent, ss, offset, force, name)
            else:
                vb = _lane_bytes(es, row, soff, doff, *strides)
                assert (cls, name) == (0, "rows_reflect_kernel<%d,%d,%s>" % (vb, 1 if force & 2 else 0, NEG[negate])), (
                    extent, ss, offset, force, name)


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
        negate = bool(n & 1)
        n += 1
        extent, ss = (h, rows, planes), (1, pitch, pitch * (rows + 2))
        cls, name = _reflect(buf, dtype, negate, extent, ss, ss, 0, offset + h, offset, force, seed=n)  # (ghost cells below their sources)
        if h > 1 or rows * planes > 1 or force & 1:  # (h == 1: single cells a pitch apart, the degenerate shape of the copies)
            assert (cls, name) == (2, "generic_reflect_kernel<%d,%s>" % (es, NEG[negate])), (extent, ss, offset, force, name)
        else:  # a single cell: a row of one element
            assert (cls, name) == (0, "rows_reflect_kernel<%d,%d,%s>" % (es, 1 if force & 2 else 0, NEG[negate])), (extent, offset, force, name)


def test_kernel_parity_streaming_by_size_and_second_grid_stride_pass():
    import torch
    buf = torch.empty(2 * SLACK + (64 << 20) + 4096, dtype=torch.uint8, device="cuda")
    # 32 MiB in one move, the mirrored dim the plane index: the size rule itself picks the non-temporal instantiation
    extent, ss = (2048, 1024, 2), (1, 2048, 2048 * 1024)
    assert _reflect(buf, cd.DOUBLE, True, extent, ss, ss, 2, 0, 2 * 2048 * 1024 + 8, 0) == (0, "rows_reflect_kernel<16,1,true>")
    assert _reflect(buf, cd.FLOAT, False, extent, ss, ss, 2, 1, 2 * 2048 * 1024 + 8, 0) == (0, "rows_reflect_kernel<16,0,false>")  # (16 MiB)
    assert _reflect(buf, cd.DOUBLE, False, (2047, 1024, 2), ss, ss, 1, 0, 2 * 2048 * 1024 + 8, 0) == (0, "rows_reflect_kernel<8,0,false>")
    # the element-wise kernel launches at most 8192 workgroups of 256 lanes: more elements than that take a second pass
    extent, ss = (3, 8192 * 128 + 77, 1), (1, 3, 0)
    assert _reflect(buf, cd.HALF, True, extent, ss, ss, 0, 5, 3 * (8192 * 128 + 80), 0) == (2, "generic_reflect_kernel<2,true>")


def test_kernel_names_as_the_design_document_spells_them():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    assert "`rows_reflect_kernel<VB,STREAM,NEG>`" in text and "`generic_reflect_kernel<ES,NEG>`" in text
    import torch
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    seen = set()
    for dtype, negate in itertools.product((cd.HALF, cd.DOUBLE_COMPLEX), (False, True)):
        seen.add(_reflect(buf, dtype, negate, (32, 5, 3), (1, 40, 300), (1, 40, 300), 1, 0, 2000, 0)[1])
        seen.add(_reflect(buf, dtype, negate, (3, 5, 3), (1, 40, 300), (1, 40, 300), 0, 0, 2000, 0)[1])
    assert all(re.fullmatch(r"rows_reflect_kernel<(2|4|8|16),[01],(true|false)>|generic_reflect_kernel<(2|4|8|16),(true|false)>", s) for s in seen)
    assert seen == {"rows_reflect_kernel<16,0,false>", "rows_reflect_kernel<16,0,true>", "generic_reflect_kernel<2,false>",
                    "generic_reflect_kernel<2,true>", "generic_reflect_kernel<16,false>", "generic_reflect_kernel<16,true>"}


# ---- lists -----------------------------------------------------------------------------------------------------------------
def _mirror_move(extent, ss, ds, mirrored, soff, doff):
    signed = list(ss)
    signed[mirrored] = -ss[mirrored]
    return cd.make_move(extent, signed, ds, soff + (extent[mirrored] - 1) * ss[mirrored], doff, 0, 0)


def _run_mirror_list(moves, dtype, negate, flags=0):
    """the list through cudecompExtRunMoves (mode 5 / 6) inside ONE device buffer; every byte of it against numpy applying the
    moves one by one; launches and elements per class against cudecompExtDescribeMoves.  Returns the described launches."""
    import torch
    es, rb = AB.element_bytes(dtype), AB.real_bytes(dtype)
    mode = cd.MOVES_REFLECT_NEGATE if negate else cd.MOVES_REFLECT
    src = [ML.cells(m.extent, m.ss, m.src_off) for m in moves]
    dst = [ML.cells(m.extent, m.ds, m.dst_off) for m in moves]
    everything = np.concatenate(src + dst)
    assert everything.min() >= 0 and np.unique(everything).size == everything.size, "the cells of the list overlap"
    cells = int(everything.max()) + 1
    want = np.full(2 * SLACK + cells * es, RB.POISON, dtype=np.uint8)
    body = want[SLACK:want.size - SLACK].reshape(-1, es)
    for i, c in enumerate(src):
        body[c] = RB.payload(dtype, c.size, 50 + i)
    dev = torch.from_numpy(want.copy()).cuda()
    for s, d in zip(src, dst):
        x = body[s].copy()
        if negate:
            RB.flip_signs(x, rb)
        body[d] = x
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


@pytest.mark.parametrize("negate", [False, True], ids=["copy", "sign_flip"])
def test_eight_siblings_share_one_interleaved_launch(negate):
    """eight moves of one kernel choice with 1 .. 300 workgroups each: one launch, served round robin, padded to 8 x 300"""
    targets = [1, 300, 2, 99, 5, 150, 17, 40]
    moves, at = [], 0
    for i, t in enumerate(targets):  # rows of 32 fp64: 16 lanes per row, 64 rows per workgroup
        planes = 3 if t % 3 == 0 else 1
        rows = 64 * (t // planes) - (5 if t > 1 and planes == 1 else 0)
        extent, mirrored = ((32, rows, planes), 2) if planes > 1 else ((32, rows, 1), 1)
        ss = (1, 34, 34 * rows + 2)
        span = ML.span(extent, ss)
        moves.append(_mirror_move(extent, ss, ss, mirrored, at, at + span + 6))
        at += 2 * span + 16
    (l,) = _run_mirror_list(moves, cd.DOUBLE, negate)
    assert (l["kind"], l["n"], l["interleave"], l["blocks"]) == (K_ROWS_REFLECT, 8, 1, 8 * 300), l
    assert [b - a for a, b in zip(l["first_block"], l["first_block"][1:])] == targets and l["index"] == list(range(8))


@pytest.mark.parametrize("dtype,negate", [(cd.HALF, False), (cd.BFLOAT16, True), (cd.FLOAT_COMPLEX, True)], ids=["fp16", "bf16_flip", "complex64_flip"])
def test_a_mixed_list_of_nine_moves(dtype, negate):
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
        moves.append(_mirror_move(extent, ss, ss, mirrored, at, at + span + 4))
        at = -(-(at + 2 * span + 8) // 8) * 8  # every move starts from a 16-byte boundary (2-byte elements) plus its phase
    described = _run_mirror_list(moves, dtype, negate)
    assert len(moves) == 9 and len(described) >= 3
    assert {l["kind"] for l in described} == {K_ROWS_REFLECT, K_GENERIC_REFLECT}
    assert sorted(i for l in described for i in l["index"]) == list(range(9))
    if es == 2:
        assert {l["vec"] for l in described if l["kind"] == K_ROWS_REFLECT} >= {2, 16}


# ---- single-rank pencils ---------------------------------------------------------------------------------------------------
SHAPES = {"13x10x11": (13, 10, 11), "5x6x7": (5, 6, 7)}
PERMS = list(itertools.permutations((0, 1, 2)))
HALOS = [(1, 1, 1), (2, 1, 3), (3, 3, 3)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
PERIODS = list(itertools.product((0, 1), repeat=3))
MIRRORS = list(itertools.product((1, -1), (0, 1)))  # (parity, centering)


@pytest.mark.parametrize("order", PERMS, ids=["".join(map(str, o)) for o in PERMS])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_rank_pencils(shape, order):
    """every axis, halo set, padding, period mix, centering and parity; the seven data types in turn (every type meets every
    mirror, period mix, halo and axis).  (update, reflection) over dims 0, 1, 2 on a pencil that is poison outside its interior:
    whole pencils against the definition applied dim by dim and against numpy.pad; the small shape also every dim alone."""
    cases = []
    for axis, halo, padding, periods, (parity, centering) in itertools.product(range(3), HALOS, PADDINGS, PERIODS, MIRRORS):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering])
    assert len(cases) == 576 and len({(c[4], c[5], c[6]) for c in cases}) == 28
    args = {"gdims": SHAPES[shape], "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases, "single_dims": shape == "5x6x7"}
    assert RB.sequence_sweep(0, 1, args) == []


def test_update_and_reflection_are_complements():
    """from a poisoned pencil, (update, reflection) over all dims: no ghost cell holds poison, no interior cell has changed
    (tests/reflect_bodies.py sequence_sweep reports both by name); and with the reflection left out of a non-periodic dim the
    poison stays, so the check can fail"""
    import torch
    from tests import gpu_bodies as B
    args = {"gdims": (13, 10, 11), "pdims": (1, 1),
            "cases": [[axis, (2, 1, 3), per, (1, 0, 2), cd.DOUBLE, -1, 1] for axis in range(3) for per in ((0, 0, 0), (1, 0, 1), (0, 1, 0))]}
    assert RB.sequence_sweep(0, 1, args) == []
    h, gd, g = B._setup(0, 1, args)
    halo, periods = (2, 1, 3), (1, 0, 1)
    p = g.pencil_info(0, 0, halo, (0, 0, 0))
    start = np.full((int(p.size), 8), RB.POISON, dtype=np.uint8)
    AB.pencil3(p, start)[RB.interior_index(p)] = RB.payload(cd.DOUBLE, 13 * 10 * 11, 1).reshape(11, 10, 13, 8)
    dev, ptr = RB._device_pencil(start)
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, 0, halo), 1) * 8)
    for dim in range(3):
        cd.cudecompUpdateHalos(0, h, gd, ptr, work, cd.DOUBLE, halo, periods, dim, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    after = dev.cpu().numpy()[SLACK:-SLACK].reshape(-1, 8)
    assert np.all(AB.pencil3(p, after)[AB.slab(p, 1, "L", 1)] == RB.POISON) and np.all(AB.pencil3(p, after)[AB.slab(p, 1, "H", 1)] == RB.POISON)
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)


# ---- four ranks sharing the GPU --------------------------------------------------------------------------------------------
def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (10, 9, 11): slabs of 5 + 5, 5 + 4 and 6 + 5 cells, every rank an edge rank.  Non-periodic and mixed
    periods; after (update, reflection) over dims 0, 1, 2 every rank's pencil, halos included, is its slice of numpy.pad of the
    global array axis by axis -- parity +1 as it is, parity -1 with the sign rule.  One halo backend: the reflection does not
    communicate."""
    cases = []
    for periods, axis, (halo, padding), (parity, centering) in itertools.product(((0, 0, 0), (1, 0, 1), (0, 1, 0)), range(3),
                                                                                 (((1, 2, 1), (0, 0, 0)), ((3, 1, 2), (1, 0, 2))), MIRRORS):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering])
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "cases": cases, "single_dims": True}
    for failures in run_ranks(4, "tests.reflect_bodies", "sequence_sweep", args, timeout=300, fresh=False):
        assert failures == []


# ---- hipGraph, asynchrony --------------------------------------------------------------------------------------------------
def test_captured_sequence_replays_on_fresh_data():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 0, 1), "padding": (0, 1, 0), "parity": -1,
                  "centering": 0},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ((1, 2, 0),) * 3, "axis": 1, "halo": (2, 1, 2),
                  "periods": (0, 0, 0), "dtype": cd.HALF_COMPLEX, "parity": 1, "centering": 1}):
        assert run_ranks(1, "tests.reflect_bodies", "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three reflection calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (0, 0, 0)}
    res = run_ranks(1, "tests.reflect_bodies", "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["reflect_host_ms"] < 0.25 * res["total_ms"], res
