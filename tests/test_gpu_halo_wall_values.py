"""Wall values (cudecomp_halo_wall_values.h: cudecompAmdSetWallHalos{X,Y,Z}) on the GPU: the wall kernels move by move with source
and destination in ONE buffer (every byte of it, poison slack on both sides included); lists of wall-moves through the kernel
layer's batching; IEEE edge values; single-rank pencils of every axis, memory order, halo width, padding, period mix, centering,
parity, `sides` and data type against the definition applied dim by dim (tests/wall_values_bodies.py); a linear field extended
exactly; four ranks sharing the GPU on a ragged 2 x 2 grid; capture into a hipGraph; asynchrony.  Everything is compared byte for
byte against numpy built from AB.typed_add and RB.flip_signs; only where the expected real is a NaN is "a NaN of that type" enough
(AB.mismatches).  Buffers start as a poison byte."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import move_lists as ML
from tests import reflect_bodies as RB
from tests import wall_values_bodies as WB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = RB.SLACK
K_ROWS_WALL, K_GENERIC_WALL = 37, 38
NEG = {False: "false", True: "true"}
ARITH = {cd.HALF: "_Float16", cd.HALF_COMPLEX: "_Float16", cd.BFLOAT16: "__bf16", cd.FLOAT: "float", cd.FLOAT_COMPLEX: "float",
         cd.DOUBLE: "double", cd.DOUBLE_COMPLEX: "double"}


def _typed(dtype, cells, seed):
    """finite reals of `dtype` for `cells` cells: uint8 (cells, es)"""
    nc = AB.TYPES[dtype][1]
    return np.ascontiguousarray(AB.bits_of(dtype, AB.typed_cells(dtype, seed, 0, 0, cells, nc))).view(np.uint8).reshape(cells, -1)


def _layer_index(extent, mirrored):
    """the index along dim `mirrored` of every cell of a move, in the order of ML.cells (dim 0 fastest)"""
    return np.indices([int(e) for e in extent][::-1]).reshape(3, -1)[::-1][mirrored]


def _addends(dtype, layers, salt):
    """`layers` distinct elements of `dtype` (exact small multiples of 1/4): (bytes of all of them, list of element bytes)"""
    nc = AB.TYPES[dtype][1]
    elems = WB.elements_of(dtype, WB.layer_values(salt % 3, salt & 1, layers, nc, salt), nc)
    return b"".join(elems), elems


def _expect_move(dtype, body, src, dst, extent, mirrored, side, negate, elems):
    """numpy: body[dst] = +-body[src] + addend of the destination's ghost layer (side 0: layer extent - 1 - j, side 1: layer j)"""
    j = _layer_index(extent, mirrored)
    layer = (int(extent[mirrored]) - 1 - j) if side == 0 else j
    x = body[src].copy()
    out = np.empty_like(x)
    for k in range(int(extent[mirrored])):
        sel = layer == k
        out[sel] = WB.wall_cells(dtype, x[sel], -1 if negate else 1, elems[k])
    body[dst] = out


def _wall(buf, dtype, negate, side, extent, ss, ds, mirrored, soff, doff, force, seed=0):
    """one wall-move through cudecompExtWall3D inside the device buffer `buf`: the source block (strides `ss`, all positive here)
    begins `soff` elements past the slack and is read backwards along dim `mirrored`; the destination block begins at `doff`.  The
    buffer is poisoned, the source cells receive finite reals; afterwards EVERY byte of the buffer -- slack, source cells, the cells
    between rows -- against numpy.  Returns (kernel class, kernel name)."""
    import torch
    es = AB.element_bytes(dtype)
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
    body[src] = _typed(dtype, src.size, seed)
    view = buf[:nbytes]
    view.copy_(torch.from_numpy(want))
    raw, elems = _addends(dtype, extent[mirrored], seed)
    _expect_move(dtype, body, src, dst, extent, mirrored, side, negate, elems)
    base = buf.data_ptr() + SLACK
    cls = cd.cudecompExtWall3D(base + first * es, base + doff * es, dtype, negate, side, raw, extent, signed, ds, force,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    got = view.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (AB.NAMES[dtype], negate, side, extent, ss, ds, mirrored, soff, doff, force, cls, name,
                           "%d bytes differ, first at byte %d of the buffer (source at %d, destination at %d)"
                           % (bad.size, bad[0], SLACK + soff * es, SLACK + doff * es))
    return cls, name


def _lane_bytes(es, length, *elements):
    """the reflection's lane-width rule: the widest of 16, 8, 4, 2 bytes (not below the element) that divides the row; 2-byte
    elements whose bases or strides (`elements`, in elements) sit at 2 mod 4 take 2-byte lanes"""
    vb = 16
    while vb > es and (length * es) % vb:
        vb //= 2
    if es == 2 and any(e % 2 for e in elements):
        vb = 2
    return vb


def _rows_name(dtype, vb, stream, negate):
    return "rows_wall_kernel<%s,%d,%d,%s>" % (ARITH[dtype], vb, stream, NEG[negate])


def _generic_name(dtype, negate):
    return "generic_wall_kernel<%s,%d,%s>" % (ARITH[dtype], AB.element_bytes(dtype), NEG[negate])


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows(dtype):
    """row length x row pitch (length + 0, + 3) x extent along the mirrored dim (1, 2, 3, 8) as the row index and as the plane
    index x base offset (every phase of the 16-byte grid and one past it) x fast path, forced element-wise, forced streaming; the
    sign flip on every second case, the side changing every two; addends distinct per layer.  The kernel and its name on every
    case."""
    import torch
    es = AB.element_bytes(dtype)
    buf = torch.empty(2 * SLACK + 2 * (134 * 8 * 4 + 64) * es, dtype=torch.uint8, device="cuda")
    n = 0
    for length, extra, m, as_plane in itertools.product(LENGTHS, (0, 3), (1, 2, 3, 8), (False, True)):
        pitch = length + extra
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
            negate, side = bool(n & 1), (n >> 1) & 1
            n += 1
            soff, doff = offset, offset + span + 3
            cls, name = _wall(buf, dtype, negate, side, extent, ss, ds, mirrored, soff, doff, force, seed=n)
            if force & 1 or row == 1:  # (rows of one element a pitch apart have no contiguous dim: a degenerate shape)
                assert (cls, name) == (2, _generic_name(dtype, negate)), (extent, ss, offset, force, name)
            else:
                vb = _lane_bytes(es, row, soff, doff, *strides)
                assert (cls, name) == (0, _rows_name(dtype, vb, 1 if force & 2 else 0, negate)), (extent, ss, offset, force, name)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_mirrored_fastest_dim(dtype):
    """the mirrored dim as the fastest one: rows of 1..8 elements reversed in themselves, a row pitch apart -- the element-wise
    kernel by itself, whatever is forced; one and many rows and planes, every base phase"""
    import torch
    es = AB.element_bytes(dtype)
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    n = 0
    for h, (rows, planes), pitch, offset, force in itertools.product(range(1, 9), ((1, 1), (9, 7), (300, 1), (1, 40)), (17,),
                                                                     range(16 // es + 2), (0, 1, 2)):
        negate, side = bool(n & 1), (n >> 1) & 1
        n += 1
        extent, ss = (h, rows, planes), (1, pitch, pitch * (rows + 2))
        cls, name = _wall(buf, dtype, negate, side, extent, ss, ss, 0, offset + h, offset, force, seed=n)  # (ghost cells below their sources)
        if h > 1 or rows * planes > 1 or force & 1:  # (h == 1: single cells a pitch apart, the degenerate shape of the copies)
            assert (cls, name) == (2, _generic_name(dtype, negate)), (extent, ss, offset, force, name)
        else:  # a single cell: a row of one element
            assert (cls, name) == (0, _rows_name(dtype, es, 1 if force & 2 else 0, negate)), (extent, offset, force, name)


def test_kernel_parity_streaming_by_size_and_second_grid_stride_pass():
    import torch
    buf = torch.empty(2 * SLACK + (64 << 20) + 4096, dtype=torch.uint8, device="cuda")
    # 32 MiB in one move, the mirrored dim the plane index: the size rule itself picks the non-temporal instantiation
    extent, ss = (2048, 1024, 2), (1, 2048, 2048 * 1024)
    assert _wall(buf, cd.DOUBLE, True, 0, extent, ss, ss, 2, 0, 2 * 2048 * 1024 + 8, 0) == (0, "rows_wall_kernel<double,16,1,true>")
    assert _wall(buf, cd.FLOAT, False, 1, extent, ss, ss, 2, 1, 2 * 2048 * 1024 + 8, 0) == (0, "rows_wall_kernel<float,16,0,false>")  # (16 MiB)
    # the element-wise kernel launches at most 8192 workgroups of 256 lanes: more elements than that take a second pass
    extent, ss = (3, 8192 * 128 + 77, 1), (1, 3, 0)
    assert _wall(buf, cd.HALF, True, 0, extent, ss, ss, 0, 5, 3 * (8192 * 128 + 80), 0) == (2, "generic_wall_kernel<_Float16,2,true>")


# ---- lists -----------------------------------------------------------------------------------------------------------------
def _wall_move(extent, ss, ds, mirrored, soff, doff, side):
    signed = list(ss)
    signed[mirrored] = -ss[mirrored]
    m = cd.make_move(extent, signed, ds, soff + (extent[mirrored] - 1) * ss[mirrored], doff, 0, 0)
    m.peer = side
    return m


def _run_wall_list(moves, mirrored_dims, dtype, negate, flags=0):
    """the list through cudecompExtRunMoves (mode 11 / 12) inside ONE device buffer; every byte of it against numpy applying the
    moves one by one; launches and elements per class against cudecompExtDescribeMoves.  Returns the described launches."""
    import torch
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    mode = cd.MOVES_WALL_NEGATE if negate else cd.MOVES_WALL
    src = [ML.cells(m.extent, m.ss, m.src_off) for m in moves]
    dst = [ML.cells(m.extent, m.ds, m.dst_off) for m in moves]
    everything = np.concatenate(src + dst)
    assert everything.min() >= 0 and np.unique(everything).size == everything.size, "the cells of the list overlap"
    cells = int(everything.max()) + 1
    want = np.full(2 * SLACK + cells * es, RB.POISON, dtype=np.uint8)
    body = want[SLACK:want.size - SLACK].reshape(-1, es)
    for i, c in enumerate(src):
        body[c] = _typed(dtype, c.size, 50 + i)
    dev = torch.from_numpy(want.copy()).cuda()
    sides = [WB.elements_of(dtype, WB.layer_values(1, side, cd.MAX_WALL_HALO, nc), nc) for side in (0, 1)]
    for m, s, d, mirrored in zip(moves, src, dst, mirrored_dims):
        _expect_move(dtype, body, s, d, tuple(m.extent), mirrored, m.peer, negate, sides[m.peer])
    ptrs = [dev.data_ptr() + SLACK, 0, 0]
    described = ML.describe(moves, ptrs, es, mode, dtype, flags)
    launches, elements, total = cd.cudecompExtRunMoves(moves, ptrs, es, mode, dtype, b"".join(sides[0] + sides[1]), flags, None,
                                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    what = [(l["kind"], l["vec"], l["n"], l["interleave"], l["blocks"]) for l in described]
    assert total == len(described), what
    assert launches == [sum(1 for l in described if l["cls"] == c) for c in range(3)], what
    assert elements == [sum(l["elements"] for l in described if l["cls"] == c) for c in range(3)], what
    bad = np.nonzero(dev.cpu().numpy() != want)[0]
    assert bad.size == 0, ("%d bytes differ, first at byte %d" % (bad.size, bad[0] if bad.size else -1), what)
    return described


@pytest.mark.parametrize("negate", [False, True], ids=["plain", "sign_flip"])
def test_eight_siblings_share_one_interleaved_launch(negate):
    """eight moves of one kernel choice with 1 .. 300 workgroups each, sides alternating, layers as rows and as planes: one launch,
    served round robin, padded to 8 x 300 -- every move finds ITS row of the addend table"""
    targets = [1, 300, 2, 99, 5, 150, 17, 40]
    moves, mirrored_dims, at = [], [], 0
    for i, t in enumerate(targets):  # rows of 32 fp64: 16 lanes per row, 64 rows per workgroup
        if t % 3 == 0:  # three layers as planes of 64 * (t / 3) rows
            extent, mirrored = (32, 64 * (t // 3), 3), 2
        else:  # 8 or 2 layers as the rows of t planes: one workgroup per plane
            extent, mirrored = (32, 8 if t % 8 == 0 else 2, t), 1
        ss = (1, 34, 34 * extent[1] + 2)
        span = ML.span(extent, ss)
        moves.append(_wall_move(extent, ss, ss, mirrored, at, at + span + 6, i & 1))
        mirrored_dims.append(mirrored)
        at += 2 * span + 16
    (l,) = _run_wall_list(moves, mirrored_dims, cd.DOUBLE, negate)
    assert (l["kind"], l["n"], l["interleave"]) == (K_ROWS_WALL, 8, 1), l
    assert l["blocks"] == 8 * 300 and l["index"] == list(range(8)), l
    assert [b - a for a, b in zip(l["first_block"], l["first_block"][1:])] == targets, l


@pytest.mark.parametrize("dtype,negate", [(cd.HALF, False), (cd.BFLOAT16, True), (cd.FLOAT_COMPLEX, True)], ids=["fp16", "bf16_flip", "complex64_flip"])
def test_a_mixed_list_of_nine_moves(dtype, negate):
    """row moves at several lane widths (2-byte rows at 2 mod 4 among them), the mirrored dim as the row and as the plane index,
    mirrored fastest dims and a single cell: several launches, every byte against numpy applying the moves one by one"""
    es = AB.element_bytes(dtype)
    shapes = [((64, 5, 3), (1, 64, 330), 1, 0), ((64, 5, 3), (1, 64, 330), 2, 0), ((33, 4, 2), (1, 35, 150), 1, 1),
              ((3, 9, 7), (1, 13, 130), 0, 0), ((130, 2, 1), (1, 131, 0), 1, 2), ((1, 1, 1), (1, 1, 1), 0, 3),
              ((8, 37, 2), (1, 8, 300), 2, 0), ((2, 50, 1), (1, 5, 0), 0, 1), ((1025, 3, 2), (1, 1028, 3100), 1, 0)]
    moves, at = [], 0
    for i, (extent, ss, mirrored, phase) in enumerate(shapes):
        span = ML.span(extent, ss)
        at += phase
        moves.append(_wall_move(extent, ss, ss, mirrored, at, at + span + 4, (i // 2) & 1))
        at = -(-(at + 2 * span + 8) // 8) * 8  # every move starts from a 16-byte boundary (2-byte elements) plus its phase
    described = _run_wall_list(moves, [s[2] for s in shapes], dtype, negate)
    assert len(moves) == 9 and len(described) >= 3
    assert {l["kind"] for l in described} == {K_ROWS_WALL, K_GENERIC_WALL}
    assert sorted(i for l in described for i in l["index"]) == list(range(9))
    if es == 2:
        assert {l["vec"] for l in described if l["kind"] == K_ROWS_WALL} >= {2, 16}


# ---- edge values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [cd.HALF, cd.BFLOAT16, cd.FLOAT, cd.DOUBLE], ids=["fp16", "bf16", "fp32", "fp64"])
def test_edge_values(dtype):
    """every pair (mirror, addend) of AB.edge_table -- zeros, subnormals, the largest finite numbers, infinities, NaNs -- in both
    parities through both kernels: 24 mirrors along a row, one addend per launch.  Where the expected real is a NaN any NaN of the
    type will do; every other real bit for bit."""
    import torch
    kind = AB.kind_of(dtype)
    u, es = AB.FORMATS[kind][0], AB.element_bytes(dtype)
    table = AB.edge_table(kind)
    n = len(table)
    stream = torch.cuda.current_stream().cuda_stream
    src = torch.from_numpy(np.ascontiguousarray(table).view(np.uint8).copy()).cuda()
    dst = torch.empty(n * es, dtype=torch.uint8, device="cuda")
    for negate, force in itertools.product((False, True), (0, 1)):
        for addend in table:
            dst.fill_(RB.POISON)
            cls = cd.cudecompExtWall3D(src.data_ptr(), dst.data_ptr(), dtype, negate, 1, np.array([addend], dtype=u), (n, 1, 1), (1, -n, 0),
                                       (1, n, 0), force, stream)
            torch.cuda.synchronize()
            assert cls == (2 if force else 0)
            got = dst.cpu().numpy().view(u)
            mirror = table ^ u(1 << (8 * es - 1)) if negate else table
            want = AB.bits_of(dtype, AB.typed_add(dtype, mirror.astype(u), np.full(n, addend, dtype=u)))
            bad = AB.mismatches(kind, got, want)
            assert not bad.any(), (AB.NAMES[dtype], negate, force, hex(int(addend)), [hex(int(x)) for x in table[bad]],
                                   [hex(int(x)) for x in got[bad]], [hex(int(x)) for x in want[bad]])


# ---- single-rank pencils ---------------------------------------------------------------------------------------------------
SHAPES = {"13x10x11": (13, 10, 11), "5x6x7": (5, 6, 7)}
PERMS = list(itertools.permutations((0, 1, 2)))
HALOS = [(1, 1, 1), (2, 1, 3), (3, 3, 3)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
PERIODS = list(itertools.product((0, 1), repeat=3))
MIRRORS = list(itertools.product((1, -1), (0, 1)))  # (parity, centering)


def _admitted(gdims, halo, periods, centering):
    """the refusal rule: h + centering <= interior along every non-periodic dim that has a halo"""
    return all(periods[d] or halo[d] == 0 or halo[d] + centering <= gdims[d] for d in range(3))


@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("order", PERMS, ids=["".join(map(str, o)) for o in PERMS])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_rank_pencils(shape, order, axis):
    """every halo set, padding, period mix, centering, parity and `sides`; the seven data types in turn.  (update, wall values) over
    dims 0, 1, 2 on a pencil that is poison outside its interior: whole pencils against the definition applied dim by dim."""
    cases = []
    for halo, padding, periods, (parity, centering), sides in itertools.product(HALOS, PADDINGS, PERIODS, MIRRORS, (1, 2, 3)):
        if _admitted(SHAPES[shape], halo, periods, centering):
            cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering, sides])
    assert len(cases) == 576 and len({(c[4], c[5], c[6], c[7]) for c in cases}) == 84
    args = {"gdims": SHAPES[shape], "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases}
    assert WB.wall_sweep(0, 1, args) == []


def test_the_widest_halo():
    """h = 8 along the 13-cell dim, as the fastest, the middle and the slowest memory axis; every type"""
    cases = [[axis, (8, 1, 1), (0, 1, 0), (1, 0, 0), dtype, parity, 0, 3] for axis in range(3)
             for dtype, parity in zip(AB.ALL_TYPES, itertools.cycle((-1, 1)))]
    for order in ((0, 1, 2), (1, 0, 2), (2, 1, 0)):
        assert WB.wall_sweep(0, 1, {"gdims": (13, 10, 11), "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases}) == []


# ---- a linear field, and sides -----------------------------------------------------------------------------------------------
def _line_pencil(h, gd, g, dtype, axis, halo, n_dim, dim):
    """a pencil of u = 3 + 2 i along `dim` (i the interior index), poison outside the interior"""
    p = g.pencil_info(0, axis, halo, (0, 0, 0))
    real = AB.TYPES[dtype][0]
    ax, n = RB._dim_axis(p, dim)
    shape = [1, 1, 1]
    shape[ax] = n
    line = (3.0 + 2.0 * (np.arange(n) - halo[dim])).astype(real).reshape(shape)
    full = np.ascontiguousarray(np.broadcast_to(line, AB.pencil3(p, np.zeros(int(p.size), dtype=real)).shape))
    start = np.full((int(p.size), np.dtype(real).itemsize), RB.POISON, dtype=np.uint8)
    AB.pencil3(p, start)[RB.interior_index(p)] = AB.pencil3(p, full.reshape(-1).view(np.uint8).reshape(int(p.size), -1))[RB.interior_index(p)]
    return p, start, full


@pytest.mark.parametrize("dtype", [cd.DOUBLE, cd.FLOAT], ids=["fp64", "fp32"])
def test_a_linear_field_is_extended_exactly(dtype):
    """cell-centred u = 3 + 2 x on integers, h = 3, both walls.  Dirichlet: parity -1 and a = 2 u(wall) -- the wall lies half a cell
    outside the first / last interior cell.  Neumann: parity +1 and a_k = -+(2 k + 1) * 2, the distance between ghost cell k and its
    mirror image times the gradient.  Either way every ghost cell along the dim holds the linear extension, exactly."""
    import torch
    from tests import gpu_bodies as B
    gdims = (12, 9, 10)
    args = {"gdims": gdims, "pdims": (1, 1)}
    h, gd, g = B._setup(0, 1, args)
    stream = torch.cuda.current_stream().cuda_stream
    real = AB.TYPES[dtype][0]
    for axis, dim in itertools.product(range(3), range(3)):
        halo = [0, 0, 0]
        halo[dim] = 3
        n = gdims[dim]
        for parity in (-1, 1):
            p, start, full = _line_pencil(h, gd, g, dtype, axis, halo, n, dim)
            if parity == -1:
                low, high = [2.0 * (3.0 + 2.0 * -0.5)] * 3, [2.0 * (3.0 + 2.0 * (n - 0.5))] * 3
            else:
                low, high = [-(2 * k + 1) * 2.0 for k in range(3)], [(2 * k + 1) * 2.0 for k in range(3)]
            dev, ptr = RB._device_pencil(start)
            cd.cudecompAmdSetWallHalos(axis, h, gd, ptr, dtype, parity, 0, 3, low, high, halo, (0, 0, 0), dim, None, stream)
            torch.cuda.synchronize()
            got = dev.cpu().numpy()[SLACK:-SLACK].view(real)
            assert np.array_equal(got, full.reshape(-1)), (AB.NAMES[dtype], axis, dim, parity)
    cd.cudecompGridDescDestroy(h, gd)


def test_sides():
    """sides = 1 leaves the high ghost cells poison; two calls -- the low wall with parity -1 and centering 1, the high wall with
    parity +1 and centering 0 -- equal the restatement with the two calls in that order"""
    import torch
    from tests import gpu_bodies as B
    gdims, halo, periods, dtype = (13, 10, 11), (2, 1, 3), (0, 0, 0), cd.FLOAT_COMPLEX
    h, gd, g = B._setup(0, 1, {"gdims": gdims, "pdims": (1, 1)})
    stream = torch.cuda.current_stream().cuda_stream
    nc, es = 2, 8
    world = WB.typed_world(dtype, gdims, 3)
    for axis, dim in itertools.product(range(3), range(3)):
        p = g.pencil_info(0, axis, halo, (0, 0, 0))
        start, lo = WB._start_and_lo(p, world, halo)
        low, high = WB.layer_values(dim, 0, halo[dim], nc), WB.layer_values(dim, 1, halo[dim], nc)
        calls = [(-1, 1, 1, low, None), (1, 0, 2, None, high)]
        dev, ptr = RB._device_pencil(start)
        for done, (parity, centering, sides, lo_values, hi_values) in enumerate(calls, 1):
            cd.cudecompAmdSetWallHalos(axis, h, gd, ptr, dtype, parity, centering, sides, lo_values, hi_values, halo, periods, dim, None, stream)
            torch.cuda.synchronize()
            steps = [[], [], []]  # (the other dims get no call: their ghost cells stay poison, and are sources as poison)
            steps[dim] = calls[:done]
            want = WB.rank_slice(p, WB.global_reference(dtype, world, halo, periods, steps), lo)
            diff = RB.first_difference(dev.cpu().numpy(), RB._with_slack(want), es)
            assert diff is None, (axis, dim, done, diff)
            high_slab = AB.pencil3(p, dev.cpu().numpy()[SLACK:-SLACK].reshape(-1, es))[AB.slab(p, dim, "H", halo[dim])]
            assert np.all(high_slab == RB.POISON) == (done == 1), (axis, dim, done)
    cd.cudecompGridDescDestroy(h, gd)


# ---- four ranks sharing the GPU --------------------------------------------------------------------------------------------
def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (10, 9, 11): slabs of 5 + 5, 5 + 4 and 6 + 5 cells, every rank an edge rank.  Non-periodic and mixed
    periods; after (update, wall values) over dims 0, 1, 2 every rank's pencil, halos included, is its slice of the definition
    applied dim by dim to the global array.  One halo backend: the call does not communicate."""
    cases = []
    for periods, axis, (halo, padding), (parity, centering), sides in itertools.product(
            ((0, 0, 0), (1, 0, 1), (0, 1, 0)), range(3), (((1, 2, 1), (0, 0, 0)), ((3, 1, 2), (1, 0, 2))), MIRRORS, (3, 1, 2)):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering, sides])
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "cases": cases}
    for failures in run_ranks(4, "tests.wall_values_bodies", "wall_sweep", args, timeout=300, fresh=False):
        assert failures == []


# ---- hipGraph, asynchrony --------------------------------------------------------------------------------------------------
def test_captured_sequence_replays_with_the_captured_addends():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 0, 1), "padding": (0, 1, 0), "parity": -1,
                  "centering": 0},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ((1, 2, 0),) * 3, "axis": 1, "halo": (2, 1, 2),
                  "periods": (0, 0, 0), "dtype": cd.HALF_COMPLEX, "parity": 1, "centering": 1}):
        assert run_ranks(1, "tests.wall_values_bodies", "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (0, 0, 0)}
    res = run_ranks(1, "tests.wall_values_bodies", "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["wall_host_ms"] < 0.25 * res["total_ms"], res
