"""Wall planes (cudecomp_halo_wall_planes.h: cudecompAmdSetWallPlaneHalos{X,Y,Z}) on the GPU: the two wall-plane kernels move by
move with source and destination in ONE buffer and the plane in another (every byte of both, poison slack on both sides included);
lists of wall-plane moves through the kernel layer's batching; IEEE edge values; single-rank pencils of every axis, memory order,
halo width, padding, period mix, centering, parity, `sides` and data type against the definition applied dim by dim
(tests/wall_planes_bodies.py); constant planes against cudecompAmdSetWallHalos; a field linear along the wall extended exactly; four
ranks sharing the GPU on a ragged 2 x 2 grid; capture into a hipGraph with the plane contents changed between replays; asynchrony.
Everything is compared byte for byte against numpy built from AB.typed_add and RB.flip_signs; only where the expected real is a NaN
is "a NaN of that type" enough (AB.mismatches).  Buffers start as a poison byte."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import move_lists as ML
from tests import reflect_bodies as RB
from tests import wall_planes_bodies as WPB
from tests import wall_values_bodies as WB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = RB.SLACK
K_ROWS_WALL_PLANE, K_GENERIC_WALL_PLANE = 41, 42
NEG = {False: "false", True: "true"}
ARITH = {cd.HALF: "_Float16", cd.HALF_COMPLEX: "_Float16", cd.BFLOAT16: "__bf16", cd.FLOAT: "float", cd.FLOAT_COMPLEX: "float",
         cd.DOUBLE: "double", cd.DOUBLE_COMPLEX: "double"}


def _typed(dtype, cells, seed):
    """finite reals of `dtype` for `cells` cells: uint8 (cells, es)"""
    nc = AB.TYPES[dtype][1]
    return np.ascontiguousarray(AB.bits_of(dtype, AB.typed_cells(dtype, seed, 0, 0, cells, nc))).view(np.uint8).reshape(cells, -1)


def _wall_plane(buf, pbuf, dtype, negate, side, extent, ss, ps, mirrored, soff, doff, poff, force, seed=0):
    """one wall-plane move through cudecompExtWallPlane3D: source and destination (strides `ss`) inside the device buffer `buf`, the
    source block `soff` elements past the slack and read backwards along dim `mirrored`, the destination block at `doff`; the plane
    block (strides `ps`) `poff` elements past the slack of `pbuf`, read backwards along `mirrored` on the low side (0).  Both buffers
    are poisoned, the source cells receive finite reals, the plane cells entries that are distinct per cell; afterwards EVERY byte of
    `buf` against numpy and every byte of `pbuf` against what it held.  Returns (kernel class, kernel name)."""
    import torch
    es = AB.element_bytes(dtype)
    signed, psigned = list(ss), list(ps)
    first = soff + (extent[mirrored] - 1) * ss[mirrored]  # the source cell of index 0 along the mirrored dim
    signed[mirrored] = -ss[mirrored]
    pfirst = poff
    if side == 0:
        pfirst = poff + (extent[mirrored] - 1) * ps[mirrored]
        psigned[mirrored] = -ps[mirrored]
    src, dst, pc = ML.cells(extent, signed, first), ML.cells(extent, ss, doff), ML.cells(extent, psigned, pfirst)
    nbytes = 2 * SLACK + (max(int(src.max()), int(dst.max())) + 1) * es
    pbytes = 2 * SLACK + (int(pc.max()) + 1) * es
    assert nbytes <= buf.numel() and pbytes <= pbuf.numel() and src.min() >= 0 and pc.min() >= 0
    if src.size <= (1 << 20):
        both = np.concatenate([src, dst])
        assert np.unique(both).size == both.size, "source and destination cells overlap"
        assert np.unique(pc).size == pc.size
    want = np.full(nbytes, RB.POISON, dtype=np.uint8)
    body = want[SLACK:nbytes - SLACK].reshape(-1, es)
    body[src] = _typed(dtype, src.size, seed)
    pwant = np.full(pbytes, RB.POISON, dtype=np.uint8)
    pbody = pwant[SLACK:pbytes - SLACK].reshape(-1, es)
    pbody[pc] = WPB.entries(dtype, np.arange(pc.size) + 31 * seed)
    view, pview = buf[:nbytes], pbuf[:pbytes]
    view.copy_(torch.from_numpy(want))
    pview.copy_(torch.from_numpy(pwant))
    body[dst] = WPB.wall_cells(dtype, body[src], -1 if negate else 1, pbody[pc])
    base, pbase = buf.data_ptr() + SLACK, pbuf.data_ptr() + SLACK
    cls = cd.cudecompExtWallPlane3D(base + first * es, base + doff * es, pbase + pfirst * es, dtype, negate, extent, signed, ss, psigned,
                                    force, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    bad = np.nonzero(view.cpu().numpy() != want)[0]
    assert bad.size == 0, (AB.NAMES[dtype], negate, side, extent, ss, ps, mirrored, soff, doff, poff, force, cls, name,
                           "%d bytes differ, first at byte %d of the buffer (source at %d, destination at %d)"
                           % (bad.size, bad[0], SLACK + soff * es, SLACK + doff * es))
    assert np.array_equal(pview.cpu().numpy(), pwant), ("the plane buffer was written", extent, ss, ps, force, name)
    return cls, name


def _lane_bytes(es, extent, ss, ps, mirrored, soff, doff, poff):
    """the rule for three operands (source and destination share `ss`): the two dims that are not mirrored merge into longer rows
    only if contiguous in the pencil AND in the plane; rows need a fastest dim contiguous on all operands that is not the mirrored
    one; then the widest of 16, 8, 4, 2 bytes, not below the element, that divides the row length, the three bases and every row and
    plane stride.  None: the element-wise kernel."""
    dims = sorted([(extent[i], ss[i], ps[i]) for i in range(3) if i != mirrored and extent[i] > 1], key=lambda d: d[1])
    if len(dims) == 2 and dims[1][1] == dims[0][0] * dims[0][1] and dims[1][2] == dims[0][0] * dims[0][2]:
        dims = [(dims[0][0] * dims[1][0], dims[0][1], dims[0][2])]
    live = extent[mirrored] > 1
    if (dims and (dims[0][1] != 1 or dims[0][2] != 1)) or (live and (ss[mirrored] == 1 or ps[mirrored] == 1)):
        return None
    counts = [dims[0][0] if dims else 1, soff, doff, poff] + [s for d in dims[1:] for s in d[1:]]
    counts += [ss[mirrored], ps[mirrored]] if live else []
    vb = 16
    while vb > es and any((c * es) % vb for c in counts):
        vb //= 2
    return vb


def _rows_name(dtype, vb, stream, negate):
    return "rows_wall_plane_kernel<%s,%d,%d,%s>" % (ARITH[dtype], vb, stream, NEG[negate])


def _generic_name(dtype, negate):
    return "generic_wall_plane_kernel<%s,%d,%s>" % (ARITH[dtype], AB.element_bytes(dtype), NEG[negate])


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130)


def rows_grid(es):
    """the cases of test_kernel_parity_rows: (n, negate, side, extent, ss, ps, mirrored, soff, doff, poff, force).  Source and
    destination share the phase `offset` of the 16-byte grid; the plane in three turns -- its phase equal to theirs (0), shifted by
    one element (1), a pitch different from the pencil's (2) -- and every turn meets every phase and every `force`"""
    n = 0
    for length, extra, m, as_plane in itertools.product(LENGTHS, (0, 3), (1, 2, 3, 8, 9), (False, True)):
        pitch = length + extra
        for offset, turn, force in itertools.product(range(16 // es + 2), (0, 1, 2), (0, 1, 2)):
            negate, side = bool(n & 1), (n >> 1) & 1
            n += 1
            ppitch = pitch + (1 if turn == 2 else 0)
            if as_plane:
                extent, mirrored = (length, 3, m), 2
                ss, ps = (1, pitch, pitch * 3 + 5), (1, ppitch, ppitch * 3 + 5)
            else:
                extent, mirrored = (length, m, 3), 1
                ss, ps = (1, pitch, pitch * m + 5), (1, ppitch, ppitch * m + 5)
            soff = offset
            doff = offset + -(-(ML.span(extent, ss) + 3) // 16) * 16
            yield n, negate, side, extent, ss, ps, mirrored, soff, doff, doff + (1 if turn == 1 else 0), force


def mirrored_fastest_grid(es):
    """the cases of test_kernel_parity_mirrored_fastest_dim, same fields; ghost cells below their sources; every turn of the plane
    meets every phase and every `force`"""
    n = 0
    for h, (rows, planes), pitch, offset, turn, force in itertools.product(range(1, 10), ((1, 1), (9, 7), (300, 1), (1, 40)), (19,),
                                                                           range(16 // es + 2), (0, 1, 2), (0, 1, 2)):
        negate, side = bool(n & 1), (n >> 1) & 1
        n += 1
        ppitch = pitch + (2 if turn == 2 else 0)
        extent, ss, ps = (h, rows, planes), (1, pitch, pitch * (rows + 2)), (1, ppitch, ppitch * (rows + 2))
        yield n, negate, side, extent, ss, ps, 0, offset + h, offset, offset + (1 if turn == 1 else 0), force


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows(dtype):
    """row length x row pitch (length + 0, + 3) x extent along the mirrored dim (1, 2, 3, 8, 9) as the row index and as the plane
    index x base offset (every phase of the 16-byte grid and one past it) x fast path, forced element-wise, forced streaming; the
    sign flip on every second case, the side changing every two; the plane in three turns (rows_grid).  The kernel and its name on
    every case."""
    import torch
    es = AB.element_bytes(dtype)
    buf = torch.empty(2 * SLACK + 2 * (134 * 9 * 4 + 64) * es, dtype=torch.uint8, device="cuda")
    pbuf = torch.empty(2 * SLACK + 2 * (135 * 9 * 4 + 64) * es, dtype=torch.uint8, device="cuda")
    rows_seen, generic_seen, widths, narrowed = 0, 0, set(), {0: 0, 2: 0}
    for n, negate, side, extent, ss, ps, mirrored, soff, doff, poff, force in rows_grid(es):
        cls, name = _wall_plane(buf, pbuf, dtype, negate, side, extent, ss, ps, mirrored, soff, doff, poff, force, seed=n)
        vb = _lane_bytes(es, extent, ss, ps, mirrored, soff, doff, poff)
        alone = _lane_bytes(es, extent, ss, ss, mirrored, soff, doff, doff)  # (the pencil's own width: the plane at its phase and pitch)
        if not force & 1 and vb is not None and alone is not None and vb < alone:
            narrowed[force] += 1  # only the plane -- its base or its pitch -- narrows the lanes of the rows kernel
        if force & 1 or vb is None:
            assert (cls, name) == (2, _generic_name(dtype, negate)), (extent, ss, ps, soff, force, name)
            generic_seen += 1
        else:
            assert (cls, name) == (0, _rows_name(dtype, vb, 1 if force & 2 else 0, negate)), (extent, ss, ps, soff, force, name)
            rows_seen += 1
            widths.add(vb)
    assert rows_seen > generic_seen > 0 and widths == {w for w in (2, 4, 8, 16) if w >= es}
    assert es == 16 or (narrowed[0] > 0 and narrowed[2] > 0), narrowed  # (16-byte elements: lanes are never narrower than one)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_mirrored_fastest_dim(dtype):
    """the mirrored dim as the fastest one: rows of 1..9 elements reversed in themselves, a row pitch apart -- the element-wise
    kernel by itself, whatever is forced; one and many rows and planes, every base phase; the plane in the same three turns"""
    import torch
    es = AB.element_bytes(dtype)
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    pbuf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for n, negate, side, extent, ss, ps, mirrored, soff, doff, poff, force in mirrored_fastest_grid(es):
        cls, name = _wall_plane(buf, pbuf, dtype, negate, side, extent, ss, ps, mirrored, soff, doff, poff, force, seed=n)
        h, rows, planes = extent
        if h > 1 or rows * planes > 1 or force & 1:  # (h == 1: single cells a pitch apart, the degenerate shape of the copies)
            assert (cls, name) == (2, _generic_name(dtype, negate)), (extent, ss, soff, force, name)
        else:  # a single cell: a row of one element
            assert (cls, name) == (0, _rows_name(dtype, es, 1 if force & 2 else 0, negate)), (extent, soff, force, name)


def test_kernel_parity_streaming_by_size_and_second_grid_stride_pass():
    import torch
    buf = torch.empty(2 * SLACK + (64 << 20) + 4096, dtype=torch.uint8, device="cuda")
    pbuf = torch.empty(2 * SLACK + (32 << 20) + 4096, dtype=torch.uint8, device="cuda")
    # 32 MiB in one move, the mirrored dim the plane index: the size rule itself picks the non-temporal instantiation
    extent, ss = (2048, 1024, 2), (1, 2048, 2048 * 1024)
    assert _wall_plane(buf, pbuf, cd.DOUBLE, True, 0, extent, ss, ss, 2, 0, 2 * 2048 * 1024 + 8, 0, 0) == (
        0, "rows_wall_plane_kernel<double,16,1,true>")
    assert _wall_plane(buf, pbuf, cd.FLOAT, False, 1, extent, ss, ss, 2, 4, 2 * 2048 * 1024 + 8, 4, 0) == (
        0, "rows_wall_plane_kernel<float,16,0,false>")  # (16 MiB)
    # the element-wise kernel launches at most 8192 workgroups of 256 lanes: more elements than that take a second pass
    extent, ss = (3, 8192 * 128 + 77, 1), (1, 3, 0)
    assert _wall_plane(buf, pbuf, cd.HALF, True, 0, extent, ss, (1, 4, 0), 0, 5, 3 * (8192 * 128 + 80), 1, 0) == (
        2, "generic_wall_plane_kernel<_Float16,2,true>")


# ---- lists -----------------------------------------------------------------------------------------------------------------
def _run_plane_list(pairs, mirrored_dims, dtype, negate, flags=0):
    """the list through cudecompExtRunMoves (mode 13 / 14): the pencil cells in ONE device buffer, the low and the high plane in two
    more; every byte of the first against numpy applying the moves one by one, every byte of the planes against what they held;
    launches and elements per class against cudecompExtDescribeMoves.  Returns the described launches."""
    import torch
    es = AB.element_bytes(dtype)
    mode = cd.MOVES_WALL_PLANE_NEGATE if negate else cd.MOVES_WALL_PLANE
    moves, operands = [m for m, _ in pairs], [o for _, o in pairs]
    src = [ML.cells(m.extent, m.ss, m.src_off) for m in moves]
    dst = [ML.cells(m.extent, m.ds, m.dst_off) for m in moves]
    pcs = [ML.cells(m.extent, ps, off) for m, (off, ps) in pairs]
    everything = np.concatenate(src + dst)
    assert everything.min() >= 0 and np.unique(everything).size == everything.size, "the cells of the list overlap"
    want = np.full(2 * SLACK + (int(everything.max()) + 1) * es, RB.POISON, dtype=np.uint8)
    body = want[SLACK:want.size - SLACK].reshape(-1, es)
    for i, c in enumerate(src):
        body[c] = _typed(dtype, c.size, 50 + i)
    pcells = max(int(c.max()) for c in pcs) + 1
    planes = [np.full(2 * SLACK + pcells * es, RB.POISON, dtype=np.uint8) for _ in (0, 1)]
    for i, (m, c) in enumerate(zip(moves, pcs)):  # every move ITS entries: distinct per move and cell
        assert c.min() >= 0
        planes[m.peer][SLACK:-SLACK].reshape(-1, es)[c] = WPB.entries(dtype, np.arange(c.size) + 4001 * i)
    for m, s, d, c in zip(moves, src, dst, pcs):
        body[d] = WPB.wall_cells(dtype, body[s], -1 if negate else 1, planes[m.peer][SLACK:-SLACK].reshape(-1, es)[c])
    dev = torch.from_numpy(want.copy()).cuda()
    body0 = want.copy()
    body0[SLACK:-SLACK].reshape(-1, es)[np.concatenate(dst)] = RB.POISON
    dev.copy_(torch.from_numpy(body0))
    dplanes = [torch.from_numpy(p).cuda() for p in planes]
    ptrs = [dev.data_ptr() + SLACK, dplanes[0].data_ptr() + SLACK, dplanes[1].data_ptr() + SLACK]
    described = cd.cudecompExtDescribeMoves(moves, ptrs, es, mode, dtype, flags, planes=operands)
    launches, elements, total = cd.cudecompExtRunMoves(moves, ptrs, es, mode, dtype, None, flags, None,
                                                       torch.cuda.current_stream().cuda_stream, planes=operands)
    torch.cuda.synchronize()
    what = [(l["kind"], l["vec"], l["n"], l["interleave"], l["blocks"]) for l in described]
    assert total == len(described), what
    assert launches == [sum(1 for l in described if l["cls"] == c) for c in range(3)], what
    assert elements == [sum(l["elements"] for l in described if l["cls"] == c) for c in range(3)], what
    bad = np.nonzero(dev.cpu().numpy() != want)[0]
    assert bad.size == 0, ("%d bytes differ, first at byte %d" % (bad.size, bad[0] if bad.size else -1), what)
    for side in (0, 1):
        assert np.array_equal(dplanes[side].cpu().numpy(), planes[side]), ("a plane buffer was written", side, what)
    return described


@pytest.mark.parametrize("negate", [False, True], ids=["plain", "sign_flip"])
def test_eight_siblings_share_one_interleaved_launch(negate):
    """eight moves of one kernel choice with 1 .. 300 workgroups each, sides alternating, layers as rows and as planes: one launch,
    served round robin, padded to 8 x 300 -- every move finds ITS plane operand"""
    targets = [1, 300, 2, 99, 5, 150, 17, 40]
    pairs, mirrored_dims, at = [], [], 0
    for i, t in enumerate(targets):  # rows of 32 fp64: 16 lanes per row, 64 rows per workgroup
        if t % 3 == 0:  # three layers as planes of 64 * (t / 3) rows
            extent, mirrored = (32, 64 * (t // 3), 3), 2
        else:  # 8 or 2 layers as the rows of t planes: one workgroup per plane
            extent, mirrored = (32, 8 if t % 8 == 0 else 2, t), 1
        ss = (1, 34, 34 * extent[1] + 2)
        ps = (1, 36, 36 * extent[1] + 4) if i % 3 == 1 else ss  # (another pitch, still 16-byte aligned)
        span = ML.span(extent, ss)
        pairs.append(WPB.plane_move(extent, ss, mirrored, at, at + span + 6, i & 1, ps, poff=at // 2 * 2))
        mirrored_dims.append(mirrored)
        at += 2 * span + 16
    (l,) = _run_plane_list(pairs, mirrored_dims, cd.DOUBLE, negate)
    assert (l["kind"], l["n"], l["interleave"], l["vec"]) == (K_ROWS_WALL_PLANE, 8, 1, 16), l
    assert l["blocks"] == 8 * 300 and l["index"] == list(range(8)), l
    assert [b - a for a, b in zip(l["first_block"], l["first_block"][1:])] == targets, l


@pytest.mark.parametrize("dtype,negate", [(cd.HALF, False), (cd.BFLOAT16, True), (cd.FLOAT_COMPLEX, True)], ids=["fp16", "bf16_flip", "complex64_flip"])
def test_a_mixed_list_of_nine_moves(dtype, negate):
    """row moves at several lane widths (2-byte rows at 2 mod 4 among them, and rows only the plane narrows), the mirrored dim as the
    row and as the plane index, mirrored fastest dims and a single cell: several launches, every byte against numpy applying the moves
    one by one"""
    es = AB.element_bytes(dtype)
    shapes = [((64, 5, 3), (1, 64, 328), 1, 0), ((64, 5, 3), (1, 64, 328), 2, 0), ((33, 4, 2), (1, 35, 150), 1, 1),
              ((3, 9, 7), (1, 13, 130), 0, 0), ((130, 2, 1), (1, 131, 0), 1, 2), ((1, 1, 1), (1, 1, 1), 0, 3),
              ((8, 37, 2), (1, 8, 300), 2, 0), ((2, 50, 1), (1, 5, 0), 0, 1), ((1025, 3, 2), (1, 1028, 3100), 1, 0)]
    pairs, at = [], 0
    for i, (extent, ss, mirrored, phase) in enumerate(shapes):
        span = ML.span(extent, ss)
        at += phase
        ps = (1, ss[1] + 1, ss[2] + 7) if i == 1 else ss  # (move 1: only the plane's pitches narrow the lanes)
        doff = -(-(at + span + 4) // 8) * 8 + phase  # source, destination and plane at one phase of the 16-byte grid ...
        pairs.append(WPB.plane_move(extent, ss, mirrored, at, doff, (i // 2) & 1, ps, poff=at + (1 if i == 6 else 0)))  # (... but for move 6)
        at = -(-(doff + span + 8) // 8) * 8  # every move starts from a 16-byte boundary (2-byte elements) plus its phase
    described = _run_plane_list(pairs, [s[2] for s in shapes], dtype, negate)
    assert len(pairs) == 9 and len(described) >= 3
    assert {l["kind"] for l in described} == {K_ROWS_WALL_PLANE, K_GENERIC_WALL_PLANE}
    assert sorted(i for l in described for i in l["index"]) == list(range(9))
    if es == 2:
        assert {l["vec"] for l in described if l["kind"] == K_ROWS_WALL_PLANE} >= {2, 16}


# ---- edge values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [cd.HALF, cd.BFLOAT16, cd.FLOAT, cd.DOUBLE], ids=["fp16", "bf16", "fp32", "fp64"])
def test_edge_values(dtype):
    """every pair (mirror, addend) of AB.edge_table -- zeros, subnormals, the largest finite numbers, infinities, NaNs -- in both
    parities through both kernels: the 24 mirrors along every row, the addends from a plane whose row r holds addend r, so one launch
    covers all 576 pairs.  Where the expected real is a NaN any NaN of the type will do; every other real bit for bit."""
    import torch
    kind = AB.kind_of(dtype)
    u, es = AB.FORMATS[kind][0], AB.element_bytes(dtype)
    table = AB.edge_table(kind)
    n = len(table)
    stream = torch.cuda.current_stream().cuda_stream
    mirrors, addends = np.tile(table, n), np.repeat(table, n)  # cell (row r, column c): mirror c, addend r
    src = torch.from_numpy(mirrors.view(np.uint8).copy()).cuda()
    plane = torch.from_numpy(addends.view(np.uint8).copy()).cuda()
    dst = torch.empty(n * n * es, dtype=torch.uint8, device="cuda")
    for negate, force in itertools.product((False, True), (0, 1)):
        dst.fill_(RB.POISON)
        # rows of the source run backwards (every row holds the same 24 mirrors), rows of the plane forwards
        cls = cd.cudecompExtWallPlane3D(src.data_ptr() + (n - 1) * n * es, dst.data_ptr(), plane.data_ptr(), dtype, negate, (n, n, 1),
                                        (1, -n, 0), (1, n, 0), (1, n, 0), force, stream)
        torch.cuda.synchronize()
        assert cls == (2 if force else 0)
        got = dst.cpu().numpy().view(u)
        mirror = mirrors ^ u(1 << (8 * es - 1)) if negate else mirrors
        want = AB.bits_of(dtype, AB.typed_add(dtype, mirror.astype(u), addends.astype(u)))
        bad = AB.mismatches(kind, got, want)
        assert not bad.any(), (AB.NAMES[dtype], negate, force, [hex(int(x)) for x in mirrors[bad]], [hex(int(x)) for x in addends[bad]],
                               [hex(int(x)) for x in got[bad]], [hex(int(x)) for x in want[bad]])
        assert np.array_equal(plane.cpu().numpy().view(u), addends) and np.array_equal(src.cpu().numpy().view(u), mirrors)


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
    """every halo set, padding, period mix, centering, parity and `sides` of the wall values' sweep; the seven data types in turn.
    (update, wall planes) over dims 0, 1, 2 on a pencil that is poison outside its interior: whole pencils against the definition
    applied dim by dim; the number of cases admitted is stated."""
    cases = []
    for halo, padding, periods, (parity, centering), sides in itertools.product(HALOS, PADDINGS, PERIODS, MIRRORS, (1, 2, 3)):
        if _admitted(SHAPES[shape], halo, periods, centering):
            cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering, sides])
    assert len(cases) == 576 and len({(c[4], c[5], c[6], c[7]) for c in cases}) == 84
    args = {"gdims": SHAPES[shape], "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases}
    assert WPB.plane_sweep(0, 1, args) == []


def test_a_halo_of_nine_layers():
    """h = 9 along the 13-cell dim, as the fastest, the middle and the slowest memory axis; every type"""
    cases = [[axis, (9, 1, 1), (0, 1, 0), (1, 0, 0), dtype, parity, centering, 3] for axis in range(3)
             for dtype, parity, centering in zip(AB.ALL_TYPES, itertools.cycle((-1, 1)), itertools.cycle((0, 0, 1)))]
    assert len(cases) == 21
    for order in ((0, 1, 2), (1, 0, 2), (2, 1, 0)):
        assert WPB.plane_sweep(0, 1, {"gdims": (13, 10, 11), "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases}) == []


# ---- constant planes reproduce the wall values -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_constant_planes_reproduce_the_wall_values(dtype):
    """each plane filled with the converted per-layer addends of cudecompAmdSetWallHalos (exact in every type, the same at every
    position): the pencil is byte-identical to the one the existing call produces from the same start.  Three axes, three dims, both
    parities, sides 1, 2 and 3."""
    import torch
    from tests import gpu_bodies as B
    gdims, halo, periods, padding = (13, 10, 11), (2, 1, 3), (0, 0, 0), (1, 2, 0)
    h, gd, g = B._setup(0, 1, {"gdims": gdims, "pdims": (1, 1)})
    stream = torch.cuda.current_stream().cuda_stream
    nc, es = AB.TYPES[dtype][1], AB.element_bytes(dtype)
    world = WB.typed_world(dtype, gdims, 3)
    compared = 0
    for axis, dim in itertools.product(range(3), range(3)):
        p = g.pencil_info(0, axis, halo, padding)
        start, lo = WB._start_and_lo(p, world, halo)
        hd = halo[dim]
        values = [WB.layer_values(dim, side, hd, nc) for side in (0, 1)]
        shape, elements = cd.wall_plane_shape(p, dim, halo)
        a = [int(x) for x in p.order].index(dim)
        planes = []
        for side in (0, 1):  # layer k along memory position a, the same element everywhere else (padding positions included)
            host = np.empty((shape[2], shape[1], shape[0], es), dtype=np.uint8)
            for k, element in enumerate(WB.elements_of(dtype, values[side], nc)):
                at = [slice(None)] * 3
                at[2 - a] = k
                host[tuple(at)] = np.frombuffer(element, dtype=np.uint8)
            assert host.size == elements * es
            planes.append(RB._device_pencil(host))
        for parity, sides in itertools.product((1, -1), (1, 2, 3)):
            dev_a, ptr_a = RB._device_pencil(start)
            dev_b, ptr_b = RB._device_pencil(start)
            cd.cudecompAmdSetWallHalos(axis, h, gd, ptr_a, dtype, parity, 0, sides, values[0] if sides & 1 else None,
                                       values[1] if sides & 2 else None, halo, periods, dim, padding, stream)
            cd.cudecompAmdSetWallPlaneHalos(axis, h, gd, ptr_b, dtype, parity, 0, sides, planes[0][1] if sides & 1 else None,
                                            planes[1][1] if sides & 2 else None, halo, periods, dim, padding, stream)
            torch.cuda.synchronize()
            got, want = dev_b.cpu().numpy(), dev_a.cpu().numpy()
            assert RB.first_difference(got, want, es) is None, (axis, dim, parity, sides, RB.first_difference(got, want, es))
            assert np.any(want != RB._with_slack(start))  # (the existing call did write)
            compared += 1
    assert compared == 54
    cd.cudecompGridDescDestroy(h, gd)


def test_an_overlapping_plane_is_refused_from_the_cached_plan_too():
    """the first call builds and caches the plan; a second call whose plane lies on the pencil, or one byte into either end of it, is
    INVALID_USAGE with the overlap's message and writes nothing; a plane that ends where the pencil begins is accepted"""
    import ctypes as C

    import torch
    from tests import gpu_bodies as B
    gdims, halo, dtype, es = (13, 10, 11), (2, 1, 3), cd.DOUBLE, 8
    h, gd, g = B._setup(0, 1, {"gdims": gdims, "pdims": (1, 1)})
    stream = torch.cuda.current_stream().cuda_stream
    L = cd.lib()
    plans = C.c_int64(-1)
    for axis, dim in itertools.product(range(3), range(3)):
        p = g.pencil_info(0, axis, halo, (0, 0, 0))
        _, elements = cd.wall_plane_shape(p, dim, halo)
        # one allocation: [plane | pencil | plane], so that "ends where the pencil begins" is an address inside it
        raw = torch.zeros((2 * elements + int(p.size)) * es, dtype=torch.uint8, device="cuda")
        pencil = raw.data_ptr() + elements * es
        before, after = raw.data_ptr(), pencil + int(p.size) * es
        cd.cudecompAmdSetWallPlaneHalos(axis, h, gd, pencil, dtype, -1, 0, 3, before, after, halo, (0, 0, 0), dim, None, stream)
        torch.cuda.synchronize()
        assert L.cudecompExtHaloPlanCount(h, gd, C.byref(plans)) == cd.RESULT_SUCCESS
        cached, kept = plans.value, raw.cpu().numpy().copy()
        for low, high in ((pencil, after), (before, after - 1), (before + 1, after), (before, pencil + 8)):
            with pytest.raises(cd.CudecompError) as e:
                cd.cudecompAmdSetWallPlaneHalos(axis, h, gd, pencil, dtype, -1, 0, 3, low, high, halo, (0, 0, 0), dim, None, stream)
            assert e.value.code == cd.RESULT_INVALID_USAGE, (axis, dim, e.value.code)
        cd.cudecompAmdSetWallPlaneHalos(axis, h, gd, pencil, dtype, -1, 0, 1, before, pencil, halo, (0, 0, 0), dim, None, stream)  # (not named)
        torch.cuda.synchronize()
        assert L.cudecompExtHaloPlanCount(h, gd, C.byref(plans)) == cd.RESULT_SUCCESS and plans.value == cached + 1
        assert np.array_equal(raw.cpu().numpy(), kept)  # (zeros everywhere: -0 + 0 = +0, and the refused calls wrote nothing)
    cd.cudecompGridDescDestroy(h, gd)


# ---- a field linear along the wall -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [cd.DOUBLE, cd.FLOAT], ids=["fp64", "fp32"])
def test_a_field_linear_along_the_wall_is_extended_exactly(dtype):
    """cell-centred u = 3 + 2 x + 5 y on integers, x along `dim`, y along the next dim, h = 3, both walls.  Dirichlet planes
    2 u(wall; y) with parity -1 -- the wall lies half a cell outside the first / last interior cell: every ghost cell along the dim
    holds the linear extension, exactly."""
    import torch
    from tests import gpu_bodies as B
    gdims = (12, 9, 10)
    h, gd, g = B._setup(0, 1, {"gdims": gdims, "pdims": (1, 1)})
    stream = torch.cuda.current_stream().cuda_stream
    real = AB.TYPES[dtype][0]
    es = np.dtype(real).itemsize
    for axis, dim in itertools.product(range(3), range(3)):
        halo = [0, 0, 0]
        halo[dim] = 3
        ydim = (dim + 1) % 3
        p = g.pencil_info(0, axis, halo, (0, 0, 0))
        ax, n = RB._dim_axis(p, dim)
        ay, ny = RB._dim_axis(p, ydim)
        xs, ys = [1, 1, 1], [1, 1, 1]
        xs[ax], ys[ay] = n, ny
        x, y = (np.arange(n) - 3.0).reshape(xs), np.arange(ny, dtype=np.float64).reshape(ys)
        view_shape = AB.pencil3(p, np.zeros(int(p.size), dtype=real)).shape
        full = np.ascontiguousarray(np.broadcast_to(3.0 + 2.0 * x + 5.0 * y, view_shape)).astype(real)
        start = np.full((int(p.size), es), RB.POISON, dtype=np.uint8)
        AB.pencil3(p, start)[RB.interior_index(p)] = AB.pencil3(p, full.reshape(-1).view(np.uint8).reshape(int(p.size), -1))[RB.interior_index(p)]
        shape, elements = cd.wall_plane_shape(p, dim, halo)
        ks = [1, 1, 1]
        ks[ax] = 3
        planes = []
        for wall in (-0.5, gdims[dim] - 0.5):  # the plane's index along `dim` is the layer: the same Dirichlet value on every layer
            host = np.broadcast_to(2.0 * (3.0 + 2.0 * wall + 5.0 * y) + 0.0 * np.arange(3.0).reshape(ks), (shape[2], shape[1], shape[0]))
            planes.append(RB._device_pencil(np.ascontiguousarray(host).astype(real).reshape(-1).view(np.uint8)))
            assert host.size == elements
        dev, ptr = RB._device_pencil(start)
        cd.cudecompAmdSetWallPlaneHalos(axis, h, gd, ptr, dtype, -1, 0, 3, planes[0][1], planes[1][1], halo, (0, 0, 0), dim, None, stream)
        torch.cuda.synchronize()
        got = dev.cpu().numpy()[SLACK:-SLACK].view(real)
        assert np.array_equal(got, full.reshape(-1)), (AB.NAMES[dtype], axis, dim)
    cd.cudecompGridDescDestroy(h, gd)


# ---- four ranks sharing the GPU --------------------------------------------------------------------------------------------
def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (10, 9, 11): slabs of 5 + 5, 5 + 4 and 6 + 5 cells, every rank an edge rank.  Non-periodic and mixed
    periods; each rank's planes are its slab of the global planes; after (update, wall planes) over dims 0, 1, 2 every rank's pencil,
    halos included, is its slice of the definition applied dim by dim to the global array."""
    cases = []
    for periods, axis, (halo, padding), (parity, centering), sides in itertools.product(
            ((0, 0, 0), (1, 0, 1), (0, 1, 0)), range(3), (((1, 2, 1), (0, 0, 0)), ((3, 1, 2), (1, 0, 2))), MIRRORS, (3, 1, 2)):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], parity, centering, sides])
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "cases": cases}
    for failures in run_ranks(4, "tests.wall_planes_bodies", "plane_sweep", args, timeout=300, fresh=False):
        assert failures == []


# ---- hipGraph, asynchrony --------------------------------------------------------------------------------------------------
def test_a_replayed_graph_reads_the_planes_as_they_are_then():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 0, 1), "padding": (0, 1, 0), "parity": -1,
                  "centering": 0},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ((1, 2, 0),) * 3, "axis": 1, "halo": (2, 1, 2),
                  "periods": (0, 0, 0), "dtype": cd.HALF_COMPLEX, "parity": 1, "centering": 1}):
        assert run_ranks(1, "tests.wall_planes_bodies", "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (0, 0, 0)}
    res = run_ranks(1, "tests.wall_planes_bodies", "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["wall_host_ms"] < 0.25 * res["total_ms"], res
