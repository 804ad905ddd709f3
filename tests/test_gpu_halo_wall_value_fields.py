"""Multi-field wall values (cudecomp_halo_wall_value_fields.h: cudecompAmdSetWallFieldHalos{X,Y,Z}) on the GPU: the wall field-move
kernels through cudecompExtRunWallFieldMoves in ONE arena that holds every field with 256 bytes of slack around each -- every byte
against numpy built from WB.wall_cells; a call split into four launches; IEEE edge values in the last slot of a launch;
single-rank pencils of every axis, memory order, halo width, padding, period mix, centering and `sides` with 3 and 5 fields of
mixed parities against single calls on clones; the widest halo; four ranks on a ragged 2 x 2 grid; capture into a hipGraph;
asynchrony.  Everything is compared byte for byte; only where the expected real is a NaN is "a NaN of that type" enough."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import move_lists as ML
from tests import reflect_bodies as RB
from tests import wall_value_fields_bodies as FB
from tests import wall_values_bodies as WB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = 256  # bytes between any two fields (and before the first, after the last) that no move may touch
POISON = RB.POISON
K_ROWS_FIELDS_WALL, K_GENERIC_FIELDS_WALL = 39, 40
ARITH = {cd.HALF: "_Float16", cd.HALF_COMPLEX: "_Float16", cd.BFLOAT16: "__bf16", cd.FLOAT: "float", cd.FLOAT_COMPLEX: "float",
         cd.DOUBLE: "double", cd.DOUBLE_COMPLEX: "double"}
MASKS = ("none", "all", "alternating", "first", "last")


def mask_of(kind, n):
    every = (1 << n) - 1
    return {"none": 0, "all": every, "alternating": 0xAAAAAAAA & every, "first": 1, "last": 1 << (n - 1)}[kind]


def spell(d, dtype):
    """the template spelling of a launch cudecompExtDescribeWallFieldMoves describes (csrc/kernels.cc spellKernelName)"""
    if d["kind"] == K_ROWS_FIELDS_WALL:
        return "rows_fields_wall_kernel<%s,%d,%d>" % (ARITH[dtype], d["vec"], d["access"])
    assert d["kind"] == K_GENERIC_FIELDS_WALL, d
    return "generic_fields_wall_kernel<%s,%d>" % (ARITH[dtype], AB.element_bytes(dtype))


def _typed(dtype, cells, seed):
    """finite reals of `dtype` for `cells` cells: uint8 (cells, es)"""
    nc = AB.TYPES[dtype][1]
    return np.ascontiguousarray(AB.bits_of(dtype, AB.typed_cells(dtype, seed, 0, 0, cells, nc))).view(np.uint8).reshape(cells, -1)


def _layer_index(extent, mirrored):
    """the index along dim `mirrored` of every cell of a move, in the order of ML.cells (dim 0 fastest)"""
    return np.indices([int(e) for e in extent][::-1]).reshape(3, -1)[::-1][mirrored]


def _raw(dtype, elems):
    """elems[f][side] = list of element bytes per ghost layer -> the bytes the Run hook takes: (fields, 2, MAX_WALL_HALO) elements"""
    es = AB.element_bytes(dtype)
    raw = bytearray(len(elems) * 2 * cd.MAX_WALL_HALO * es)
    for f, per_field in enumerate(elems):
        for side in (0, 1):
            for k, e in enumerate(per_field[side]):
                at = ((f * 2 + side) * cd.MAX_WALL_HALO + k) * es
                raw[at:at + es] = e
    return bytes(raw)


def _run(buf, dtype, extent, strides, mirrored, n_fields, mask, side_list, force, offsets, seed):
    """the wall-moves of `side_list` (0 low, 1 high) of the geometry (extent, strides) mirrored along dim `mirrored`, for n_fields fields
    whose bases lie offsets[f] elements into their regions of the arena `buf`.  The arena is poisoned, the source cells receive
    finite reals; afterwards EVERY byte of it -- slack, source cells, the cells between rows -- against numpy: dst = s_f * src + the
    addend of field f, side and ghost layer (WB.wall_cells).  Returns (kernel name, described launches)."""
    import torch
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    h = int(extent[mirrored])
    span = ML.span(extent, strides)
    part = span + 3 + (span + 3) % 2  # (even: the 2-byte cases decide their alignment by the fields' offsets alone)
    region = (max(offsets) + 4 * part) * es + SLACK  # [side A source | side A destination | side B source | side B destination]
    region += -region % 16
    total = SLACK + n_fields * region
    assert total <= buf.numel(), (total, buf.numel())
    want = np.full(total, POISON, dtype=np.uint8)
    bases = [SLACK + f * region + offsets[f] * es for f in range(n_fields)]
    backwards = [-s if d == mirrored else s for d, s in enumerate(strides)]
    first = (h - 1) * int(strides[mirrored])  # the source cell of index 0 along the mirrored dim
    elems = [[WB.elements_of(dtype, FB.addend_values(f, side, h, nc, seed), nc) for side in (0, 1)] for f in range(n_fields)]
    moves, todo = [], []
    for i, side in enumerate(side_list):
        src_off, dst_off = 2 * i * part, (2 * i + 1) * part
        m = cd.make_move(extent, backwards, strides, src_off=src_off + first, dst_off=dst_off, src_buf=0, dst_buf=0)
        m.peer = side
        moves.append(m)
        todo.append((side, ML.cells(extent, backwards, src_off + first), ML.cells(extent, strides, dst_off)))
    j = _layer_index(extent, mirrored)
    for f in range(n_fields):
        body = want[bases[f]:bases[f] + 4 * part * es].reshape(-1, es)
        for i, (side, src, dst) in enumerate(todo):
            body[src] = _typed(dtype, src.size, seed * 64 + f * 2 + i)
    view = buf[:total]
    view.copy_(torch.from_numpy(want))
    for f in range(n_fields):
        body = want[bases[f]:bases[f] + 4 * part * es].reshape(-1, es)
        parity = -1 if (mask >> f) & 1 else 1
        for side, src, dst in todo:
            layer = (h - 1 - j) if side == 0 else j
            x = body[src].copy()
            out = np.empty_like(x)
            for k in range(h):
                sel = layer == k
                out[sel] = WB.wall_cells(dtype, x[sel], parity, elems[f][side][k])
            body[dst] = out
    ptr = buf.data_ptr()
    assert ptr % 256 == 0
    fields = [ptr + b for b in bases]
    raw = _raw(dtype, elems)
    desc = cd.cudecompExtDescribeWallFieldMoves(moves, fields, dtype, raw, mask, force)
    n = cd.cudecompExtRunWallFieldMoves(moves, fields, dtype, raw, mask, force, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    what = (AB.NAMES[dtype], extent, strides, mirrored, n_fields, hex(mask), side_list, force, offsets, name)
    per = min(32, 2048 // (len(side_list) * h * es))
    assert n == len(desc) == -(-n_fields // per), what + (n, desc)
    assert name == spell(desc[-1], dtype) and len({(d["kind"], d["access"]) for d in desc}) == 1, what + (desc,)
    assert [d["first_field"] for d in desc] == list(range(0, n_fields, per)) and sum(d["fields"] for d in desc) == n_fields, what
    got = view.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, what + ("%d bytes differ, first at byte %d of the arena (fields begin at %s, regions of %d bytes)"
                                  % (bad.size, bad[0], bases[:4], region),)
    rows = name.startswith("rows_")
    if force & 1:
        assert not rows, what
    elif rows:  # (the reflection's rule: non-temporal from 32 MiB per field, or forced)
        streaming = bool(force & 2) or int(np.prod(extent)) * es >= (32 << 20)
        assert desc[0]["access"] == (1 if streaming else 0), what + (desc,)
    return name, desc


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130)
COMBINATIONS = list(itertools.product((2, 3, 9, 32), MASKS, (0, 1, 2), (1, 2)))  # fields x mask x force x sides


def _arena(dtype, cells_per_part):
    import torch
    es = AB.element_bytes(dtype)
    return torch.empty(SLACK + 32 * ((24 + 4 * (cells_per_part + 4)) * es + SLACK + 16), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows(dtype):
    """type x row length x row pitch (length + 0, + 3) x mirrored extent (1, 2, 3, 8) as the row index and as the plane index: the
    whole cross of geometries, each with one draw (a seeded shuffle, walked round) of field count {2, 3, 9, 32} x mask of signs (none,
    all, alternating, only field 0, only the last field) x fast path / forced element-wise / forced streaming x one / two sides (a
    single side alternately the low and the high one); all 120 combinations must have come up.  Base offsets: every phase of the
    16-byte grid and one past it, another one for every field -- for 2-byte types every second draw keeps all fields dword-aligned,
    the others put some at 2 mod 4.  Addends distinct per field, side and layer.  Kernel name and launch count on every case."""
    es = AB.element_bytes(dtype)
    buf = _arena(dtype, 133 * 8 * 3 + 133 * 3 * 8 + 64)
    rng = np.random.RandomState(300 + dtype)
    order = rng.permutation(len(COMBINATIONS))
    phases = 16 // es + 2
    seen, lanes, kernels, draw = set(), set(), set(), 0
    for length, extra, thick, where in itertools.product(LENGTHS, (0, 3), (1, 2, 3, 8), (1, 2)):
        pitch = length + extra
        rows, planes = (thick, 3) if where == 1 else (3, thick)
        extent, strides = (length, rows, planes), (1, pitch, pitch * rows + 5)  # (planes never continue one another)
        n, mask_kind, force, sides = COMBINATIONS[order[draw % len(order)]]
        draw += 1
        k = int(rng.randint(phases))
        aligned = es == 2 and draw % 2 == 0
        offsets = [2 * ((f + k) % 4) for f in range(n)] if aligned else [(f + k) % phases for f in range(n)]
        side_list = (0, 1) if sides == 2 else (draw & 1,)
        name, desc = _run(buf, dtype, extent, strides, where, n, mask_of(mask_kind, n), side_list, force, offsets, draw)
        seen.add((n, mask_kind, force, sides))
        kernels.add(name.split("<")[0])
        if length >= 2 and not force & 1:
            assert name.startswith("rows_fields_wall_kernel<"), (extent, strides, name)
        if name.startswith("rows_"):
            lanes.add(desc[0]["vec"])
            if es == 2 and not aligned:  # consecutive fields sit at consecutive phases: one of them is at 2 mod 4
                assert desc[0]["vec"] == 2, (extent, strides, offsets, desc)
            if (es >= 4 or (aligned and pitch % 2 == 0 and strides[2] % 2 == 0)) and extra != 0:  # (no fusion of rows: the row length decides)
                want = 16
                while want > es and (length * es) % want:
                    want //= 2
                assert desc[0]["vec"] == want, (extent, strides, desc)
    assert len(seen) == len(COMBINATIONS) == 120, sorted(set(COMBINATIONS) - seen)
    # (2-byte rows of 8 bytes modulo 16 do not occur among these lengths: 8-byte lanes are not asked of them)
    assert lanes >= ({2, 4, 16} if es == 2 else {v for v in (4, 8, 16) if v >= es}), lanes
    assert kernels == {"rows_fields_wall_kernel", "generic_fields_wall_kernel"}, kernels


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_mirrored_dim_fastest(dtype):
    """the mirrored dim as the fastest memory axis: rows of 1, 2, 3 and 8 elements, reversed in themselves, a row pitch apart -- the
    element-wise kernel by itself, whatever is forced"""
    es = AB.element_bytes(dtype)
    buf = _arena(dtype, 131 * 303 + 64)
    phases = 16 // es + 2
    c = 0
    for thick, (rows, planes), pitch, sides in itertools.product((1, 2, 3, 8), ((9, 7), (37, 3), (1, 40), (300, 1)), (9, 16, 131), (1, 2)):
        n = (2, 3, 9, 32)[c % 4]
        force = (0, 1, 2)[(c // 4) % 3]
        mask_kind = MASKS[(c // 12) % 5]
        c += 1
        if pitch * (rows + 3) * planes > 131 * 303:
            continue
        extent, strides = (thick, rows, planes), (1, pitch, pitch * (rows + 3))
        side_list = (0, 1) if sides == 2 else (c & 1,)
        name, _ = _run(buf, dtype, extent, strides, 0, n, mask_of(mask_kind, n), side_list, force, [(f + c) % phases for f in range(n)], c)
        if thick > 1 or rows == 1 or planes == 1 or force & 1:  # (one cell thick has no direction: long enough rows of cells may fuse)
            assert name.startswith("generic_fields_wall_kernel<"), (extent, strides, name)


def test_kernel_parity_second_grid_stride_pass():
    """the element-wise kernel launches at most 8192 workgroups of 256 lanes per field: more elements than that take a second pass"""
    import torch
    cells = 8192 * 256 + 257
    buf = torch.empty(SLACK + 2 * ((8 + 4 * (2 * cells + 8)) * 2 + 2 * SLACK), dtype=torch.uint8, device="cuda")
    name, desc = _run(buf, cd.HALF, (cells, 2, 1), (1, cells + 1, 0), 1, 2, 2, (0,), 1, [1, 4], 3)
    assert name.startswith("generic_fields_wall_kernel<") and desc[0]["blocks_per_field"] == 8192, (name, desc)


def test_kernel_parity_streaming_by_size():
    """32 MiB per field in one move: the size rule itself picks the non-temporal instantiation; 16 MiB stays cached"""
    import torch
    buf = torch.empty(SLACK + 2 * (4 * ((32 << 20) + 4096) + 2 * SLACK), dtype=torch.uint8, device="cuda")
    extent, strides = (2048, 1024, 2), (1, 2048, 2048 * 1024)
    assert _run(buf, cd.DOUBLE, extent, strides, 2, 2, 1, (1,), 0, [0, 1], 5)[0] == "rows_fields_wall_kernel<double,16,1>"
    assert _run(buf, cd.FLOAT, extent, strides, 2, 2, 2, (0,), 0, [0, 4], 6)[0] == "rows_fields_wall_kernel<float,16,0>"


# ---- a split call ------------------------------------------------------------------------------------------------------------
def test_a_call_split_into_four_launches():
    """32 complex128 fields, h = 8, both sides, on a pencil 13 cells along the dim: F = 2048 / (2 * 8 * 16) = 8 fields per launch,
    four launches; field 8, 9, 31 ... each gets its own addends and its own parity (every field against its single call)"""
    cases = [[axis, (8, 1, 1), (0, 1, 1), (0, 0, 0), cd.DOUBLE_COMPLEX, 0, 3, 32] for axis in range(3)]
    cases += [[0, (8, 1, 1), (0, 1, 1), (1, 0, 0), cd.DOUBLE_COMPLEX, 0, sides, 19] for sides in (1, 2)]  # one side: 16 per launch
    for order in ((0, 1, 2), (2, 1, 0)):
        args = {"gdims": (13, 6, 5), "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases, "must_launch": True}
        assert FB.fields_sweep(0, 1, args) == []
    assert FB.launches_expected(32, 2, 8, 16) == 4 and FB.launches_expected(19, 1, 8, 16) == 2


# ---- edge values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [cd.HALF, cd.BFLOAT16, cd.FLOAT, cd.DOUBLE], ids=["fp16", "bf16", "fp32", "fp64"])
def test_edge_values(dtype):
    """every pair (mirror, addend) of AB.edge_table -- zeros, subnormals, the largest finite numbers, infinities, NaNs -- in both
    parities through both kernels, the field in the LAST slot of a three-field launch: 24 mirrors along a row, one addend per
    launch.  Where the expected real is a NaN any NaN of the type will do; every other real bit for bit.  The two fields in front
    carry ordinary numbers and other addends."""
    import torch
    kind = AB.kind_of(dtype)
    u, es = AB.FORMATS[kind][0], AB.element_bytes(dtype)
    table = AB.edge_table(kind)
    n = len(table)
    stream = torch.cuda.current_stream().cuda_stream
    pitch = 2 * n * es + SLACK  # a field: [sources | destinations | slack]
    host = np.full(3 * pitch, POISON, dtype=np.uint8)
    for f in range(3):
        host[f * pitch:f * pitch + n * es] = np.ascontiguousarray(table if f == 2 else np.roll(table, 3 + f)[::-1]).view(np.uint8)
    dev = torch.from_numpy(host.copy()).cuda()
    fields = [dev.data_ptr() + f * pitch for f in range(3)]
    move = cd.make_move((n, 1, 1), (1, -2 * n, 0), (1, 2 * n, 0), src_off=0, dst_off=n, src_buf=0, dst_buf=0)
    move.peer = 1
    others = [table[20], table[21]]  # (1.5 and -2.75)
    for negate, force in itertools.product((False, True), (0, 1)):
        for addend in table:
            dev.copy_(torch.from_numpy(host))
            elems = [[[], [np.array([a], dtype=u).tobytes()]] for a in (others[0], others[1], addend)]
            launches = cd.cudecompExtRunWallFieldMoves([move], fields, dtype, _raw(dtype, elems), 4 if negate else 0, force, stream)
            torch.cuda.synchronize()
            assert launches == 1 and cd.cudecompExtLastKernelName().startswith("generic_fields_wall" if force else "rows_fields_wall")
            got = dev.cpu().numpy()
            for f, (a, flipped) in enumerate(zip((others[0], others[1], addend), (False, False, negate))):
                src = host[f * pitch:f * pitch + n * es].view(u)
                mirror = src ^ u(1 << (8 * es - 1)) if flipped else src
                want = AB.bits_of(dtype, AB.typed_add(dtype, mirror.astype(u), np.full(n, a, dtype=u)))
                mine = got[f * pitch + n * es:f * pitch + 2 * n * es].view(u)
                bad = AB.mismatches(kind, mine, want)
                assert not bad.any(), (AB.NAMES[dtype], f, negate, force, hex(int(addend)), [hex(int(x)) for x in src[bad]],
                                       [hex(int(x)) for x in mine[bad]], [hex(int(x)) for x in want[bad]])
                assert np.array_equal(got[f * pitch:f * pitch + n * es], host[f * pitch:f * pitch + n * es])  # the sources stay
                assert np.all(got[f * pitch + 2 * n * es:(f + 1) * pitch] == POISON)  # ... and so does the slack


# ---- single-rank pencils ---------------------------------------------------------------------------------------------------
SHAPES = {"13x10x11": (13, 10, 11), "5x6x7": (5, 6, 7)}
PERMS = list(itertools.permutations((0, 1, 2)))
HALOS = [(1, 1, 1), (2, 1, 3), (3, 3, 3)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
PERIODS = list(itertools.product((0, 1), repeat=3))


def _admitted(gdims, halo, periods, centering):
    """the refusal rule: h + centering <= interior along every non-periodic dim that has a halo"""
    return all(periods[d] or halo[d] == 0 or halo[d] + centering <= gdims[d] for d in range(3))


@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("order", PERMS, ids=["".join(map(str, o)) for o in PERMS])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_rank_pencils(shape, order, axis):
    """the halo sets, paddings, period mixes, centerings and `sides` of tests/test_gpu_halo_wall_values.py; 3 and 5 fields with mixed
    parities, the seven data types in turn: each field byte-identical to the single call on a clone, the launches by the rule"""
    cases = []
    for halo, padding, periods, centering, sides in itertools.product(HALOS, PADDINGS, PERIODS, (0, 1), (1, 2, 3)):
        if _admitted(SHAPES[shape], halo, periods, centering):
            cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], centering, sides, (3, 5)[(len(cases) // 7) % 2]])
    assert len(cases) == 288 and len({(c[4], c[7]) for c in cases}) == 14
    args = {"gdims": SHAPES[shape], "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases, "must_launch": True}
    assert FB.fields_sweep(0, 1, args) == []


def test_the_widest_halo():
    """h = 8 along the 13-cell dim, as the fastest, the middle and the slowest memory axis; every type; 2, 3 and 9 fields"""
    cases = [[axis, (8, 1, 1), (0, 1, 0), (1, 0, 0), dtype, 0, 3, n] for axis in range(3)
             for dtype, n in zip(AB.ALL_TYPES, itertools.cycle((2, 3, 9)))]
    for order in ((0, 1, 2), (1, 0, 2), (2, 1, 0)):
        args = {"gdims": (13, 10, 11), "pdims": (1, 1), "mem_order": (order,) * 3, "cases": cases, "must_launch": True}
        assert FB.fields_sweep(0, 1, args) == []


def test_one_field_is_the_single_call():
    """n_fields == 1: the single call's kernels (the sweep checks the name) and launches, its bytes"""
    cases = [[axis, (2, 1, 3), (0, 1, 0), (0, 1, 0), dtype, centering, sides, 1]
             for axis, (dtype, centering, sides) in itertools.product(range(3), ((cd.DOUBLE, 0, 3), (cd.HALF, 1, 1), (cd.FLOAT_COMPLEX, 0, 2)))]
    assert FB.fields_sweep(0, 1, {"gdims": (13, 10, 11), "pdims": (1, 1), "cases": cases, "must_launch": True}) == []


# ---- four ranks sharing the GPU --------------------------------------------------------------------------------------------
def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (10, 9, 11): slabs of 5 + 5, 5 + 4 and 6 + 5 cells, every rank an edge rank along the split dims.
    Non-periodic and mixed periods; 3 and 5 fields; every field of every rank against the single call on a clone; a rank launches
    exactly where it owns a wall that `sides` names (the launch rule counts the sides it writes)"""
    cases = []
    for periods, axis, (halo, padding), centering, sides in itertools.product(
            ((0, 0, 0), (1, 0, 1), (0, 1, 0)), range(3), (((1, 2, 1), (0, 0, 0)), ((3, 1, 2), (1, 0, 2))), (0, 1), (3, 1, 2)):
        cases.append([axis, halo, periods, padding, AB.ALL_TYPES[len(cases) % 7], centering, sides, (3, 5)[len(cases) % 2]])
    args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "cases": cases, "must_launch": True}
    for failures in run_ranks(4, "tests.wall_value_fields_bodies", "fields_sweep", args, timeout=300, fresh=False):
        assert failures == []


# ---- hipGraph, asynchrony --------------------------------------------------------------------------------------------------
def test_captured_calls_replay_with_the_captured_lists():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 0, 1), "padding": (0, 1, 0), "n_fields": 3},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ((1, 2, 0),) * 3, "axis": 1, "halo": (2, 1, 2),
                  "periods": (0, 0, 0), "dtype": cd.HALF_COMPLEX, "centering": 1, "n_fields": 5}):
        assert run_ranks(1, "tests.wall_value_fields_bodies", "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (0, 0, 0)}
    res = run_ranks(1, "tests.wall_value_fields_bodies", "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["wall_host_ms"] < 0.25 * res["total_ms"], res
