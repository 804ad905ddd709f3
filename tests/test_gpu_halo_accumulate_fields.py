"""Multi-field halo accumulation (cudecomp_halo_accumulate_fields.h: cudecompAmdAccumulateFieldHalos{X,Y,Z}) on the GPU: the adding and
taking field-move kernels against torch index arithmetic on small integers (every byte of every field buffer and of the workspace,
with slack around each); single-rank pencils of every axis, memory order, halo width, period mix, padding and dim against single
accumulations on clones, ordered plans among them; the workspace bound; ranks sharing the GPU over every halo transport the other
multi-rank halo tests drive here; the adjoint identity with the multi-field update; capture into a hipGraph; the number of
launches.  Everything is compared byte for byte: there is no tolerance anywhere."""
import itertools
import os

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import accumulate_fields_bodies as FB
from tests.mp import run_ranks
from tests.test_halo_accumulate_fields_plan import ADD, ADD_TAKE, ES, NC, TAKE, spell

pytestmark = pytest.mark.gpu

SLACK = 256  # bytes between any two buffers (and before the first, after the last) that no move may touch
SELF = {"CUDECOMP_TEST_SELF_EXCHANGE": "1"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "libfake_rccl.so")
# operation -> (mode, where the source lies, where the destination lies)
ADD_WORK_TO_FIELD, ADD_FIELD_TO_FIELD, TAKE_FIELD_TO_WORK, ADD_TAKE_FIELD_TO_FIELD = range(4)
OPS = {ADD_WORK_TO_FIELD: (ADD, "work", "field"), ADD_FIELD_TO_FIELD: (ADD, "field", "field"),
       TAKE_FIELD_TO_WORK: (TAKE, "field", "work"), ADD_TAKE_FIELD_TO_FIELD: (ADD_TAKE, "field", "field")}


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
    """One device buffer that holds every field buffer and the workspace of a case: integers of [lo, 8] in every real of `dtype`,
    exact in all seven types, sums of two included.  A case copies the pristine values in, runs its launch and compares EVERY byte
    with what torch index arithmetic on the pristine values gives: dst = src or dst = dst + src, then zero into the source cells."""

    def __init__(self, dtype, nbytes, lo=-8):
        import torch
        self.dtype, self.es, self.nc, self.rb = dtype, ES[dtype], NC[dtype], ES[dtype] // NC[dtype]
        g = torch.Generator(device="cuda")
        g.manual_seed(1234)
        nbytes += -nbytes % 16
        self.init = torch.randint(lo, 9, (nbytes // self.rb,), device="cuda", generator=g).to(_torch_real(dtype))
        self.buf = torch.empty_like(self.init)

    def run(self, extent, pitch_strides, n_fields, op, sides, force, offsets, work_offset, shifts=(0, 0)):
        """`sides` moves of the geometry (extent, pencil strides `pitch_strides`; dense in the workspace) for n_fields fields whose
        bases lie offsets[f] elements into their regions, the workspace work_offset elements into its own; shifts[s]: elements side
        s lies further into the pencils.  Returns (kernel name, description, source cells as element numbers of the arena)."""
        import torch
        es, nc, rb = self.es, self.nc, self.rb
        mode, src_at, dst_at = OPS[op]
        dev = self.buf.device
        face = int(extent[0]) * int(extent[1]) * int(extent[2])
        span = _span(extent, pitch_strides) + max(shifts)
        # a field's region: [side 0 source | side 0 destination | side 1 source | side 1 destination], each `part` apart
        part = span + 3 + (span + 3) % 2  # (even: the 2-byte cases decide their alignment by the fields' offsets alone)
        region = (max(offsets) + 4 * part) * es + SLACK
        region += -region % 16
        slot = face * n_fields + 6  # elements between the two sides' pieces of the workspace
        work_bytes = (work_offset + 2 * slot) * es + SLACK
        work_bytes += -work_bytes % 16
        total = SLACK + n_fields * region + work_bytes
        assert total <= self.buf.numel() * rb, (total, self.buf.numel() * rb)
        buf, init = self.buf[:total // rb], self.init[:total // rb]
        self.last_elements = total // es
        buf.copy_(init)
        bases = [SLACK + f * region + offsets[f] * es for f in range(n_fields)]  # bytes from the start of the arena
        work = SLACK + n_fields * region + work_offset * es
        expected = init.clone()
        E, I = expected.view(-1, nc), init.view(-1, nc)
        base_el = torch.tensor([b // es for b in bases], dtype=torch.int64, device=dev)[:, None]
        f_el = torch.arange(n_fields, dtype=torch.int64, device=dev)[:, None]
        dense = (1, int(extent[0]), int(extent[0]) * int(extent[1]))
        kp, kd = _cells(extent, pitch_strides, dev)[None, :], _cells(extent, dense, dev)[None, :]
        moves, sources = [], []
        for s in range(sides):
            src_pencil, dst_pencil = (2 * s) * part + shifts[s], (2 * s + 1) * part + shifts[s]
            in_work = work // es + s * slot + f_el * face + kd
            if src_at == "work":
                m = cd.make_move(extent, dense, pitch_strides, src_off=s * slot, dst_off=dst_pencil, src_buf=2, dst_buf=0)
                src, dst = in_work, base_el + dst_pencil + kp
            elif dst_at == "work":
                m = cd.make_move(extent, pitch_strides, dense, src_off=src_pencil, dst_off=s * slot, src_buf=0, dst_buf=2)
                src, dst = base_el + src_pencil + kp, in_work
            else:
                m = cd.make_move(extent, pitch_strides, pitch_strides, src_off=src_pencil, dst_off=dst_pencil, src_buf=0, dst_buf=1)
                src, dst = base_el + src_pencil + kp, base_el + dst_pencil + kp
            moves.append(m)
            src, dst = src.reshape(-1), dst.reshape(-1)
            E[dst] = I[dst] + I[src] if mode in (ADD, ADD_TAKE) else I[src]
            if mode in (TAKE, ADD_TAKE):
                E[src] = 0
            sources.append(src)
        ptr = buf.data_ptr()
        assert ptr % 256 == 0
        fields = [ptr + b for b in bases]
        desc = cd.cudecompExtDescribeFieldMovesOp(moves, fields, ptr + work, face, es, mode, self.dtype, force)
        n = cd.cudecompExtRunFieldMovesOp(moves, fields, ptr + work, face, es, mode, self.dtype, force, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        name = cd.cudecompExtLastKernelName()
        what = (self.dtype, extent, pitch_strides, n_fields, op, sides, force, offsets, work_offset, shifts, name)
        assert n == 1 and name == spell(desc, es, self.dtype), what + (desc,)
        assert desc["blocks"] == n_fields * desc["blocks_per_field"], what + (desc,)
        got, want = buf.view(torch.uint8), expected.view(torch.uint8)
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).reshape(-1)
            raise AssertionError(what + ("%d bytes differ, first at byte %d of the arena (fields begin at %s, the workspace at %d)"
                                         % (bad.numel(), int(bad[0]), bases[:4], work),))
        rows = name.startswith("rows_")
        if force & 1:
            assert not rows, what
        elif rows:
            assert desc["access"] == (1 if force & 2 else 0), what + (desc,)
        return name, desc, torch.cat(sources)


LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130, 1025)
COMBINATIONS = list(itertools.product((2, 3, 9, 32), range(4), (1, 2), (0, 1, 2)))  # fields x operation x sides x force


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows(dtype):
    """type (four element sizes) x row length x row pitch (length + 0, 1, 3: rows fused, rows at alternating phases, odd) x rows x
    planes: the whole cross of geometries, each with three draws (a seeded shuffle, walked round) of field count {2, 3, 9, 32} x
    operation (add workspace -> field, add field -> field, take field -> workspace, add-take field -> field) x one / two sides x
    fast path / forced element-wise / forced streaming; all 96 combinations must have come up.  Base offsets 0 .. 16 / es + 1
    elements, another one for every field (field f: (f + k) mod (16 / es + 2)) and for the workspace."""
    es = ES[dtype]
    arena = _Arena(dtype, SLACK + 32 * ((12 + 4 * (1028 * 37 * 3 + 20)) * es + 2 * SLACK) + (2 * (1025 * 37 * 3 * 32 + 8) + 12) * es + 2 * SLACK)
    rng = np.random.RandomState(100 + dtype)
    order = rng.permutation(len(COMBINATIONS))
    phases = 16 // es + 2
    seen, lanes, kernels, draw = set(), set(), set(), 0
    for length, extra, rows, planes in itertools.product(LENGTHS, (0, 1, 3), (1, 5, 37), (1, 3)):
        pitch = length + extra
        extent, strides = (length, rows, planes), (1, pitch, pitch * rows + 5)  # (planes never continue one another)
        for _ in range(3):
            n, op, sides, force = COMBINATIONS[order[draw % len(order)]]
            draw += 1
            k = int(rng.randint(phases))
            offsets = [(f + k) % phases for f in range(n)]
            name, desc, _ = arena.run(extent, strides, n, op, sides, force, offsets, int(rng.randint(phases)))
            seen.add((n, op, sides, force))
            kernels.add(name.split("<")[0])
            mode = OPS[op][0]
            assert desc["kind"] in {ADD: (25, 26), TAKE: (27, 28), ADD_TAKE: (29, 30)}[mode], (name, desc)
            if length >= 2 and not force & 1:
                assert name.startswith("rows_fields_"), (extent, strides, name)
            if name.startswith("rows_"):
                lanes.add(desc["vec"])
                if es == 2 and n >= 2:  # consecutive fields sit at consecutive phases: one of them is at 2 mod 4
                    assert desc["vec"] == 2, (extent, strides, offsets, desc)
                if es >= 4 and extra != 0 and OPS[op][1:] == ("field", "field"):  # (no fusion of rows: the row length decides)
                    want = 16
                    while want > es and (length * es) % want:
                        want //= 2
                    assert desc["vec"] == want, (extent, strides, desc)
    assert len(seen) == len(COMBINATIONS) == 96, sorted(set(COMBINATIONS) - seen)
    assert lanes == ({2} if es == 2 else {v for v in (4, 8, 16) if v >= es}), lanes
    assert kernels == {"rows_fields_accumulate_kernel", "rows_fields_take_kernel", "generic_fields_accumulate_kernel",
                       "generic_fields_take_kernel"}, kernels


@pytest.mark.parametrize("dtype", [cd.HALF, cd.BFLOAT16], ids=["fp16", "bf16"])
def test_kernel_parity_two_byte_lanes_follow_every_field(dtype):
    """2-byte elements: all bases dword-aligned and even strides -> 16-byte lanes; ONE field of nine at 2 mod 4 -> 2-byte lanes for
    the whole launch; both compared byte for byte"""
    arena = _Arena(dtype, 1 << 22)
    extent, strides = (64, 5, 3), (1, 66, 66 * 5 + 6)
    for op in OPS:
        name, desc, _ = arena.run(extent, strides, 9, op, 2, 0, [0, 2, 4, 6, 8, 0, 2, 4, 6], 2)
        assert (name.startswith("rows_fields_"), desc["vec"]) == (True, 16), (op, name)
        name, desc, _ = arena.run(extent, strides, 9, op, 2, 0, [0, 2, 4, 6, 8, 0, 3, 4, 6], 2)
        assert (name.startswith("rows_fields_"), desc["vec"]) == (True, 2), (op, name)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_faces_one_element_thick(dtype):
    """the face along the fastest memory axis: extent (1, h, d), cells a row pitch apart -- the element-wise kernels by themselves"""
    es = ES[dtype]
    arena = _Arena(dtype, max(es, 4) << 23)
    phases = 16 // es + 2
    c = 0
    for (h, d), pitch, op, sides in itertools.product(((9, 7), (37, 3), (1, 40), (300, 1)), (3, 16, 131), OPS, (1, 2)):
        n = (2, 3, 9, 32)[c % 4]
        force = (0, 1, 2)[(c // 4) % 3]
        c += 1
        extent, strides = (1, h, d), (1, pitch, pitch * (h + 3))
        name, _, _ = arena.run(extent, strides, n, op, sides, force, [(f + c) % phases for f in range(n)], c % phases)
        assert name.startswith("generic_fields_take_kernel<" if OPS[op][0] == TAKE else "generic_fields_accumulate_kernel<"), (extent, strides, name)
    # two cells per row along the fastest axis (halo 2): rows again
    name, _, _ = arena.run((2, 9, 7), (1, 13, 13 * 11), 3, ADD_WORK_TO_FIELD, 2, 0, [0, 1, 2], 0)
    assert name.startswith("rows_fields_accumulate_kernel<")


def test_kernel_parity_second_grid_stride_pass():
    """the element-wise kernels launch at most 8192 workgroups of 256 lanes per field: more elements than that take a second pass"""
    arena = _Arena(cd.HALF, SLACK + 2 * ((4 * (8192 * 256 + 260) + 8) * 2 + 2 * SLACK) + (2 * (2 * (8192 * 256 + 257) + 8) + 8) * 2 + 2 * SLACK)
    for op in OPS:
        name, desc, _ = arena.run((8192 * 256 + 257, 1, 1), (1, 0, 0), 2, op, 1, 1, [1, 4], 3)
        assert name.startswith("generic_fields_") and desc["blocks_per_field"] == 8192, (name, desc)


@pytest.mark.parametrize("dtype", [cd.HALF, cd.FLOAT, cd.DOUBLE, cd.DOUBLE_COMPLEX], ids=["fp16", "fp32", "fp64", "complex128"])
def test_after_a_take_exactly_the_source_cells_are_zero(dtype):
    """a payload without a zero (integers 1 .. 8) and the plain take, which makes no sums: afterwards the zero bytes of the arena
    are exactly the source cells of the moves -- their neighbours in the rows' gaps, between the planes and around the fields are
    not"""
    import torch
    arena = _Arena(dtype, 1 << 22, lo=1)
    for extent, strides, force in (((7, 5, 3), (1, 9, 9 * 5 + 5), 0), ((33, 5, 3), (1, 36, 36 * 5 + 5), 2), ((1, 9, 7), (1, 13, 13 * 12), 0),
                                   ((9, 5, 3), (1, 12, 12 * 5 + 7), 1)):
        name, _, sources = arena.run(extent, strides, 3, TAKE_FIELD_TO_WORK, 2, force, [0, 1, 2], 1)
        used = arena.buf.view(-1, arena.nc)[:arena.last_elements]  # fields, workspace and the slack around them
        zero = torch.zeros(used.shape[0], dtype=torch.bool, device="cuda")
        zero[sources] = True
        is_zero = (used.view(torch.uint8) == 0).all(dim=1)
        assert is_zero.shape == zero.shape and torch.equal(is_zero, zero), (extent, strides, name)
        assert int(zero.sum()) == 2 * 3 * int(np.prod(extent))


# ---- single-rank pencils ---------------------------------------------------------------------------------------------------
GDIMS = (11, 9, 7)
ORDERS = {"default": None, "contiguous": ((0, 1, 2), (1, 2, 0), (2, 0, 1)), "mixed": ((1, 0, 2), (2, 1, 0), (0, 2, 1))}
HALOS = [(1, 1, 1), (2, 0, 3), (3, 2, 1)]
PERIODS = [(1, 1, 1), (1, 0, 1), (0, 0, 0)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
OTHER_TYPES = [t for t in AB.ALL_TYPES if t not in (cd.DOUBLE, cd.HALF)]
LAUNCHES = {"self": 1, "packed": 2}  # (one more where the plan is ordered: FB.fields_sweep)


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("halo", HALOS, ids=["h111", "h203", "h321"])
def test_single_rank_full_cross_fp64_fp16(layout, halo):
    """every axis, period mix, padding and dim, 2, 3 and 9 fields, clear 0 and 1; dims 2, 1, 0 in sequence as well (edges and
    corners); whole buffers against single calls on clones; a self-periodic fields call is ONE data-movement launch"""
    for periods, padding in itertools.product(PERIODS, PADDINGS):
        args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
                "dtypes": [cd.DOUBLE, cd.HALF], "n_fields": [2, 3, 9], "all_dims": True, "launches": LAUNCHES}
        assert FB.fields_sweep(0, 1, args) == []


@pytest.mark.parametrize("layout,halo,periods,padding", [("default", (3, 2, 1), (1, 1, 1), (1, 2, 0)), ("contiguous", (1, 1, 1), (1, 0, 1), (0, 0, 0)),
                                                         ("mixed", (2, 0, 3), (1, 1, 1), (1, 2, 0))], ids=["default", "contiguous", "mixed"])
def test_single_rank_other_types(layout, halo, periods, padding):
    args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
            "dtypes": OTHER_TYPES, "n_fields": [2, 3, 9], "all_dims": True, "launches": LAUNCHES}
    assert FB.fields_sweep(0, 1, args) == []


def test_single_rank_ordered_self_periodic():
    """halo 3 on an extent of 5: halo <= interior < 2 x halo, the two faces overlap in one cell -- one launch per side, low side
    first, and the bits of the single call (every sum of the bit arm rounds, so the order shows)"""
    for layout in ORDERS:
        args = {"gdims": (5, 9, 7), "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": (3, 1, 1), "periods": (1, 1, 1), "padding": (0, 1, 0),
                "dtypes": [cd.DOUBLE, cd.HALF, cd.BFLOAT16], "n_fields": [2, 9], "all_dims": True, "launches": LAUNCHES, "expect_ordered": True}
        assert FB.fields_sweep(0, 1, args) == []


def test_one_field_is_the_single_call():
    args = {"gdims": GDIMS, "pdims": (1, 1), "halo": (2, 1, 1), "periods": (1, 1, 1), "padding": (0, 1, 0), "dtypes": [cd.DOUBLE, cd.HALF]}
    assert FB.one_field_is_the_single_call(0, 1, args) == []


def test_adjoint_of_the_multi_field_update():
    args = {"gdims": (12, 10, 9), "pdims": (1, 1), "halo": (2, 1, 3), "periods": (1, 1, 1), "padding": (1, 0, 2), "n": 3}
    assert FB.adjoint(0, 1, args) == []


# ---- ranks sharing the GPU -------------------------------------------------------------------------------------------------
def _jobs(pdims, backend, gdims=(10, 9, 11), guard=False, **more):
    jobs = []
    for periods, halo, padding in (((1, 1, 1), (1, 2, 1), (0, 0, 0)), ((0, 0, 0), (2, 1, 2), (1, 0, 2)), ((1, 0, 1), (1, 1, 3), (0, 0, 0))):
        args = dict({"gdims": gdims, "pdims": pdims, "halo_backend": backend, "halo": halo, "periods": periods, "padding": padding,
                     "dtypes": [cd.DOUBLE, cd.HALF], "n_fields": [3], "all_dims": True, "guard": guard,
                     "expect_kernels": any(periods) or tuple(pdims) != (1, 1)}, **more)  # (one rank without a period has no neighbour at all)
        jobs.append({"fn": "fields_sweep", "id": "hb%d P%dx%d periods %s halo %s" % ((backend,) + tuple(pdims) + (periods, halo)), "args": args})
    return jobs


@pytest.mark.parametrize("nranks,pdims", [(2, (2, 1)), (4, (2, 2))], ids=["two_ranks", "four_ranks_ragged"])
@pytest.mark.parametrize("backend", [cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM], ids=["MPI", "NVSHMEM"])
def test_ranks_peer_transports(nranks, pdims, backend):
    for failures in run_ranks(nranks, "tests.accumulate_fields_bodies", "many", {"jobs": _jobs(pdims, backend)}, timeout=300):
        assert failures == []


def test_two_ranks_ordered():
    """a dim of 9 split over two ranks: slabs of 5 and 4 with halo 3 -- both ranks add low side first, one launch per side"""
    args = {"gdims": (7, 9, 7), "pdims": (2, 1), "halo_backend": cd.HALO_COMM_MPI, "halo": (1, 3, 1), "periods": (1, 1, 1),
            "dtypes": [cd.DOUBLE, cd.HALF], "n_fields": [3], "axes": [0], "all_dims": True, "expect_ordered": True, "expect_kernels": True}
    for failures in run_ranks(2, "tests.accumulate_fields_bodies", "fields_sweep", args, timeout=300):
        assert failures == []


@pytest.mark.parametrize("nranks,pdims", [(2, (2, 1)), (4, (2, 2))], ids=["two_ranks", "four_ranks_ragged"])
def test_ranks_rccl_stand_in(nranks, pdims):
    """NCCL enum; the workspace holds exactly 3 x the queried size inside a poisoned buffer; pack and addition: two launches"""
    if not os.path.exists(SHIM):
        pytest.skip("tests/shim/libfake_rccl.so not built")
    mem_order = ORDERS["contiguous"] if nranks == 2 else None
    jobs = _jobs(pdims, cd.HALO_COMM_NCCL, guard=True, launches=LAUNCHES, mem_order=mem_order)
    for failures in run_ranks(nranks, "tests.accumulate_fields_bodies", "many", {"jobs": jobs}, timeout=300, extra_env={"CUDECOMP_TEST_RCCL_SHIM": SHIM}):
        assert failures == []


def test_one_rank_real_rccl_and_one_sided_with_a_single_member():
    """CUDECOMP_TEST_SELF_EXCHANGE=1: the rank is its own neighbour but packs, exchanges (real librccl; the one-sided transport) and
    adds: two data-movement launches per call; over librccl with the workspace at exactly its size"""
    jobs = []
    for backend in (cd.HALO_COMM_NCCL, cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM):
        jobs += _jobs((1, 1), backend, guard=backend == cd.HALO_COMM_NCCL, mem_order=ORDERS["contiguous"], n_fields=[3, 9], self_exchange=True,
                      launches=LAUNCHES if backend == cd.HALO_COMM_NCCL else None)
    # ... and an ordered plan that travels: three launches
    jobs.append({"fn": "fields_sweep", "id": "ordered", "args": {
        "gdims": (5, 9, 7), "pdims": (1, 1), "halo_backend": cd.HALO_COMM_NCCL, "halo": (3, 1, 1), "periods": (1, 1, 1), "dtypes": [cd.DOUBLE],
        "n_fields": [3], "self_exchange": True, "launches": LAUNCHES, "expect_ordered": True, "expect_kernels": True, "guard": True}})
    for failures in run_ranks(1, "tests.accumulate_fields_bodies", "many", {"jobs": jobs}, timeout=300, extra_env=SELF):
        assert failures == []


# ---- hipGraph --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clear", [0, 1])
def test_captured_call_replays_on_refilled_fields(clear):
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 1, 1), "padding": (0, 1, 0), "dim": 1},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "axis": 1, "dim": 1, "halo": (2, 1, 2),
                  "periods": (1, 1, 1), "dtype": cd.HALF}):
        assert run_ranks(1, "tests.accumulate_fields_bodies", "graph_replay", dict(args, clear=clear), timeout=300)[0] == []


@pytest.mark.parametrize("clear", [0, 1])
def test_captured_call_one_sided_self_exchange(clear):
    args = {"gdims": (40, 36, 30), "pdims": (1, 1), "halo_backend": cd.HALO_COMM_NVSHMEM, "halo": (1, 2, 1), "periods": (1, 1, 1), "dim": 2,
            "clear": clear}
    assert run_ranks(1, "tests.accumulate_fields_bodies", "graph_replay", args, timeout=300, extra_env=SELF)[0] == []
