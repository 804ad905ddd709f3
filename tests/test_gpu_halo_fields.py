"""Multi-field halo updates (cudecomp_halo_fields.h: cudecompAmdUpdateFieldHalos{X,Y,Z}) on the GPU: the field-move kernels
against numpy-style index arithmetic (every byte of every field buffer and of the workspace, with slack around each); single-rank
pencils of every axis, memory order, halo width, period mix, padding and dim against single cudecompUpdateHalos calls on clones;
the workspace bound; ranks sharing the GPU over every halo transport the other multi-rank halo tests drive here; capture into a
hipGraph; the number of launches.  Everything is compared byte for byte: there is no tolerance anywhere."""
import itertools
import os

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fields_bodies as FB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = 256  # bytes between any two buffers (and before the first, after the last) that no move may touch
SELF = {"CUDECOMP_TEST_SELF_EXCHANGE": "1"}
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "libfake_rccl.so")
FIELD_TO_WORK, WORK_TO_FIELD, FIELD_TO_FIELD = 0, 1, 2


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
def _cells(extent, strides, device):
    import torch
    k = [torch.arange(int(e), dtype=torch.int64, device=device) * int(s) for e, s in zip(extent, strides)]
    return (k[0][:, None, None] + k[1][None, :, None] + k[2][None, None, :]).reshape(-1)


def _span(extent, strides):
    return sum((int(e) - 1) * int(s) for e, s in zip(extent, strides)) + 1


def _spell(d, es):
    return "rows_fields_kernel<%d,%d>" % (d["vec"], d["access"]) if d["kind"] == 22 else "generic_fields_kernel<%d>" % es


class _Arena:
    """One device buffer that holds every field buffer and the workspace of a case, random bytes throughout; a case copies the
    pristine bytes in, runs its launch and compares EVERY byte with what index arithmetic on the pristine bytes gives."""

    def __init__(self, nbytes):
        import torch
        g = torch.Generator(device="cuda")
        g.manual_seed(1234)
        self.init = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
        self.buf = torch.empty_like(self.init)

    def run(self, es, extent, pitch_strides, n_fields, direction, sides, force, offsets, work_offset, expect_rows=None, shifts=(0, 0)):
        """`sides` moves of the geometry (extent, pencil strides `pitch_strides`; dense in the workspace) for n_fields fields whose
        bases lie offsets[f] elements into their regions, the workspace work_offset elements into its own.  A geometry PER SIDE: lists
        of `sides` extents and strides; shifts[s]: elements side s lies further into the pencils.  Returns the kernel."""
        import torch
        dev = self.buf.device
        extents = list(extent) if isinstance(extent[0], (tuple, list)) else [extent] * sides
        strides = list(pitch_strides) if isinstance(pitch_strides[0], (tuple, list)) else [pitch_strides] * sides
        assert len(extents) == len(strides) == sides
        face = max(int(e[0]) * int(e[1]) * int(e[2]) for e in extents)  # between the fields' pieces of the workspace
        span = max(_span(e, st) for e, st in zip(extents, strides)) + max(shifts)
        # a field's region: [side 0 source | side 0 destination | side 1 source | side 1 destination], each `span + 3` apart
        part = span + 3 + (span + 3) % 2  # (even: the 2-byte cases decide their alignment by the fields' offsets alone)
        region = (max(offsets) + 4 * part) * es + SLACK
        region += -region % 16
        slot = face * n_fields + 6  # elements between the two sides' pieces of the workspace
        work_bytes = (work_offset + 2 * slot) * es + SLACK
        work_bytes += -work_bytes % 16
        total = SLACK + n_fields * region + work_bytes
        assert total <= self.buf.numel(), (total, self.buf.numel())
        buf, init = self.buf[:total], self.init[:total]
        buf.copy_(init)
        bases = [SLACK + f * region + offsets[f] * es for f in range(n_fields)]          # bytes from the start of the arena
        work = SLACK + n_fields * region + work_offset * es
        moves = []
        expected = init.clone()
        E, I = expected.view(-1, es), init.view(-1, es)
        base_el = torch.tensor([b // es for b in bases], dtype=torch.int64, device=dev)[:, None]
        f_el = torch.arange(n_fields, dtype=torch.int64, device=dev)[:, None]
        for s in range(sides):
            extent, pitch_strides = extents[s], strides[s]
            dense = (1, int(extent[0]), int(extent[0]) * int(extent[1]))
            kp, kd = _cells(extent, pitch_strides, dev)[None, :], _cells(extent, dense, dev)[None, :]
            src_pencil, dst_pencil = (2 * s) * part + shifts[s], (2 * s + 1) * part + shifts[s]
            if direction == FIELD_TO_WORK:
                m = cd.make_move(extent, pitch_strides, dense, src_off=src_pencil, dst_off=s * slot, src_buf=0, dst_buf=2)
                src, dst = base_el + src_pencil + kp, work // es + s * slot + f_el * face + kd
            elif direction == WORK_TO_FIELD:
                m = cd.make_move(extent, dense, pitch_strides, src_off=s * slot, dst_off=dst_pencil, src_buf=2, dst_buf=0)
                src, dst = work // es + s * slot + f_el * face + kd, base_el + dst_pencil + kp
            else:
                m = cd.make_move(extent, pitch_strides, pitch_strides, src_off=src_pencil, dst_off=dst_pencil, src_buf=0, dst_buf=1)
                src, dst = base_el + src_pencil + kp, base_el + dst_pencil + kp
            moves.append(m)
            E[dst.reshape(-1)] = I[src.reshape(-1)]
        ptr = buf.data_ptr()
        assert ptr % 256 == 0
        fields = [ptr + b for b in bases]
        desc = cd.cudecompExtDescribeFieldMoves(moves, fields, ptr + work, face, es, force)
        n = cd.cudecompExtRunFieldMoves(moves, fields, ptr + work, face, es, force, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        name = cd.cudecompExtLastKernelName()
        what = (es, extents, strides, n_fields, direction, sides, force, offsets, work_offset, shifts, name)
        assert n == 1 and name == _spell(desc, es), what + (desc,)
        assert desc["blocks"] == n_fields * desc["blocks_per_field"], what + (desc,)
        if not torch.equal(buf, expected):
            bad = torch.nonzero(buf != expected).reshape(-1)
            raise AssertionError(what + ("%d bytes differ, first at byte %d of the arena (fields begin at %s, the workspace at %d)"
                                         % (bad.numel(), int(bad[0]), bases[:4], work),))
        if force & 1:
            assert name == "generic_fields_kernel<%d>" % es, what
        elif expect_rows is not None:
            assert name.startswith("rows_fields_kernel<" if expect_rows else "generic_fields_kernel<"), what
            if expect_rows:
                assert name.endswith(",1>" if force & 2 else ",0>"), what
        return name, desc


LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130, 1025)


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_rows(es):
    """element size x row length x row pitch (length + 0, 1, 3: rows fused, rows at alternating phases, odd) x rows x planes: the
    whole cross of geometries, each with three draws (seeded) of field count {2, 3, 9, 32} x direction (field -> workspace,
    workspace -> field, field -> field) x one / two sides x fast path / forced element-wise / forced streaming; all 72 combinations
    must have come up.  Base offsets 0 .. 16 / es + 1 elements, another one for every field (field f: (f + k) mod (16 / es + 2))
    and for the workspace."""
    arena = _Arena(SLACK + 32 * ((12 + 4 * (1028 * 37 * 3 + 20)) * es + 2 * SLACK) + (2 * (1025 * 37 * 3 * 32 + 8) + 12) * es + 2 * SLACK)
    rng = np.random.RandomState(es)
    phases = 16 // es + 2
    seen, lanes = set(), set()
    for length, extra, rows, planes in itertools.product(LENGTHS, (0, 1, 3), (1, 5, 37), (1, 3)):
        pitch = length + extra
        extent, strides = (length, rows, planes), (1, pitch, pitch * rows + 5)  # (planes never continue one another)
        for _ in range(3):
            n, direction, sides, force = (2, 3, 9, 32)[rng.randint(4)], int(rng.randint(3)), int(rng.randint(2)) + 1, (0, 1, 2)[rng.randint(3)]
            k = int(rng.randint(phases))
            offsets = [(f + k) % phases for f in range(n)]
            name, desc = arena.run(es, extent, strides, n, direction, sides, force, offsets, int(rng.randint(phases)),
                                   expect_rows=True if length >= 2 else None)
            seen.add((n, direction, sides, force))
            if desc["kind"] == 22:
                lanes.add(desc["vec"])
                if es == 2 and n >= 2:  # consecutive fields sit at consecutive phases: one of them is at 2 mod 4
                    assert desc["vec"] == 2, (extent, strides, offsets, desc)
                if es >= 4 and extra != 0 and direction == FIELD_TO_FIELD:  # (no fusion of rows: the row length decides)
                    want = 16
                    while want > es and (length * es) % want:
                        want //= 2
                    assert desc["vec"] == want, (extent, strides, desc)
    assert len(seen) == 72, sorted(set(itertools.product((2, 3, 9, 32), range(3), (1, 2), (0, 1, 2))) - seen)
    assert lanes == ({2} if es == 2 else {v for v in (4, 8, 16) if v >= es}), lanes


def test_kernel_parity_two_byte_lanes_follow_every_field():
    """2-byte elements: all bases dword-aligned and even strides -> 16-byte lanes; ONE field of nine at 2 mod 4 -> 2-byte lanes for
    the whole launch; both compared byte for byte"""
    arena = _Arena(1 << 22)
    extent, strides = (64, 5, 3), (1, 66, 66 * 5 + 6)
    for direction in (FIELD_TO_WORK, WORK_TO_FIELD, FIELD_TO_FIELD):
        name, desc = arena.run(2, extent, strides, 9, direction, 2, 0, [0, 2, 4, 6, 8, 0, 2, 4, 6], 2, expect_rows=True)
        assert name == "rows_fields_kernel<16,0>", (direction, name)
        name, desc = arena.run(2, extent, strides, 9, direction, 2, 0, [0, 2, 4, 6, 8, 0, 3, 4, 6], 2, expect_rows=True)
        assert name == "rows_fields_kernel<2,0>", (direction, name)


def test_kernel_parity_two_sides_that_differ():
    """ONE kernel choice for the launch when the two sides are not alike: the narrower side's lanes (24-byte rows beside 256-byte
    ones), the element-wise kernel as soon as one side is a face one element thick, 2-byte lanes as soon as one side of 2-byte
    elements lies at 2 mod 4; three fields, every direction, one launch each, every byte compared"""
    arena = _Arena(1 << 20)
    row, short, thin = ((64, 5, 3), (1, 66, 66 * 5 + 6)), ((6, 5, 3), (1, 66, 66 * 5 + 6)), ((1, 9, 7), (1, 13, 13 * 11))
    for es, (a, b), shifts, kernel in ((4, (row, short), (0, 0), "rows_fields_kernel<8,0>"), (8, (row, thin), (0, 0), "generic_fields_kernel<8>"),
                                       (2, (row, row), (0, 0), "rows_fields_kernel<16,0>"), (2, (row, row), (2, 1), "rows_fields_kernel<2,0>")):
        for direction in (FIELD_TO_WORK, WORK_TO_FIELD, FIELD_TO_FIELD):
            name, _ = arena.run(es, (a[0], b[0]), (a[1], b[1]), 3, direction, 2, 0, [0, 0, 0], 0, shifts=shifts)
            assert name == kernel, (es, a, b, shifts, direction, name)


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_faces_one_element_thick(es):
    """the face along the fastest memory axis: extent (1, h, d), cells a row pitch apart -- the element-wise kernel by itself"""
    arena = _Arena(max(es, 4) << 23)
    phases = 16 // es + 2
    c = 0
    for (h, d), pitch, direction, sides in itertools.product(((9, 7), (37, 3), (1, 40), (300, 1)), (3, 16, 131), range(3), (1, 2)):
        n = (2, 3, 9, 32)[c % 4]
        force = (0, 1, 2)[(c // 4) % 3]
        c += 1
        extent, strides = (1, h, d), (1, pitch, pitch * (h + 3))
        name, _ = arena.run(es, extent, strides, n, direction, sides, force, [(f + c) % phases for f in range(n)], c % phases,
                            expect_rows=False)
        assert name == "generic_fields_kernel<%d>" % es, (extent, strides, name)
    # two cells per row along the fastest axis (halo 2): rows again
    name, _ = arena.run(es, (2, 9, 7), (1, 13, 13 * 11), 3, FIELD_TO_WORK, 2, 0, [0, 1, 2], 0, expect_rows=True)
    assert name.startswith("rows_fields_kernel<")


def test_kernel_parity_second_grid_stride_pass():
    """the element-wise kernel launches at most 8192 workgroups of 256 lanes per field: more elements than that take a second pass"""
    arena = _Arena(SLACK + 2 * ((4 * (8192 * 256 + 260) + 8) * 2 + 2 * SLACK) + (2 * (2 * (8192 * 256 + 257) + 8) + 8) * 2 + 2 * SLACK)
    for direction in (FIELD_TO_WORK, FIELD_TO_FIELD):
        name, desc = arena.run(2, (8192 * 256 + 257, 1, 1), (1, 0, 0), 2, direction, 1, 1, [1, 4], 3)
        assert name == "generic_fields_kernel<2>" and desc["blocks_per_field"] == 8192, (name, desc)


# ---- single-rank pencils ---------------------------------------------------------------------------------------------------
GDIMS = (11, 9, 7)
ORDERS = {"default": None, "contiguous": ((0, 1, 2), (1, 2, 0), (2, 0, 1)), "mixed": ((1, 0, 2), (2, 1, 0), (0, 2, 1))}
HALOS = [(1, 1, 1), (2, 0, 3), (3, 2, 1)]
PERIODS = [(1, 1, 1), (1, 0, 1), (0, 0, 0)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
OTHER_TYPES = [t for t in AB.ALL_TYPES if t not in (cd.DOUBLE, cd.HALF)]


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("halo", HALOS, ids=["h111", "h203", "h321"])
def test_single_rank_full_cross_fp64_fp16(layout, halo):
    """every axis, period mix, padding and dim, 2, 3 and 9 fields; dims 0, 1, 2 in sequence as well (edges and corners); whole
    buffers against single calls on clones; a self-periodic fields call is ONE data-movement launch"""
    for periods, padding in itertools.product(PERIODS, PADDINGS):
        args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
                "dtypes": [cd.DOUBLE, cd.HALF], "n_fields": [2, 3, 9], "all_dims": True, "launches": {"self": 1, "packed": 2}}
        assert FB.fields_sweep(0, 1, args) == []


@pytest.mark.parametrize("layout,halo,periods,padding", [("default", (3, 2, 1), (1, 1, 1), (1, 2, 0)), ("contiguous", (1, 1, 1), (1, 0, 1), (0, 0, 0)),
                                                         ("mixed", (2, 0, 3), (1, 1, 1), (1, 2, 0))], ids=["default", "contiguous", "mixed"])
def test_single_rank_other_types(layout, halo, periods, padding):
    args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
            "dtypes": OTHER_TYPES, "n_fields": [2, 3, 9], "all_dims": True}
    assert FB.fields_sweep(0, 1, args) == []


def test_one_field_is_the_single_call():
    args = {"gdims": GDIMS, "pdims": (1, 1), "halo": (2, 1, 1), "periods": (1, 1, 1), "padding": (0, 1, 0), "dtypes": [cd.DOUBLE, cd.HALF]}
    assert FB.one_field_is_the_single_call(0, 1, args) == []


# ---- ranks sharing the GPU -------------------------------------------------------------------------------------------------
def _jobs(pdims, backend, gdims=(10, 9, 11), guard=False, **more):
    jobs = []
    for periods, halo, padding in (((1, 1, 1), (1, 2, 1), (0, 0, 0)), ((0, 0, 0), (2, 1, 2), (1, 0, 2)), ((1, 0, 1), (1, 1, 3), (0, 0, 0))):
        args = dict({"gdims": gdims, "pdims": pdims, "halo_backend": backend, "halo": halo, "periods": periods, "padding": padding,
                     "dtypes": [cd.DOUBLE, cd.HALF], "n_fields": [3], "all_dims": True, "guard": guard,
                     "expect_kernels": any(periods) or tuple(pdims) != (1, 1)}, **more)  # (one rank without a period has no neighbour at all)
        jobs.append({"fn": "fields_sweep", "id": "hb%d P%dx%d periods %s halo %s" % ((backend,) + tuple(pdims) + (periods, halo)), "args": args})
    return jobs


def _some_single_plan_is_direct(gdims, pdims, nranks, mem_order):
    """the sweep holds a case where ONE field would travel straight from the pencil (dim the slowest axis, no padding)"""
    spec = cd.make_grid_spec(gdims, pdims, mem_order or ((0, 1, 2),) * 3)
    kinds = set()
    for r, axis, dim in itertools.product(range(nranks), range(3), range(3)):
        for periods in ((1, 1, 1), (1, 0, 1)):
            single = cd.cudecompExtPlanHalo(spec, r, axis, (1, 2, 1), periods, dim, (0, 0, 0), False)
            fields = cd.cudecompExtPlanHaloFields(spec, r, axis, (1, 2, 1), periods, dim, (0, 0, 0), 3, False)
            kinds.add((single.kind, fields.kind))
    return (3, 2) in kinds and not any(f == 3 for _, f in kinds)


@pytest.mark.parametrize("nranks,pdims", [(2, (2, 1)), (4, (2, 2))], ids=["two_ranks", "four_ranks_ragged"])
@pytest.mark.parametrize("backend", [cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM], ids=["MPI", "NVSHMEM"])
def test_ranks_peer_transports(nranks, pdims, backend):
    for failures in run_ranks(nranks, "tests.fields_bodies", "many", {"jobs": _jobs(pdims, backend)}, timeout=300):
        assert failures == []


@pytest.mark.parametrize("nranks,pdims", [(2, (2, 1)), (4, (2, 2))], ids=["two_ranks", "four_ranks_ragged"])
def test_ranks_rccl_stand_in(nranks, pdims):
    """NCCL enum: a single field's faces along the slowest axis would travel DIRECT; three fields are packed.  The workspace
    holds exactly 3 x the queried size inside a poisoned buffer."""
    if not os.path.exists(SHIM):
        pytest.skip("tests/shim/libfake_rccl.so not built")
    # (two ranks along one dim: only the axis-contiguous layout has a pencil whose slowest axis is the split one)
    mem_order = ORDERS["contiguous"] if nranks == 2 else None
    assert _some_single_plan_is_direct((10, 9, 11), pdims, nranks, mem_order)
    jobs = _jobs(pdims, cd.HALO_COMM_NCCL, guard=True, launches={"self": 1, "packed": 2}, mem_order=mem_order)
    for failures in run_ranks(nranks, "tests.fields_bodies", "many", {"jobs": jobs}, timeout=300, extra_env={"CUDECOMP_TEST_RCCL_SHIM": SHIM}):
        assert failures == []


def test_one_rank_real_rccl_and_one_sided_with_a_single_member():
    """CUDECOMP_TEST_SELF_EXCHANGE=1: the rank is its own neighbour but packs, exchanges (real librccl; the one-sided transport) and
    unpacks: two data-movement launches per call; over librccl with the workspace at exactly its size"""
    jobs = []
    for backend in (cd.HALO_COMM_NCCL, cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM):
        jobs += _jobs((1, 1), backend, guard=backend == cd.HALO_COMM_NCCL, mem_order=ORDERS["contiguous"], n_fields=[3, 9],
                      launches={"self": 2, "packed": 2} if backend == cd.HALO_COMM_NCCL else None)
    for failures in run_ranks(1, "tests.fields_bodies", "many", {"jobs": jobs}, timeout=300, extra_env=SELF):
        assert failures == []


# ---- hipGraph --------------------------------------------------------------------------------------------------------------
def test_captured_fields_call_replays_on_refilled_fields():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 1, 1), "padding": (0, 1, 0), "dim": 1},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "axis": 1, "dim": 1, "halo": (2, 1, 2),
                  "periods": (1, 1, 1), "dtype": cd.HALF}):
        assert run_ranks(1, "tests.fields_bodies", "graph_replay", args, timeout=300)[0] == []


def test_captured_fields_call_one_sided_self_exchange():
    args = {"gdims": (40, 36, 30), "pdims": (1, 1), "halo_backend": cd.HALO_COMM_NVSHMEM, "halo": (1, 2, 1), "periods": (1, 1, 1), "dim": 2}
    assert run_ranks(1, "tests.fields_bodies", "graph_replay", args, timeout=300, extra_env=SELF)[0] == []


# ---- launches ----------------------------------------------------------------------------------------------------------------
def test_nine_fields_one_launch_self_periodic_two_packed():
    """n = 9: one data-movement launch when self-periodic; pack and unpack, two, when the faces travel (self-exchange over librccl)"""
    args = {"gdims": (20, 18, 16), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (1, 1, 1), "dtypes": [cd.DOUBLE], "n_fields": [9],
            "expect_kernels": True}
    assert run_ranks(1, "tests.fields_bodies", "fields_sweep", dict(args, launches={"self": 1, "packed": 2}), timeout=300)[0] == []
    assert run_ranks(1, "tests.fields_bodies", "fields_sweep", dict(args, halo_backend=cd.HALO_COMM_NCCL, launches={"self": 2, "packed": 2}),
                     timeout=300, extra_env=SELF)[0] == []
