"""Multi-field transposes (cudecomp_transpose_fields.h: cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX}) on the GPU: the
field-move kernels of kernels_field_transpose.hip against index arithmetic (every byte of every input, output and of the workspace,
with slack around each); single-rank cycles under every triple of memory orders, halos and padding on either side, in and out of
place, against single cudecompTranspose* calls on clones; ranks sharing the GPU over every transport; capture into a hipGraph; the
number of launches.  Everything is compared byte for byte: there is no tolerance anywhere."""
import itertools
import os
import subprocess

import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import cases as K
from tests import transpose_fields_bodies as TB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = 256  # bytes between any two buffers (and before the first, after the last) that no move may touch
SELF = {"CUDECOMP_TEST_SELF_EXCHANGE": "1"}
# the one-sided transport copies its chunks with the copy engines: no launch of its own reaches cudecompExtDataLaunchCount, so the
# launch counts below are exactly the call's (tests/test_gpu_native_transpose_fields.py runs the compute-unit copies, the default
# between ranks that share a GPU)
ENGINES = {"CUDECOMP_PEER_COPY_ENGINE": "sdma"}
SHIM_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim")
SHIM = os.path.join(SHIM_DIR, "libfake_rccl.so")
K_TRANSPOSE, K_ROWS, K_GENERIC = 24, 22, 23


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
def _cells(extent, strides, device):
    import torch
    k = [torch.arange(int(e), dtype=torch.int64, device=device) * int(s) for e, s in zip(extent, strides)]
    return (k[0][:, None, None] + k[1][None, :, None] + k[2][None, None, :]).reshape(-1)


def _span(extent, strides):
    return sum((int(e) - 1) * int(s) for e, s in zip(extent, strides)) + 1


def _spell(d):
    if d["kind"] == K_TRANSPOSE:
        return "transpose_fields_kernel<%d,%d,%d,%d,%d,%s>" % (d["es"], d["vec"], d["ti"], d["tj"], d["access"], "true" if d["guard"] else "false")
    if d["kind"] == K_ROWS:
        return "rows_fields_kernel<%d,%d>" % (d["vec"], d["access"])
    return "generic_fields_kernel<%d>" % d["es"]


class _Arena:
    """One device buffer that holds every input, every output and the workspace of a case, random bytes throughout; a case copies
    the pristine bytes in, runs its list and compares EVERY byte with what index arithmetic on the pristine bytes gives: the cells
    around every destination are poison that must come back untouched."""

    def __init__(self, nbytes):
        import torch
        g = torch.Generator(device="cuda")
        g.manual_seed(4321)
        self.init = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
        self.buf = torch.empty_like(self.init)

    def run(self, es, geometries, n_fields, force, in_off=None, out_off=None, work_off=0, odd_step=False):
        """geometries: (extent, source strides, destination strides, source buffer, destination buffer) per move; buffers 0 the
        inputs, 1 the outputs, 2 the workspace.  Field f's input begins in_off[f] elements into its region, its output out_off[f],
        the workspace work_off.  Returns (launch descriptions, kernel launched last)."""
        import torch
        dev = self.buf.device
        in_off, out_off = in_off or [0] * n_fields, out_off or [0] * n_fields
        nxt = [0, 0, 0]  # next free element of an input region / an output region / the workspace
        moves, steps, placed = [], [], []
        for extent, ss, ds, sb, db in geometries:
            off, step = [0, 0], 0
            for side, (buf, strides) in enumerate(((sb, ss), (db, ds))):
                span = _span(extent, strides)
                off[side] = nxt[buf]
                if buf == 2:
                    step = span + 2 + (span % 2 if not odd_step else 1 - span % 2)  # (even unless the case asks for pieces at 2 mod 4)
                    nxt[2] += n_fields * step + 4
                else:
                    nxt[buf] += span + 3 + (span + 3) % 2
            moves.append(cd.make_move(extent, ss, ds, src_off=off[0], dst_off=off[1], src_buf=sb, dst_buf=db))
            steps.append(step)
            placed.append((extent, ss, ds, sb, db, off[0], off[1], step))
        region = [((max(o) + nxt[b]) * es + SLACK + 15) // 16 * 16 for b, o in ((0, in_off), (1, out_off))]
        work_bytes = ((work_off + nxt[2]) * es + SLACK + 15) // 16 * 16
        total = SLACK + n_fields * (region[0] + region[1]) + work_bytes
        assert total <= self.buf.numel(), (total, self.buf.numel())
        buf, init = self.buf[:total], self.init[:total]
        buf.copy_(init)
        base = [[SLACK + f * region[0] + in_off[f] * es for f in range(n_fields)],
                [SLACK + n_fields * region[0] + f * region[1] + out_off[f] * es for f in range(n_fields)]]
        work = SLACK + n_fields * (region[0] + region[1]) + work_off * es
        expected = init.clone()
        E, I = expected.view(-1, es), init.view(-1, es)
        f_el = torch.arange(n_fields, dtype=torch.int64, device=dev)[:, None]

        def cells(bufid, off, step, extent, strides):
            if bufid == 2:
                return work // es + off + f_el * step + _cells(extent, strides, dev)[None, :]
            b = torch.tensor([x // es for x in base[bufid]], dtype=torch.int64, device=dev)[:, None]
            return b + off + _cells(extent, strides, dev)[None, :]
        written = torch.zeros(total // es, dtype=torch.int32, device=dev)
        for extent, ss, ds, sb, db, so, do, step in placed:
            src, dst = cells(sb, so, step, extent, ss).reshape(-1), cells(db, do, step, extent, ds).reshape(-1)
            E[dst] = I[src]
            written[dst] += 1
            written[src] += 2
        assert int(written.max()) <= 2 and not bool(((written % 2 == 1) & (written > 1)).any()), "the case's own cells overlap"
        ptr = buf.data_ptr()
        assert ptr % 256 == 0
        ins, outs = [ptr + b for b in base[0]], [ptr + b for b in base[1]]
        desc = cd.cudecompExtDescribeFieldMoveList(moves, steps, ins, outs, ptr + work, es, force)
        n = cd.cudecompExtRunFieldMoveList(moves, steps, ins, outs, ptr + work, es, force, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        name = cd.cudecompExtLastKernelName()
        what = (es, [g[0] for g in geometries], n_fields, force, in_off, out_off, work_off, name)
        assert n == len(desc) and name == _spell(desc[-1]), what + (desc,)
        for d in desc:
            assert d["blocks"] == n_fields * d["blocks_per_field"], what + (d,)
        if not torch.equal(buf, expected):
            bad = torch.nonzero(buf != expected).reshape(-1)
            raise AssertionError(what + ("%d bytes differ, first at byte %d of the arena (inputs begin at %s, outputs at %s, the "
                                         "workspace at %d)" % (bad.numel(), int(bad[0]), base[0][:4], base[1][:4], work),))
        return desc, name


def _three_directions(extent, ss, ds):
    """one geometry as a list of three moves: input -> workspace, workspace -> output, input -> output"""
    return [(extent, ss, ds, 0, 2), (extent, ss, ds, 2, 1), (extent, ss, ds, 0, 1)]


def _transposing(ei, ej, ek, pad_s=2, pad_d=4):
    """(extent, source strides, destination strides) of a move whose source rows run along dim 0 and destination rows along dim 1,
    strides larger than the extents on both sides, planes that never continue one another"""
    sj, di = ei + pad_s, ej + pad_d
    return (ei, ej, ek), (1, sj, sj * ej + 6), (di, 1, di * ei + 10)


# (element size, lane width, tile i, tile j) of every shape transpose_fields_kernel is instantiated in
SHAPES = [(2, 8, 128, 128), (2, 1, 64, 64), (4, 4, 64, 128), (4, 1, 64, 64), (8, 2, 64, 64), (8, 1, 64, 64), (16, 1, 32, 32)]


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_transposing(es):
    """for every instantiation of transpose_fields_kernel that a move can reach: whole tiles (the unguarded form), a shape that
    ends inside a tile along i and j but keeps the lane width, and odd extents (element-wise lanes); 2-3 planes, strides larger
    than the extents, no edge above 300 elements; lists of three moves over 2 and 3 fields; cached and forced non-temporal access"""
    arena = _Arena(48 << 20)
    seen = set()
    c = 0
    for (e, vw, ti, tj) in [s for s in SHAPES if s[0] == es]:
        shapes = []
        if vw > 1 or es == 16:
            shapes.append(((ti * (2 if 2 * ti <= 300 else 1), tj * (2 if 2 * tj <= 300 else 1), 2), 0, False))  # whole tiles
            if vw > 1:
                shapes.append(((ti + 3 * vw, tj // 2 + vw, 3), 0, True))  # ends inside a tile, whole vectors
            else:
                shapes.append(((ti + 8, tj // 2 + 5, 3), 0, True))
        else:
            # element-wise lanes: odd extents; 2-byte elements also whole tiles of a field at 2 mod 4 (the unguarded form)
            shapes.append(((ti + 5, 37, 3), 0, True))
            shapes.append(((ti + 9, tj + 1, 2), 0, True))
            if es == 2:
                shapes.append(((64, 128, 2), 1, False))
        for (extent, odd, guard), force in itertools.product(shapes, (0, 2)):
            n = 2 + c % 2
            c += 1
            geo = _transposing(*extent)
            offs = [(f + 1) % 2 if odd else 2 * (f % 3) for f in range(n)]
            desc, name = arena.run(es, _three_directions(*geo), n, force, in_off=offs, out_off=offs[::-1], work_off=2 * (c % 3))
            assert len(desc) == 1 and desc[0]["index"] == [0, 1, 2], (extent, desc)
            d = desc[0]
            assert (d["kind"], d["vec"], d["ti"], d["tj"], d["guard"], d["access"]) == (K_TRANSPOSE, vw, ti, tj, int(guard), force), (extent, d)
            seen.add(name)
    reachable = {"transpose_fields_kernel<%d,%d,%d,%d,%d,%s>" % (e, vw, ti, tj, s, g) for (e, vw, ti, tj) in SHAPES if e == es
                 for s in (0, 2) for g in (("true", "false") if vw > 1 or e in (2, 16) else ("true",))}
    assert seen == reachable, sorted(reachable - seen)


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_rows_and_generic(es):
    """rows contiguous on both sides (row length x pitch x rows x planes) and everything else -- one element per row, extents
    below 4, forced -- as lists of three moves over 2 and 3 fields, cached and forced non-temporal; 2-byte rows at 2 mod 4"""
    arena = _Arena(16 << 20)
    kinds, access, lanes = set(), set(), set()
    c = 0
    for length, extra, rows, planes in itertools.product((1, 2, 3, 8, 9, 33, 130), (0, 1, 3), (1, 5, 37), (1, 3)):
        pitch = length + extra
        extent, ss = (length, rows, planes), (1, pitch, pitch * rows + 5)
        ds = (1, pitch + 2, (pitch + 2) * rows + 7)
        n, force = 2 + c % 2, (0, 2, 1)[c % 3]
        c += 1
        phases = 16 // es + 2
        offs = [(f + c) % phases for f in range(n)]
        desc, name = arena.run(es, _three_directions(extent, ss, ds), n, force, in_off=offs, out_off=offs[::-1], work_off=c % phases)
        for d in desc:
            kinds.add(d["kind"])
            access.add((d["kind"], d["access"]))
            if d["kind"] == K_ROWS:
                lanes.add(d["vec"])
                if es == 2:  # consecutive fields sit at consecutive phases: one of them is at 2 mod 4
                    assert d["vec"] == 2, (extent, offs, d)
        if force & 1:
            assert all(d["kind"] == K_GENERIC for d in desc), desc
        elif length >= 2:
            assert all(d["kind"] == K_ROWS and d["access"] == (1 if force & 2 else 0) for d in desc), (extent, desc)
    # 2-byte elements on dword-aligned rows take wide lanes
    if es == 2:
        desc, _ = arena.run(2, _three_directions((64, 5, 3), (1, 66, 336), (1, 68, 346)), 3, 0, in_off=[0, 2, 4], out_off=[4, 2, 0], work_off=2)
        assert [d["vec"] for d in desc] == [16], desc
        lanes.add(16)
        desc, _ = arena.run(2, _three_directions((64, 5, 3), (1, 66, 336), (1, 68, 346)), 3, 0, in_off=[0, 3, 4], out_off=[4, 2, 0], work_off=2)
        # (per move: the one that reads the workspace and writes the outputs touches no field at 2 mod 4 and keeps its lanes)
        assert {i: d["vec"] for d in desc for i in d["index"]} == {0: 2, 1: 16, 2: 2}, desc
        # ... and so do workspace pieces an odd step apart
        desc, _ = arena.run(2, [((64, 5, 3), (1, 66, 336), (1, 68, 346), 0, 2)], 3, 0, odd_step=True)
        assert desc[0]["vec"] == 2, desc
    # faces one element thick along the fastest axis, and transposing shapes with an extent below 4: element-wise
    for (h, d_), pitch in itertools.product(((9, 7), (37, 3), (1, 40), (300, 1)), (3, 16, 131)):
        extent, st = (1, h, d_), (1, pitch, pitch * (h + 3))
        desc, name = arena.run(es, _three_directions(extent, st, st), 2 + c % 2, (0, 2)[c % 2])
        c += 1
        assert [d["kind"] for d in desc] == [K_GENERIC] and name == "generic_fields_kernel<%d>" % es, desc
    desc, name = arena.run(es, _three_directions(*_transposing(3, 50, 2)), 3, 0)
    assert [d["kind"] for d in desc] == [K_GENERIC], desc
    assert kinds == {K_ROWS, K_GENERIC} and {(K_ROWS, 0), (K_ROWS, 1), (K_GENERIC, 0)} <= access, (kinds, access)
    assert lanes == ({2, 16} if es == 2 else {v for v in (4, 8, 16) if v >= es}), lanes


def test_kernel_parity_thirty_two_fields_and_nine_moves():
    """32 fields once; a list of nine moves once: two launches (eight moves and one); a list whose moves take all three kinds of
    kernel: three launches"""
    arena = _Arena(64 << 20)
    offs = [2 * (f % 5) for f in range(32)]
    desc, name = arena.run(8, _three_directions(*_transposing(70, 44, 2)), 32, 0, in_off=offs, out_off=offs[::-1], work_off=3)
    assert len(desc) == 1 and desc[0]["kind"] == K_TRANSPOSE and name.startswith("transpose_fields_kernel<8,2,64,64,0,true>")
    desc, _ = arena.run(2, _three_directions(*_transposing(136, 72, 2)), 32, 2, in_off=offs, out_off=offs[::-1], work_off=4)
    assert len(desc) == 1 and (desc[0]["kind"], desc[0]["vec"]) == (K_TRANSPOSE, 8), desc
    desc, _ = arena.run(4, _three_directions((33, 7, 3), (1, 36, 300), (1, 40, 333)), 32, 0, in_off=offs, out_off=offs)
    assert len(desc) == 1 and desc[0]["kind"] == K_ROWS
    geo = _transposing(68, 36, 2)
    nine = [(geo[0], geo[1], geo[2], (0, 2, 0)[i % 3], (2, 1, 1)[i % 3]) for i in range(9)]
    for n in (2, 3):
        desc, _ = arena.run(8, nine, n, 0)
        assert [d["index"] for d in desc] == [list(range(8)), [8]], desc
    rows = ((33, 7, 3), (1, 36, 300), (1, 40, 333))
    thin = ((1, 9, 7), (1, 13, 200), (1, 13, 200))
    mixed = [geo + (0, 2), rows + (0, 1), thin + (2, 1), geo + (0, 1), rows + (0, 2)]
    desc, _ = arena.run(8, mixed, 3, 0)
    assert [(d["kind"], d["index"]) for d in desc] == [(K_TRANSPOSE, [0, 3]), (K_ROWS, [1, 4]), (K_GENERIC, [2])], desc


# ---- single-rank cycles ------------------------------------------------------------------------------------------------------
HALO_CASES = {"in_x": ([(1, 2, 1), (0, 0, 0), (0, 0, 0)], [(1, 0, 2), (0, 0, 0), (0, 0, 0)]),
              "in_y": ([(0, 0, 0), (2, 1, 1), (0, 0, 0)], [(0, 0, 0), (0, 1, 1), (0, 0, 0)]),
              "all": ([(1, 1, 2), (2, 1, 1), (1, 2, 1)], [(1, 0, 0), (0, 1, 0), (0, 0, 2)])}
OTHER_TYPES = [t for t in AB.ALL_TYPES if t not in (cd.DOUBLE, cd.HALF)]


def _mo_id(m):
    return "".join("".join(map(str, r)) for r in m)


@pytest.mark.parametrize("mo", K.mem_order_combos(), ids=_mo_id)
def test_single_rank_full_cross_fp64_fp16(mo):
    """every triple of memory orders of tests/test_gpu_transpose.py, the four ops as a cycle, out of place and in place; halos and
    padding on the X pencil only, the Y pencil only (each op then has them on its input only or its output only) and on all three;
    2, 3 and 9 fields.  One data-movement launch out of place, two in place with differing layouts, none for the no-op."""
    for gdims, (halos, pads) in itertools.product(((10, 9, 11), (16, 12, 20)), HALO_CASES.values()):
        args = {"gdims": gdims, "pdims": (1, 1), "mem_order": mo, "halos": halos, "pads": pads, "dtypes": [cd.DOUBLE, cd.HALF],
                "n_fields": [2, 3, 9], "local_launches": True}
        assert TB.fields_cycle(0, 1, args) == []


@pytest.mark.parametrize("mo", [((0, 1, 2),) * 3, ((0, 1, 2), (1, 2, 0), (2, 0, 1)), ((1, 0, 2), (2, 1, 0), (0, 2, 1))], ids=_mo_id)
def test_single_rank_other_types(mo):
    for gdims, (halos, pads) in itertools.product(((10, 9, 11), (16, 12, 20)), HALO_CASES.values()):
        args = {"gdims": gdims, "pdims": (1, 1), "mem_order": mo, "halos": halos, "pads": pads, "dtypes": OTHER_TYPES,
                "n_fields": [2, 3, 9], "local_launches": True}
        assert TB.fields_cycle(0, 1, args) == []


def test_one_field_is_the_single_call():
    halos, pads = HALO_CASES["all"]
    for mo in (None, ((0, 1, 2), (1, 2, 0), (2, 0, 1))):
        args = {"gdims": (10, 9, 11), "pdims": (1, 1), "mem_order": mo, "halos": halos, "pads": pads, "dtypes": [cd.DOUBLE, cd.HALF]}
        assert TB.one_field_is_the_single_call(0, 1, args) == []
    assert TB.one_field_is_the_single_call(0, 1, {"gdims": (12, 12, 12), "pdims": (1, 1)}) == []  # (in place: the rotation)


# ---- ranks sharing the GPU -------------------------------------------------------------------------------------------------
ZERO = [(0, 0, 0)] * 3
RANK_GRIDS = [(2, (2, 1)), (3, (3, 1)), (4, (2, 2))]
CONTIGUOUS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
ELIDING = ((1, 2, 0), (2, 0, 1), (0, 1, 2))  # the split axis is the slowest of every input pencil: a single transpose sends from there


def _jobs(pdims, backend, gdims=(10, 9, 11), guard=False, launches="predict", n_fields=(3,), **more):
    jobs = []
    for mo, (halos, pads) in list(itertools.product((None, CONTIGUOUS), ((ZERO, ZERO), HALO_CASES["all"]))) + [(ELIDING, (ZERO, ZERO))]:
        args = dict({"gdims": gdims, "pdims": pdims, "transpose_backend": backend, "mem_order": mo, "halos": halos, "pads": pads,
                     "dtypes": [cd.DOUBLE, cd.HALF], "n_fields": list(n_fields), "guard": guard, "launches": launches,
                     "expect_kernels": True}, **more)
        jobs.append({"fn": "fields_cycle", "id": "tb%d P%dx%d %s halos %s" % ((backend,) + tuple(pdims) + (_mo_id(mo) if mo else "default", halos)),
                     "args": args})
    return jobs


def _some_single_plan_elides(pdims, nranks, symmetric):
    """the sweep holds a case whose SINGLE plan sends from the input or receives into the output, so the forced staging is used"""
    found = False
    for mo in (((0, 1, 2),) * 3, CONTIGUOUS, ELIDING):
        spec = cd.make_grid_spec((10, 9, 11), pdims, mo)
        for r, op, inplace in itertools.product(range(nranks), cd.OPS, (False, True)):
            single = cd.cudecompExtPlanTranspose(spec, r, op, None, None, None, None, inplace, False, symmetric)
            fields, _, _ = cd.cudecompExtPlanTransposeFields(spec, r, op, None, None, None, None, inplace, False, symmetric, 0, 3)
            if single.exchange and (single.send_buf != 2 or single.recv_buf != 2):
                found = True
                assert fields.send_buf == 2 and fields.recv_buf == 2 and fields.n_pack == fields.nranks == fields.n_unpack
    return found


@pytest.mark.parametrize("nranks,pdims", RANK_GRIDS, ids=["two_ranks", "three_ranks", "four_ranks"])
@pytest.mark.parametrize("backend", [cd.TRANSPOSE_COMM_MPI_P2P, cd.TRANSPOSE_COMM_NVSHMEM], ids=["MPI_P2P", "NVSHMEM"])
def test_ranks_peer_transports(nranks, pdims, backend):
    """ragged (10, 9, 11), a full cycle of 3 fields with and without halos; every call makes exactly the launches
    planFieldMoveLaunches predicts; the NVSHMEM workspace comes from cudecompMalloc"""
    assert _some_single_plan_elides(pdims, nranks, True)
    for failures in run_ranks(nranks, "tests.transpose_fields_bodies", "many", {"jobs": _jobs(pdims, backend)}, timeout=300, extra_env=ENGINES):
        assert failures == []


@pytest.fixture(scope="module")
def shim_env():
    if not os.path.exists(SHIM):
        subprocess.run(["make", "-C", SHIM_DIR], check=True, capture_output=True)
    return {"CUDECOMP_TEST_RCCL_SHIM": SHIM}


@pytest.mark.parametrize("nranks,pdims", RANK_GRIDS, ids=["two_ranks", "three_ranks", "four_ranks"])
def test_ranks_rccl_stand_in(nranks, pdims, shim_env):
    """NCCL enum through the stand-in: a single field would be sent from its input or received into its output; three fields are
    staged.  The workspace holds exactly 3 x the queried size inside a poisoned buffer whose outside stays untouched."""
    assert _some_single_plan_elides(pdims, nranks, False)
    jobs = _jobs(pdims, cd.TRANSPOSE_COMM_NCCL, guard=True)
    if nranks == 4:  # an even grid: exactly two data-movement launches per call (RCCL launches none of its own through the kernel layer)
        jobs += [j for j in _jobs(pdims, cd.TRANSPOSE_COMM_NCCL, gdims=(16, 16, 16), launches=2, guard=True) if j["args"]["halos"] == ZERO]
    for failures in run_ranks(nranks, "tests.transpose_fields_bodies", "many", {"jobs": jobs}, timeout=300, extra_env=shim_env):
        assert failures == []


def test_ranks_pipelined_and_fused_enums_take_the_plain_path():
    """one case each over NVSHMEM_PL and NVSHMEM_SM; an even grid on 2 x 2 makes exactly two data-movement launches per call"""
    jobs = []
    for backend in (cd.TRANSPOSE_COMM_NVSHMEM_PL, cd.TRANSPOSE_COMM_NVSHMEM_SM):
        jobs += _jobs((2, 2), backend)[3:4]
        jobs += _jobs((2, 2), backend, gdims=(16, 16, 16), launches=2)[:1]
    jobs += [j for j in _jobs((2, 2), cd.TRANSPOSE_COMM_NVSHMEM, gdims=(16, 16, 16), launches=2) if j["args"]["halos"] == ZERO]
    for failures in run_ranks(4, "tests.transpose_fields_bodies", "many", {"jobs": jobs}, timeout=300, extra_env=ENGINES):
        assert failures == []


def test_one_rank_real_rccl_and_one_sided_with_a_single_member():
    """CUDECOMP_TEST_SELF_EXCHANGE=1: the rank is its own peer but packs, exchanges (real librccl; the one-sided transport) and
    unpacks: two data-movement launches per call; 3 and 9 fields; over librccl with the workspace at exactly its size"""
    jobs = []
    for backend, path in ((cd.TRANSPOSE_COMM_NCCL, "rccl"), (cd.TRANSPOSE_COMM_MPI_P2P, None), (cd.TRANSPOSE_COMM_NVSHMEM, None)):
        jobs += _jobs((1, 1), backend, guard=backend == cd.TRANSPOSE_COMM_NCCL, launches=2, n_fields=(3, 9),
                      **({"expect_path": [path]} if path else {}))
    for failures in run_ranks(1, "tests.transpose_fields_bodies", "many", {"jobs": jobs}, timeout=300, extra_env=SELF):
        assert failures == []


# ---- hipGraph --------------------------------------------------------------------------------------------------------------
def test_captured_fields_call_replays_on_refilled_fields():
    halos, pads = HALO_CASES["all"]
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halos": halos, "pads": pads, "op": "XToY"},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": CONTIGUOUS, "op": "YToZ", "dtype": cd.HALF}):
        assert run_ranks(1, "tests.transpose_fields_bodies", "graph_replay", args, timeout=300)[0] == []


def test_captured_fields_call_one_sided_self_exchange():
    args = {"gdims": (40, 36, 30), "pdims": (1, 1), "transpose_backend": cd.TRANSPOSE_COMM_NVSHMEM, "op": "ZToY"}
    assert run_ranks(1, "tests.transpose_fields_bodies", "graph_replay", args, timeout=300, extra_env=SELF)[0] == []
