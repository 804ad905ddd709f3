"""Halo accumulation (cudecomp_amd.h: cudecompAmdAccumulateHalos{X,Y,Z}) on the GPU: the add kernels move by move against
numpy in all seven data types; single-rank pencils of every axis, memory order, halo width, period mix and padding; four
ranks sharing the GPU over the MPI, NVSHMEM and (stand-in) NCCL transports; real librccl with one member; config 5's per-rank
pencil at full size; capture into a hipGraph; updates and accumulations interleaved on one workspace.  Expected values come
from the numpy restatement of the contract in tests/accumulate_bodies.py and are compared bit for bit, whole pencils."""
import itertools
import os

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")
ORDERS = {"default": None, "contiguous": ((0, 1, 2), (1, 2, 0), (2, 0, 1))}
SELF = {"CUDECOMP_TEST_SELF_EXCHANGE": "1"}


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
def _reals(dtype, rng, n, values):
    """n reals of `dtype` as the numpy array the reference adds with (bf16: uint16 bit patterns)"""
    real = AB.TYPES[dtype][0]
    if values == "ints":
        v = rng.integers(0, 8, n).astype(np.float64)
        return np.frombuffer(AB.to_bytes(v, dtype).tobytes(), dtype=np.uint16 if real == "bf16" else real).copy()
    if real in (np.float32, np.float64):
        return rng.standard_normal(n).astype(real)
    # fp16 / bf16: magnitudes in [2^-3, 2^3) or zero -- the fp32 sum of two such values is exact, so one rounding, as on the device
    mant_bits, bias = (10, 15) if real == np.float16 else (7, 127)
    bits = (rng.integers(0, 2, n) << 15) | (rng.integers(bias - 3, bias + 3, n) << mant_bits) | rng.integers(0, 1 << mant_bits, n)
    bits = np.where(rng.integers(0, 8, n) == 0, 0, bits).astype(np.uint16)
    return bits.view(np.float16).copy() if real == np.float16 else bits


def _add(dtype, a, b):
    if AB.TYPES[dtype][0] == "bf16":
        import torch
        s = torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16) + torch.from_numpy(b.view(np.int16).copy()).view(torch.bfloat16)
        return s.view(torch.int16).numpy().view(np.uint16)
    return a + b  # numpy adds in the arrays' own precision (float16: one rounding of the exact sum)


def _accumulate(dtype, extent, ss, ds, src_len, dst_len, so, do, seed, values, modes=(0, 1, 2)):
    import torch
    nc, es = AB.TYPES[dtype][1], AB.element_bytes(dtype)
    rng = np.random.default_rng(seed)
    src = _reals(dtype, rng, (src_len + so) * nc, values)
    dst0 = _reals(dtype, rng, (dst_len + do) * nc, values)
    k = np.indices([int(e) for e in extent]).reshape(3, -1)
    cs = so + k[0] * ss[0] + k[1] * ss[1] + k[2] * ss[2]
    cdst = do + k[0] * ds[0] + k[1] * ds[1] + k[2] * ds[2]
    assert np.unique(cdst).size == cdst.size
    exp = dst0.copy().reshape(-1, nc)
    exp[cdst] = _add(dtype, exp[cdst].reshape(-1), src.reshape(-1, nc)[cs].reshape(-1)).reshape(-1, nc)
    exp = exp.reshape(-1).view(np.uint8)
    d_src = torch.from_numpy(src.view(np.uint8)).cuda()
    for force in modes:
        d_dst = torch.from_numpy(dst0.view(np.uint8).copy()).cuda()
        cls = cd.cudecompExtAccumulate3D(d_src.data_ptr() + es * so, d_dst.data_ptr() + es * do, dtype, extent, ss, ds, force,
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()  # EVERY byte of the destination buffer: cells outside the move untouched
        assert np.array_equal(got, exp), (AB.NAMES[dtype], values, extent, ss, ds, so, do, force, cls, cd.cudecompExtLastKernelName())
        name = cd.cudecompExtLastKernelName()
        assert cls in (0, 2) and name.startswith("generic_accumulate_kernel" if cls == 2 else "rows_accumulate_kernel"), (cls, name)
        if force & 1:
            assert cls == 2


ROW_SHAPES = [(64, 7, 3, 80, 64, 0, 0), (128, 33, 5, 128, 128, 0, 0), (6, 10, 11, 12, 9, 1, 2), (2, 37, 9, 40, 2, 3, 0),
              (1, 5, 4, 9, 1, 0, 1), (1000, 3, 1, 1024, 1000, 8, 16), (513, 4, 4, 515, 600, 1, 1), (7, 9, 5, 7, 7, 0, 0),
              (1025, 3, 2, 1027, 1031, 5, 3), (3, 40, 6, 50, 5, 2, 1)]


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows(dtype):
    # rows of many lengths and pitches (1-element and h-element rows among them), fast path, forced generic, streaming access.
    # cudecompExtAccumulate3D launches ONE move; batches of two add-moves in one (interleaved) launch -- both kernels -- are what
    # every single-rank periodic call of test_single_rank_all_types_all_axes runs (a rank that is its own neighbour)
    for w, h, d, sp, dp, so, do in ROW_SHAPES:
        ss, ds = (1, sp, sp * (h + 2)), (1, dp, dp * (h + 1))
        for values in ("ints", "random"):
            _accumulate(dtype, (w, h, d), ss, ds, ss[2] * d + 64, ds[2] * d + 64, so, do, w, values)


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_base_offsets(dtype):
    # 0-15 elements on both sides: bases at every alignment; 2-byte elements take wide lanes only at dword-aligned addresses
    for so, do in itertools.product(range(16), range(16)):
        if (so * 16 + do) % 5:
            continue
        _accumulate(dtype, (96, 5, 3), (1, 100, 500), (1, 98, 490), 1500, 1470, so, do, so * 16 + do, "ints", modes=(0, 2))
        _accumulate(dtype, (64, 64, 2), (1, 64, 4096), (64, 1, 4096), 8192, 8192, so, do, so + 100 * do, "random", modes=(0,))
    for so, do in ((1, 0), (0, 1), (3, 7), (15, 15), (2, 0)):
        _accumulate(dtype, (96, 5, 3), (1, 100, 500), (1, 98, 490), 1500, 1470, so, do, so, "random")


def test_kernel_choice_of_add_moves():
    """rows contiguous on both sides take rows_accumulate_kernel with the lane width of the row copy; a source that is not
    unit-stride, or the fastest dims swapped, take the element-wise kernel -- never a transposing one"""
    import torch
    a = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    b = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def run(dtype, extent, ss, ds, so=0, do=0):
        es = AB.element_bytes(dtype)
        cls = cd.cudecompExtAccumulate3D(a.data_ptr() + so * es, b.data_ptr() + do * es, dtype, extent, ss, ds, 0, s)
        torch.cuda.synchronize()
        return cls, cd.cudecompExtLastKernelName()

    assert run(cd.DOUBLE, (64, 8, 2), (1, 64, 512), (1, 66, 600)) == (0, "rows_accumulate_kernel<double,16,0>")
    assert run(cd.DOUBLE, (63, 8, 2), (1, 64, 512), (1, 66, 600)) == (0, "rows_accumulate_kernel<double,8,0>")
    assert run(cd.FLOAT, (66, 8, 2), (1, 80, 800), (1, 70, 700)) == (0, "rows_accumulate_kernel<float,8,0>")
    assert run(cd.HALF, (64, 8, 2), (1, 64, 512), (1, 66, 600)) == (0, "rows_accumulate_kernel<_Float16,16,0>")
    assert run(cd.HALF, (64, 8, 2), (1, 64, 512), (1, 66, 600), so=1) == (0, "rows_accumulate_kernel<_Float16,2,0>")
    assert run(cd.BFLOAT16, (64, 8, 2), (1, 64, 512), (1, 67, 670)) == (0, "rows_accumulate_kernel<__bf16,2,0>")
    assert run(cd.HALF_COMPLEX, (3, 8, 2), (1, 64, 512), (1, 67, 670)) == (0, "rows_accumulate_kernel<_Float16,4,0>")
    assert run(cd.DOUBLE_COMPLEX, (3, 8, 2), (1, 64, 512), (1, 67, 670)) == (0, "rows_accumulate_kernel<double,16,0>")
    assert run(cd.DOUBLE, (64, 8, 2), (1, 64, 512), (8, 1, 600)) == (2, "generic_accumulate_kernel<double,1>")
    assert run(cd.FLOAT_COMPLEX, (64, 8, 1), (2, 128, 0), (1, 64, 0)) == (2, "generic_accumulate_kernel<float,2>")


# ---- single rank -------------------------------------------------------------------------------------------------------------
SINGLE = [((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((2, 3, 1), (1, 0, 1), (1, 0, 2)), ((3, 2, 2), (0, 1, 1), (0, 1, 1))]


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("halo,periods,padding", SINGLE, ids=["h111", "h231", "h322"])
def test_single_rank_all_types_all_axes(layout, halo, periods, padding):
    """dims 2, 1, 0 (two add-moves per launch: a rank that is its own neighbour), whole pencil against the restatement, all
    seven types, X / Y / Z pencils; and <U x, y> == <x, A y> with cudecompUpdateHalos as the witness"""
    args = {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods,
            "padding": padding, "adjoint": True}
    assert AB.accumulate_sweep(0, 1, args) == []


def test_single_rank_interior_narrower_than_two_halos():
    # the two faces overlap: one launch each, low face first
    for gdims, halo in (((3, 5, 4), (2, 2, 2)), ((5, 3, 3), (3, 2, 3))):
        args = {"gdims": gdims, "pdims": (1, 1), "halo": halo, "periods": (1, 1, 1), "padding": (1, 0, 1), "adjoint": True}
        assert AB.accumulate_sweep(0, 1, args) == []


# ---- four ranks on the shared GPU ------------------------------------------------------------------------------------------
def _jobs4(backends, dtypes=None):
    jobs = []
    for backend in backends:
        for pdims in ((2, 2), (1, 4), (4, 1)):
            for halo, periods, padding in (((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((2, 3, 1), (0, 1, 0), (1, 0, 2)),
                                           ((3, 2, 2), (1, 0, 1), (0, 1, 1))):
                args = {"gdims": (30, 24, 22), "pdims": pdims, "halo_backend": backend, "halo": halo, "periods": periods,
                        "padding": padding}
                if dtypes:
                    args["dtypes"] = dtypes
                jobs.append({"fn": "accumulate_sweep", "id": "hb%d P%dx%d %s" % ((backend,) + pdims + (halo,)), "args": args})
    return jobs


@pytest.mark.parametrize("backend", [cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM], ids=["MPI", "NVSHMEM"])
def test_four_ranks_peer_transports(backend):
    for failures in run_ranks(4, "tests.accumulate_bodies", "many", {"jobs": _jobs4([backend])}, timeout=600):
        assert failures == []


def test_four_ranks_rccl_stand_in():
    if not os.path.exists(SHIM):
        pytest.skip("tests/shim/libfake_rccl.so not built")
    for failures in run_ranks(4, "tests.accumulate_bodies", "many", {"jobs": _jobs4([cd.HALO_COMM_NCCL])}, timeout=600,
                              extra_env={"CUDECOMP_TEST_RCCL_SHIM": SHIM}):
        assert failures == []


def test_one_rank_real_rccl_and_one_sided_with_a_single_member():
    """CUDECOMP_TEST_SELF_EXCHANGE=1: the rank is its own neighbour but packs, exchanges (real librccl; the one-sided
    transport) and adds what arrived"""
    jobs = []
    for backend in (cd.HALO_COMM_NCCL, cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM):
        for halo, periods, padding in SINGLE:
            jobs.append({"fn": "accumulate_sweep", "id": "self hb%d %s" % (backend, halo), "args": {
                "gdims": (26, 20, 23), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "halo_backend": backend, "halo": halo,
                "periods": periods, "padding": padding}})
    for failures in run_ranks(1, "tests.accumulate_bodies", "many", {"jobs": jobs}, timeout=600, extra_env=SELF):
        assert failures == []


# ---- full size, graphs, interleaving -----------------------------------------------------------------------------------------
def test_full_size_config5_pencil_every_cell():
    """BASELINE config 5's per-rank X pencil, 2048 x 1024 x 256 interior cells, halo 1, fp64, periodic: dims 2, 1, 0, every
    cell compared on the device"""
    res = run_ranks(1, "tests.accumulate_bodies", "full_size", {"gdims": (2048, 1024, 256), "halo": (1, 1, 1)}, timeout=600)[0]
    assert res["failures"] == [], res
    assert res["changed"] > 0
    assert res["kernels"][0].startswith("rows_accumulate_kernel<double,") and res["kernels"][1].startswith("rows_accumulate_kernel<double,")
    assert res["kernels"][2] == "generic_accumulate_kernel<double,1>", res["kernels"]


def test_streaming_choice_by_size():
    """a move of 32 MiB and more streams its source by itself (no force bit): 40 MiB of fp32, every byte compared"""
    import torch
    n = 10 << 20
    rng = np.random.default_rng(3)
    src, dst = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    d_src, d_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    cls = cd.cudecompExtAccumulate3D(d_src.data_ptr(), d_dst.data_ptr(), cd.FLOAT, (4096, n // 4096, 1), (1, 4096, 0), (1, 4096, 0), 0,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (cls, cd.cudecompExtLastKernelName()) == (0, "rows_accumulate_kernel<float,16,1>")
    assert np.array_equal(d_dst.cpu().numpy(), dst + src)


def test_captured_with_pack_exchange_add_on_the_one_sided_transport():
    """one rank exchanging with itself over the stream-ordered one-sided transport (CUDECOMP_TEST_SELF_EXCHANGE=1): pack ->
    exchange -> add along 2, 1, 0 captured into one hipGraph and replayed on fresh data"""
    args = {"gdims": (40, 36, 30), "pdims": (1, 1), "halo_backend": cd.HALO_COMM_NVSHMEM, "halo": (1, 2, 1), "periods": (1, 1, 1),
            "padding": (0, 1, 0)}
    assert run_ranks(1, "tests.accumulate_bodies", "graph_and_interleave", args, timeout=300, extra_env=SELF)[0] == []


def test_captured_into_one_graph_and_interleaved_with_updates():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 1, 1), "padding": (0, 1, 0)},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "axis": 1, "halo": (2, 1, 2),
                  "periods": (1, 0, 1)}):
        assert run_ranks(1, "tests.accumulate_bodies", "graph_and_interleave", args, timeout=300)[0] == []
    args = {"gdims": (30, 24, 22), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_NVSHMEM, "halo": (1, 2, 1), "periods": (1, 0, 1),
            "padding": (0, 0, 1), "capture": False}
    for failures in run_ranks(4, "tests.accumulate_bodies", "graph_and_interleave", args, timeout=300):
        assert failures == []
