"""Halo accumulation (cudecomp_amd.h: cudecompAmdAccumulateHalos{X,Y,Z}) on the GPU: the add kernels move by move against
numpy in all seven data types; single-rank pencils of every axis, memory order, halo width, period mix and padding; four
ranks sharing the GPU over the MPI, NVSHMEM and (stand-in) NCCL transports; real librccl with one member; config 5's per-rank
pencil at full size; capture into a hipGraph; updates and accumulations interleaved on one workspace.  Expected values come
from the numpy restatement of the contract in tests/accumulate_bodies.py and are compared bit for bit, whole pencils.

Those tests store integers 0..7 (every sum exact in every type): they check WHERE cells go.  WHAT is added is checked by the
tests below the "arithmetic" rule, against AB.typed_add (numpy; bf16 from integers and fp32 alone; pinned on the CPU by
tests/test_accumulate_reference.py):
  * all 24 x 24 pairs of a table of edge values per format (signed zeros, smallest / largest subnormals, smallest normal, ties
    at 1, overflow ties at the largest finite, infinities, a quiet NaN and a NaN with payload 1) through the fast, the forced
    element-wise and the streaming path at every lane width the type has, and through a transposed destination;
  * 2^18 reals per type of uniformly random bit patterns, of nearly cancelling pairs and of subnormal operands;
  * two launches from one initial destination: byte-equal, NaN cells included;
  * the element-wise kernel's second grid-stride pass (moves of more than 8192 x 256 elements);
  * pencils of non-integer reals on overlapping faces, one rank and four, where the restatement with the two additions in the
    other order differs -- so the stated order (low face first) shows.
Comparison rule of these: where the expected real is a NaN the device real must be a NaN -- ANY NaN: the contract leaves sign
and payload open, and the host's default NaN differs from the device's in the sign bit --; every other real, and every byte
outside the move, bit for bit.  No cell is excluded and there is no tolerance anywhere."""
import itertools
import os

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import edge_arithmetic as EA
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
    ran = []
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
        ran.append((cls, name))
    return ran


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


# ---- arithmetic: edge values, dense bit patterns, run-to-run identity ------------------------------------------------------------
def _accumulate_bits(dtype, extent, ss, ds, so, do, a, b, modes=(0, 1, 2), seed=0):
    """One add-move whose n-th element (dim 0 fastest) holds the reals a[n] in the destination and b[n] in the source -- a, b: bit
    patterns of shape (elements, reals per element); every other byte of both buffers random.  Launched once per mode from the same
    initial destination; the WHOLE destination buffer against AB.typed_add under the comparison rule of the module docstring.
    Returns [(class, kernel name, destination bytes after)] per mode."""
    import torch
    nc, es, kind = AB.TYPES[dtype][1], AB.element_bytes(dtype), AB.kind_of(dtype)
    u = AB.FORMATS[kind][0]
    k = np.indices([int(e) for e in extent][::-1]).reshape(3, -1)[::-1]  # k[i]: index along dim i, dim 0 fastest
    cs = so + k[0] * ss[0] + k[1] * ss[1] + k[2] * ss[2]
    cdst = do + k[0] * ds[0] + k[1] * ds[1] + k[2] * ds[2]
    assert a.shape == b.shape == (cs.size, nc) and a.dtype == u and b.dtype == u
    assert np.unique(cdst).size == cdst.size and cs.min() >= 0 and cdst.min() >= 0
    rng = np.random.default_rng([seed, AB.ALL_TYPES.index(dtype)])
    src = rng.integers(0, 256, (int(cs.max()) + 9) * es, dtype=np.uint8).view(u).reshape(-1, nc)
    dst0 = rng.integers(0, 256, (int(cdst.max()) + 9) * es, dtype=np.uint8).view(u).reshape(-1, nc)
    src[cs], dst0[cdst] = b, a
    exp = dst0.copy()
    exp[cdst] = AB.typed_add(dtype, a, b)
    inside = np.zeros(exp.shape, dtype=bool)
    inside[cdst] = True
    d_src = torch.from_numpy(src.view(np.uint8).reshape(-1)).cuda()
    ran = []
    for force in modes:
        d_dst = torch.from_numpy(dst0.view(np.uint8).reshape(-1).copy()).cuda()
        cls = cd.cudecompExtAccumulate3D(d_src.data_ptr() + es * so, d_dst.data_ptr() + es * do, dtype, extent, ss, ds, force,
                                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        name = cd.cudecompExtLastKernelName()
        raw = d_dst.cpu().numpy()
        got = raw.view(u).reshape(-1, nc)
        where = (AB.NAMES[dtype], extent, ss, ds, so, do, force, cls, name)
        assert np.array_equal(got[~inside], exp[~inside]), ("a real outside the move changed",) + where
        bad = np.argwhere(AB.mismatches(kind, got, exp) & inside)
        assert bad.size == 0, where + tuple("cell %d real %d: %#x + %#x gave %#x, expected %#x" % (
            c, r, dst0[c, r], src[cs[np.nonzero(cdst == c)[0][0]], r], got[c, r], exp[c, r]) for c, r in bad[:4]) + ("%d reals wrong" % len(bad),)
        ran.append((cls, name, raw))
    return ran


# the pairs laid into elements, the (w, h, d) shapes of 576 elements and the (real type, reals per element, lane widths) table are
# shared with the edge-value tests of the other adding kernels: tests/edge_arithmetic.py
_pair_elements, EDGE_SHAPES, EDGE_KERNELS = EA.pair_elements, EA.SHAPES, EA.KERNELS


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_arithmetic_on_edge_values(dtype):
    """all pairs of the edge table: destination element i*K + j holds table[i], the source's holds table[j], so every dword and
    every 16-byte lane mixes classes (a NaN or an infinity beside an ordinary value in a packed pair)"""
    a, b = _pair_elements(dtype, *AB.all_pairs(AB.edge_table(AB.kind_of(dtype))))
    exp = AB.classes(AB.kind_of(dtype), AB.typed_add(dtype, a, b))
    assert exp["nan"].any() and exp["inf"].any() and exp["zero"].any() and exp["subnormal"].any()
    seen = set()
    for w, h, d in EDGE_SHAPES:  # even pitches and bases: 2-byte elements keep their wide lanes
        ran = _accumulate_bits(dtype, (w, h, d), (1, w + 6, (w + 6) * (h + 1)), (1, w + 2, (w + 2) * (h + 2)), 4, 8, a, b)
        seen |= {name for _, name, _ in ran}
    t, nc, widths = EDGE_KERNELS[dtype]
    assert seen == {"rows_accumulate_kernel<%s,%d,%d>" % (t, vb, st) for vb in widths for st in (0, 1)} | {"generic_accumulate_kernel<%s,%d>" % (t, nc)}
    if AB.element_bytes(dtype) == 2:  # odd bases: 2-byte lanes whatever the row length
        ran = _accumulate_bits(dtype, (96, 3, 2), (1, 102, 408), (1, 98, 490), 1, 3, a, b, modes=(0, 2))
        assert [name for _, name, _ in ran] == ["rows_accumulate_kernel<%s,2,%d>" % (t, st) for st in (0, 1)]
    # a transposed destination (rows of the source become columns): the element-wise kernel with no force bit
    (cls, name, _), = _accumulate_bits(dtype, (36, 4, 4), (1, 40, 200), (4, 1, 150), 2, 2, a, b, modes=(0,))
    assert (cls, name) == (2, "generic_accumulate_kernel<%s,%d>" % (t, nc))


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_arithmetic_on_dense_bit_patterns(dtype):
    """2^18 reals per draw: uniformly random patterns, nearly cancelling pairs, subnormal operands (AB.dense_draws)"""
    kind, nc = AB.kind_of(dtype), AB.TYPES[dtype][1]
    n = (1 << 18) // nc
    for name, (a, b) in AB.dense_draws(kind, 1 << 18, 7).items():
        a, b = a.reshape(n, nc), b.reshape(n, nc)
        exp = AB.classes(kind, AB.typed_add(dtype, a, b))  # a draw that contains none of these is not testing them
        assert exp["subnormal"].any() and exp["zero"].any(), (kind, name)
        if name == "uniform":
            assert exp["inf"].any() and exp["nan"].any(), kind
        ran = _accumulate_bits(dtype, (512, n // 1024, 2), (1, 520, 520 * (n // 1024 + 1)), (1, 516, 516 * (n // 1024)), 0, 0, a, b)
        assert [cls for cls, _, _ in ran] == [0, 2, 0], ran


def test_two_runs_give_the_same_bytes():
    """run-to-run identity, NaN cells included: bf16 pairs of the edge table, each path launched twice from one initial destination"""
    a, b = _pair_elements(cd.BFLOAT16, *AB.all_pairs(AB.edge_table("bf16")))
    first = _accumulate_bits(cd.BFLOAT16, (96, 3, 2), (1, 102, 408), (1, 98, 490), 4, 8, a, b)
    second = _accumulate_bits(cd.BFLOAT16, (96, 3, 2), (1, 102, 408), (1, 98, 490), 4, 8, a, b)
    for (c1, n1, raw1), (c2, n2, raw2) in zip(first, second):
        assert (c1, n1) == (c2, n2) and np.array_equal(raw1, raw2), (n1, n2)
    for (_, n1, raw1) in first[1:]:  # ... and the three paths agree with one another, NaN payloads included
        assert np.array_equal(raw1, first[0][2]), n1


# ---- the grid-stride pass of the element-wise kernel -------------------------------------------------------------------------------
# The classifier launches at most 8192 workgroups of 256 lanes: moves of more than 2,097,152 elements take a second pass.  Integer
# payload: these are about WHICH cells are visited -- an unvisited cell keeps its value, a cell visited twice gets the source twice.
GRID_STRIDE = [
    ("fp16 gathered", cd.HALF, (1, 1500, 1400), (0, 3, 4503), (0, 1, 1504), "generic_accumulate_kernel<_Float16,1>"),
    ("complex64 strided destination", cd.FLOAT_COMPLEX, (1, 1500, 1400), (0, 3, 4503), (0, 2, 3002), "generic_accumulate_kernel<float,2>"),
    ("fp32 short tail", cd.FLOAT, (1, 2097152 + 257, 1), (0, 2, 0), (0, 1, 0), "generic_accumulate_kernel<float,1>"),
]


@pytest.mark.parametrize("what,dtype,extent,ss,ds,kernel", GRID_STRIDE, ids=[c[0].replace(" ", "_") for c in GRID_STRIDE])
def test_generic_kernel_second_grid_stride_pass(what, dtype, extent, ss, ds, kernel):
    n = extent[0] * extent[1] * extent[2]
    assert n > 8192 * 256
    src_len = 1 + sum((e - 1) * s for e, s in zip(extent, ss))
    dst_len = 1 + sum((e - 1) * s for e, s in zip(extent, ds))
    ran = _accumulate(dtype, extent, ss, ds, src_len + 64, dst_len + 64, 2, 4, 9, "ints", modes=(0,))  # spare cells past the end compared too
    assert ran == [(2, kernel)]


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


# ---- the stated order, visible: non-integer reals on overlapping faces ---------------------------------------------------------------
OVERLAPPING = [((3, 5, 4), (2, 2, 2)), ((5, 3, 3), (3, 2, 3))]


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("gdims,halo", OVERLAPPING, ids=["g354_h222", "g533_h323"])
def test_single_rank_overlapping_faces_in_the_stated_order(layout, gdims, halo):
    """payload of non-integer reals, the restatement in the element type's arithmetic: LF += H, THEN HF += L.  Every sum rounds,
    so a cell of both faces tells the order: accumulate_sweep also restates the two additions swapped and requires a difference"""
    args = {"gdims": gdims, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": (1, 1, 1), "padding": (1, 0, 1),
            "payload": "typed", "overlap": True}
    assert AB.accumulate_sweep(0, 1, args) == []


def test_single_rank_typed_payload_without_overlap():
    # the control: faces apart (one launch for both additions), same payload
    args = {"gdims": (33, 20, 27), "pdims": (1, 1), "halo": (2, 3, 1), "periods": (1, 1, 1), "payload": "typed"}
    assert AB.accumulate_sweep(0, 1, args) == []


def _jobs4_typed(backend):
    """gdims (20, 22, 21) over four ranks: slabs of 5 and 6 cells with halo 3 -- every slab at least one halo wide (the planner
    accepts it), the slabs of 5 narrower than two (their two additions read the workspace one after the other): ordered and
    unordered ranks in one grid"""
    jobs = []
    for pdims, periods, padding in (((1, 4), (1, 1, 1), (0, 0, 0)), ((1, 4), (1, 0, 1), (0, 0, 0)), ((4, 1), (1, 1, 1), (0, 0, 0)),
                                    ((4, 1), (1, 0, 1), (0, 0, 0)), ((4, 1), (1, 1, 1), (1, 0, 2))):
        args = {"gdims": (20, 22, 21), "pdims": pdims, "halo_backend": backend, "halo": (3, 3, 3), "periods": periods,
                "padding": padding, "dtypes": [cd.FLOAT, cd.HALF, cd.BFLOAT16], "payload": "typed", "overlap": True}
        jobs.append({"fn": "accumulate_sweep", "id": "typed hb%d P%dx%d periods %s padding %s" % ((backend,) + pdims + (periods, padding)),
                     "args": args})
    return jobs


@pytest.mark.parametrize("backend", [cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM], ids=["MPI", "NVSHMEM"])
def test_four_ranks_overlapping_faces_in_the_stated_order(backend):
    jobs = _jobs4_typed(backend)
    for job in jobs:  # on the CPU first: the planner accepts every rank, and the grid mixes ordered and unordered packed plans
        a = job["args"]
        spec = cd.make_grid_spec(a["gdims"], a["pdims"], ((0, 1, 2),) * 3)
        ordered = set()
        for r, axis, dim in itertools.product(range(4), range(3), range(3)):
            p = cd.cudecompExtPlanHaloAccumulate(spec, r, axis, a["halo"], a["periods"], dim, a["padding"], True)
            if p.kind == 2:
                ordered.add(bool(p.reserved & 2))
        assert ordered == {False, True}, job["id"]
    for failures in run_ranks(4, "tests.accumulate_bodies", "many", {"jobs": jobs}, timeout=600):
        assert failures == []


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
