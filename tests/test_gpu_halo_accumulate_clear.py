"""Halo accumulate-and-clear (cudecomp_amd_fill.h: cudecompAmdAccumulateAndClearHalos{X,Y,Z}) on the GPU.

The call is defined as  accumulate(dim); fill(dim, NULL)  with the same arguments, byte for byte.  So: the four take kernels move
by move and list by list through cudecompExtRunMoves (modes 3 and 4; EVERY byte of the source and the destination buffer, poison
slack on both sides, against numpy); their arithmetic on IEEE edge values; single-rank pencils of every axis, memory order, halo
width, period mix, padding and dim against (a) the library's own two calls on a copy and (b) the numpy restatement
(tests/accumulate_clear_bodies.py); dims 2, 1, 0 in sequence; interiors narrower than two halos; ranks sharing the GPU over every
halo transport; the deposit loop the feature is for; capture into a hipGraph; asynchrony.

Tolerance 0 everywhere.  Payloads of everything compared byte for byte are finite (AB.typed_cells / AB.initial_cells), so no NaN
arises whose payload the contract leaves open; the arithmetic test alone feeds NaNs and infinities and compares with the class
rule of tests/test_gpu_halo_accumulate.py (AB.mismatches: an expected NaN may be any NaN, everything else bit for bit)."""
import itertools
import os

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import accumulate_clear_bodies as CB
from tests import move_lists as ML
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim", "libfake_rccl.so")
SELF = {"CUDECOMP_TEST_SELF_EXCHANGE": "1"}
TAKE, ADD_TAKE = cd.MOVES_TAKE, cd.MOVES_ADD_TAKE
GENERIC, STREAMING = 1, 2  # flags of cudecompExtRunMoves
TYPE_OF_ES = {2: cd.HALF, 4: cd.FLOAT, 8: cd.DOUBLE, 16: cd.DOUBLE_COMPLEX}
LENGTHS = (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65, 127, 130, 1000, 1025)  # (tests/test_gpu_halo_fill.py)
CHUNK_BYTES = 48 << 20


@pytest.fixture(scope="module", autouse=True)
def no_rank_pool_beside_the_kernel_tests():
    """the kernel tests use the GPU from the process that runs them: a rank pool of earlier multi-rank tests ends first"""
    from tests import mp
    mp.pool_stop()


def _run_chunked(cases, es, mode, dtype, seed=0):
    """cases: (extent, ss, ds, so, do, flags), each one launch of its own; packed behind one another into regions that start on
    256-element boundaries (so `so` and `do` alone set the phase), a buffer pair per CHUNK_BYTES.  Returns the launch of every case."""
    out, packer, flags_of = [], ML.Packer(gap=3, align=256), []

    def flush():
        if packer.moves:
            for ls in CB.run_take_lists([([m], f) for m, f in zip(packer.moves, flags_of)], es, mode, dtype, seed + len(out), check_cells=False):
                assert len(ls) == 1, ls
                out.append(ls[0])
    for extent, ss, ds, so, do, flags in cases:
        if max(packer.len) * es > CHUNK_BYTES:
            flush()
            packer, flags_of = ML.Packer(gap=3, align=256), []
        packer.add(extent, ss, ds, so, do)
        flags_of.append(flags)
    flush()
    assert len(out) == len(cases)
    return out


def _check_row_choice(es, mode, case, launch):
    """what the classifier must offer a take-move, restated from the move alone: when the live dim with the smallest source stride
    is unit-stride on both sides (or no dim is live) the row kernel, everything else and every forced case the element-wise one.
    Lane width where the rows stay rows (dim 1 continues dim 0 on neither side): the widest of 16, 8, 4, 2 bytes that holds whole
    elements and divides the row -- 2-byte elements with a base or a stride at 2 mod 4: 2-byte lanes."""
    extent, ss, ds, so, do, flags = case
    rows, generic = (12, 13) if mode == TAKE else (14, 15)
    live = sorted((s, d, e) for e, s, d in zip(extent, ss, ds) if e > 1)
    if flags & GENERIC or (live and live[0][:2] != (1, 1)):
        assert (launch["kind"], launch["vec"], launch["access"], launch["cls"]) == (generic, es, 0, 2), (case, launch)
        return
    assert (launch["kind"], launch["cls"]) == (rows, 0) and launch["access"] == (1 if flags & STREAMING else 0), (case, launch)
    if len(live) >= 2 and live[0][2] == extent[0] and live[1][0] != extent[0] and live[1][1] != extent[0]:
        want = 16
        while want > es and extent[0] * es % want:
            want //= 2
        if es == 2 and ((so | do) & 1 or any((s | d) & 1 for s, d, _ in live[1:])):
            want = 2
        assert launch["vec"] == want, (case, launch)


def _row_cases(es, lengths, extras, rows_list, planes_list):
    """row length x pitch (length + 0 / 1 / 3) x rows x planes x base offsets: source and destination each over every phase of the
    16-byte grid and one past it (equal phases under all three paths, crossed phases on the fast path)"""
    P = 16 // es + 2
    cases = []
    for length, extra, rows, planes in itertools.product(lengths, extras, rows_list, planes_list):
        sp, dp = length + extra, length + (extra + 2 if extra else 0)
        ss, ds = (1, sp, sp * rows + 5), (1, dp, dp * rows + 7)  # (planes never continue one another)
        for o in range(P):
            for flags in (0, GENERIC, STREAMING):
                cases.append(((length, rows, planes), ss, ds, o, o, flags))
            cases.append(((length, rows, planes), ss, ds, o, (2 * o + 1) % P, 0))
    return cases


# ---- kernel parity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [TAKE, ADD_TAKE], ids=["take", "add_take"])
@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_rows(es, mode):
    cases = _row_cases(es, LENGTHS, (0, 1, 3), (1, 5, 37), (1, 3))
    launches = _run_chunked(cases, es, mode, TYPE_OF_ES[es], seed=es)
    seen = set()
    for case, l in zip(cases, launches):
        _check_row_choice(es, mode, case, l)
        seen.add((l["kind"], l["vec"], l["access"]))
    rows, generic = (12, 13) if mode == TAKE else (14, 15)
    every = {(rows, v, a) for v in (16, 8, 4, 2) if v >= es for a in (0, 1)} | {(generic, es, 0)}
    # (no length of LENGTHS gives 2-byte elements rows of 8 mod 16 bytes: their 8-byte lanes run in the all-types and arithmetic tests)
    assert every - ({(rows, 8, 0), (rows, 8, 1)} if es == 2 else set()) <= seen <= every, seen


@pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
def test_kernel_parity_rows_add_take_all_types(dtype):
    """mode 4 in all seven element types on a reduced cross of the row shapes"""
    es = AB.element_bytes(dtype)
    cases = _row_cases(es, (1, 3, 4, 8, 12, 17, 64, 130, 1025), (0, 3), (1, 5), (3,))
    launches = _run_chunked(cases, es, ADD_TAKE, dtype, seed=100 + AB.ALL_TYPES.index(dtype))
    names = set()
    for case, l in zip(cases, launches):
        _check_row_choice(es, ADD_TAKE, case, l)
        names.add(CB.kernel_name_of(l))
    t, nc = CB.ARITH_NAMES[l["arith"]], AB.TYPES[dtype][1]
    assert names == {"rows_accumulate_take_kernel<%s,%d,%d>" % (t, v, a) for v in (16, 8, 4, 2) if v >= es for a in (0, 1)} | \
        {"generic_accumulate_take_kernel<%s,%d>" % (t, nc)}, names
    assert all(n.split("<")[1].startswith(t + ",") for n in names), names


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_faces_one_element_thick(es):
    """the face along the fastest memory axis, extent (1, h, d): the pack of the fused call takes it out of the pencil (cells a row
    pitch apart) into a dense slot; the wrap addition adds one such face onto another.  Element-wise kernels, with no force bit."""
    dtype = TYPE_OF_ES[es]
    P = 16 // es + 2
    take, add_take = [], []
    for (h, d), pitch, o in itertools.product(((9, 7), (37, 3), (1, 40), (300, 1)), (3, 16, 131), range(P)):
        apart = (1, pitch, pitch * (h + 3))
        for flags in (0, GENERIC, STREAMING):
            take.append(((1, h, d), apart, (1, 1, h), o, (o + 1) % P, flags))
            add_take.append(((1, h, d), apart, (1, pitch + 2, (pitch + 2) * (h + 1)), o, (2 * o + 1) % P, flags))
    for l in _run_chunked(take, es, TAKE, dtype):
        assert (l["cls"], CB.kernel_name_of(l)) == (2, "generic_take_kernel<%d>" % es), l
    for l in _run_chunked(add_take, es, ADD_TAKE, dtype):
        assert l["cls"] == 2 and CB.kernel_name_of(l).startswith("generic_accumulate_take_kernel<"), l
    # a face two elements thick (halo 2): rows again
    two = [((2, 9, 7), (1, 13, 13 * 11), (1, 2, 18), 1, 0, 0)]
    assert _run_chunked(two, es, TAKE, dtype)[0]["kind"] == 12
    two = [((2, 9, 7), (1, 13, 13 * 11), (1, 13, 13 * 12), 1, 2, 0)]
    assert _run_chunked(two, es, ADD_TAKE, dtype)[0]["kind"] == 14


# ---- batching --------------------------------------------------------------------------------------------------------------------
def counts_of(launch):
    return [b - a for a, b in zip(launch["first_block"], launch["first_block"][1:])]


@pytest.mark.parametrize("mode,dtype", [(TAKE, cd.DOUBLE), (ADD_TAKE, cd.DOUBLE), (TAKE, cd.HALF), (ADD_TAKE, cd.BFLOAT16), (ADD_TAKE, cd.FLOAT_COMPLEX)],
                         ids=["take_8", "add_take_fp64", "take_2", "add_take_bf16", "add_take_complex64"])
def test_lists_share_interleaved_launches(mode, dtype):
    """two sibling moves (the two sides of one fused call) and eight moves of unequal size, each list in ONE interleaved launch,
    rows and element-wise; a filler workgroup that does not leave, or a move decoded with another's geometry, changes a byte"""
    es = AB.element_bytes(dtype)
    for flags in (0, GENERIC):
        p = ML.Packer(gap=3, align=256)
        for _ in range(2):  # low side, high side: the same slab twice
            p.add((64, 9, 7), (1, 70, 70 * 11), (1, 64, 64 * 9))
        (ls,) = CB.run_take_lists([(p.moves, flags)], es, mode, dtype, seed=1)
        assert len(ls) == 1 and (ls[0]["n"], ls[0]["interleave"]) == (2, 1), ls
        p = ML.Packer(gap=3, align=256)
        for h, d in ((1, 1), (2, 1), (400, 7), (5, 1), (70, 3), (1, 2), (16, 2), (150, 7)):
            p.add((64, h, d), (1, 70, 70 * (h + 1)), (1, 66, 66 * (h + 2)))
        (ls,) = CB.run_take_lists([(p.moves, flags)], es, mode, dtype, seed=2)
        counts = counts_of(ls[0])
        assert len(ls) == 1 and (ls[0]["n"], ls[0]["interleave"]) == (8, 1) and ls[0]["blocks"] == 8 * max(counts), ls
        assert max(counts) >= 10 * min(counts) and len(set(counts)) >= 4, counts
        assert ls[0]["kind"] == {(TAKE, 0): 12, (TAKE, 1): 13, (ADD_TAKE, 0): 14, (ADD_TAKE, 1): 15}[(mode, flags)]


def test_second_grid_stride_pass_and_streaming_by_size():
    # the element-wise kernels launch at most 8192 workgroups of 256 lanes: a list with more elements than that takes a second pass
    n = 8192 * 256 + 257
    for mode, dtype, name in ((TAKE, cd.HALF, "generic_take_kernel<2>"), (ADD_TAKE, cd.FLOAT, "generic_accumulate_take_kernel<float,1>")):
        es = AB.element_bytes(dtype)
        p = ML.Packer(gap=3, align=256)
        p.add((n, 1, 1), (1, 0, 0), (1, 0, 0), 1, 2)
        p.add((1, 300, 7), (1, 5, 1600), (1, 1, 300))
        (ls,) = CB.run_take_lists([(p.moves, GENERIC)], es, mode, dtype, seed=3)
        assert len(ls) == 1 and ls[0]["n"] == 2 and ls[0]["elements"] > 8192 * 256 and max(counts_of(ls[0])) == 8192, ls
        assert cd.cudecompExtLastKernelName() == name
    # 40 MiB in one contiguous move: the streaming instantiation with no force bit; 32 MiB less one element: not
    for mode, dtype, names in ((TAKE, cd.DOUBLE, ("rows_take_kernel<16,1>", "rows_take_kernel<8,0>")),
                               (ADD_TAKE, cd.DOUBLE, ("rows_accumulate_take_kernel<double,16,1>", "rows_accumulate_take_kernel<double,8,0>"))):
        (ls,) = CB.run_take_lists([([cd.make_move((5 << 20, 1, 1), (1, 0, 0), (1, 0, 0), 0, 0)], 0)], 8, mode, dtype, seed=4)
        assert (ls[0]["access"], cd.cudecompExtLastKernelName()) == (1, names[0]), ls
        (ls,) = CB.run_take_lists([([cd.make_move(((4 << 20) - 1, 1, 1), (1, 0, 0), (1, 0, 0), 0, 0)], 0)], 8, mode, dtype, seed=5)
        assert (ls[0]["access"], cd.cudecompExtLastKernelName()) == (0, names[1]), ls


# ---- arithmetic ------------------------------------------------------------------------------------------------------------------
def _add_take_bits(dtype, extent, ss, ds, so, do, a, b, seed=0):
    """One add-take whose n-th element (dim 0 fastest) holds the reals a[n] in the destination and b[n] in the source (bit
    patterns, shape (elements, reals per element)); every other byte of both buffers random.  Fast, forced element-wise and
    forced streaming path from the same initial buffers.  Destination: AB.mismatches against AB.typed_add inside the move, bit for
    bit outside.  Source: zero bytes inside the move, bit for bit outside.  Returns the kernel names."""
    import torch
    nc, es, kind = AB.TYPES[dtype][1], AB.element_bytes(dtype), AB.kind_of(dtype)
    u = AB.FORMATS[kind][0]
    cs, cdst = ML.cells(extent, ss, so), ML.cells(extent, ds, do)
    assert a.shape == b.shape == (cs.size, nc) and np.unique(cdst).size == cdst.size and np.unique(cs).size == cs.size
    rng = np.random.default_rng([seed, AB.ALL_TYPES.index(dtype)])
    src0 = rng.integers(0, 256, (int(cs.max()) + 9) * es, dtype=np.uint8).view(u).reshape(-1, nc)
    dst0 = rng.integers(0, 256, (int(cdst.max()) + 9) * es, dtype=np.uint8).view(u).reshape(-1, nc)
    src0[cs], dst0[cdst] = b, a
    exp, exp_src = dst0.copy(), src0.copy()
    exp[cdst] = AB.typed_add(dtype, a, b)
    exp_src[cs] = 0
    inside = np.zeros(exp.shape, dtype=bool)
    inside[cdst] = True
    names = []
    for flags in (0, GENERIC, STREAMING):
        d_src, d_dst = torch.from_numpy(src0.view(np.uint8).reshape(-1).copy()).cuda(), torch.from_numpy(dst0.view(np.uint8).reshape(-1).copy()).cuda()
        cd.cudecompExtRunMoves([cd.make_move(extent, ss, ds, so, do)], [d_src.data_ptr(), d_dst.data_ptr(), None], es, ADD_TAKE, dtype, None,
                               flags, None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        name = cd.cudecompExtLastKernelName()
        got = d_dst.cpu().numpy().view(u).reshape(-1, nc)
        where = (AB.NAMES[dtype], extent, ss, ds, so, do, flags, name)
        assert np.array_equal(got[~inside], exp[~inside]), ("a real outside the move changed",) + where
        bad = np.argwhere(AB.mismatches(kind, got, exp) & inside)
        assert bad.size == 0, where + tuple("cell %d real %d: gave %#x, expected %#x" % (c, r, got[c, r], exp[c, r]) for c, r in bad[:4]) + ("%d reals wrong" % len(bad),)
        assert np.array_equal(d_src.cpu().numpy().view(u).reshape(-1, nc), exp_src), ("the source is not cleared cell for cell",) + where
        names.append(name)
    return names


REAL_TYPES = [cd.HALF, cd.BFLOAT16, cd.FLOAT, cd.DOUBLE]


@pytest.mark.parametrize("dtype", REAL_TYPES, ids=[AB.NAMES[t] for t in REAL_TYPES])
def test_arithmetic_on_edge_values_and_dense_bit_patterns(dtype):
    """the add arithmetic is shared with kernels_accumulate.hip (kernels_arith.h): all 24 x 24 pairs of the edge table at every lane
    width the type has, and 2^16 reals per draw of uniformly random patterns, nearly cancelling pairs and subnormal operands"""
    kind, es = AB.kind_of(dtype), AB.element_bytes(dtype)
    a, b = AB.all_pairs(AB.edge_table(kind))
    a, b = a.reshape(-1, 1), b.reshape(-1, 1)
    exp = AB.classes(kind, AB.typed_add(dtype, a, b))
    assert exp["nan"].any() and exp["inf"].any() and exp["zero"].any() and exp["subnormal"].any()
    seen = set()
    for w, h, d in ((96, 3, 2), (36, 4, 4), (18, 8, 4), (9, 16, 4)):  # (lane widths 16, 8, 4, 2 for 2-byte elements)
        seen |= set(_add_take_bits(dtype, (w, h, d), (1, w + 6, (w + 6) * (h + 1)), (1, w + 2, (w + 2) * (h + 2)), 4, 8, a, b))
    t = CB.ARITH_NAMES[{cd.HALF: 1, cd.BFLOAT16: 2, cd.FLOAT: 3, cd.DOUBLE: 4}[dtype]]
    assert seen == {"rows_accumulate_take_kernel<%s,%d,%d>" % (t, vb, s) for vb in (16, 8, 4, 2) if vb >= es for s in (0, 1)} | \
        {"generic_accumulate_take_kernel<%s,1>" % t}, seen
    n = 1 << 16
    for name, (a, b) in AB.dense_draws(kind, n, 7).items():
        a, b = a.reshape(n, 1), b.reshape(n, 1)
        exp = AB.classes(kind, AB.typed_add(dtype, a, b))
        assert exp["subnormal"].any() and exp["zero"].any(), (kind, name)
        _add_take_bits(dtype, (512, n // 1024, 2), (1, 520, 520 * (n // 1024 + 1)), (1, 516, 516 * (n // 1024)), 0, 0, a, b, seed=1)


# ---- single rank -------------------------------------------------------------------------------------------------------------------
GDIMS = (11, 9, 7)
ORDERS = {"default": None, "contiguous": ((0, 1, 2), (1, 2, 0), (2, 0, 1)), "mixed": ((1, 0, 2), (2, 1, 0), (0, 2, 1))}
HALOS = [(1, 1, 1), (2, 0, 3), (3, 2, 1)]
PERIODS = [(1, 1, 1), (1, 0, 1), (0, 0, 0)]
PADDINGS = [(0, 0, 0), (1, 2, 0)]
FIVE_TYPES = [t for t in AB.ALL_TYPES if t not in (cd.DOUBLE, cd.HALF)]


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("halo", HALOS, ids=["h111", "h203", "h321"])
def test_single_rank_full_cross_fp64_fp16(layout, halo):
    """every axis, period mix, padding and dim; whole guarded pencils against the library's two calls and against numpy"""
    for periods, padding in itertools.product(PERIODS, PADDINGS):
        args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
                "dtypes": [cd.DOUBLE, cd.HALF]}
        assert CB.fused_sweep(0, 1, args) == []


@pytest.mark.parametrize("layout,halo,periods,padding", [("default", (3, 2, 1), (1, 1, 1), (1, 2, 0)), ("contiguous", (1, 1, 1), (1, 0, 1), (0, 0, 0)),
                                                         ("mixed", (2, 0, 3), (1, 1, 1), (1, 2, 0))], ids=["default", "contiguous", "mixed"])
def test_single_rank_other_types(layout, halo, periods, padding):
    args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
            "dtypes": FIVE_TYPES, "sequence": True}
    assert CB.fused_sweep(0, 1, args) == []


@pytest.mark.parametrize("layout", list(ORDERS))
def test_dims_in_sequence(layout):
    """fused along 2, 1, 0 equals, over the whole pencil, accumulate 2, 1, 0 then fill 0, 1, 2, and accumulate / fill interleaved
    per dim: a cleared ghost cell is only ever added into cells that are themselves cleared by the end"""
    for halo, periods, padding, payload in (((1, 1, 1), (1, 1, 1), (0, 0, 0), "typed"), ((3, 2, 1), (1, 0, 1), (1, 2, 0), "typed"),
                                            ((2, 0, 3), (0, 1, 1), (1, 2, 0), "ints"), ((3, 2, 1), (0, 0, 0), (0, 0, 0), "typed")):
        args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
                "dtypes": [cd.DOUBLE, cd.BFLOAT16, cd.FLOAT_COMPLEX], "dims": (), "sequence": True, "payload": payload}
        assert CB.fused_sweep(0, 1, args) == []


def test_interior_narrower_than_two_halos():
    """the ordered case: the two faces overlap, LF += H THEN HF += L, every sum rounds (typed payload), so the order shows in the
    bits; the shapes of tests/test_gpu_halo_accumulate.py.  On one rank (the wrap additions clear) and exchanging with itself
    (the packs clear, the ordered additions read the workspace)."""
    for gdims, halo in (((3, 5, 4), (2, 2, 2)), ((5, 3, 3), (3, 2, 3))):
        args = {"gdims": gdims, "pdims": (1, 1), "halo": halo, "periods": (1, 1, 1), "padding": (1, 0, 1), "sequence": True,
                "dtypes": [cd.DOUBLE, cd.FLOAT, cd.HALF, cd.BFLOAT16]}
        spec = cd.make_grid_spec(gdims, (1, 1), ((0, 1, 2),) * 3)
        assert any(cd.cudecompExtPlanHaloAccumulateClear(spec, 0, 0, halo, (1, 1, 1), dim, (1, 0, 1)).reserved & 2 for dim in range(3))
        assert CB.fused_sweep(0, 1, args) == []
        assert run_ranks(1, "tests.accumulate_clear_bodies", "fused_sweep", dict(args, halo_backend=cd.HALO_COMM_NVSHMEM), timeout=300,
                         extra_env=SELF)[0] == []


# ---- ranks sharing the GPU -------------------------------------------------------------------------------------------------------
def _jobs(pdims, backend):
    jobs = []
    for periods, halo, padding in (((1, 1, 1), (1, 2, 1), (0, 0, 0)), ((0, 0, 0), (2, 1, 2), (1, 0, 2)), ((1, 0, 1), (1, 1, 3), (0, 1, 0))):
        args = {"gdims": (10, 9, 11), "pdims": pdims, "halo_backend": backend, "halo": halo, "periods": periods, "padding": padding,
                "dtypes": [cd.DOUBLE, cd.HALF, cd.DOUBLE_COMPLEX], "sequence": True}
        jobs.append({"fn": "fused_sweep", "id": "hb%d P%dx%d periods %s halo %s" % ((backend,) + pdims + (periods, halo)), "args": args})
    return jobs


@pytest.mark.parametrize("nranks,pdims", [(2, (2, 1)), (4, (2, 2))], ids=["two_ranks", "four_ranks"])
@pytest.mark.parametrize("backend", [cd.HALO_COMM_MPI, cd.HALO_COMM_NVSHMEM], ids=["MPI", "NVSHMEM"])
def test_ranks_peer_transports(backend, nranks, pdims):
    """periodic, non-periodic and mixed; whole pencils on every rank against the two-call form run on the same ranks, and numpy"""
    for failures in run_ranks(nranks, "tests.accumulate_clear_bodies", "many", {"jobs": _jobs(pdims, backend)}, timeout=600):
        assert failures == []


@pytest.mark.parametrize("nranks,pdims", [(2, (2, 1)), (4, (2, 2))], ids=["two_ranks", "four_ranks"])
def test_ranks_rccl_stand_in(nranks, pdims):
    if not os.path.exists(SHIM):
        pytest.skip("tests/shim/libfake_rccl.so not built")
    for failures in run_ranks(nranks, "tests.accumulate_clear_bodies", "many", {"jobs": _jobs(pdims, cd.HALO_COMM_NCCL)}, timeout=600,
                              extra_env={"CUDECOMP_TEST_RCCL_SHIM": SHIM}):
        assert failures == []


def test_one_rank_real_rccl_with_a_single_member():
    """CUDECOMP_TEST_SELF_EXCHANGE=1: the rank is its own neighbour but packs (and clears), exchanges over real librccl and adds
    what arrived"""
    jobs = [{"fn": "fused_sweep", "id": "self %s" % (halo,), "args": {
        "gdims": (10, 9, 11), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "halo_backend": cd.HALO_COMM_NCCL, "halo": halo,
        "periods": periods, "padding": padding, "dtypes": [cd.DOUBLE, cd.HALF_COMPLEX], "sequence": True}}
        for halo, periods, padding in (((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((2, 3, 1), (1, 0, 1), (1, 0, 2)))]
    for failures in run_ranks(1, "tests.accumulate_clear_bodies", "many", {"jobs": jobs}, timeout=600, extra_env=SELF):
        assert failures == []


# ---- the deposit loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,pdims", [(1, (1, 1)), (2, (2, 1))], ids=["one_rank", "two_ranks"])
def test_deposit_loop(nranks, pdims):
    """three steps of deposit then fused 2, 1, 0 after a single initial fill, against the existing loop fill -- deposit --
    accumulate every step"""
    jobs = [{"fn": "deposit_loop", "id": "periods %s" % (periods,),
             "args": {"gdims": (12, 10, 9), "pdims": pdims, "halo_backend": cd.HALO_COMM_MPI, "halo": (1, 2, 1), "periods": periods,
                      "padding": padding, "dtypes": [cd.DOUBLE, cd.BFLOAT16]}}
            for periods, padding in (((1, 1, 1), (0, 0, 0)), ((1, 0, 1), (0, 1, 0)))]
    for failures in run_ranks(nranks, "tests.accumulate_clear_bodies", "many", {"jobs": jobs}, timeout=300):
        assert failures == []


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def test_captured_into_one_graph_on_a_single_rank():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 1, 1), "padding": (0, 1, 0)},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "axis": 1, "halo": (2, 1, 2),
                  "periods": (1, 0, 1)}):
        assert run_ranks(1, "tests.accumulate_clear_bodies", "graph_replay", args, timeout=300)[0] == []


def test_captured_with_pack_exchange_add_on_the_one_sided_transport():
    """one rank exchanging with itself over the stream-ordered one-sided transport: take-pack -> exchange -> add along 2, 1, 0
    captured into one hipGraph and replayed on fresh data"""
    args = {"gdims": (40, 36, 30), "pdims": (1, 1), "halo_backend": cd.HALO_COMM_NVSHMEM, "halo": (1, 2, 1), "periods": (1, 1, 1),
            "padding": (0, 1, 0)}
    assert run_ranks(1, "tests.accumulate_clear_bodies", "graph_replay", args, timeout=300, extra_env=SELF)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three fused calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (1, 1, 1)}
    res = run_ranks(1, "tests.accumulate_clear_bodies", "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["fused_host_ms"] < 0.25 * res["total_ms"], res
