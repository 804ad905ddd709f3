"""Halo fill (cudecomp_amd_fill.h: cudecompAmdFillHalos{X,Y,Z}) on the GPU: the fill kernels move by move (every byte of a
destination buffer with poison slack on both sides); single-rank pencils of every axis, memory order, halo width, period mix,
padding, dim and value against the numpy restatement of tests/fill_bodies.py; cudecompUpdateHalos as the oracle of WHICH bytes
change; four ranks sharing the GPU on a ragged 2 x 2 grid; the clear -- deposit -- accumulate loop the feature is for; capture
into a hipGraph; asynchrony.  Everything is compared byte for byte: there is no tolerance anywhere.

Fill values (tests/fill_bodies.py): all bytes of the element distinct, and NULL; buffers start filled with a poison byte that
occurs in neither."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fill_bodies as FB
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = 256  # poison bytes before and after everything a move may touch
ROWS_0, ROWS_STREAM = "rows_fill_kernel<16,0>", "rows_fill_kernel<16,1>"


# ---- kernel parity ---------------------------------------------------------------------------------------------------------
def _cells(extent, ds):
    """element offsets of the cells of a move"""
    k = [np.arange(int(e), dtype=np.int64) * int(d) for e, d in zip(extent, ds)]
    return (k[0][:, None, None] + k[1][None, :, None] + k[2][None, None, :]).reshape(-1)


def _fill(buf, es, extent, ds, offset, value, force, cells=None, shift=0):
    """one fill-move through cudecompExtFill3D at `offset` elements (and `shift` bytes) past the slack of the device buffer
    `buf`, poisoned first; EVERY byte of the buffer (the slack on both sides included) against numpy.  Returns (kernel class,
    kernel name)."""
    import torch
    cells = (_cells(extent, ds) if cells is None else cells) + offset
    nbytes = SLACK + shift + (int(cells.max()) + 1) * es + SLACK
    assert nbytes <= buf.numel() and (cells.size > (1 << 20) or np.unique(cells).size == cells.size)
    view = buf[:nbytes]
    view.fill_(FB.POISON)
    cls = cd.cudecompExtFill3D(buf.data_ptr() + SLACK + shift + offset * es, es, value, extent, ds, force,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    want = np.full(nbytes, FB.POISON, dtype=np.uint8)
    want[SLACK + shift:nbytes - SLACK].reshape(-1, es)[cells] = np.frombuffer(value, dtype=np.uint8) if value is not None else 0
    got = view.cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (es, extent, ds, offset, force, cls, name, "%d bytes differ, first at byte %d of the buffer (the move begins at %d)"
                           % (bad.size, bad[0], SLACK + shift + offset * es))
    return cls, name


def _check_choice(es, extent, ds, force, cls, name):
    """rows whose fastest dim is contiguous in the destination (or a single cell) take the row kernel, everything else and every
    forced case the element-wise one"""
    live = [(e, s) for e, s in zip(extent, ds) if e > 1]
    rows = not (force & 1) and (not live or min(s for _, s in live) == 1)
    if rows:
        assert (cls, name) == (0, ROWS_STREAM if force & 2 else ROWS_0), (es, extent, ds, force, cls, name)
    else:
        assert (cls, name) == (2, "generic_fill_kernel<%d>" % es), (es, extent, ds, force, cls, name)


LENGTHS = (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65, 127, 130, 1000, 1025)


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_rows(es):
    """element size x row length x base offset (0 .. 16 / es + 1 elements: every phase of the 16-byte grid, and one past it) x row
    pitch (length + 0, 1, 3: rows fused, rows at alternating phases, odd) x rows x planes; fast path, forced element-wise, forced
    streaming.  The value with distinct bytes everywhere, NULL on one case in seven."""
    import torch
    buf = torch.empty(2 * SLACK + (1028 * 37 + 5) * 3 * 16 + 64 * 16, dtype=torch.uint8, device="cuda")
    n = 0
    for length, extra, rows, planes in itertools.product(LENGTHS, (0, 1, 3), (1, 5, 37), (1, 3)):
        pitch = length + extra
        extent, ds = (length, rows, planes), (1, pitch, pitch * rows + 5)  # (planes never continue one another)
        cells = _cells(extent, ds)
        for offset, force in itertools.product(range(16 // es + 2), (0, 1, 2)):
            value = None if n % 7 == 3 else FB.value_bytes(es)
            n += 1
            cls, name = _fill(buf, es, extent, ds, offset, value, force, cells)
            _check_choice(es, extent, ds, force, cls, name)
            if es == 2 and offset % 2 == 1 and length * es >= 64 and force == 0:
                assert name == ROWS_0, "2-byte elements at 2 mod 4 keep the 16-byte lanes"


@pytest.mark.parametrize("es", [2, 4, 8, 16])
def test_kernel_parity_faces_one_element_thick(es):
    """the face along the fastest memory axis: extent (1, h, d), cells a row pitch apart -- the element-wise kernel by itself"""
    import torch
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for (h, d), pitch, offset, value in itertools.product(((9, 7), (37, 3), (1, 40), (300, 1)), (3, 16, 131), range(16 // es + 2),
                                                          (FB.value_bytes(es), None)):
        extent, ds = (1, h, d), (1, pitch, pitch * (h + 3))
        for force in (0, 1, 2):
            cls, name = _fill(buf, es, extent, ds, offset, value, force)
            assert (cls, name) == (2, "generic_fill_kernel<%d>" % es), (extent, ds, force, cls, name)
    # two cells per row along the fastest axis (halo 2): rows again
    cls, name = _fill(buf, es, (2, 9, 7), (1, 13, 13 * 11), 1, FB.value_bytes(es), 0)
    assert (cls, name) == (0, ROWS_0)


@pytest.mark.parametrize("es", [4, 8, 16])
def test_kernel_parity_elements_aligned_to_half_their_size(es):
    """complex elements need only the alignment of their real type: every cell es / 2 bytes off the element grid (for 16-byte
    elements also 4 and 12 bytes off).  An element then straddles two 16-byte slots at some phases, and the pattern a slot
    receives is the element rotated.  Rows, forced element-wise, forced streaming, and a face one element thick."""
    import torch
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    for shift in ((es // 2,) if es < 16 else (8, 4, 12)):
        for length, rows, offset, force in itertools.product((1, 2, 3, 7, 16, 33, 130), (1, 5), range(16 // es + 2), (0, 1, 2)):
            extent, ds = (length, rows, 3), (1, length + 1, (length + 1) * rows + 5)
            value = None if (length + offset) % 5 == 0 else FB.value_bytes(es)
            cls, name = _fill(buf, es, extent, ds, offset, value, force, shift=shift)
            _check_choice(es, extent, ds, force, cls, name)
        for offset in range(16 // es + 2):
            cls, name = _fill(buf, es, (1, 9, 7), (1, 13, 13 * 12), offset, FB.value_bytes(es), 0, shift=shift)
            assert (cls, name) == (2, "generic_fill_kernel<%d>" % es)


def test_kernel_parity_streaming_by_size_and_second_grid_stride_pass():
    import torch
    # 40 MiB in one contiguous move: non-temporal stores with no force bit; 32 MiB less one element: cached
    buf = torch.empty(2 * SLACK + (40 << 20) + 64, dtype=torch.uint8, device="cuda")
    assert _fill(buf, 8, (5 << 20, 1, 1), (1, 0, 0), 1, FB.value_bytes(8), 0) == (0, ROWS_STREAM)
    assert _fill(buf, 4, (2048, 4096, 1), (1, 2048, 0), 3, FB.value_bytes(4), 0) == (0, ROWS_STREAM)  # (32 MiB of fused rows)
    assert _fill(buf, 4, ((8 << 20) - 1, 1, 1), (1, 0, 0), 0, FB.value_bytes(4), 0) == (0, ROWS_0)
    # the element-wise kernel launches at most 8192 workgroups of 256 lanes: more elements than that take a second pass
    assert _fill(buf, 2, (8192 * 256 + 257, 1, 1), (1, 0, 0), 1, FB.value_bytes(2), 1) == (2, "generic_fill_kernel<2>")
    assert _fill(buf, 4, (1, 1500, 1400), (0, 2, 3002), 2, FB.value_bytes(4), 0) == (2, "generic_fill_kernel<4>")


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
    """every axis, period mix, padding, dim and value; whole pencils against the restatement"""
    for periods, padding in itertools.product(PERIODS, PADDINGS):
        args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
                "dtypes": [cd.DOUBLE, cd.HALF]}
        assert FB.fill_sweep(0, 1, args) == []


@pytest.mark.parametrize("layout,halo,periods,padding", [("default", (3, 2, 1), (1, 1, 1), (1, 2, 0)), ("contiguous", (1, 1, 1), (1, 0, 1), (0, 0, 0)),
                                                         ("mixed", (2, 0, 3), (1, 1, 1), (1, 2, 0))], ids=["default", "contiguous", "mixed"])
def test_single_rank_other_types(layout, halo, periods, padding):
    # the five other element types on every axis and dim; also dims 0, 1, 2 on one pencil, in two orders
    args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
            "dtypes": OTHER_TYPES, "all_dims": True}
    assert FB.fill_sweep(0, 1, args) == []


def test_all_dims_cover_every_ghost_cell_when_periodic():
    """halo_periods all true, dims 0, 1, 2: every cell that is neither interior nor padding holds the value, edges and corners
    included, and nothing else changed"""
    import torch
    from tests.half_bodies import global_index
    from tests import gpu_bodies as B
    halo, padding = (1, 2, 1), (1, 0, 2)
    h, gd, g = B._setup(0, 1, {"gdims": GDIMS, "pdims": (1, 1)})
    for axis in range(3):
        p = g.pencil_info(0, axis, halo, padding)
        data = torch.full((int(p.size) * 4,), FB.POISON, dtype=torch.uint8, device="cuda")
        for dim in (1, 2, 0):
            cd.cudecompFillHalos(axis, h, gd, data.data_ptr(), cd.FLOAT, halo, (1, 1, 1), dim, padding, FB.value_bytes(4),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ghost = np.zeros(int(p.size), dtype=bool)  # not padding ...
        AB.pencil3(p, ghost)[tuple(slice(0, int(p.shape[k]) - int(p.padding[int(p.order[k])])) for k in (2, 1, 0))] = True
        ghost &= global_index(p, GDIMS) < 0        # ... and not interior
        want = np.full((int(p.size), 4), FB.POISON, dtype=np.uint8)
        want[ghost] = np.frombuffer(FB.value_bytes(4), dtype=np.uint8)
        assert ghost.any() and np.array_equal(data.cpu().numpy(), want.reshape(-1)), axis
    cd.cudecompGridDescDestroy(h, gd)


# ---- the update as the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,halo,periods,padding", [("default", (1, 1, 1), (1, 1, 1), (0, 0, 0)), ("default", (3, 2, 1), (1, 0, 1), (1, 2, 0)),
                                                         ("contiguous", (2, 0, 3), (1, 1, 1), (1, 2, 0)), ("mixed", (3, 2, 1), (0, 0, 0), (0, 0, 0)),
                                                         ("mixed", (1, 1, 1), (1, 1, 0), (1, 2, 0))])
def test_the_update_changes_the_same_bytes(layout, halo, periods, padding):
    args = {"gdims": GDIMS, "pdims": (1, 1), "mem_order": ORDERS[layout], "halo": halo, "periods": periods, "padding": padding,
            "dtypes": [cd.DOUBLE, cd.HALF, cd.FLOAT_COMPLEX]}
    assert FB.update_as_oracle(0, 1, args) == []


# ---- four ranks sharing the GPU --------------------------------------------------------------------------------------------
def test_four_ranks_ragged_grid():
    """2 x 2 ranks, gdims (10, 9, 11): slabs of 5 + 5, 5 + 4 and 6 + 5 cells.  Periodic, non-periodic (edge ranks keep their outer
    sides: every rank is an edge rank here) and mixed; whole pencils on every rank; the update as the oracle across ranks too.
    One halo backend: the call does not communicate."""
    jobs = []
    for periods, halo, padding in (((1, 1, 1), (1, 2, 1), (0, 0, 0)), ((0, 0, 0), (2, 1, 2), (1, 0, 2)), ((1, 0, 1), (1, 1, 3), (0, 1, 0))):
        args = {"gdims": (10, 9, 11), "pdims": (2, 2), "halo_backend": cd.HALO_COMM_MPI, "halo": halo, "periods": periods,
                "padding": padding, "dtypes": [cd.DOUBLE, cd.HALF, cd.DOUBLE_COMPLEX], "all_dims": True}
        jobs.append({"fn": "fill_sweep", "id": "periods %s halo %s" % (periods, halo), "args": args})
        jobs.append({"fn": "update_as_oracle", "id": "update, periods %s halo %s" % (periods, halo), "args": dict(args, dtypes=[cd.DOUBLE])})
    for failures in run_ranks(4, "tests.fill_bodies", "many", {"jobs": jobs}, timeout=300):
        assert failures == []


# ---- the deposit loop --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,pdims", [(1, (1, 1)), (2, (2, 1))], ids=["one_rank", "two_ranks"])
def test_deposit_loop(nranks, pdims):
    jobs = [{"fn": "deposit_loop", "id": "periods %s" % (periods,),
             "args": {"gdims": (12, 10, 9), "pdims": pdims, "halo_backend": cd.HALO_COMM_MPI, "halo": (1, 2, 1), "periods": periods,
                      "padding": padding, "dtypes": [cd.DOUBLE, cd.BFLOAT16]}}
            for periods, padding in (((1, 1, 1), (0, 0, 0)), ((1, 0, 1), (0, 1, 0)))]
    for failures in run_ranks(nranks, "tests.fill_bodies", "many", {"jobs": jobs}, timeout=300):
        assert failures == []


# ---- hipGraph, asynchrony --------------------------------------------------------------------------------------------------
def test_captured_fill_keeps_the_captured_value():
    for args in ({"gdims": (40, 36, 30), "pdims": (1, 1), "halo": (1, 2, 1), "periods": (1, 1, 1), "padding": (0, 1, 0)},
                 {"gdims": (33, 20, 27), "pdims": (1, 1), "mem_order": ORDERS["contiguous"], "axis": 1, "halo": (2, 1, 2),
                  "periods": (1, 0, 1), "dtype": cd.HALF}):
        assert run_ranks(1, "tests.fill_bodies", "graph_replay", args, timeout=300)[0] == []


def test_calls_return_before_the_gpu_is_done():
    """100 kernels over 1 GiB each are enqueued first; the three fill calls return while they run"""
    args = {"gdims": (64, 48, 40), "pdims": (1, 1), "halo": (1, 1, 1), "periods": (1, 1, 1)}
    res = run_ranks(1, "tests.fill_bodies", "returns_before_the_gpu_is_done", args, timeout=300)[0]
    assert res["failures"] == [], res
    assert res["pending_after_the_calls"], res
    assert res["fill_host_ms"] < 0.25 * res["total_ms"], res
