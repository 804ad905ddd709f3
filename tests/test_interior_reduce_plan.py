"""How the interior reductions (cudecomp_interior_reduce.h) would run, without a GPU: cudecompExtDescribeReduce3D over the sweep the
GPU tests run on the device -- row lengths, pitches, every phase of the 16-byte grid, the four real sizes, real and complex elements,
and a readable range of 0 or 16 bytes around the box.  What no GPU test can check without faulting is checked here: the lowest and
the highest byte a launch reads lie inside the readable range, for the first and the last row too.  Also: the workgroups per field
stay under the cap the workspace size stands for, the kernel kinds, and the library's code objects (17, each below 400,000 bytes)."""
import itertools
import os

import pytest

import cudecomp_amd as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_ROWS_REDUCE, K_GENERIC_REDUCE = 43, 44
LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130)
# data type -> (bytes of one real, reals per element): the four real sizes, real and complex
TYPES = {cd.HALF: (2, 1), cd.BFLOAT16: (2, 1), cd.HALF_COMPLEX: (2, 2), cd.FLOAT: (4, 1), cd.FLOAT_COMPLEX: (4, 2), cd.DOUBLE: (8, 1),
         cd.DOUBLE_COMPLEX: (8, 2)}
BASE = 1 << 32


def sweep(dtype):
    """(extent, strides, first-cell address) of the sweep: rows of every length with pitch + 0 and + 3, at every phase of the 16-byte
    grid a real of the type can have"""
    rs, nc = TYPES[dtype]
    for length, extra, (rows, planes) in itertools.product(LENGTHS, (0, 3), ((1, 1), (3, 2), (5, 1))):
        pitch = length + extra
        for phase in range(0, 16, rs):
            yield (length, rows, planes), (1, pitch, pitch * rows + 5), BASE + phase


def span_of(extent, strides, es):
    return (sum((e - 1) * s for e, s in zip(extent, strides)) + 1) * es


def bytes_read_row_by_row(address, extent, strides, es, before, after):
    """(lowest byte read, one past the highest) relative to `address`, by the row kernel's own decode applied to every row of the
    box: a row at byte offset row_off holds bytes [ph, ph + n) of its 16-byte slots, ph the phase of its address; slot c is read
    as one aligned vector when it lies wholly inside the readable range, and otherwise only where it overlaps the row"""
    span = span_of(extent, strides, es)
    n = extent[0] * es
    lo, hi = None, None
    for k in range(extent[2]):
        for j in range(extent[1]):
            row_off = (j * strides[1] + k * strides[2]) * es
            ph = (address + row_off) % 16
            for c in range((ph + n + 15) // 16):
                first, end = max(16 * c, ph), min(16 * c + 16, ph + n)
                if first >= end:
                    continue
                slot_off = row_off - ph + 16 * c
                if slot_off >= -before and slot_off + 16 <= span + after:
                    a, b = slot_off, slot_off + 16
                else:
                    a, b = row_off - ph + first, row_off - ph + end
                lo, hi = (a if lo is None else min(lo, a)), (b if hi is None else max(hi, b))
    return lo, hi


@pytest.mark.parametrize("dtype", list(TYPES), ids=["fp16", "bf16", "complex_fp16", "fp32", "complex64", "fp64", "complex128"])
def test_no_launch_reads_outside_the_readable_range(dtype):
    """What keeps a launch inside the range is the row kernel's test of every vector (`slot_off >= rd_lo && slot_off + 16 <=
    rd_hi`, else the reals inside the row only); planReduce's read_lo / read_hi are a closed form of its outcome for the box's first
    and last cell.  Held here: the closed form lies in the range, and equals the kernel's decode mirrored on the host over EVERY
    row, so a plan whose row offsets or phases the closed form does not describe shows.  The kernel's branch itself runs on the
    device in tests/test_gpu_interior_reduce.py::test_kernel_parity with nothing readable around a box off the 16-byte grid."""
    rs, nc = TYPES[dtype]
    es, n = rs * nc, 0
    for (extent, strides, address), op, before, after, force in itertools.product(sweep(dtype), (0, 1, 2), (0, 16), (0, 16), (0, 1)):
        d = cd.cudecompExtDescribeReduce3D(address, address + (1 << 20), dtype, op, extent, strides, before, after, force)
        what = (dtype, extent, strides, address - BASE, op, before, after, force, d)
        span = span_of(extent, strides, es)
        assert -before <= d["read_lo"] <= 0 and span <= d["read_hi"] <= span + after, what
        assert 1 <= d["blocks"] <= cd.REDUCE_MAX_BLOCKS, what
        # rows unless forced; a complex dot product pairs the two reals of an element inside one aligned vector
        split = op == cd.REDUCE_DOT and nc == 2 and (address % es) != 0
        if force & 1 or split:
            assert (d["kind"], d["vec"]) == (K_GENERIC_REDUCE, es), what
            assert (d["read_lo"], d["read_hi"]) == (0, span), what
        else:
            assert (d["kind"], d["vec"]) == (K_ROWS_REDUCE, 16), what
            # whole aligned vectors where the range holds them, the cells alone where it does not
            below, above = address % 16, -(address + span) % 16
            whole = lambda slot: -before <= slot and slot + 16 <= span + after  # noqa: E731
            assert d["read_lo"] == (-below if whole(-below) else 0), what
            assert d["read_hi"] == (span + above if whole(span + above - 16) else span), what
            assert (address + d["read_lo"]) % 16 == 0 or d["read_lo"] == 0, what
            # ... and that is what the kernel's decode gives when it is applied to every row, not only to the first and last cell
            assert (d["read_lo"], d["read_hi"]) == bytes_read_row_by_row(address, extent, strides, es, before, after), what
        n += 1
    assert n == 9 * 2 * 3 * (16 // rs) * 3 * 2 * 2 * 2


def test_operands_of_a_dot_product_off_each_others_grid_go_element_by_element():
    for shift, kind in ((0, K_ROWS_REDUCE), (16, K_ROWS_REDUCE), (8, K_GENERIC_REDUCE), (4, K_GENERIC_REDUCE)):
        d = cd.cudecompExtDescribeReduce3D(BASE, BASE + 4096 + shift, cd.FLOAT, cd.REDUCE_DOT, (33, 4, 2), (1, 40, 200), 64, 64)
        assert d["kind"] == kind, (shift, d)
        d = cd.cudecompExtDescribeReduce3D(BASE, BASE + 4096 + shift, cd.FLOAT, cd.REDUCE_SUM, (33, 4, 2), (1, 40, 200), 64, 64)
        assert d["kind"] == K_ROWS_REDUCE, (shift, d)  # (b is not looked at)
    # no contiguous dim: element by element
    d = cd.cudecompExtDescribeReduce3D(BASE, 0, cd.DOUBLE, cd.REDUCE_SUM, (5, 4, 3), (2, 12, 60))
    assert (d["kind"], d["vec"]) == (K_GENERIC_REDUCE, 8), d


def test_workgroups_stay_under_the_cap_and_rows_merge():
    """the cap is what keeps the workspace at n_fields * 32 KiB: boxes of any size"""
    cap = cd.REDUCE_MAX_BLOCKS
    for extent, strides, blocks in (
            ((512, 512, 512), (1, 512, 512 * 512), cap),            # contiguous: one long row, cut into rows of 4080 bytes
            ((512, 512, 512), (1, 514, 514 * 514), cap),            # 4-KiB rows, four per tile
            ((256, 4, 1), (1, 256, 1024), 1),                       # merged: 8 KiB are three cut rows, one tile
            ((256, 4, 257), (1, 258, 258 * 6), 257),                # four rows per tile and plane: more partials than stage two has lanes
            ((256, 4, 2049), (1, 258, 258 * 6), cap),               # more tiles than the cap: the stride loop takes a second pass
            ((1, 1, 1), (1, 1, 1), 1), ((7, 1, 1), (1, 7, 7), 1)):
        d = cd.cudecompExtDescribeReduce3D(BASE, 0, cd.DOUBLE, cd.REDUCE_SUM, extent, strides, 1 << 20, 1 << 20)
        assert d["kind"] == K_ROWS_REDUCE and d["blocks"] == blocks, (extent, strides, d)
    # an empty box: no stage one, nothing read
    for extent in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        d = cd.cudecompExtDescribeReduce3D(BASE, 0, cd.DOUBLE, cd.REDUCE_SUM, extent, (1, 8, 64))
        assert (d["blocks"], d["read_lo"], d["read_hi"]) == (0, 0, 0), d
    assert cd.cudecompAmdReduceInteriorWorkspaceBytes(32) == 32 * cap * 16 <= 1 << 20


def test_bad_arguments_of_the_describing_entry_are_refused():
    for args in ((BASE, 0, 99, 0, (4, 4, 4), (1, 4, 16)), (BASE, 0, cd.DOUBLE, 3, (4, 4, 4), (1, 4, 16)),
                 (BASE, 0, cd.DOUBLE, 0, (4, -4, 4), (1, 4, 16)), (BASE, 0, cd.DOUBLE, 0, (4, 4, 4), (1, -4, 16))):
        with pytest.raises(cd.CudecompError) as e:
            cd.cudecompExtDescribeReduce3D(*args)
        assert e.value.code == cd.RESULT_INVALID_USAGE


def test_the_library_keeps_its_seventeen_code_objects():
    from tests.test_abi import _code_objects
    sizes = _code_objects(os.path.join(ROOT, "cudecomp_amd", "lib", "libcudecomp.so"))
    assert len(sizes) == 17, sizes
    assert max(sizes) < 400_000, sizes
