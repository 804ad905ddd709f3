"""How the interior combinations (cudecomp_interior_combine.h) would run, without a GPU: cudecompExtDescribeCombine3D over the sweep
of tests/test_interior_reduce_plan.py -- row lengths, two pitches, every phase of the 16-byte grid, the seven data types, a readable
range of 0 or 16 bytes around the box, forced and unforced, the four operations.  Held: the form follows the stated rules (rows
against elements for a misaligned field, unequal phases of x and y, a complex field off its element boundary, a forced class);
contiguous dims merge and a long row is cut into rows of 4080 bytes; an empty box makes no launch; the lowest and the highest byte read
of x and of y lie inside the readable range and equal the kernel's decode mirrored over every row; AX reads nothing of y; the bytes
stored, by a host mirror of the row kernel's slot decode, are exactly the bytes of the box's cells; and the new kinds come after the
plane updates'."""
import itertools

import pytest

import cudecomp_amd as cd
from tests.test_interior_planes_plan import K_GENERIC_PLANES, K_ROWS_PLANES, bytes_of_the_box, bytes_stored
from tests.test_interior_reduce_plan import BASE, TYPES, bytes_read_row_by_row, span_of, sweep

K_ROWS_COMBINE, K_GENERIC_COMBINE = 51, 52
OPS = (cd.COMBINE_AXPY, cd.COMBINE_XPBY, cd.COMBINE_AXPBY, cd.COMBINE_AX)
IDS = ["fp16", "bf16", "complex_fp16", "fp32", "complex64", "fp64", "complex128"]
FAR = 1 << 20  # x lies this many bytes above y: the same phase of the 16-byte grid


@pytest.mark.parametrize("dtype", list(TYPES), ids=IDS)
def test_exactly_the_bytes_of_the_box_are_stored_and_no_load_leaves_the_readable_range(dtype):
    rs, nc = TYPES[dtype]
    es, n, kinds = rs * nc, 0, set()
    for (extent, strides, address), op, around, force in itertools.product(sweep(dtype), OPS, (0, 16), (0, 1)):
        d = cd.cudecompExtDescribeCombine3D(address, address + FAR, dtype, op, extent, strides, around, around, force)
        what = (dtype, extent, strides, address - BASE, op, around, force, d)
        span = span_of(extent, strides, es)
        assert -around <= d["read_x_lo"] <= 0 and span <= d["read_x_hi"] <= span + around, what
        assert (d["write_lo"], d["write_hi"]) == (0, span), what
        if op == cd.COMBINE_AX:
            assert (d["read_y_lo"], d["read_y_hi"]) == (0, 0), what
        else:
            assert (d["read_y_lo"], d["read_y_hi"]) == (d["read_x_lo"], d["read_x_hi"]), what
        # rows unless forced; a complex field sits on a boundary of its element (the sweep's addresses are on boundaries of the real)
        kind = K_GENERIC_COMBINE if force & 1 or address % es else K_ROWS_COMBINE
        kinds.add(kind)
        assert d["kind"] == kind and d["vec"] == (es if kind == K_GENERIC_COMBINE else 16) and d["blocks"] >= 1, what
        if kind == K_GENERIC_COMBINE:
            assert (d["read_x_lo"], d["read_x_hi"]) == (0, span), what
        else:
            assert (d["read_x_lo"], d["read_x_hi"]) == bytes_read_row_by_row(address, extent, strides, es, around, around), what
            if around == 0:  # (what is stored does not depend on what may be read): the planes' mirror of the same slot decode
                stored, union = bytes_stored(K_ROWS_PLANES, dtype, address, extent, strides)
                assert union == bytes_of_the_box(extent, strides, es), what
                assert sum(b - a for a, b in stored) == sum(b - a for a, b in union), what  # no byte is stored twice
                assert (union[0][0], union[-1][1]) == (d["write_lo"], d["write_hi"]), what
        n += 1
    assert n == 9 * 2 * 3 * (16 // rs) * 4 * 2 * 2
    assert kinds == ({K_ROWS_COMBINE, K_GENERIC_COMBINE})


def test_rows_against_elements_for_each_cause():
    box = ((33, 4, 2), (1, 40, 200), 64, 64)
    for op in OPS:
        describe = lambda y, x, dtype=cd.FLOAT, force=0: cd.cudecompExtDescribeCombine3D(y, x, dtype, op, *box, force)["kind"]  # noqa: E731
        assert describe(BASE, BASE + FAR) == K_ROWS_COMBINE
        assert describe(BASE + 4, BASE + FAR + 4) == K_ROWS_COMBINE and describe(BASE + 12, BASE + FAR + 28) == K_ROWS_COMBINE
        # a misaligned field: y or x off the boundary of its real
        assert describe(BASE + 2, BASE + FAR + 2) == K_GENERIC_COMBINE
        assert describe(BASE + 1, BASE + FAR + 1) == K_GENERIC_COMBINE
        # unequal phases of x and y on the 16-byte grid
        for shift in (4, 8, 12):
            assert describe(BASE, BASE + FAR + shift) == K_GENERIC_COMBINE, shift
            assert describe(BASE + shift, BASE + FAR) == K_GENERIC_COMBINE, shift
        # a complex field off its element boundary, x and y at one phase all the same
        assert describe(BASE + 8, BASE + FAR + 8, cd.FLOAT_COMPLEX) == K_ROWS_COMBINE
        assert describe(BASE + 4, BASE + FAR + 4, cd.FLOAT_COMPLEX) == K_GENERIC_COMBINE
        assert describe(BASE + 8, BASE + FAR + 8, cd.DOUBLE_COMPLEX) == K_GENERIC_COMBINE
        assert describe(BASE + 2, BASE + FAR + 2, cd.HALF_COMPLEX) == K_GENERIC_COMBINE
        assert describe(BASE + 4, BASE + FAR + 4, cd.HALF_COMPLEX) == K_ROWS_COMBINE
        # a forced class
        assert describe(BASE, BASE + FAR, force=1) == K_GENERIC_COMBINE
        # no contiguous dim
        d = cd.cudecompExtDescribeCombine3D(BASE, BASE + FAR, cd.DOUBLE, op, (5, 4, 3), (2, 12, 60))
        assert (d["kind"], d["vec"], d["write_lo"], d["write_hi"]) == (K_GENERIC_COMBINE, 8, 0, span_of((5, 4, 3), (2, 12, 60), 8)), d


def test_contiguous_dims_merge_and_a_long_row_is_cut():
    cap = 2048  # csrc/kernels_batch.h kCombineBlocks
    for extent, strides, row_bytes, rows, last, blocks in (
            ((512, 512, 512), (1, 512, 512 * 512), 4080, -(-(1 << 30) // 4080), (1 << 30) % 4080, cap),  # contiguous: one long row of 2^30 bytes, cut
            ((512, 512, 512), (1, 514, 514 * 514), 4096, 512 * 512, 4096, cap),   # 4-KiB rows with gaps: nothing merges
            ((512, 4, 512), (1, 512, 512 * 6), 16384, 512, 16384, 640),           # dims 0 and 1 merge: rows of 16 KiB, 5 tile columns x 128 tile rows of four
            ((8, 512, 4), (1, 9, 9 * 512), 64, 2048, 64, 16),                     # dims 1 and 2 merge: 2048 rows, 8 lanes each, 128 rows per tile
            ((600, 1, 1), (1, 600, 600), 4080, 2, 720, 1),                        # 4800 bytes: two rows, the second what is left
            ((510, 1, 1), (1, 510, 510), 4080, 1, 4080, 1),                       # exactly one chunk: not cut
            ((256, 4, 1), (1, 256, 1024), 4080, 3, 32, 1),                        # merged: 8 KiB are three cut rows
            ((1, 1, 1), (1, 1, 1), 8, 1, 8, 1), ((7, 1, 1), (1, 7, 7), 56, 1, 56, 1)):
        for op in OPS:
            d = cd.cudecompExtDescribeCombine3D(BASE, BASE + FAR * 4096, cd.DOUBLE, op, extent, strides, 1 << 20, 1 << 20)
            assert d["kind"] == K_ROWS_COMBINE, (extent, strides, d)
            assert (d["row_bytes"], d["rows"], d["last_row_bytes"], d["blocks"]) == (row_bytes, rows, last, blocks), (extent, strides, d)


def test_large_boxes_take_the_row_form_and_fill_the_device():
    for extent, dtype in itertools.product(((512, 512, 512), (514, 3, 70000), (2, 100000, 300), (1 << 20, 4, 4), (3, 5, 1 << 22)),
                                           (cd.HALF, cd.DOUBLE_COMPLEX)):
        pitch = (extent[0] + 7) // 8 * 8
        strides = (1, pitch, pitch * extent[1])
        es = 2 if dtype == cd.HALF else 16
        for op in OPS:
            d = cd.cudecompExtDescribeCombine3D(BASE, BASE + (1 << 40), dtype, op, extent, strides, 1 << 20, 1 << 20)
            assert d["kind"] == K_ROWS_COMBINE and 256 <= d["blocks"] <= 2048, (extent, d)
            assert (d["write_lo"], d["write_hi"]) == (0, span_of(extent, strides, es)), (extent, d)


def test_an_empty_box_makes_no_launch():
    for extent, op in itertools.product(((0, 4, 4), (4, 0, 4), (4, 4, 0)), OPS):
        d = cd.cudecompExtDescribeCombine3D(BASE, BASE + FAR, cd.DOUBLE, op, extent, (1, 8, 64))
        assert all(d[k] == 0 for k in ("blocks", "read_x_lo", "read_x_hi", "read_y_lo", "read_y_hi", "write_lo", "write_hi")), d


def test_the_new_kinds_come_after_the_plane_updates():
    assert K_GENERIC_PLANES < K_ROWS_COMBINE < K_GENERIC_COMBINE
    d = cd.cudecompExtDescribeCombine3D(BASE, BASE + FAR, cd.DOUBLE, 0, (8, 4, 4), (1, 9, 40))
    assert d["kind"] == K_ROWS_COMBINE == K_ROWS_PLANES + 3
    assert cd.cudecompExtDescribePlanes3D(BASE, cd.DOUBLE, 0, 1, (8, 4, 4), (1, 9, 40))["kind"] == K_ROWS_PLANES == 48  # (the pinned choices stay)


def test_bad_arguments_of_the_describing_entry_are_refused():
    for args in ((BASE, BASE + FAR, 99, 0, (4, 4, 4), (1, 4, 16)), (BASE, BASE + FAR, cd.DOUBLE, 4, (4, 4, 4), (1, 4, 16)),
                 (BASE, BASE + FAR, cd.DOUBLE, -1, (4, 4, 4), (1, 4, 16)), (BASE, BASE + FAR, cd.DOUBLE, 0, (4, -4, 4), (1, 4, 16)),
                 (BASE, BASE + FAR, cd.DOUBLE, 0, (4, 4, 4), (1, -4, 16)), (BASE, BASE + FAR, cd.DOUBLE, 0, (4, 4, 4), (1, 4, 16), -1, 0)):
        with pytest.raises(cd.CudecompError) as e:
            cd.cudecompExtDescribeCombine3D(*args)
        assert e.value.code == cd.RESULT_INVALID_USAGE
