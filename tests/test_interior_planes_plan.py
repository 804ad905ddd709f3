"""How the interior plane updates (cudecomp_interior_planes.h) would run, without a GPU: cudecompExtDescribePlanes3D over the sweep of
tests/test_interior_profile_plan.py -- row lengths, three pitches, every phase of the 16-byte grid, the kept dim at each memory
position, the seven data types, a readable range of 0 or 16 bytes around the box, forced and unforced.  The kernels update in
place, so what counts most is what they STORE: the set of bytes stored, by a host mirror of the kernels' slot decode over every row,
equals the bytes of the box's cells exactly; write_lo / write_hi are 0 and the box's span; the lowest and the highest byte read lie
inside the readable range; the form follows the stated rules; an empty box makes no launch."""
import itertools

import pytest

import cudecomp_amd as cd
from tests.test_interior_profile_plan import IDS, sweep
from tests.test_interior_reduce_plan import BASE, TYPES, bytes_read_row_by_row, span_of

K_ROWS_PLANES, K_COLUMNS_PLANES, K_GENERIC_PLANES = 48, 49, 50
OPS = (cd.PLANES_ADD, cd.PLANES_MUL)


def contiguous_dim(extent, strides):
    """planPlanes' rule: of stride 1, and of several such the one longer than a cell"""
    c = None
    for d in range(3):
        if strides[d] == 1 and (c is None or (extent[c] == 1 and extent[d] > 1)):
            c = d
    return c


def expected_kind(dtype, op, keep, extent, strides, address, force):
    """the rules of csrc/kernels.h planPlanes"""
    rs, nc = TYPES[dtype]
    es = rs * nc
    c = contiguous_dim(extent, strides)
    if force & 1 or c is None or address % rs or (op == cd.PLANES_MUL and nc == 2 and address % es):
        return K_GENERIC_PLANES
    if keep != c:
        return K_ROWS_PLANES
    others = [d for d in range(3) if d != keep and extent[d] > 1]
    return K_COLUMNS_PLANES if all((strides[d] * es) % 16 == 0 for d in others) else K_GENERIC_PLANES


def merged(intervals):
    out = []
    for a, b in sorted(intervals):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def bytes_of_the_box(extent, strides, es):
    """the cells' bytes relative to the first cell, as merged intervals (the sweep's dim 0 has stride 1)"""
    assert strides[0] == 1
    return merged([((j * strides[1] + k * strides[2]) * es, (j * strides[1] + k * strides[2] + extent[0]) * es)
                   for k in range(extent[2]) for j in range(extent[1])])


def bytes_stored(kind, dtype, address, extent, strides):
    """the kernels' decode on the host (csrc/kernels_planes.hip): the fast forms walk the 16-byte slots of every row of the contiguous
    dim -- a slot wholly inside the row is one 16-byte store, any other is stored real by real where a WHOLE real lies inside the
    row -- the row kernel with each row's own phase, the column kernel with the phase of the box's first cell for all rows; the
    element-wise kernel stores each cell.  Returns (intervals as stored, with overlaps kept; merged intervals)."""
    rs, nc = TYPES[dtype]
    es = rs * nc
    stored = []
    if kind == K_GENERIC_PLANES:
        for k, j, i in itertools.product(range(extent[2]), range(extent[1]), range(extent[0])):
            off = (i * strides[0] + j * strides[1] + k * strides[2]) * es
            stored.append((off, off + es))
        return stored, merged(stored)
    c = contiguous_dim(extent, strides)
    o1, o2 = [d for d in range(3) if d != c]
    n = extent[c] * es
    slots = (n + 14 + 15) // 16
    for b, a in itertools.product(range(extent[o2]), range(extent[o1])):
        row_off = (a * strides[o1] + b * strides[o2]) * es
        ph = (address if kind == K_COLUMNS_PLANES else address + row_off) % 16
        for col in range(slots):
            first, end = max(16 * col, ph), min(16 * col + 16, ph + n)
            if first >= end:
                continue
            lo, hi, slot_off = first - 16 * col, end - 16 * col, row_off - ph + 16 * col
            if (lo, hi) == (0, 16):
                stored.append((slot_off, slot_off + 16))
            else:
                stored.extend((slot_off + q * rs, slot_off + q * rs + rs) for q in range(16 // rs) if lo <= q * rs and q * rs + rs <= hi)
    return stored, merged(stored)


@pytest.mark.parametrize("dtype", list(TYPES), ids=IDS)
def test_exactly_the_bytes_of_the_box_are_stored_and_no_load_leaves_the_readable_range(dtype):
    rs, nc = TYPES[dtype]
    es, n, kinds = rs * nc, 0, set()
    for (extent, strides, address), keep, op, around, force in itertools.product(sweep(dtype), range(3), OPS, (0, 16), (0, 1)):
        d = cd.cudecompExtDescribePlanes3D(address, dtype, op, keep, extent, strides, around, around, force)
        what = (dtype, extent, strides, address - BASE, keep, op, around, force, d)
        span = span_of(extent, strides, es)
        assert -around <= d["read_lo"] <= 0 and span <= d["read_hi"] <= span + around, what
        assert (d["write_lo"], d["write_hi"]) == (0, span), what
        kind = expected_kind(dtype, op, keep, extent, strides, address, force)
        kinds.add(kind)
        assert d["kind"] == kind and d["vec"] == (es if kind == K_GENERIC_PLANES else 16) and d["blocks"] >= 1, what
        if kind == K_GENERIC_PLANES:
            assert (d["read_lo"], d["read_hi"]) == (0, span), what
        elif strides[1] != 1:  # (rows of one cell at pitch 1 lie along dim 1: the reduce test's mirror takes dim 0 for the rows)
            assert (d["read_lo"], d["read_hi"]) == bytes_read_row_by_row(address, extent, strides, es, around, around), what
        if around == 0:  # (what is stored does not depend on what may be read)
            stored, union = bytes_stored(kind, dtype, address, extent, strides)
            assert union == bytes_of_the_box(extent, strides, es), what
            assert sum(b - a for a, b in stored) == sum(b - a for a, b in union), what  # no byte is stored twice
            assert (union[0][0], union[-1][1]) == (d["write_lo"], d["write_hi"]), what
        n += 1
    assert n == 9 * 3 * 3 * (16 // rs) * 3 * 2 * 2 * 2
    assert kinds == {K_ROWS_PLANES, K_COLUMNS_PLANES, K_GENERIC_PLANES}


def test_the_mirror_notices_a_slot_stored_whole_at_a_row_end():
    """the check above has teeth: a decode that stored every touched slot whole would store bytes outside the box"""
    extent, strides, address = (7, 3, 2), (1, 10, 35), BASE + 4
    stored, union = bytes_stored(K_ROWS_PLANES, cd.FLOAT, address, extent, strides)
    assert union == bytes_of_the_box(extent, strides, 4)
    widened = merged([(a - (address + a) % 16, a - (address + a) % 16 + 16) for a, b in stored])
    assert widened != union


def test_boxes_off_the_grid_go_element_by_element():
    box = ((33, 4, 2), (1, 40, 200), 64, 64)
    for keep, fast in ((0, K_COLUMNS_PLANES), (1, K_ROWS_PLANES), (2, K_ROWS_PLANES)):
        for op in OPS:
            assert cd.cudecompExtDescribePlanes3D(BASE, cd.FLOAT, op, keep, *box)["kind"] == fast
            assert cd.cudecompExtDescribePlanes3D(BASE + 2, cd.FLOAT, op, keep, *box)["kind"] == K_GENERIC_PLANES  # off the real's boundary
            # a complex field half an element off: the product pairs the two reals of an element inside one vector, the sum does not
            d = cd.cudecompExtDescribePlanes3D(BASE + 4, cd.FLOAT_COMPLEX, op, keep, *box)
            assert d["kind"] == (K_GENERIC_PLANES if op == cd.PLANES_MUL else fast), (keep, op, d)
    # rows that do not share their phase: the column form needs pitches of whole 16 bytes
    assert cd.cudecompExtDescribePlanes3D(BASE, cd.FLOAT, 0, 0, (33, 4, 2), (1, 41, 200), 64, 64)["kind"] == K_GENERIC_PLANES
    # no contiguous dim: element by element, whichever dim is kept
    for keep in range(3):
        d = cd.cudecompExtDescribePlanes3D(BASE, cd.DOUBLE, 0, keep, (5, 4, 3), (2, 12, 60))
        assert (d["kind"], d["vec"], d["write_lo"], d["write_hi"]) == (K_GENERIC_PLANES, 8, 0, span_of((5, 4, 3), (2, 12, 60), 8)), d


def test_large_boxes_take_the_fast_forms_and_fill_the_device():
    for extent, dtype in itertools.product(((512, 512, 512), (514, 3, 70000), (2, 100000, 300), (1 << 20, 4, 4), (3, 5, 1 << 22)),
                                           (cd.HALF, cd.DOUBLE_COMPLEX)):
        pitch = (extent[0] + 7) // 8 * 8
        strides = (1, pitch, pitch * extent[1])
        es = 2 if dtype == cd.HALF else 16
        for keep, op in itertools.product(range(3), OPS):
            d = cd.cudecompExtDescribePlanes3D(BASE, dtype, op, keep, extent, strides, 1 << 20, 1 << 20)
            assert d["kind"] == (K_COLUMNS_PLANES if keep == 0 else K_ROWS_PLANES), (extent, keep, d)
            assert 1 <= d["blocks"] < 1 << 31 and (d["write_lo"], d["write_hi"]) == (0, span_of(extent, strides, es)), (extent, keep, d)


def test_an_empty_box_makes_no_launch():
    for extent, keep, op in itertools.product(((0, 4, 4), (4, 0, 4), (4, 4, 0)), range(3), OPS):
        d = cd.cudecompExtDescribePlanes3D(BASE, cd.DOUBLE, op, keep, extent, (1, 8, 64))
        assert (d["blocks"], d["read_lo"], d["read_hi"], d["write_lo"], d["write_hi"]) == (0, 0, 0, 0, 0), d


def test_bad_arguments_of_the_describing_entry_are_refused():
    for args in ((BASE, 99, 0, 0, (4, 4, 4), (1, 4, 16)), (BASE, cd.DOUBLE, 2, 0, (4, 4, 4), (1, 4, 16)),
                 (BASE, cd.DOUBLE, -1, 0, (4, 4, 4), (1, 4, 16)), (BASE, cd.DOUBLE, 0, 3, (4, 4, 4), (1, 4, 16)),
                 (BASE, cd.DOUBLE, 0, -1, (4, 4, 4), (1, 4, 16)), (BASE, cd.DOUBLE, 0, 0, (4, -4, 4), (1, 4, 16)),
                 (BASE, cd.DOUBLE, 0, 0, (4, 4, 4), (1, -4, 16)), (BASE, cd.DOUBLE, 0, 0, (4, 4, 4), (1, 4, 16), -1, 0)):
        with pytest.raises(cd.CudecompError) as e:
            cd.cudecompExtDescribePlanes3D(*args)
        assert e.value.code == cd.RESULT_INVALID_USAGE
