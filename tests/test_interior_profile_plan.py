"""How the interior profiles (cudecomp_interior_profile.h) would run, without a GPU: cudecompExtDescribeProfile3D over the sweep the
GPU tests run on the device -- row lengths, three pitches, every phase of the 16-byte grid, the kept dim at each memory position, the
seven data types, a readable range of 0 or 16 bytes around the box.  What no GPU test can check without faulting is checked here:
the lowest and the highest byte a launch reads lie inside the readable range.  Also: the form is chosen by the stated rules, parts x
entries never exceed what the workspace holds, an empty box makes no launch, and the workspace function is the header's formula."""
import itertools
import re

import pytest

import cudecomp_amd as cd
from tests.test_interior_reduce_plan import BASE, LENGTHS, TYPES, bytes_read_row_by_row, span_of

K_ROWS_PROFILE, K_COLUMNS_PROFILE, K_GENERIC_PROFILE = 45, 46, 47
IDS = ["fp16", "bf16", "complex_fp16", "fp32", "complex64", "fp64", "complex128"]


def pitches(length, es):
    """the row itself, + 3 elements, and the next multiple of 16 bytes beyond the row (tests/interior_profile_bodies.py)"""
    per = 16 // es  # elements per 16 bytes (element sizes 2, 4, 8, 16)
    return (length, length + 3, (length // per + 1) * per)


def sweep(dtype):
    rs, nc = TYPES[dtype]
    es = rs * nc
    for length, (rows, planes) in itertools.product(LENGTHS, ((1, 1), (3, 2), (5, 1))):
        for which, pitch in enumerate(pitches(length, es)):
            for phase in range(0, 16, rs):
                yield (length, rows, planes), (1, pitch, pitch * (rows + 1) if which == 2 else pitch * rows + 5), BASE + phase


def expected_kind(dtype, op, keep, extent, strides, address, force):
    """the rules of csrc/kernels.h planProfile"""
    rs, nc = TYPES[dtype]
    es = rs * nc
    if force & 1 or (op == cd.REDUCE_DOT and nc == 2 and address % es):
        return K_GENERIC_PROFILE
    c = None  # the contiguous dim: of stride 1, and of several such the one longer than a cell
    for d in range(3):
        if strides[d] == 1 and (c is None or (extent[c] == 1 and extent[d] > 1)):
            c = d
    if c is None:
        return K_GENERIC_PROFILE
    if keep != c:
        return K_ROWS_PROFILE
    others = [d for d in range(3) if d != keep and extent[d] > 1]
    return K_COLUMNS_PROFILE if all((strides[d] * es) % 16 == 0 for d in others) else K_GENERIC_PROFILE


def capacity(n_fields, length):
    """the header's formula, in pairs of doubles per field"""
    return max(length, cd.PROFILE_PAIRS_PER_FIELD)


@pytest.mark.parametrize("dtype", list(TYPES), ids=IDS)
def test_no_launch_reads_outside_the_readable_range_and_the_form_follows_the_rules(dtype):
    """the fast forms test every vector (`slot_off >= rd_lo && slot_off + 16 <= rd_hi`, else the reals inside the row only), the row
    kernel through the tile walk it shares with the scalar reduction, the column kernel with one phase for all rows; planProfile's
    read_lo / read_hi are a closed form of the outcome.  Held here: the closed form lies in the range and equals the slot decode
    mirrored on the host over EVERY row of the box (rows along the contiguous dim: the same bytes whichever dim is kept)."""
    rs, nc = TYPES[dtype]
    es, n, kinds = rs * nc, 0, set()
    for (extent, strides, address), keep, op, around, force in itertools.product(sweep(dtype), range(3), (0, 1, 2), (0, 16), (0, 1)):
        d = cd.cudecompExtDescribeProfile3D(address, address + (1 << 20), dtype, op, keep, extent, strides, around, around, force)
        what = (dtype, extent, strides, address - BASE, keep, op, around, force, d)
        span = span_of(extent, strides, es)
        assert -around <= d["read_lo"] <= 0 and span <= d["read_hi"] <= span + around, what
        assert d["entries"] == extent[keep] and 1 <= d["parts"] <= cd.PROFILE_MAX_PARTS, what
        assert d["parts"] * d["entries"] * 16 <= cd.cudecompAmdProfileInteriorWorkspaceBytes(1, extent[keep]), what
        kind = expected_kind(dtype, op, keep, extent, strides, address, force)
        kinds.add(kind)
        assert d["kind"] == kind and d["vec"] == (es if kind == K_GENERIC_PROFILE else 16), what
        if kind == K_GENERIC_PROFILE:
            assert (d["read_lo"], d["read_hi"]) == (0, span), what
        elif strides[1] != 1:  # (rows of one cell at pitch 1 lie along dim 1: the mirror below takes dim 0 for the rows)
            assert (d["read_lo"], d["read_hi"]) == bytes_read_row_by_row(address, extent, strides, es, around, around), what
        n += 1
    assert n == 9 * 3 * 3 * (16 // rs) * 3 * 3 * 2 * 2
    assert kinds == {K_ROWS_PROFILE, K_COLUMNS_PROFILE, K_GENERIC_PROFILE}


def test_boxes_off_the_grid_go_element_by_element():
    for shift, kind in ((0, K_COLUMNS_PROFILE), (16, K_COLUMNS_PROFILE), (8, K_GENERIC_PROFILE), (4, K_GENERIC_PROFILE)):
        for keep, fast in ((0, K_COLUMNS_PROFILE), (1, K_ROWS_PROFILE), (2, K_ROWS_PROFILE)):
            d = cd.cudecompExtDescribeProfile3D(BASE, BASE + 4096 + shift, cd.FLOAT, cd.REDUCE_DOT, keep, (33, 4, 2), (1, 40, 200), 64, 64)
            assert d["kind"] == (fast if kind == K_COLUMNS_PROFILE else kind), (shift, keep, d)
            d = cd.cudecompExtDescribeProfile3D(BASE, BASE + 4096 + shift, cd.FLOAT, cd.REDUCE_SUM, keep, (33, 4, 2), (1, 40, 200), 64, 64)
            assert d["kind"] == fast, (shift, keep, d)  # (b is not looked at)
    # rows that do not share their phase: the column form needs pitches of whole 16 bytes
    d = cd.cudecompExtDescribeProfile3D(BASE, 0, cd.FLOAT, cd.REDUCE_SUM, 0, (33, 4, 2), (1, 41, 200), 64, 64)
    assert d["kind"] == K_GENERIC_PROFILE, d
    # no contiguous dim: element by element, whichever dim is kept
    for keep in range(3):
        d = cd.cudecompExtDescribeProfile3D(BASE, 0, cd.DOUBLE, cd.REDUCE_SUM, keep, (5, 4, 3), (2, 12, 60))
        assert (d["kind"], d["vec"]) == (K_GENERIC_PROFILE, 8), d
    # a field off the boundary of its real type
    d = cd.cudecompExtDescribeProfile3D(BASE + 2, 0, cd.FLOAT, cd.REDUCE_SUM, 1, (33, 4, 2), (1, 40, 200), 64, 64)
    assert d["kind"] == K_GENERIC_PROFILE, d


def test_parts_times_entries_fit_the_workspace_for_boxes_of_any_size():
    """the cap on the parts per entry is what lets the workspace depend on the number of fields and on L alone"""
    n = 0
    for extent, dtype, force in itertools.product(((512, 512, 512), (514, 3, 70000), (2, 100000, 300), (1 << 20, 4, 4), (7, 1, 1),
                                                   (1, 1, 1), (70000, 70000, 2), (3, 5, 1 << 22)), (cd.HALF, cd.DOUBLE_COMPLEX), (0, 1)):
        pitch = (extent[0] + 7) // 8 * 8
        strides = (1, pitch, pitch * extent[1])
        for keep in range(3):
            d = cd.cudecompExtDescribeProfile3D(BASE, BASE + (1 << 50), dtype, cd.REDUCE_DOT, keep, extent, strides, 1 << 20, 1 << 20, force)
            L = extent[keep]
            assert d["entries"] == L and 1 <= d["parts"] <= min(cd.PROFILE_MAX_PARTS, max(1, cd.PROFILE_PAIRS_PER_FIELD // L)), (extent, keep, d)
            assert d["parts"] * L <= capacity(1, L), (extent, keep, d)
            assert d["final_lanes"] in (1, 64) and d["blocks"] >= 1, d
            if force == 0:
                assert d["kind"] == (K_COLUMNS_PROFILE if keep == 0 else K_ROWS_PROFILE), (extent, keep, d)
            n += 1
    assert n == 8 * 2 * 2 * 3


def test_an_empty_box_makes_no_launch():
    for extent, keep in itertools.product(((0, 4, 4), (4, 0, 4), (4, 4, 0)), range(3)):
        d = cd.cudecompExtDescribeProfile3D(BASE, 0, cd.DOUBLE, cd.REDUCE_SUM, keep, extent, (1, 8, 64))
        assert (d["blocks"], d["parts"], d["read_lo"], d["read_hi"], d["final_lanes"]) == (0, 0, 0, 0, 0), d
        assert d["entries"] == extent[keep]  # 0: nothing is written; else zeros are, by the final stage alone


def test_the_workspace_function_is_the_headers_formula_and_monotone():
    text = " ".join(open(cd.__file__.replace("cudecomp_amd/__init__.py", "include/cudecomp_interior_profile.h")).read().split())
    assert re.search(r"bytes\(n_fields, length\) = n_fields \* max\(length, 65536\) \* 16", text)
    assert "min(1024, max(1, 65536 / L))" in text
    assert (cd.PROFILE_PAIRS_PER_FIELD, cd.PROFILE_MAX_PARTS) == (65536, 1024)
    lengths = (0, 1, 2, 511, 512, 65535, 65536, 65537, 1 << 20, 1 << 31)
    for n in range(1, 33):
        sizes = [cd.cudecompAmdProfileInteriorWorkspaceBytes(n, length) for length in lengths]
        assert sizes == [n * max(length, 65536) * 16 for length in lengths]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        if n > 1:
            assert all(cd.cudecompAmdProfileInteriorWorkspaceBytes(n - 1, length) <= s for length, s in zip(lengths, sizes))


def test_bad_arguments_of_the_describing_entry_are_refused():
    for args in ((BASE, 0, 99, 0, 0, (4, 4, 4), (1, 4, 16)), (BASE, 0, cd.DOUBLE, 3, 0, (4, 4, 4), (1, 4, 16)),
                 (BASE, 0, cd.DOUBLE, 0, 3, (4, 4, 4), (1, 4, 16)), (BASE, 0, cd.DOUBLE, 0, -1, (4, 4, 4), (1, 4, 16)),
                 (BASE, 0, cd.DOUBLE, 0, 0, (4, -4, 4), (1, 4, 16)), (BASE, 0, cd.DOUBLE, 0, 0, (4, 4, 4), (1, -4, 16)),
                 (BASE, 0, cd.DOUBLE, 0, 0, (4, 4, 4), (1, 4, 16), -1, 0)):
        with pytest.raises(cd.CudecompError) as e:
            cd.cudecompExtDescribeProfile3D(*args)
        assert e.value.code == cd.RESULT_INVALID_USAGE
