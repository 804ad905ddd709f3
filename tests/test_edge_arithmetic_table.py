"""tests/edge_arithmetic.py on the CPU: the conditions the GPU tests of the adding kernels rely on, asserted so that they cannot
drift.  (1) The expected results of the 576 pairs and of every dense draw contain every class of result they are there for.  (2)
The one lenient rule of the comparison -- an expected NaN is matched by any NaN -- covers few cells.  (3) The comparison can fail:
references that are wrong in the ways a kernel could be wrong differ from the expected sums in reals that are not NaN."""
import numpy as np
import pytest

from tests import accumulate_bodies as AB
from tests import edge_arithmetic as EA
from tests import edge_arithmetic_bodies as EB

import cudecomp_amd as cd

TYPES = pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
DENSE = 1 << 16  # reals per dense draw in tests/test_gpu_halo_edge_arithmetic.py


def _count(dtype, bits):
    return {k: int(v.sum()) for k, v in AB.classes(AB.kind_of(dtype), bits).items()}


def test_shapes_and_kernel_table():
    assert all(w * h * d == 576 for w, h, d in EA.SHAPES)
    assert set(EA.KERNELS) == set(AB.ALL_TYPES)
    for dtype, (real, nc, widths) in EA.KERNELS.items():
        es = AB.element_bytes(dtype)
        assert nc == AB.TYPES[dtype][1] and real == {"fp16": "_Float16", "bf16": "__bf16", "fp32": "float", "fp64": "double"}[AB.kind_of(dtype)]
        reached = set()
        for w, _, _ in EA.SHAPES:  # the lane-width rule of the row kernels on these row lengths
            vb = 16
            while vb > es and (w * es) % vb:
                vb //= 2
            reached.add(vb)
        assert reached == set(widths) == {v for v in (16, 8, 4, 2) if v >= es}, (dtype, reached)


def test_name_sets_of_the_wall_plane_and_field_wall_kernels():
    """every lane width of the type x both accesses (x both signs: the wall plane's is a template argument) and the element-wise
    kernels, which carry the element size in bytes: 90 and 45 names over the seven data types"""
    planes = [EA.wall_plane_names(d) for d in AB.ALL_TYPES]
    fields = [EA.field_wall_names(d) for d in AB.ALL_TYPES]
    assert sum(len(s) for s in planes) == 90 and sum(len(s) for s in fields) == 45
    assert "rows_wall_plane_kernel<__bf16,8,1,true>" in EA.wall_plane_names(cd.BFLOAT16)
    assert "generic_wall_plane_kernel<float,8,false>" in EA.wall_plane_names(cd.FLOAT_COMPLEX)
    assert "rows_fields_wall_kernel<_Float16,4,0>" in EA.field_wall_names(cd.HALF_COMPLEX)
    assert "generic_fields_wall_kernel<double,16>" in EA.field_wall_names(cd.DOUBLE_COMPLEX)
    for dtype, p, f in zip(AB.ALL_TYPES, planes, fields):
        n = len(EA.KERNELS[dtype][2])
        assert len(p) == 4 * n + 2 and len(f) == 2 * n + 1
        # (a real and a complex type of one real format share their row kernels, never their element-wise ones)
        assert all("<%s," % EA.KERNELS[dtype][0] in name for name in p | f)


@pytest.mark.parametrize("negate", [False, True], ids=["plain", "flipped"])
@TYPES
def test_every_class_of_result_occurs_among_the_wall_pairs(dtype, negate):
    """EA.expected_wall over the pairs, the first of a pair as the mirror: every class, NaNs in under a quarter, and both wrong wall
    references differ from it in reals that are not NaN"""
    a, b = EA.pairs(dtype)
    want = EA.expected_wall(dtype, a, b, negate)
    c = _count(dtype, want)
    print(AB.NAMES[dtype], "negate", negate, c, "of", want.size)
    assert c["nan"] and c["inf"] and c["zero"] and c["subnormal"], c
    assert 4 * c["nan"] < want.size, c
    for wrong in (EA.flip_the_addend, EA.flip_after_the_addition):  # (wrong for either parity: neither flips the mirror alone)
        n = int(EA.wrong_outside_nan(dtype, wrong(dtype, a, b), want).sum())
        print(AB.NAMES[dtype], wrong.__name__, n)
        assert n >= 1, wrong.__name__
    # (the sums of the other parity are not these either: a kernel that forgot the flip, or flipped unasked, is told apart)
    assert EA.wrong_outside_nan(dtype, EA.expected_wall(dtype, a, b, not negate), want).any()


@TYPES
def test_the_edge_entries_as_doubles_give_their_patterns_back(dtype):
    kind = AB.kind_of(dtype)
    table = AB.edge_table(kind)
    wide, nan = EA.edge_doubles(dtype)
    assert wide.dtype == np.float64 and wide.shape == nan.shape == (24,) and int(nan.sum()) == 2
    assert np.array_equal(np.isnan(wide), nan)
    real = dtype if AB.TYPES[dtype][1] == 1 else {cd.HALF_COMPLEX: cd.HALF, cd.FLOAT_COMPLEX: cd.FLOAT, cd.DOUBLE_COMPLEX: cd.DOUBLE}[dtype]
    back = AB.to_bytes(wide[~nan], real).view(table.dtype)  # (to_bytes itself asserts that nothing was rounded)
    assert np.array_equal(back, table[~nan])
    if kind != "fp64":  # 16- and 32-bit formats: the doubles are not the patterns, and the signed zeros and subnormals survive
        assert np.signbit(wide[1]) and wide[1] == 0 and wide[2] > 0 and wide[3] < 0

@TYPES
def test_pairs_layout(dtype):
    a, b = EA.pairs(dtype)
    nc = AB.TYPES[dtype][1]
    table = AB.edge_table(AB.kind_of(dtype))
    assert a.shape == b.shape == (576, nc) and a.dtype == b.dtype == table.dtype
    n = np.arange(576)
    assert np.array_equal(a[:, 0], table[n // 24]) and np.array_equal(b[:, 0], table[n % 24])
    if nc == 2:  # the imaginary part: pair (7 n + 5) mod 576, a bijection, so both parts see every pair
        other = (7 * n + 5) % 576
        assert np.unique(other).size == 576
        assert np.array_equal(a[:, 1], table[other // 24]) and np.array_equal(b[:, 1], table[other % 24])
        assert (a[:, 0] != a[:, 1]).any() and (b[:, 0] != b[:, 1]).all()


@pytest.mark.parametrize("negate", [False, True], ids=["plain", "flipped"])
@TYPES
def test_every_class_of_result_occurs_among_the_pairs(dtype, negate):
    a, b = EA.pairs(dtype)
    want = EA.expected(dtype, a, b, negate)
    c = _count(dtype, want)
    print(AB.NAMES[dtype], "negate", negate, c, "of", want.size)
    assert c["nan"] and c["inf"] and c["zero"] and c["subnormal"], c
    assert 4 * c["nan"] < want.size, c  # (94 of 576 per real)
    # the wall kernels' order of operands gives the same classes: IEEE addition commutes, and a NaN is a NaN in either order
    wall = EA.expected_wall(dtype, b, a, negate)
    assert not AB.mismatches(AB.kind_of(dtype), wall, want).any()


@pytest.mark.parametrize("negate", [False, True], ids=["plain", "flipped"])
@TYPES
def test_every_class_of_result_occurs_in_the_dense_draws(dtype, negate):
    for name, (a, b) in EA.draws(dtype, DENSE, negate).items():
        assert a.size == b.size == DENSE and a.shape[1] == AB.TYPES[dtype][1]
        want = EA.expected(dtype, a, b, negate)
        c = _count(dtype, want)
        print(AB.NAMES[dtype], "negate", negate, name, c)
        assert c["zero"] and c["subnormal"], (name, c)
        if name == "uniform":
            assert c["inf"] and c["nan"], c
        assert 10 * c["nan"] < want.size, (name, c)  # (at most 5.9 %: the fp16 uniform draw)


@TYPES
def test_the_flip_of_the_draws_restores_the_pair(dtype):
    """b is handed over flipped for the flipping modes: the kernel's flip gives the sums of the plain draw"""
    for (name, (a, b)), (_, (a1, b1)) in zip(EA.draws(dtype, 4096, False).items(), EA.draws(dtype, 4096, True).items()):
        assert np.array_equal(a, a1) and np.array_equal(EA.flip(dtype, b1), b)
        assert np.array_equal(EA.expected(dtype, a, b, False), EA.expected(dtype, a1, b1, True)), name


@TYPES
def test_the_table_tells_a_wrong_reference_apart(dtype):
    a, b = EA.pairs(dtype)
    flipped, plain = EA.expected(dtype, a, b, True), EA.expected(dtype, a, b, False)
    n = int(EA.wrong_outside_nan(dtype, EA.flip_after_the_addition(dtype, a, b), flipped).sum())
    print(AB.NAMES[dtype], "flip after the addition:", n)
    assert n >= 1
    n = int(EA.wrong_outside_nan(dtype, EA.flip_the_destination(dtype, a, b), flipped).sum())
    print(AB.NAMES[dtype], "flip of the destination:", n)
    assert n >= 1
    for want in (plain, flipped):
        n = int(EA.wrong_outside_nan(dtype, EA.flush_subnormal_results(dtype, want), want).sum())
        print(AB.NAMES[dtype], "subnormal results flushed:", n)
        assert n >= 1
    # ... and a right one is not: the expected sums against themselves, and against a copy with other NaNs in the NaN cells
    assert not AB.mismatches(AB.kind_of(dtype), plain, plain).any()
    other_nan = np.where(AB.classes(AB.kind_of(dtype), plain)["nan"], ~np.zeros_like(plain), plain)
    assert not AB.mismatches(AB.kind_of(dtype), other_nan, plain).any() and not np.array_equal(other_nan, plain)


@pytest.mark.parametrize("layout", list(EB.ORDERS))
@pytest.mark.parametrize("call", ["fold", "fold_fields", "accumulate_fields", "wall_values", "wall_fields", "wall_planes"])
def test_the_expected_pencils_of_the_public_calls_hold_every_class(call, layout):
    """tests/edge_arithmetic_bodies.py: among the cells the calls add into (the wall calls: write), per family and data type, there
    are NaN, infinite, zero and subnormal results, and NaNs in under a quarter of them (a fill stride that breaks this is the thing to
    change).  The wall-value calls add every entry of the edge table somewhere; on the periodic dim no wall call writes a cell."""
    import math
    assert math.gcd(EB.STRIDE, 576) == 1 and math.gcd(EB.STRIDE, 1152) == 1
    assert math.gcd(EB.PLANE_STRIDE, 1152) == 1 and EB.PLANE_STRIDE != EB.STRIDE
    args = dict(EB.PENCILS, mem_order=EB.ORDERS[layout])
    tallies = EB.result_classes(call, args)
    print(call, layout, {AB.NAMES[d]: t for d, t in tallies.items()})
    assert set(tallies) == set(EB.PENCILS["dtypes"]) and all(t["reals"] > 0 for t in tallies.values())
    assert EB.class_failures(call, args) == []
    if call in EB.WALL_CALLS:
        n = {"wall_values": 12, "wall_fields": 6, "wall_planes": 12}[call]
        every = list(EB.cases(call, args))
        assert len(every) == 3 * 4 * 3 * n
        for label, _, _, dim, _, start, want, masks in every:
            assert bool(masks[0].any()) == (not EB.PENCILS["periods"][dim]), label
            for s, w, m in zip(start, want, masks):
                assert np.array_equal(s[~m], w[~m]), label  # (the definition changes the ghost cells it names and nothing else)
    if call in ("wall_values", "wall_fields"):
        entries = EB.addend_entries(call, args)
        assert all(entries[d] == set(range(24)) for d in EB.PENCILS["dtypes"]), entries


@pytest.mark.parametrize("negate", [False, True], ids=["plain", "flipped"])
def test_the_table_tells_a_truncating_bf16_apart(negate):
    a, b = EA.pairs(cd.BFLOAT16)
    want = EA.expected(cd.BFLOAT16, a, b, negate)
    n = int(EA.wrong_outside_nan(cd.BFLOAT16, EA.bf16_truncated(a, b, negate), want).sum())
    print("bf16 truncated, negate", negate, ":", n)
    assert n >= 1
    # (of the dense draws only the uniform one rounds: differences of neighbours and sums of subnormals are exact)
    a, b = EA.draws(cd.BFLOAT16, DENSE, negate)["uniform"]
    assert EA.wrong_outside_nan(cd.BFLOAT16, EA.bf16_truncated(a, b, negate), EA.expected(cd.BFLOAT16, a, b, negate)).any()
