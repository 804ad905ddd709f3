"""The arithmetic reference of the halo-accumulation tests (tests/accumulate_bodies.py typed_add) pinned without a GPU, three
ways: bf16 against torch.bfloat16 on the CPU; fp16 and fp32 against "the sum in float64, rounded once to the type"; hand-written
ties, overflows, subnormals and signed zeros of the 2-byte types with the expected bits as literals.  Everything is compared
bit for bit except NaN results, which are compared by class (the x86 default NaN has the sign bit set, the GPU's has not, and
the contract leaves it open).

Why the float64 route is a valid second statement: the sum of two p-bit numbers, rounded first to q >= 2p + 2 bits and then to
p bits, equals the sum rounded once (the double rounding is innocuous).  fp32: p = 24, float64 has 53 >= 50.  fp16: p = 11,
22 + 2 = 24 <= 53.  bf16 (p = 8) through fp32: 24 >= 18 -- which is why the contract's "RNE of the fp32 sum" is the correctly
rounded bf16 sum."""
import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB

N = 1 << 20


def _patterns(kind, seed):
    u, m, e = AB.FORMATS[kind]
    rng = np.random.default_rng(seed)
    draw = lambda: rng.integers(0, 1 << (1 + m + e), size=N, dtype=np.uint64).astype(u)  # noqa: E731
    ta, tb = AB.all_pairs(AB.edge_table(kind))
    return np.concatenate([draw(), ta]), np.concatenate([draw(), tb])


def _same(kind, got, want):
    """NaN class identical, every other result bit-identical"""
    got_nan, want_nan = AB.classes(kind, got)["nan"], AB.classes(kind, want)["nan"]
    assert np.array_equal(got_nan, want_nan)
    bad = np.nonzero(~want_nan & (got != want))[0]
    assert bad.size == 0, (kind, bad[:5], got[bad[:5]], want[bad[:5]])


def test_edge_table_holds_what_it_says():
    for kind, (u, m, e) in AB.FORMATS.items():
        t = AB.edge_table(kind)
        c = AB.classes(kind, t)
        assert (c["zero"].sum(), c["subnormal"].sum(), c["inf"].sum(), c["nan"].sum()) == (2, 4, 2, 2), kind
        assert t.dtype == u and len(t) == 24
    assert {0x7c01, 0x7e00, 0x7bff, 0xfbff, 0x3c00, 0x3c01, 0x1000, 0x0001, 0x03ff, 0x0400} <= set(AB.edge_table("fp16").tolist())
    assert {0x7f81, 0x7fc0, 0x7f7f, 0x3f80, 0x3f81, 0x3b80, 0x0001, 0x007f, 0x0080} <= set(AB.edge_table("bf16").tolist())
    assert {0x7f800001, 0x7fc00000, 0x7f7fffff, 0x3f800001, 0x33800000} <= set(AB.edge_table("fp32").tolist())
    assert {0x7ff0000000000001, 0x7ff8000000000000, 0x7fefffffffffffff, 0x3ff0000000000001} <= set(AB.edge_table("fp64").tolist())
    f16 = AB.edge_table("fp16").view(np.float16).astype(np.float64)
    assert {1.0, -1.0, 1.5, -2.75, 2.0 ** -11, 65504.0, 16.0, 2.0 ** -24, 2.0 ** -14} <= set(f16[np.isfinite(f16)].tolist())


def test_bf16_against_torch_bfloat16():
    import torch
    a, b = _patterns("bf16", 1)
    want = (torch.from_numpy(a.view(np.int16)).view(torch.bfloat16) + torch.from_numpy(b.view(np.int16)).view(torch.bfloat16))
    want = want.view(torch.int16).numpy().view(np.uint16)
    got = AB.typed_add(cd.BFLOAT16, a, b)
    assert got.dtype == np.uint16
    _same("bf16", got, want)
    c = AB.classes("bf16", got)  # the bulk draw reaches every class
    assert c["nan"].any() and c["inf"].any() and c["zero"].any() and c["subnormal"].any()


@pytest.mark.parametrize("dtype,kind", [(cd.HALF, "fp16"), (cd.FLOAT, "fp32"), (cd.BFLOAT16, "bf16")], ids=["fp16", "fp32", "bf16"])
def test_against_the_sum_in_float64_rounded_once(dtype, kind):
    a, b = _patterns(kind, 2)
    got = AB.typed_add(dtype, a, b)
    assert got.dtype == a.dtype
    with np.errstate(all="ignore"):
        if kind == "bf16":  # (beyond what the issue asks: the same statement for bf16, rounding float64 -> bf16 with integers)
            wide = (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64) + (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
            want = _round_float64_to_bf16(wide)
        else:
            f = {"fp16": np.float16, "fp32": np.float32}[kind]
            want = (a.view(f).astype(np.float64) + b.view(f).astype(np.float64)).astype(f).view(a.dtype)
    _same(kind, got, want)
    native = AB.typed_add(dtype, a.view(np.float16), b.view(np.float16)) if kind == "fp16" else None
    if native is not None:  # both forms of the operands give the same bits
        assert native.dtype == np.float16 and np.array_equal(native.view(np.uint16)[~AB.classes(kind, got)["nan"]], got[~AB.classes(kind, got)["nan"]])


def _round_float64_to_bf16(x):
    """float64 -> bf16 bit patterns, one rounding to nearest even, with integers (finite results that fit are all that differ
    from the fp32 route; overflow and NaN handled apart)"""
    u = np.ascontiguousarray(x).view(np.uint64)
    sign = ((u >> np.uint64(63)) << np.uint64(15)).astype(np.uint16)
    mag = np.abs(x)
    with np.errstate(all="ignore"):
        # scale so that one unit is the bf16 spacing at this magnitude: spacing = 2^(max(e, -126) - 7)
        e = np.floor(np.log2(np.where(mag > 0, mag, 1.0))).astype(np.int64)
        e = np.where(np.ldexp(1.0, e) > mag, e - 1, e)  # (log2 may round up at the top of a binade)
        e = np.maximum(e, -126)
        q = np.rint(np.ldexp(mag, 7 - e))               # exact scaling; rint rounds half to even
        val = np.ldexp(q, e - 7)                        # a bf16 number or 2^128
    f = val.astype(np.float32)                          # exact (or inf)
    out = (f.view(np.uint32) >> 16).astype(np.uint16)
    out = np.where(np.isnan(x), np.uint16(0x7fc0), out | sign)
    return out


H, B = cd.HALF, cd.BFLOAT16
HAND = [
    # fp16 (10 stored significand bits: ulp of 1 is 2^-10 = 0x1400, half of it 0x1000)
    (H, 0x3c00, 0x1000, 0x3c00, "1 + 2^-11 -> 1 (tie to even, down)"),
    (H, 0x3c01, 0x1000, 0x3c02, "(1 + 2^-10) + 2^-11 -> 1 + 2^-9 (tie to even, up)"),
    (H, 0x3c00, 0x1001, 0x3c01, "just above the tie -> up"),
    (H, 0x7bff, 0x4c00, 0x7c00, "65504 + 16 -> inf (tie at the top rounds to the even 2^16)"),
    (H, 0x7bff, 0x4bff, 0x7bff, "65504 + 15.99 (largest fp16 below 16) -> 65504"),
    (H, 0xfbff, 0xcc00, 0xfc00, "-65504 - 16 -> -inf"),
    (H, 0x0001, 0x0001, 0x0002, "min subnormal twice"),
    (H, 0x03ff, 0x0001, 0x0400, "largest subnormal + min subnormal -> smallest normal"),
    (H, 0x8000, 0x8000, 0x8000, "-0 + -0 -> -0"),
    (H, 0x8000, 0x0000, 0x0000, "-0 + +0 -> +0"),
    (H, 0x4248, 0xc248, 0x0000, "x + (-x) -> +0"),
    (H, 0x0400, 0x83ff, 0x0001, "smallest normal - largest subnormal -> min subnormal"),
    # bf16 (7 stored significand bits: ulp of 1 is 2^-7 = 0x3c00, half of it 0x3b80)
    (B, 0x3f80, 0x3b80, 0x3f80, "1 + 2^-8 -> 1 (tie to even, down)"),
    (B, 0x3f81, 0x3b80, 0x3f82, "(1 + 2^-7) + 2^-8 -> 1 + 2^-6 (tie to even, up)"),
    (B, 0x3f80, 0x3b81, 0x3f81, "just above the tie -> up"),
    (B, 0x7f7f, 0x7b00, 0x7f80, "max finite + half its ulp -> inf"),
    (B, 0x7f7f, 0x7aff, 0x7f7f, "max finite + just under half its ulp -> max finite"),
    (B, 0xff7f, 0xfb00, 0xff80, "-max finite - half its ulp -> -inf"),
    (B, 0x0001, 0x0001, 0x0002, "min subnormal twice"),
    (B, 0x007f, 0x0001, 0x0080, "largest subnormal + min subnormal -> smallest normal"),
    (B, 0x8000, 0x8000, 0x8000, "-0 + -0 -> -0"),
    (B, 0x8000, 0x0000, 0x0000, "-0 + +0 -> +0"),
    (B, 0x4049, 0xc049, 0x0000, "x + (-x) -> +0"),
    (B, 0x0080, 0x807f, 0x0001, "smallest normal - largest subnormal -> min subnormal"),
]


@pytest.mark.parametrize("dtype,a,b,want,what", HAND, ids=["%s-%d" % (AB.NAMES[c[0]], i % 12) for i, c in enumerate(HAND)])
def test_hand_written_ties_and_overflows(dtype, a, b, want, what):
    for x, y in ((a, b), (b, a)):  # addition commutes, bit for bit
        got = AB.typed_add(dtype, np.array([x], dtype=np.uint16), np.array([y], dtype=np.uint16))
        assert int(got[0]) == want, "%s: %#06x + %#06x gave %#06x, not %#06x" % (what, x, y, int(got[0]), want)


def test_nan_operands_give_nan_and_inf_minus_inf_too():
    for dtype in AB.ALL_TYPES:
        kind = AB.kind_of(dtype)
        ta, tb = AB.all_pairs(AB.edge_table(kind))
        got = AB.typed_add(dtype, ta, tb)
        ca, cb, cg = AB.classes(kind, ta), AB.classes(kind, tb), AB.classes(kind, got)
        sign = ta.dtype.type(1 << (1 + AB.FORMATS[kind][1] + AB.FORMATS[kind][2] - 1))
        opposite_inf = ca["inf"] & cb["inf"] & (((ta ^ tb) & sign) != 0)
        assert np.array_equal(cg["nan"], ca["nan"] | cb["nan"] | opposite_inf), kind


def test_dense_draws_reach_what_they_are_for():
    for dtype in (cd.HALF, cd.BFLOAT16, cd.FLOAT, cd.DOUBLE):
        kind = AB.kind_of(dtype)
        for name, (a, b) in AB.dense_draws(kind, 1 << 18, 7).items():
            c = AB.classes(kind, AB.typed_add(dtype, a, b))
            assert c["subnormal"].any() and c["zero"].any(), (kind, name)
            if name == "uniform":
                assert c["inf"].any() and c["nan"].any(), kind
            if name == "subnormal":
                assert (AB.classes(kind, a)["subnormal"] | AB.classes(kind, a)["zero"]).all()
                assert (AB.classes(kind, b)["subnormal"] | AB.classes(kind, b)["zero"]).all()


def test_swapping_the_two_additions_shows_in_the_typed_restatement():
    """the typed payload of accumulate_sweep on overlapping faces: the restatement in the other order differs in some cell, in
    every type -- and not at all where the faces do not overlap"""
    from oracle import oracle as orc
    for gdims, halo, overlap in (((3, 5, 4), (2, 2, 2), True), ((5, 3, 3), (3, 2, 3), True), ((33, 20, 27), (2, 3, 1), False)):
        g = orc.Grid(gdims, (1, 1))
        for dtype in AB.ALL_TYPES:
            nc = AB.TYPES[dtype][1]
            want = AB.expected_after(g, 0, halo, (1, 1, 1), (1, 0, 1), 5, nc, typed=dtype)[2][0]
            other = AB.expected_after(g, 0, halo, (1, 1, 1), (1, 0, 1), 5, nc, typed=dtype, swapped=True)[2][0]
            differs = not np.array_equal(AB.bits_of(dtype, want), AB.bits_of(dtype, other))
            assert differs == overlap, (gdims, AB.NAMES[dtype])
