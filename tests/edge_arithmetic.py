"""IEEE edge values for every kernel that adds: the operand tables, the expected sums and the launch shapes shared by
tests/test_gpu_halo_accumulate.py (kernels_accumulate.hip) and tests/test_gpu_halo_edge_arithmetic.py (kernels_fold.hip,
kernels_field_mirror.hip, kernels_field_accumulate.hip, kernels_wall.hip, kernels_field_wall.hip, kernels_wall_plane.hip).  numpy
only: nothing here touches the GPU.
tests/test_edge_arithmetic_table.py holds the tables to the conditions the GPU tests rely on (every class of result occurs, the
NaN cells -- the only ones compared by class -- stay few, a wrong reference is told apart).

Operands are BIT PATTERNS of shape (elements, reals per element), of the unsigned type as wide as one real.  `a` is what the
destination cell holds, `b` what the source cell holds; the kernels that mirror flip the sign bits of the SOURCE first (parity -1)
and then add in the element type's arithmetic with the destination as the first operand: FB.fold_add.  The wall kernels have no
destination operand: they add the addend of the layer to the (flipped) mirror value, expected_wall below."""
import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fold_bodies as FB

# (w, h, d) with w * h * d = 576 and the lane width each row length gives an element of 2 / 4 / 8 / 16 bytes:
#   96 -> 16 16 16 16   36 -> 8 16 16 16   18 -> 4 8 16 16   9 -> 2 4 8 16
SHAPES = [(96, 3, 2), (36, 4, 4), (18, 8, 4), (9, 16, 4)]
T16, TBF, T32, T64 = "_Float16", "__bf16", "float", "double"
# data type -> (real type as the kernel templates spell it, reals per element, lane widths in bytes the type reaches)
KERNELS = {cd.HALF: (T16, 1, (16, 8, 4, 2)), cd.BFLOAT16: (TBF, 1, (16, 8, 4, 2)), cd.HALF_COMPLEX: (T16, 2, (16, 8, 4)),
           cd.FLOAT: (T32, 1, (16, 8, 4)), cd.FLOAT_COMPLEX: (T32, 2, (16, 8)), cd.DOUBLE: (T64, 1, (16, 8)),
           cd.DOUBLE_COMPLEX: (T64, 2, (16,))}
DRAW_SEED = 7
TF = {False: "false", True: "true"}


def wall_plane_names(dtype):
    """every instantiation of kernels_wall_plane.hip for the type, as cudecompExtLastKernelName spells them (the element-wise
    kernel carries the element size in bytes)"""
    t, _, widths = KERNELS[dtype]
    es = AB.element_bytes(dtype)
    return {"rows_wall_plane_kernel<%s,%d,%d,%s>" % (t, vb, s, TF[neg]) for vb in widths for s in (0, 1) for neg in (False, True)} | \
           {"generic_wall_plane_kernel<%s,%d,%s>" % (t, es, TF[neg]) for neg in (False, True)}


def field_wall_names(dtype):
    """every instantiation of kernels_field_wall.hip for the type (the sign is an argument of these kernels, not a template's)"""
    t, _, widths = KERNELS[dtype]
    return {"rows_fields_wall_kernel<%s,%d,%d>" % (t, vb, s) for vb in widths for s in (0, 1)} | \
           {"generic_fields_wall_kernel<%s,%d>" % (t, AB.element_bytes(dtype))}


def pair_elements(dtype, a, b):
    """reals -> elements: complex types take the real part from pair n and the imaginary part from pair 7 n + 5 (a bijection of
    the 576 pairs: the two parts of an element come from different rows of the table, and both see every pair)"""
    if AB.TYPES[dtype][1] == 1:
        return a.reshape(-1, 1), b.reshape(-1, 1)
    other = (np.arange(a.size) * 7 + 5) % a.size
    return np.stack([a, a[other]], axis=1), np.stack([b, b[other]], axis=1)


def pairs(dtype):
    """(a, b), each (576, reals per element): all 24 x 24 pairs of AB.edge_table of the type's real format"""
    return pair_elements(dtype, *AB.all_pairs(AB.edge_table(AB.kind_of(dtype))))


def flip(dtype, bits):
    """every sign bit flipped -- of zeros, infinities and NaNs too"""
    return np.ascontiguousarray(bits) ^ FB.sign_bit(dtype)


def expected(dtype, a, b, negate):
    """a + b, or a + (b with every sign bit flipped): the flip first, then the addition of the type, destination first"""
    return FB.fold_add(dtype, a, b, negate)


def expected_wall(dtype, src, addend, negate):
    """(src, flipped with `negate`) + addend: the wall kernels' order of operands"""
    return AB.typed_add(dtype, flip(dtype, src) if negate else np.ascontiguousarray(src), np.ascontiguousarray(addend))


def draws(dtype, n, negate):
    """{"uniform", "cancelling", "subnormal"}: (a, b) of AB.dense_draws with n REALS, laid into elements in order.  For the
    sign-flipping modes b is handed over with its sign bits already flipped, so that the kernel's own flip restores the pair the
    draw was made for (a "cancelling" pair whose b is flipped once more adds up to 2 a and never cancels)."""
    nc = AB.TYPES[dtype][1]
    out = {}
    for name, (a, b) in AB.dense_draws(AB.kind_of(dtype), n, DRAW_SEED).items():
        out[name] = (a.reshape(-1, nc), (flip(dtype, b) if negate else b).reshape(-1, nc))
    return out


# ---- references that are WRONG on purpose: what the comparison must be able to tell from `expected` -------------------------------
def flip_after_the_addition(dtype, a, b):
    """-(a + b) where a + -b is meant"""
    return flip(dtype, AB.typed_add(dtype, np.ascontiguousarray(a), np.ascontiguousarray(b)))


def flip_the_destination(dtype, a, b):
    """-a + b where a + -b is meant"""
    return AB.typed_add(dtype, flip(dtype, a), np.ascontiguousarray(b))


def flip_the_addend(dtype, mirror, addend):
    """the wall order of operands: mirror + -addend where -mirror + addend is meant (flip_after_the_addition, applied to (mirror,
    addend), is the other wrong wall reference: -(mirror + addend))"""
    return AB.typed_add(dtype, np.ascontiguousarray(mirror), flip(dtype, addend))


def edge_doubles(dtype):
    """(doubles, is_nan): the 24 entries of AB.edge_table of the type's real format as float64 -- what cudecompAmdSetWallHalos*
    and cudecompAmdSetWallFieldHalos* take as addends.  Every fp16, bf16 and fp32 pattern that is not a NaN IS a double, and the
    library's narrowing of that double gives the pattern back (tests/test_edge_arithmetic_table.py holds the round trip through
    AB.to_bytes); the fp64 entries are themselves.  What becomes of a NaN's payload on the way is unspecified: NaN by class."""
    kind = AB.kind_of(dtype)
    table = AB.edge_table(kind)
    with np.errstate(invalid="ignore"):  # (the signalling NaN of the table)
        if kind == "bf16":
            wide = (table.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        else:
            wide = table.view(AB._FLOAT_OF_KIND[kind]).astype(np.float64)
    return wide, AB.classes(kind, table)["nan"]


def flush_subnormal_results(dtype, want):
    """`want` with every subnormal real replaced by the zero of its sign"""
    want = np.ascontiguousarray(want)
    return np.where(AB.classes(AB.kind_of(dtype), want)["subnormal"], want & FB.sign_bit(dtype), want)


def bf16_truncated(a, b, negate):
    """bf16 alone: the fp32 sum cut off after 16 bits instead of rounded to nearest even (NaN sums stay NaN)"""
    x = np.ascontiguousarray(b) ^ np.uint16(0x8000) if negate else np.ascontiguousarray(b)
    with np.errstate(all="ignore"):
        s = (np.ascontiguousarray(a).astype(np.uint32) << 16).view(np.float32) + (x.astype(np.uint32) << 16).view(np.float32)
    return np.where(np.isnan(s), np.uint16(0x7fc0), (np.ascontiguousarray(s).view(np.uint32) >> 16).astype(np.uint16))


def wrong_outside_nan(dtype, got, want):
    """the reals that break the comparison rule (AB.mismatches) and whose expected value is NOT a NaN"""
    kind = AB.kind_of(dtype)
    return AB.mismatches(kind, got, want) & ~AB.classes(kind, want)["nan"]
