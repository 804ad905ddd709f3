"""Bodies of tests/test_gpu_interior_planes.py: every function runs on a rank launched by tests/mp.py (the pytest process never opens
the GPU) and returns a list of failure strings, or a dict that holds one.

The reference is numpy in the arithmetic cudecomp_interior_planes.h states, on BIT PATTERNS (the only form numpy has for bf16): the
coefficient is the fp64 product scale * coef rounded once to the real type, directly from the double (`to_real_bits`: numpy's own
conversion for fp16 / fp32, exact integer rounding for bf16; `exact_bits` is the same rounding through fractions, for the test of the
conversion itself); the update is tests/accumulate_bodies.py's typed addition and the product beside it, every product and sum
rounded on its own.  All comparisons are bit for bit (an expected NaN: any NaN)."""
import itertools
from fractions import Fraction

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests.interior_profile_bodies import Results, _position, _workspace, pitches, profile_reference
from tests.interior_reduce_bodies import (ARITH, LENGTHS, POISON, SLACK, closed_form, integers, interior_index, interior_shape, rank_slab,
                                          same_bits)

FORMS = ("planes_rows_kernel", "planes_columns_kernel", "planes_elements_kernel")
OPS = (cd.PLANES_ADD, cd.PLANES_MUL)


# ---- the definition in numpy -----------------------------------------------------------------------------------------------------
def bits_from_exact(dtype, values):
    """bit patterns (unsigned, one per real) of values that are exact in the real type of `dtype`"""
    u = AB.FORMATS[AB.kind_of(dtype)][0]
    return AB.to_bytes(values, dtype).view(u).reshape(np.shape(values))


def to_real_bits(kind, d):
    """float64 array -> bit patterns of the real type, round to nearest even DIRECTLY from the double"""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == "fp64":
            return d.view(np.uint64).copy()
        if kind == "fp32":
            return d.astype(np.float32).view(np.uint32)
        if kind == "fp16":
            return d.astype(np.float16).view(np.uint16)
        # bf16 has fp32's exponent range: fp32 rounded TO ODD (truncate towards zero, sticky bit into the last place) keeps 16 bits
        # below bf16's last place, so rounding that to nearest even with integers is rounding the double itself
        f = d.astype(np.float32)
        back = f.astype(np.float64)
        bits = f.view(np.uint32).astype(np.int64)
        inexact = ~np.isnan(d) & (back != d)
        bits = np.where(inexact & (np.abs(back) > np.abs(d)), bits - 1, bits)
        bits = np.where(inexact, bits | 1, bits).astype(np.uint64)
        r = ((bits + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
        return np.where(np.isnan(d), np.uint16(0x7fc0), r)


def exact_bits(kind, x):
    """ONE python float -> the bit pattern of the real type, by exact rational arithmetic: the nearest representable number, ties to
    the even significand, overflow to infinity past the largest finite plus half an ulp.  Independent of numpy's conversions."""
    u, m, e = AB.FORMATS[kind]
    bias, top = (1 << (e - 1)) - 1, (1 << e) - 1
    if x != x:
        return (top << m) | (1 << (m - 1))
    sign = 1 if np.signbit(x) else 0
    if x in (float("inf"), float("-inf")):
        return (sign << (m + e)) | (top << m)
    q = abs(Fraction(x))
    if q == 0:
        return sign << (m + e)
    ex = max(q.numerator.bit_length() - q.denominator.bit_length(), 1 - bias - 1)
    while Fraction(2) ** ex > q and ex > 1 - bias:
        ex -= 1
    while Fraction(2) ** (ex + 1) <= q:
        ex += 1
    ex = max(ex, 1 - bias)                      # subnormals share the smallest normal's exponent
    ulp = Fraction(2) ** (ex - m)
    n = q / ulp                                 # the significand in units of the last place
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
        k += 1
    expo = ex + bias if k >= (1 << m) else 0    # (k < 2^m: a subnormal, or zero)
    if k >= (2 << m):                           # the rounding carried into the next binade
        k >>= 1
        expo += 1
    if expo >= top:
        return (sign << (m + e)) | (top << m)
    return (sign << (m + e)) | (expo << m) | (k & ((1 << m) - 1))


def typed_mul(dtype, a, b):
    """a * b on bit patterns, as AB.typed_add adds: IEEE for fp16 / fp32 / fp64 (numpy), bf16 the RNE of the fp32 product"""
    kind = AB.kind_of(dtype)
    with np.errstate(all="ignore"):
        if kind != "bf16":
            f = AB._FLOAT_OF_KIND[kind]
            return (a.view(f) * b.view(f)).view(a.dtype)
        s = (a.astype(np.uint32) << 16).view(np.float32) * (b.astype(np.uint32) << 16).view(np.float32)
        v = np.ascontiguousarray(s).view(np.uint32).astype(np.uint64)
        r = ((v + 0x7fff + ((v >> 16) & 1)) >> 16).astype(np.uint16)
        return np.where(np.isnan(s), np.uint16(0x7fc0), r)


def negated(dtype, a):
    u, m, e = AB.FORMATS[AB.kind_of(dtype)]
    return a ^ u(1 << (m + e))


def apply_reference(dtype, op, u, c):
    """u, c: bit patterns of shape (..., nc), broadcastable; the updated cells' bit patterns"""
    u, c = np.broadcast_arrays(np.ascontiguousarray(u), np.ascontiguousarray(c))
    u, c = np.ascontiguousarray(u), np.ascontiguousarray(c)
    if op == cd.PLANES_ADD:
        return AB.typed_add(dtype, u, c)
    if u.shape[-1] == 1:
        return typed_mul(dtype, u, c)
    ur, ui, cr, ci = (np.ascontiguousarray(x) for x in (u[..., 0], u[..., 1], c[..., 0], c[..., 1]))
    re = AB.typed_add(dtype, typed_mul(dtype, ur, cr), negated(dtype, typed_mul(dtype, ui, ci)))  # (a - b is a + (-b), exactly)
    im = AB.typed_add(dtype, typed_mul(dtype, ur, ci), typed_mul(dtype, ui, cr))
    return np.stack([re, im], axis=-1)


def coefficient_bits(dtype, coef_pairs, scale):
    """(L, 2) doubles -> (L, nc) bit patterns: the fp64 product, then one rounding; real types use the first double alone"""
    nc = AB.TYPES[dtype][1]
    with np.errstate(all="ignore"):
        prod = np.float64(scale) * np.asarray(coef_pairs, dtype=np.float64)[:, :nc]
    return to_real_bits(AB.kind_of(dtype), prod)


def along(cbits, npax):
    """(L, nc) coefficients shaped to broadcast against cells (e2, e1, e0, nc) along numpy axis `npax`"""
    shape = [1, 1, 1, cbits.shape[1]]
    shape[npax] = cbits.shape[0]
    return cbits.reshape(shape)


def coefficients(L, nc, seed):
    """(L, 2) doubles, exact in every real type after a scale of -2: integers and halves; real types get a NaN as second double"""
    k = np.arange(L) + seed
    out = np.empty((L, 2))
    out[:, 0] = (k * 5 + 3) % 7 - 3 + 0.5 * (k % 2)
    out[:, 1] = (k * 3 + 1) % 5 - 2 - 0.25 * (k % 3 == 0) if nc == 2 else np.nan
    return out


def name_of(dtype, op, form):
    if form == 2:
        return "%s<%s>" % (FORMS[2], ARITH[dtype])
    mode = 0 if op == cd.PLANES_ADD else (2 if AB.TYPES[dtype][1] == 2 else 1)
    return "%s<%s,%d>" % (FORMS[form], ARITH[dtype], mode)


def expected_form(dtype, op, keep, extent, strides, address, force):
    """planPlanes' rules: 0 rows, 1 columns, 2 element-wise"""
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    if force & 1 or (op == cd.PLANES_MUL and nc == 2 and address % es):
        return 2
    c = None
    for d in range(3):
        if strides[d] == 1 and (c is None or (extent[c] == 1 and extent[d] > 1)):
            c = d
    if keep != c:
        return 0
    others = [d for d in range(3) if d != keep and extent[d] > 1]
    return 1 if all((strides[d] * es) % 16 == 0 for d in others) else 2


def sentinel(nbytes, seed=0):
    """a byte that depends on its position (and never repeats with period 16)"""
    return ((np.arange(nbytes, dtype=np.int64) * 37 + 11 + seed) % 251).astype(np.uint8)


def _first_bad(got, want, es):
    bad = np.flatnonzero(got != want)
    return "byte %d (of %d differing): got %s want %s" % (bad[0], bad.size, got[bad[0] // es * es:bad[0] // es * es + es].tolist(),
                                                         want[bad[0] // es * es:bad[0] // es * es + es].tolist())


# ---- kernel parity through cudecompExtPlanes3D ---------------------------------------------------------------------------------
def kernel_parity(rank, nranks, args):
    """for one data type: every row length, three pitches, every phase of the 16-byte grid, the kept dim at each of the three
    positions, both operations, the fast form and the forced element form, nothing and 16 bytes readable around the box,
    non-temporal access on two lengths; the box inside a buffer of position-dependent bytes; every cell of the box equal to
    numpy's, every other byte unchanged, the kernel's name and class"""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    dtype = args["dtype"]
    rs, es, nc = AB.real_bytes(dtype), AB.element_bytes(dtype), AB.TYPES[dtype][1]
    stream = torch.cuda.current_stream().cuda_stream
    scale = -2.0
    failures, n, seen = [], 0, set()
    for length, (rows, planes) in itertools.product(LENGTHS, ((1, 1), (3, 2), (5, 1))):
        for which, pitch in enumerate(pitches(length, es)):
            extent, strides = (length, rows, planes), (1, pitch, pitch * (rows + 1) if which == 2 else pitch * rows + 5)
            cells = np.array([i * strides[0] + j * strides[1] + k * strides[2]
                              for k in range(planes) for j in range(rows) for i in range(length)], dtype=np.int64)
            span = (int(cells.max()) + 1) * es
            vals = integers(cells.size, nc, n)
            u = bits_from_exact(dtype, vals).reshape(planes, rows, length, nc)
            coef = coefficients(max(extent), nc, n)
            dcoef = torch.from_numpy(coef.reshape(-1).copy()).cuda()
            forces = (0, 1, 2, 3) if length in (7, 130) else (0, 1)
            variants = list(itertools.product(range(3), OPS, forces, (0, 16)))
            wants = {(keep, op): apply_reference(dtype, op, u, along(coefficient_bits(dtype, coef[:extent[keep]], scale), 2 - keep))
                     for keep in range(3) for op in OPS}
            for phase in range(0, 16, rs):
                n += 1
                nbytes = 2 * SLACK + phase + span
                region = (nbytes + 15) // 16 * 16  # every variant's copy starts on the 16-byte grid: one phase for all
                img = sentinel(region, n)
                body = img[SLACK + phase:SLACK + phase + span].reshape(-1, es)
                body[cells] = np.ascontiguousarray(u).view(np.uint8).reshape(-1, es)
                dev = torch.from_numpy(np.tile(img, len(variants))).cuda()
                if dev.data_ptr() % 16:
                    return ["device buffers are not 16-byte aligned"]
                notes = []
                for v, (keep, op, force, readable) in enumerate(variants):
                    pa = dev.data_ptr() + v * region + SLACK + phase
                    cls = cd.cudecompExtPlanes3D(pa, dtype, op, keep, extent, strides, readable, readable, dcoef.data_ptr(), scale, force,
                                                 stream)
                    name = cd.cudecompExtLastKernelName()
                    form = expected_form(dtype, op, keep, extent, strides, pa, force)
                    seen.add(form)
                    what = "%s op %d keep %d force %d extent %s strides %s phase %d readable %d" % (
                        AB.NAMES[dtype], op, keep, force, extent, strides, phase, readable)
                    if name != name_of(dtype, op, form) or cls != (2 if form == 2 else 0):
                        failures.append("%s: kernel %s class %d, expected %s" % (what, name, cls, name_of(dtype, op, form)))
                    notes.append((what, name))
                got = dev.cpu().numpy().reshape(len(variants), region)
                for v, (keep, op, force, readable) in enumerate(variants):
                    want = img.copy()
                    want[SLACK + phase:SLACK + phase + span].reshape(-1, es)[cells] = \
                        np.ascontiguousarray(wants[keep, op]).view(np.uint8).reshape(-1, es)
                    if not np.array_equal(got[v], want):
                        inside = np.zeros(region, dtype=bool)
                        inside[SLACK + phase:SLACK + phase + span].reshape(-1, es)[cells] = True
                        where = "outside the box" if (got[v] != want)[~inside].any() else "in the box"
                        failures.append("%s: %s, %s (%s)" % (notes[v][0], where, _first_bad(got[v], want, es), notes[v][1]))
                if len(failures) > 20:
                    return failures[:20]
    if seen != {0, 1, 2}:
        failures.append("forms seen: %s" % sorted(seen))
    return failures[:20]


# ---- pencils -------------------------------------------------------------------------------------------------------------------
def nan_payloads(dtype, cells):
    """(cells, es) bytes: every real a NaN whose payload and sign depend on its position, as distinct as the format allows"""
    kind = AB.kind_of(dtype)
    u, m, e = AB.FORMATS[kind]
    nc = AB.TYPES[dtype][1]
    idx = np.arange(cells * nc, dtype=np.uint64)
    bits = (((idx & np.uint64(1)) << np.uint64(m + e)) | np.uint64(((1 << e) - 1) << m) | (np.uint64(1) + idx % np.uint64((1 << m) - 1)))
    return np.ascontiguousarray(bits.astype(u)).view(np.uint8).reshape(cells, -1)


def pencil_with_nan_ghosts(p, dtype, interior_bits):
    """uint8 image of a pencil, SLACK bytes of POISON on either side: a distinct NaN in every ghost and padding real, `interior_bits`
    (shape of the interior + (nc,)) in the interior; also the boolean mask of the interior's bytes"""
    es = AB.element_bytes(dtype)
    cells = nan_payloads(dtype, int(p.size))
    mask = np.zeros((int(p.size), es), dtype=bool)
    inner = AB.pencil3(p, cells)[interior_index(p)]
    inner[...] = np.ascontiguousarray(interior_bits).view(np.uint8).reshape(inner.shape)
    AB.pencil3(p, mask)[interior_index(p)] = True
    img = np.full(2 * SLACK + cells.size, POISON, dtype=np.uint8)
    img[SLACK:SLACK + cells.size] = cells.reshape(-1)
    full = np.zeros(img.size, dtype=bool)
    full[SLACK:SLACK + cells.size] = mask.reshape(-1)
    return img, full


def image_after(p, dtype, img, want_bits):
    es = AB.element_bytes(dtype)
    out = img.copy()
    cells = out[SLACK:SLACK + int(p.size) * es].reshape(int(p.size), es)
    inner = AB.pencil3(p, cells)[interior_index(p)]
    inner[...] = np.ascontiguousarray(want_bits).view(np.uint8).reshape(inner.shape)
    return out


def _pencil_cases(h, gd, axis, halo, padding, dtype, stream, seed, names, scale=-2.0):
    """both operations along every dim on one pencil: interior against numpy on the interior view, every other byte unchanged"""
    import torch
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
    shape = interior_shape(p, nc)
    u = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), nc, seed).reshape(shape))
    img, inside = pencil_with_nan_ghosts(p, dtype, u)
    src = torch.from_numpy(img).cuda()
    failures = []
    for op, dim in itertools.product(OPS, range(3)):
        npax = 2 - _position(p, dim)
        L = shape[npax]
        coef = coefficients(L + 2, nc, seed + dim)
        dcoef = torch.from_numpy(coef.reshape(-1).copy()).cuda()
        dev = src.clone()
        cd.cudecompAmdApplyPlanesInterior(axis, h, gd, [dev.data_ptr() + SLACK], op, dim, dcoef.data_ptr(), L, scale, dtype, halo, padding,
                                          stream)
        names.add(cd.cudecompExtLastKernelName().split("<")[0])
        got = dev.cpu().numpy()
        want = image_after(p, dtype, img, apply_reference(dtype, op, u, along(coefficient_bits(dtype, coef[:L], scale), npax)))
        if not np.array_equal(got, want):
            where = "a ghost, padding or outside byte was written" if (got != want)[~inside].any() else "interior"
            failures.append("axis %d halo %s padding %s %s op %d dim %d: %s, %s (%s)" % (
                axis, tuple(halo), tuple(padding), AB.NAMES[dtype], op, dim, where, _first_bad(got, want, es), cd.cudecompExtLastKernelName()))
    return failures


def ghosts_keep_their_bytes(rank, nranks, args):
    """one pencil with halos and padding, every axis, dim, operation and data type: ghost and padding cells hold distinct NaN
    payloads, and hold them afterwards bit for bit"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    failures, names = [], set()
    for dtype, axis in itertools.product(AB.ALL_TYPES, range(3)):
        failures += _pencil_cases(h, gd, axis, args["halo"], args["padding"], dtype, stream, 10 * AB.ALL_TYPES.index(dtype) + axis, names)
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:10]


def single_rank_sweep(rank, nranks, args):
    """shapes x memory orders x axes x halos x paddings x dims, the seven types in turn, both operations"""
    import torch
    from tests import gpu_bodies as B
    stream = torch.cuda.current_stream().cuda_stream
    failures, n, names = [], 0, set()
    for gdims, order in itertools.product(args["shapes"], args["orders"]):
        h, gd, g = B._setup(rank, nranks, {"gdims": gdims, "pdims": (1, 1), "mem_order": (order,) * 3})
        for axis, halo, padding in itertools.product(range(3), args["halos"], args["paddings"]):
            dtype = AB.ALL_TYPES[n % 7]
            n += 1
            for f in _pencil_cases(h, gd, axis, halo, padding, dtype, stream, n, names):
                failures.append("gdims %s order %s %s" % (gdims, order, f))
        cd.cudecompGridDescDestroy(h, gd)
    if not set(FORMS) <= names:
        failures.append("kernels seen: %s" % sorted(names))
    return failures[:20]


def multi_field(rank, nranks, args):
    """field f of a 3-field call is byte-identical to its single-field call with its own row of coefficients (ld >= L) and with the
    shared row (ld == 0); the call makes one launch"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype, axis in ((cd.FLOAT, 0), (cd.DOUBLE_COMPLEX, 1), (cd.HALF, 2), (cd.DOUBLE, 0)):
        nc = AB.TYPES[dtype][1]
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p, nc)
        srcs = []
        for f in range(3):
            u = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), nc, 100 * AB.ALL_TYPES.index(dtype) + f).reshape(shape))
            srcs.append(torch.from_numpy(pencil_with_nan_ghosts(p, dtype, u)[0]).cuda())
        for op, dim, shared in itertools.product(OPS, range(3), (False, True)):
            L = shape[2 - _position(p, dim)]
            ld = 0 if shared else L + 3
            rows = np.concatenate([coefficients(L + 3, nc, 7 * f + dim) for f in range(3)])  # (3 * (L + 3), 2)
            dcoef = torch.from_numpy(rows.reshape(-1).copy()).cuda()
            single = []
            for f in range(3):
                d = srcs[f].clone()
                at = dcoef.data_ptr() + (0 if shared else 16 * f * ld)
                cd.cudecompAmdApplyPlanesInterior(axis, h, gd, [d.data_ptr() + SLACK], op, dim, at, L, 0.5, dtype, halo, padding, stream)
                single.append(d.cpu().numpy())
            devs = [s.clone() for s in srcs]
            torch.cuda.synchronize()
            before = cd.cudecompExtDataLaunchCount()
            cd.cudecompAmdApplyPlanesInterior(axis, h, gd, [d.data_ptr() + SLACK for d in devs], op, dim, dcoef.data_ptr(), ld, 0.5, dtype,
                                              halo, padding, stream)
            launches = cd.cudecompExtDataLaunchCount() - before
            what = "%s axis %d op %d dim %d ld %d" % (AB.NAMES[dtype], axis, op, dim, ld)
            if launches != 1:
                failures.append("%s: %d launches" % (what, launches))
            for f in range(3):
                if not np.array_equal(devs[f].cpu().numpy(), single[f]):
                    failures.append("%s: field %d differs from its single-field call" % (what, f))
                if np.array_equal(single[f], srcs[f].cpu().numpy()):
                    failures.append("%s: field %d was not changed at all" % (what, f))
            if not shared and len({s.tobytes() for s in single}) < 3:
                failures.append("%s: the fields do not differ" % what)
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:20]


# ---- the coefficient's conversion, IEEE edge values ------------------------------------------------------------------------------
def conversion_values(kind):
    u, m, e = AB.FORMATS[kind]
    bias = (1 << (e - 1)) - 1
    # the first power of two that overflows (fp64: the largest one there is -- nothing overflows a double); the smallest subnormal
    big, tiny = 2.0 ** min(bias + 1, 1023), 2.0 ** (1 - bias - m)
    v = [1.0 + 2.0 ** -(m + 1) + 2.0 ** -30,            # just above a tie: rounds UP to 1 + 2^-m directly; through fp32, for the
         1.0 + 2.0 ** -(m + 1) - 2.0 ** -30,            # 2-byte types, the tie goes to even, 1.0.  Just below: down
         1.0 + 2.0 ** -(m + 1), 1.0 + 3 * 2.0 ** -(m + 1),  # exact ties: to even, down and up
         big, -big, big * (1 - 2.0 ** -(m + 2)), big * (1 - 2.0 ** -(m + 3)), 1e300, -1e300,  # overflow; the tie at the top; below it
         tiny, -tiny, tiny * 0.5, tiny * 0.5000001, tiny * 1.5, tiny * 0.4999, 3.3 * tiny, 2.0 ** (1 - bias) * (1 - 2.0 ** -(m + 1)),
         1e-320, -1e-320,  # subnormals of the type, ties between them, the largest subnormal's tie to the smallest normal
         0.0, -0.0, float("inf"), float("-inf"), float("nan"), 0.1, -1.0 / 3.0, 1234.56789, 2.0 / 3.0 * 2.0 ** -(bias - 3)]
    return np.array(v, dtype=np.float64)


def coefficient_conversion(rank, nranks, args):
    """ADD onto zeros returns the coefficient in T: values at which a rounding through fp32 differs from the direct one, overflow,
    subnormals, signed zeros, infinities and NaN; with scale 1 and with scales whose fp64 product rounds; through the row form (one
    conversion per workgroup), the column form (one per lane and real) and the element form.  Expected: exact rational rounding."""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    stated = {"fp16": (1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -10), "bf16": (1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -7)}
    for dtype in AB.ALL_TYPES:
        kind, nc, es = AB.kind_of(dtype), AB.TYPES[dtype][1], AB.element_bytes(dtype)
        u, m, e = AB.FORMATS[kind]
        vals = conversion_values(kind)
        if kind in stated:  # the issue's figures, spelled out: directly 1 + ulp, through fp32 1.0
            x, y = stated[kind]
            one_ulp = exact_bits(kind, y)
            if vals[0] != x or exact_bits(kind, x) != one_ulp or exact_bits(kind, float(np.float32(x))) != exact_bits(kind, 1.0):
                failures.append("%s: the reference does not give the stated values" % kind)
        L = vals.size
        pairs = np.stack([vals, np.roll(vals, 5) if nc == 2 else np.full(L, np.nan)], axis=1)
        dcoef = torch.from_numpy(pairs.reshape(-1).copy()).cuda()
        for scale in (1.0, 0.1, -3.0, 1e-3):
            with np.errstate(all="ignore"):
                prod = np.float64(scale) * pairs[:, :nc]
            cbits = np.array([[exact_bits(kind, float(x)) for x in row] for row in prod], dtype=u)
            if not (AB.mismatches(kind, to_real_bits(kind, prod), cbits) == False).all():  # noqa: E712 (the vectorised reference agrees)
                failures.append("%s scale %g: to_real_bits differs from exact_bits" % (AB.NAMES[dtype], scale))
            zeros = np.zeros((1, 1, 1, nc), dtype=u)
            for keep, force in itertools.product((0, 1), (0, 1)):
                extent = (L, 3, 1) if keep == 0 else (5, L, 1)
                pitch = (extent[0] * es + 15) // 16 * 16 // es
                strides = (1, pitch, pitch * extent[1])
                buf = torch.zeros(strides[2] * es + 32, dtype=torch.uint8, device="cuda")
                cd.cudecompExtPlanes3D(buf.data_ptr(), dtype, cd.PLANES_ADD, keep, extent, strides, 0, 32, dcoef.data_ptr(), scale, force,
                                       stream)
                name = cd.cudecompExtLastKernelName()
                got = buf.cpu().numpy()[:strides[2] * es].view(u).reshape(extent[1], pitch, nc)[:, :extent[0]]
                want = np.broadcast_to(apply_reference(dtype, cd.PLANES_ADD, zeros, along(cbits, 2 - keep))[0], got.shape)
                bad = AB.mismatches(kind, got, want)
                if bad.any():
                    at = np.argwhere(bad)[0]
                    k = at[1] if keep == 0 else at[0]
                    failures.append("%s scale %g keep %d force %d (%s): coefficient %r * scale gave %#x, want %#x (%d wrong)" % (
                        AB.NAMES[dtype], scale, keep, force, name, float(pairs[k, at[2]]), int(got[tuple(at)]), int(want[tuple(at)]), int(bad.sum())))
    return failures[:20]


def edge_values(rank, nranks, args):
    """all pairs of the type's edge table as (u, c), both operations, the three forms; complex types pair the table with two of its
    rotations.  Classes and bits as AB.mismatches compares them."""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype in AB.ALL_TYPES:
        kind, nc, es = AB.kind_of(dtype), AB.TYPES[dtype][1], AB.element_bytes(dtype)
        u, m, e = AB.FORMATS[kind]
        table = AB.edge_table(kind)
        K = len(table)
        tab = np.stack([table, np.roll(table, 7)][:nc], axis=-1)            # (K, nc): the cells' values
        ctab = np.stack([table, np.roll(table, 5)][:nc], axis=-1)           # (K, nc): the coefficients, exact in the type
        if kind == "bf16":
            wide = (ctab.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        else:
            wide = ctab.view(AB._FLOAT_OF_KIND[kind]).astype(np.float64)    # widening is exact; a NaN stays a NaN
        pairs = np.full((K, 2), np.nan)
        pairs[:, :nc] = wide
        dcoef = torch.from_numpy(pairs.reshape(-1).copy()).cuda()
        cbits = to_real_bits(kind, pairs[:, :nc])
        for op, keep, force in itertools.product(OPS, (0, 1), (0, 1)):
            # keep 0: c runs along the contiguous dim, u down the rows (column form); keep 1: u along the row, c from row to row
            cells = np.broadcast_to(tab[:, None, :] if keep == 0 else tab[None, :, :], (K, K, nc))
            pitch = (K * es + 15) // 16 * 16 // es
            img = np.zeros((K, pitch, nc), dtype=u)
            img[:, :K] = cells
            dev = torch.from_numpy(img.view(np.uint8).reshape(-1).copy()).cuda()
            cd.cudecompExtPlanes3D(dev.data_ptr(), dtype, op, keep, (K, K, 1), (1, pitch, pitch * K), 0, 0, dcoef.data_ptr(), 1.0, force, stream)
            name = cd.cudecompExtLastKernelName()
            got = dev.cpu().numpy().view(u).reshape(K, pitch, nc)[:, :K]
            want = apply_reference(dtype, op, cells, cbits[None, :, :] if keep == 0 else cbits[:, None, :])
            bad = AB.mismatches(kind, got, want)
            if bad.any():
                at = tuple(np.argwhere(bad)[0])
                failures.append("%s op %d keep %d force %d (%s): u %s c %s gave %#x want %#x (%d of %d wrong)" % (
                    AB.NAMES[dtype], op, keep, force, name, [hex(int(x)) for x in cells[at[0], at[1]]],
                    [hex(int(x)) for x in (cbits[at[1]] if keep == 0 else cbits[at[0]])], int(got[at]), int(want[at]), int(bad.sum()), bad.size))
    return failures[:20]


# ---- with the profile ------------------------------------------------------------------------------------------------------------
def round_trip_with_the_profile(rank, nranks, args):
    """integer data whose plane means are integers, planes of a power-of-two number of cells (so that -1/n and n * mean are exact):
    SUM profile, ADD with scale -1/n, SUM profile again: +0.0 in every entry, and the cells are the fluctuations"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype, axis, dim in itertools.product((cd.FLOAT, cd.DOUBLE), range(3), range(3)):
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p, 1)
        npax = 2 - _position(p, dim)
        L, n = shape[npax], int(np.prod(shape[:3])) // shape[npax]
        if n & (n - 1):
            return ["the planes along dim %d hold %d cells: not a power of two" % (dim, n)]
        fluct = np.where(np.arange(n) % 2 == 0, (np.arange(n) // 2) % 7 + 1, -((np.arange(n) // 2) % 7 + 1))  # pairs x, -x
        means = (np.arange(L) * 3) % 11 - 5
        vals = np.moveaxis((means[:, None] + fluct[None, :]).reshape([L] + [s for i, s in enumerate(shape[:3]) if i != npax]), 0, npax)
        u = bits_from_exact(dtype, vals.reshape(shape))
        img, inside = pencil_with_nan_ghosts(p, dtype, u)
        dev = torch.from_numpy(img).cuda()
        res, work = Results(L), _workspace(1, L)
        ptr = [dev.data_ptr() + SLACK]
        cd.cudecompAmdProfileInterior(axis, h, gd, ptr, None, cd.REDUCE_SUM, dim, res.buf.data_ptr(), L, work.data_ptr(), dtype, halo, padding, stream)
        cd.cudecompAmdApplyPlanesInterior(axis, h, gd, ptr, cd.PLANES_ADD, dim, res.buf.data_ptr(), L, -1.0 / n, dtype, halo, padding, stream)
        torch.cuda.synchronize()
        first = res.host()
        cd.cudecompAmdProfileInterior(axis, h, gd, ptr, None, cd.REDUCE_SUM, dim, res.buf.data_ptr(), L, work.data_ptr(), dtype, halo, padding, stream)
        second = res.host()
        what = "%s axis %d dim %d" % (AB.NAMES[dtype], axis, dim)
        if not same_bits(first, profile_reference(cd.REDUCE_SUM, vals.reshape(shape), None, npax)):
            failures.append("%s: the first profile is %s" % (what, first.tolist()))
        if not same_bits(second, np.zeros((L, 2))):
            failures.append("%s: the profile of the fluctuations is %s" % (what, second.tolist()))
        want = image_after(p, dtype, img, bits_from_exact(dtype, (vals - np.moveaxis(means.reshape(L, 1, 1), 0, npax)).reshape(shape)))
        if not np.array_equal(dev.cpu().numpy(), want):
            failures.append("%s: the cells are not the fluctuations" % what)
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:10]


# ---- several ranks -------------------------------------------------------------------------------------------------------------
def ranks_sweep(rank, nranks, args):
    """every rank passes coef + 2 * lo[dim] of ONE global coefficient array with ld = the global extent (the header's recipe): every
    owned cell equals the closed form u(x, y, z) + c[index along dim], ghost bytes are unchanged; a rank whose interior is empty
    makes no launch and changes nothing.  [failures, {case: [cells, launches]}]"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    gdims = args["gdims"]
    stream = torch.cuda.current_stream().cuda_stream
    failures, mine = [], {}
    wa, wb = closed_form(gdims)
    n = 0
    for axis, halo in itertools.product(range(3), args["halos"]):
        dtype = AB.ALL_TYPES[n % 7] if not args.get("dtype") else args["dtype"]
        n += 1
        nc, es = AB.TYPES[dtype][1], AB.element_bytes(dtype)
        padding = (0, 1, 0)
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        sa, sb = rank_slab(p, wa), rank_slab(p, wb)
        shape = interior_shape(p, nc)
        if sa.shape != shape[:3]:
            failures.append("rank %d axis %d halo %s: slab %s, interior %s" % (rank, axis, halo, sa.shape, shape))
            continue
        u = bits_from_exact(dtype, np.stack([sa, sb][:nc], axis=-1))
        img, inside = pencil_with_nan_ghosts(p, dtype, u)
        src = torch.from_numpy(img).cuda()
        cells = int(np.prod(shape[:3]))
        for dim in range(3):
            pos = _position(p, dim)
            L, N, lo = shape[2 - pos], gdims[dim], int(p.lo[pos])
            glob = np.full((2, N, 2), np.nan)           # two rows: a second field would take the second
            glob[0, :, 0] = (np.arange(N) * 3) % 7 - 3  # c[index along dim], the same array on every rank
            if nc == 2:
                glob[0, :, 1] = (np.arange(N) * 5) % 9 - 4
            dglob = torch.from_numpy(glob.reshape(-1).copy()).cuda()
            dev = src.clone()
            torch.cuda.synchronize()
            before = cd.cudecompExtDataLaunchCount()
            cd.cudecompAmdApplyPlanesInterior(axis, h, gd, [dev.data_ptr() + SLACK], cd.PLANES_ADD, dim, dglob.data_ptr() + 16 * lo, N, 1.0,
                                              dtype, halo, padding, stream)
            launches = cd.cudecompExtDataLaunchCount() - before
            got = dev.cpu().numpy()
            if cells:
                c = bits_from_exact(dtype, glob[0, lo:lo + L, :nc])
                want = image_after(p, dtype, img, apply_reference(dtype, cd.PLANES_ADD, u, along(c, 2 - pos)))
            else:
                want = img
            if not np.array_equal(got, want) or launches != (1 if cells else 0):
                where = "a ghost byte was written" if (got != want)[~inside].any() else "owned cells"
                failures.append("rank %d axis %d halo %s %s dim %d: %s; %d launches for %d cells" % (rank, axis, halo, AB.NAMES[dtype], dim,
                                                                                                  where, launches, cells))
            mine["%d %s %d" % (axis, tuple(halo), dim)] = [cells, launches]
    cd.cudecompGridDescDestroy(h, gd)
    return [failures, mine]


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def graph_replay(rank, nranks, args):
    """one call per kept position captured; a replay equals the eager call; the coefficient array's CONTENTS change, a replay equals
    an eager call with the new contents"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype, op = args.get("axis", 0), args.get("dtype", cd.DOUBLE), args.get("op", cd.PLANES_MUL)
    halo, padding = args["halo"], args.get("padding", (0, 0, 0))
    nc = AB.TYPES[dtype][1]
    p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
    shape = interior_shape(p, nc)
    u = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), nc, 5).reshape(shape))
    img, inside = pencil_with_nan_ghosts(p, dtype, u)
    src = torch.from_numpy(img).cuda()
    failures, names = [], set()
    for pos in range(3):
        dim, L = int(p.order[pos]), shape[2 - pos]
        contents = [torch.from_numpy(coefficients(L, nc, s).reshape(-1).copy()).cuda() for s in (1, 2)]
        coef = contents[0].clone()
        field, eager = src.clone(), src.clone()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())

        def call(t, sptr):
            cd.cudecompAmdApplyPlanesInterior(axis, h, gd, [t.data_ptr() + SLACK], op, dim, coef.data_ptr(), L, -2.0, dtype, halo, padding, sptr)

        with torch.cuda.stream(stream):
            call(field, stream.cuda_stream)  # warm-up
            stream.synchronize()
        names.add(cd.cudecompExtLastKernelName().split("<")[0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            call(field, torch.cuda.current_stream().cuda_stream)
        seen = []
        for it in (0, 1):
            with torch.cuda.stream(stream):
                coef.copy_(contents[it])  # the contents change on the stream; the pointers, and the graph, stay
                field.copy_(src)
                eager.copy_(src)
                graph.replay()
                call(eager, stream.cuda_stream)
                stream.synchronize()
            r, e = field.cpu().numpy(), eager.cpu().numpy()
            seen.append(r)
            want = image_after(p, dtype, img, apply_reference(dtype, op, u, along(coefficient_bits(
                dtype, contents[it].cpu().numpy().reshape(-1, 2), -2.0), 2 - pos)))
            if not np.array_equal(r, e) or not np.array_equal(r, want):
                failures.append("position %d replay %d: equals eager %s, equals numpy %s" % (pos, it, np.array_equal(r, e), np.array_equal(r, want)))
        if np.array_equal(seen[0], seen[1]):
            failures.append("position %d: the two contents give one result" % pos)
        del graph
    if len(names) != 2:  # rows for positions 1 and 2, columns or element-wise for position 0
        failures.append("kernels seen: %s" % sorted(names))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """a long run of kernels is enqueued on a stream, then plane updates: the calls return while that work is still running (an event
    recorded behind them has not completed), and the cells are right once it has"""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding, dtype = args["halo"], (0, 0, 0), cd.DOUBLE
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo, padding)
    shape = interior_shape(p, 1)
    u = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), 1, 3).reshape(shape))
    img, inside = pencil_with_nan_ghosts(p, dtype, u)
    src = torch.from_numpy(img).cuda()
    dev = src.clone()
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    dims = [int(p.order[pos]) for pos in range(3)]
    coefs = [coefficients(shape[2 - pos], 1, pos) for pos in range(3)]
    dcoefs = [torch.from_numpy(c.reshape(-1).copy()).cuda() for c in coefs]

    def calls():
        for pos in range(3):
            cd.cudecompAmdApplyPlanesInterior(0, h, gd, [dev.data_ptr() + SLACK], cd.PLANES_ADD, dims[pos], dcoefs[pos].data_ptr(),
                                              shape[2 - pos], 1.0, dtype, halo, padding, stream.cuda_stream)

    calls()  # warm-up: first-use work happens before the timed part
    torch.cuda.synchronize()
    dev.copy_(src)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.get("kernels", 100)):
        big.add_(1.0)
    t1 = time.perf_counter()
    calls()
    t2 = time.perf_counter()
    done = torch.cuda.Event()
    done.record(stream)
    pending = not done.query()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    want_bits = u
    for pos in range(3):
        want_bits = apply_reference(dtype, cd.PLANES_ADD, want_bits, along(coefficient_bits(dtype, coefs[pos], 1.0), 2 - pos))
    failures = [] if np.array_equal(dev.cpu().numpy(), image_after(p, dtype, img, want_bits)) else ["the cells differ from numpy's"]
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": failures, "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3, "host_ms": (t2 - t1) * 1e3,
            "total_ms": (t3 - t0) * 1e3}
