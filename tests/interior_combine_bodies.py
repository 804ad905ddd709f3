"""Bodies of tests/test_gpu_interior_combine.py: every function runs on a rank launched by tests/mp.py (the pytest process never opens
the GPU) and returns a list of failure strings, or a dict that holds one.

The reference is numpy in the arithmetic cudecomp_interior_combine.h states, on BIT PATTERNS (the only form numpy has for bf16): a
coefficient is the fp64 product scale * num, then the fp64 quotient by den, rounded once to the real type directly from the double
(tests/interior_planes_bodies.py `to_real_bits`, and `exact_bits` through fractions for the test of the conversion itself); t = a * x
and s = b * y are typed products (complex: four products, a difference and a sum), and the stored value is y + t, x + s, t + s or t,
every product and sum rounded on its own.  All comparisons are bit for bit (an expected NaN: any NaN, AB.mismatches)."""
import itertools
from fractions import Fraction

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests.interior_planes_bodies import (_first_bad, bits_from_exact, conversion_values, exact_bits, image_after, negated,
                                          pencil_with_nan_ghosts, sentinel, to_real_bits, typed_mul)
from tests.interior_profile_bodies import pitches
from tests.interior_reduce_bodies import (ARITH, LENGTHS, POISON, SLACK, Scratch, closed_form, integers, interior_shape, rank_slab,
                                          same_bits)

OPS = (cd.COMBINE_AXPY, cd.COMBINE_XPBY, cd.COMBINE_AXPBY, cd.COMBINE_AX)
OP_NAMES = ("axpy", "xpby", "axpby", "ax")
NAN = float("nan")


# ---- the definition in numpy -----------------------------------------------------------------------------------------------------
def coefficient_double(nc, num, den, scale):
    """(nc,) float64: (scale * num[c]) / den[0]; num None: the pair (1, 0); den None: no division"""
    with np.errstate(all="ignore"):
        v = np.float64(scale) * (np.array([1.0, 0.0]) if num is None else np.asarray(num, dtype=np.float64))[:nc]
        if den is not None:
            v = v / np.float64(np.asarray(den, dtype=np.float64).reshape(-1)[0])
    return v


def coefficient_bits(dtype, num, den, scale):
    return to_real_bits(AB.kind_of(dtype), coefficient_double(AB.TYPES[dtype][1], num, den, scale))


def scaled(dtype, c, v):
    """c * v: c (nc,) bit patterns, v (..., nc) bit patterns; the complex product (cr vr - ci vi, cr vi + ci vr)"""
    v = np.ascontiguousarray(v)
    col = lambda arr, k: np.ascontiguousarray(arr[..., k])  # noqa: E731
    like = lambda k: np.ascontiguousarray(np.broadcast_to(c[k], v.shape[:-1]))  # noqa: E731
    if v.shape[-1] == 1:
        return typed_mul(dtype, like(0), col(v, 0))[..., None]
    cr, ci, vr, vi = like(0), like(1), col(v, 0), col(v, 1)
    re = AB.typed_add(dtype, typed_mul(dtype, cr, vr), negated(dtype, typed_mul(dtype, ci, vi)))  # (p - q is p + (-q), exactly)
    im = AB.typed_add(dtype, typed_mul(dtype, cr, vi), typed_mul(dtype, ci, vr))
    return np.stack([re, im], axis=-1)


def combine_reference(dtype, op, x, y, a, b):
    """x, y: bit patterns (..., nc); a, b: (nc,) bit patterns (the one the op does not use may be None); what is stored in y"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    t = scaled(dtype, a, x) if op != cd.COMBINE_XPBY else None
    s = scaled(dtype, b, y) if op in (cd.COMBINE_XPBY, cd.COMBINE_AXPBY) else None
    if op == cd.COMBINE_AXPY:
        return AB.typed_add(dtype, y, t)
    if op == cd.COMBINE_XPBY:
        return AB.typed_add(dtype, x, s)
    if op == cd.COMBINE_AXPBY:
        return AB.typed_add(dtype, t, s)
    return t


def name_of(dtype, op, rows):
    if not rows:
        return "combine_elements_kernel<%s>" % ARITH[dtype]
    return "combine_rows_kernel<%s,%d,%s>" % (ARITH[dtype], op, "true" if AB.TYPES[dtype][1] == 2 else "false")


class Coefs:
    """the four coefficient arrays of a call on the device: `n` pairs each; a = (a_scale * a_num) / a_den, b likewise.  Real types
    get a NaN as the second double of every num pair, and every den pair a NaN as its second double: neither is ever used."""

    def __init__(self, nc, a_num, a_den, b_num, b_den, a_scale=1.0, b_scale=1.0):
        import torch
        self.nc, self.a_scale, self.b_scale = nc, a_scale, b_scale
        self.host, self.dev = {}, {}
        for key, v in (("a_num", a_num), ("a_den", a_den), ("b_num", b_num), ("b_den", b_den)):
            if v is None:
                self.host[key], self.dev[key] = None, None
                continue
            pairs = np.array(v, dtype=np.float64).reshape(-1, 2).copy()
            if key.endswith("den") or nc == 1:
                pairs[:, 1] = NAN
            self.host[key] = pairs
            self.dev[key] = torch.from_numpy(pairs.reshape(-1).copy()).cuda()

    def ptr(self, key, i=0):
        return None if self.dev[key] is None else self.dev[key].data_ptr() + 16 * i

    def kwargs(self, i=0):
        return dict(a_num=self.ptr("a_num", i), a_den=self.ptr("a_den", i), a_scale=self.a_scale, b_num=self.ptr("b_num", i),
                    b_den=self.ptr("b_den", i), b_scale=self.b_scale)

    def bits(self, dtype, i=0):
        pick = lambda key: None if self.host[key] is None else self.host[key][i]  # noqa: E731
        return (coefficient_bits(dtype, pick("a_num"), pick("a_den"), self.a_scale),
                coefficient_bits(dtype, pick("b_num"), pick("b_den"), self.b_scale))


def some_coefs(nc, seed, n=1):
    """coefficients that are ratios: a = (-1 * (3 + k, -1.5)) / 2, b = (1 * (0.5, 2)) / (4 - (k & 1) * 8): no ones, no zeros"""
    k = np.arange(n) + seed % 3
    a_num = np.stack([3.0 + k, np.full(n, -1.5)], axis=1)
    a_den = np.stack([np.full(n, 2.0), np.zeros(n)], axis=1)
    b_num = np.stack([0.5 + 0 * k, 2.0 + k], axis=1)
    b_den = np.stack([4.0 - (k & 1) * 8.0, np.zeros(n)], axis=1)
    return Coefs(nc, a_num, a_den, b_num, b_den, -1.0, 1.0)


# ---- kernel parity through cudecompExtCombine3D --------------------------------------------------------------------------------
def _boxes(dtype):
    """(extent, strides, phases, forces) of the parity sweep: the row lengths of the reduction's sweep at three pitches and every phase
    of the 16-byte grid; rows longer than a tile column (fp64: 520 reals at pitch 530, 3 rows); one contiguous box cut into two rows
    (fp64: 600 reals); more rows than a tile; more tiles than workgroups"""
    rs, es = AB.real_bytes(dtype), AB.element_bytes(dtype)
    for length, (rows, planes) in itertools.product(LENGTHS, ((1, 1), (3, 2), (5, 1))):
        for which, pitch in enumerate(pitches(length, es)):
            strides = (1, pitch, pitch * (rows + 1) if which == 2 else pitch * rows + 5)
            yield (length, rows, planes), strides, range(0, 16, rs), ((0, 1, 2, 3) if length in (7, 130) else (0, 1))
    long_row = 4096 // es + 8 * 8 // es
    yield (long_row, 3, 1), (1, long_row + 10, 3 * (long_row + 10)), sorted({0, rs, 16 - rs}), (0, 1)
    cut = 4800 // es
    yield (cut, 1, 1), (1, cut, cut), sorted({0, rs, 16 - rs}), (0, 1)
    yield (3, 1100, 1), (1, 6, 6600), (0, 16 - rs), (0, 1)
    yield (3, 2, 2100), (1, 5, 15), (0, 16 - rs), (0, 1)


def kernel_parity(rank, nranks, args):
    """for one data type: every box of _boxes, all four operations, the row form and the forced element form, nothing and 16 bytes
    readable around the box, non-temporal access on some; x and y inside buffers of position-dependent bytes at one phase of the
    16-byte grid.  Every cell of y's box equals numpy's, every other byte of y and ALL of x are unchanged, the two forms agree bit
    for bit, the kernel's name and class; and x at another phase than y goes element by element with the same cells."""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    dtype = args["dtype"]
    rs, es, nc = AB.real_bytes(dtype), AB.element_bytes(dtype), AB.TYPES[dtype][1]
    stream = torch.cuda.current_stream().cuda_stream
    failures, n, seen = [], 0, set()
    for extent, strides, phases, forces in _boxes(dtype):
        length, rows, planes = extent
        cells = (np.arange(planes)[:, None, None] * strides[2] + np.arange(rows)[None, :, None] * strides[1] +
                 np.arange(length)[None, None, :]).reshape(-1).astype(np.int64)
        span = (int(cells.max()) + 1) * es
        n += 1
        x = bits_from_exact(dtype, integers(cells.size, nc, n)).reshape(planes, rows, length, nc)
        y = bits_from_exact(dtype, integers(cells.size, nc, n + 1000)).reshape(planes, rows, length, nc)
        co = some_coefs(nc, n)
        a, b = co.bits(dtype)
        wants = {op: np.ascontiguousarray(combine_reference(dtype, op, x, y, a, b)).view(np.uint8).reshape(-1, es) for op in OPS}
        variants = list(itertools.product(OPS, forces, (0, 16)))
        for phase in phases:
            nbytes = 2 * SLACK + phase + span
            region = (nbytes + 15) // 16 * 16  # every variant's copy starts on the 16-byte grid: one phase for all
            img_y, img_x = sentinel(region, n), sentinel(region, n + 97)
            for img, vals in ((img_y, y), (img_x, x)):
                img[SLACK + phase:SLACK + phase + span].reshape(-1, es)[cells] = np.ascontiguousarray(vals).view(np.uint8).reshape(-1, es)
            dev_y = torch.from_numpy(np.tile(img_y, len(variants) + 1)).cuda()
            moved = np.zeros(region + 16, dtype=np.uint8)  # a second copy of x, one real further up the 16-byte grid
            moved[rs:rs + region] = img_x
            dev_x = torch.from_numpy(np.concatenate([img_x, moved])).cuda()
            if dev_y.data_ptr() % 16 or dev_x.data_ptr() % 16:
                return ["device buffers are not 16-byte aligned"]
            px = dev_x.data_ptr() + SLACK + phase
            notes = []
            for v, (op, force, readable) in enumerate(variants):
                py = dev_y.data_ptr() + v * region + SLACK + phase
                cls = cd.cudecompExtCombine3D(py, px, dtype, op, extent, strides, readable, readable, force=force, stream=stream, **co.kwargs())
                name = cd.cudecompExtLastKernelName()
                fast = not (force & 1) and (px % es == 0)
                seen.add(fast)
                what = "%s %s force %d extent %s strides %s phase %d readable %d" % (AB.NAMES[dtype], OP_NAMES[op], force, extent, strides,
                                                                                   phase, readable)
                if name != name_of(dtype, op, fast) or cls != (0 if fast else 2):
                    failures.append("%s: kernel %s class %d, expected %s" % (what, name, cls, name_of(dtype, op, fast)))
                notes.append((what, name))
            # x one real further up than y: their phases differ, the call goes element by element (nothing readable beyond the box there)
            shifted = dev_x.data_ptr() + region + rs + SLACK + phase
            py = dev_y.data_ptr() + len(variants) * region + SLACK + phase
            cls = cd.cudecompExtCombine3D(py, shifted, dtype, cd.COMBINE_AXPBY, extent, strides, 0, 0, stream=stream, **co.kwargs())
            if cd.cudecompExtLastKernelName() != name_of(dtype, 0, False) or cls != 2:
                failures.append("%s extent %s phase %d, x shifted: kernel %s" % (AB.NAMES[dtype], extent, phase, cd.cudecompExtLastKernelName()))
            variants_all = variants + [(cd.COMBINE_AXPBY, 1, 0)]
            notes.append(("%s axpby extent %s phase %d, x shifted" % (AB.NAMES[dtype], extent, phase), "combine_elements_kernel"))
            got = dev_y.cpu().numpy().reshape(len(variants_all), region)
            got_x = dev_x.cpu().numpy()
            if not np.array_equal(got_x[:region], img_x):
                failures.append("%s extent %s phase %d: x was written, %s" % (AB.NAMES[dtype], extent, phase, _first_bad(got_x[:region], img_x, es)))
            for v, (op, force, readable) in enumerate(variants_all):
                want = img_y.copy()
                want[SLACK + phase:SLACK + phase + span].reshape(-1, es)[cells] = wants[op]
                if not np.array_equal(got[v], want):
                    inside = np.zeros(region, dtype=bool)
                    inside[SLACK + phase:SLACK + phase + span].reshape(-1, es)[cells] = True
                    where = "outside the box" if (got[v] != want)[~inside].any() else "in the box"
                    failures.append("%s: %s, %s (%s)" % (notes[v][0], where, _first_bad(got[v], want, es), notes[v][1]))
            by_op = {}
            for v, (op, force, readable) in enumerate(variants_all):  # the forms agree bit for bit
                if not np.array_equal(got[v], by_op.setdefault(op, got[v])):
                    failures.append("%s: differs from %s" % (notes[v][0], notes[[w[0] for w in variants_all].index(op)][0]))
            if len(failures) > 20:
                return failures[:20]
    if seen != {True, False}:
        failures.append("forms seen: %s" % sorted(seen))
    return failures[:20]


# ---- pencils -------------------------------------------------------------------------------------------------------------------
def _pencil_cases(h, gd, axis, halo, padding, dtype, stream, seed, names, x_shift=0):
    """the four operations on one pair of pencils whose ghost and padding cells hold distinct NaN payloads: y's interior against numpy
    on the interior views, every other byte of y and all of x unchanged.  x_shift: bytes by which x lies off y's phase of the 16-byte
    grid (the call then goes element by element)"""
    import torch
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
    shape = interior_shape(p, nc)
    x = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), nc, seed).reshape(shape))
    y = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), nc, seed + 500).reshape(shape))
    img_x, _ = pencil_with_nan_ghosts(p, dtype, x)
    img_y, inside = pencil_with_nan_ghosts(p, dtype, y)
    top = np.zeros(img_y.size, dtype=bool)
    top[SLACK + AB.real_bytes(dtype) - 1:SLACK + int(p.size) * es:AB.real_bytes(dtype)] = True
    img_y[top & ~inside] ^= 0x80  # (y's ghosts are not x's: the other sign; still NaN)
    img_x = np.concatenate([np.full(x_shift, POISON, dtype=np.uint8), img_x])
    src_y, dev_x = torch.from_numpy(img_y).cuda(), torch.from_numpy(img_x).cuda()
    co = some_coefs(nc, seed)
    a, b = co.bits(dtype)
    failures = []
    for op in OPS:
        dev = src_y.clone()
        cd.cudecompAmdCombineInterior(axis, h, gd, [dev.data_ptr() + SLACK], [dev_x.data_ptr() + x_shift + SLACK], op, dtype, halo, padding,
                                      stream=stream, **co.kwargs())
        names.add(cd.cudecompExtLastKernelName().split("<")[0])
        if (cd.cudecompExtLastKernelName().split("<")[0] == "combine_elements_kernel") != bool(x_shift):
            failures.append("axis %d %s x_shift %d: kernel %s" % (axis, AB.NAMES[dtype], x_shift, cd.cudecompExtLastKernelName()))
        got = dev.cpu().numpy()
        want = image_after(p, dtype, img_y, combine_reference(dtype, op, x, y, a, b))
        if not np.array_equal(got, want):
            where = "a ghost, padding or outside byte was written" if (got != want)[~inside].any() else "interior"
            failures.append("axis %d halo %s padding %s %s %s: %s, %s (%s)" % (
                axis, tuple(halo), tuple(padding), AB.NAMES[dtype], OP_NAMES[op], where, _first_bad(got, want, es), cd.cudecompExtLastKernelName()))
    if not np.array_equal(dev_x.cpu().numpy(), img_x):
        failures.append("axis %d halo %s padding %s %s: x was written" % (axis, tuple(halo), tuple(padding), AB.NAMES[dtype]))
    return failures


def ghosts_keep_their_bytes(rank, nranks, args):
    """one pair of pencils with halos and padding, every axis, operation and data type: ghost and padding cells of x and of y hold
    distinct NaN payloads, hold them afterwards bit for bit, and influence nothing"""
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
    """shapes x memory orders x axes x halos x paddings, the seven types in turn, the four operations"""
    import torch
    from tests import gpu_bodies as B
    stream = torch.cuda.current_stream().cuda_stream
    failures, n, names = [], 0, set()
    for gdims, order in itertools.product(args["shapes"], args["orders"]):
        h, gd, g = B._setup(rank, nranks, {"gdims": gdims, "pdims": (1, 1), "mem_order": (order,) * 3})
        for axis, halo, padding in itertools.product(range(3), args["halos"], args["paddings"]):
            dtype = AB.ALL_TYPES[n % 7]
            n += 1
            for f in _pencil_cases(h, gd, axis, halo, padding, dtype, stream, n, names, x_shift=8 if n % 3 == 0 else 0):
                failures.append("gdims %s order %s %s" % (gdims, order, f))
        cd.cudecompGridDescDestroy(h, gd)
    if names != {"combine_rows_kernel", "combine_elements_kernel"}:  # (every third case has x eight bytes off y's phase)
        failures.append("kernels seen: %s" % sorted(names))
    return failures[:20]


def multi_field(rank, nranks, args):
    """field f of a 3-field call is byte-identical to its single-field call with its own pair of coefficients (coef_stride 1) and
    with the shared pair (coef_stride 0); the call makes one launch; x[2] == x[0]"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype, axis in ((cd.FLOAT, 0), (cd.DOUBLE_COMPLEX, 1), (cd.HALF, 2), (cd.DOUBLE, 0), (cd.BFLOAT16, 1)):
        nc = AB.TYPES[dtype][1]
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p, nc)
        image = lambda seed: torch.from_numpy(pencil_with_nan_ghosts(p, dtype, bits_from_exact(dtype, integers(  # noqa: E731
            int(np.prod(shape[:3])), nc, 100 * AB.ALL_TYPES.index(dtype) + seed).reshape(shape)))[0]).cuda()
        ys, xs = [image(f) for f in range(3)], [image(10), image(11)]
        xs.append(xs[0])  # x entries may repeat
        co = some_coefs(nc, 1, n=3)
        for op, stride in itertools.product(OPS, (1, 0)):
            single = []
            for f in range(3):
                d = ys[f].clone()
                cd.cudecompAmdCombineInterior(axis, h, gd, [d.data_ptr() + SLACK], [xs[f].data_ptr() + SLACK], op, dtype, halo, padding,
                                              stream=stream, **co.kwargs(f * stride))
                single.append(d.cpu().numpy())
            devs = [s.clone() for s in ys]
            torch.cuda.synchronize()
            before = cd.cudecompExtDataLaunchCount()
            cd.cudecompAmdCombineInterior(axis, h, gd, [d.data_ptr() + SLACK for d in devs], [t.data_ptr() + SLACK for t in xs], op, dtype,
                                          halo, padding, coef_stride=stride, stream=stream, **co.kwargs())
            launches = cd.cudecompExtDataLaunchCount() - before
            what = "%s axis %d %s coef_stride %d" % (AB.NAMES[dtype], axis, OP_NAMES[op], stride)
            if launches != 1:
                failures.append("%s: %d launches" % (what, launches))
            for f in range(3):
                if not np.array_equal(devs[f].cpu().numpy(), single[f]):
                    failures.append("%s: field %d differs from its single-field call" % (what, f))
                if np.array_equal(single[f], ys[f].cpu().numpy()):
                    failures.append("%s: field %d was not changed at all" % (what, f))
        # the pairs differ from field to field: with coef_stride 1 field 1 is not what the shared pair gives it
        a0, a1 = co.bits(dtype, 0)[0], co.bits(dtype, 1)[0]
        if np.array_equal(a0, a1):
            failures.append("%s: the fields' coefficients do not differ" % AB.NAMES[dtype])
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:20]


# ---- the coefficient's conversion ----------------------------------------------------------------------------------------------
def coefficient_conversion(rank, nranks, args):
    """AX on ones returns the coefficient in T (complex: on (1, 0), by the reference's product): values at which a rounding through
    fp32 differs from the direct one, overflow, subnormals, signed zeros, infinities and NaN as num without a den; with scales whose
    fp64 product rounds; quotients by 3, by zeros of both signs, by NaN, by infinity and by a tiny number, the product formed BEFORE
    the division; through the row form and the element form.  For real types the second double of num is a NaN throughout; the
    pointers of the unused b are NULL or point at NaN.  Expected: exact rational rounding of numpy's fp64 product and quotient."""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    stated = {"fp16": (1 + 2.0 ** -11 + 2.0 ** -30, 1 + 2.0 ** -10), "bf16": (1 + 2.0 ** -8 + 2.0 ** -30, 1 + 2.0 ** -7)}
    with np.errstate(all="ignore"):
        if (np.float64(0.1) * np.float64(3.0)) / np.float64(0.3) == np.float64(0.1) * (np.float64(3.0) / np.float64(0.3)):
            return ["the order of product and quotient does not show at (0.1 * 3) / 0.3"]
    nans = torch.full((4,), NAN, dtype=torch.float64, device="cuda")
    for dtype in AB.ALL_TYPES:
        kind, nc, es = AB.kind_of(dtype), AB.TYPES[dtype][1], AB.element_bytes(dtype)
        u, m, e = AB.FORMATS[kind]
        vals = conversion_values(kind)
        if kind in stated:  # the issue's figures, spelled out: directly 1 + ulp, through fp32 1.0
            v, w = stated[kind]
            if vals[0] != v or exact_bits(kind, v) != exact_bits(kind, w) or exact_bits(kind, float(np.float32(v))) != exact_bits(kind, 1.0):
                failures.append("%s: the reference does not give the stated values" % kind)
        # (num, den, scale): every value alone; with scales; then quotients
        cases = [(v, None, s) for s in (1.0, 0.1, -3.0, 1e-3) for v in vals]
        cases += [(1.0, 3.0, 1.0), (3.0, 0.3, 0.1), (1.0, 3.0, -1.0), (2.0, 3.0, 0.5), (1.0, 10.0, 1.0)]
        cases += [(v, d, s) for v in (1.0, -0.0, 0.0, float("inf"), NAN, 1e-300) for d in (0.0, -0.0, NAN, float("inf"), 1e-300, -7.0)
                  for s in (1.0, -2.0)]
        K = len(cases)
        second = np.roll(np.array([c[0] for c in cases]), 5)
        num = np.stack([np.array([c[0] for c in cases]), second if nc == 2 else np.full(K, NAN)], axis=1)
        den = np.array([[1.0 if c[1] is None else c[1], NAN] for c in cases])
        dnum, dden = torch.from_numpy(num.reshape(-1).copy()).cuda(), torch.from_numpy(den.reshape(-1).copy()).cuda()
        ones = bits_from_exact(dtype, np.array([[1.0, 0.0][:nc]] * 5))  # a row of five elements
        dev_x = torch.from_numpy(np.ascontiguousarray(ones).view(np.uint8).reshape(-1).copy()).cuda()
        want = np.empty((K, 5, nc), dtype=u)
        for k, (v, d, s) in enumerate(cases):
            dbl = coefficient_double(nc, num[k], None if d is None else den[k], s)
            a = np.array([exact_bits(kind, float(q)) for q in dbl], dtype=u)
            if AB.mismatches(kind, to_real_bits(kind, dbl), a).any():
                failures.append("%s case %s: to_real_bits differs from exact_bits" % (AB.NAMES[dtype], (v, d, s)))
            want[k] = combine_reference(dtype, cd.COMBINE_AX, ones, ones, a, None)
        pitch = (5 * es + 15) // 16 * 16  # bytes: each case's row of y on the 16-byte grid
        for force in (0, 1):
            buf = torch.full((K * pitch,), 0x5A, dtype=torch.uint8, device="cuda")
            for k, (v, d, s) in enumerate(cases):
                unused = (None, None) if k & 1 else (nans.data_ptr(), nans.data_ptr() + 16)
                cd.cudecompExtCombine3D(buf.data_ptr() + k * pitch, dev_x.data_ptr(), dtype, cd.COMBINE_AX, (5, 1, 1), (1, 5, 5), 0, 0,
                                        a_num=dnum.data_ptr() + 16 * k, a_den=None if d is None else dden.data_ptr() + 16 * k, a_scale=s,
                                        b_num=unused[0], b_den=unused[1], b_scale=NAN, force=force, stream=stream)
            name = cd.cudecompExtLastKernelName()
            raw = buf.cpu().numpy().reshape(K, pitch)
            got = np.ascontiguousarray(raw[:, :5 * es]).view(u).reshape(K, 5, nc)
            if not (raw[:, 5 * es:] == 0x5A).all():
                failures.append("%s force %d: bytes beyond the rows were written" % (AB.NAMES[dtype], force))
            bad = AB.mismatches(kind, got, want)
            if bad.any():
                k = int(np.argwhere(bad)[0][0])
                failures.append("%s force %d (%s): (num, den, scale) = %r gave %s, want %s (%d cases wrong)" % (
                    AB.NAMES[dtype], force, name, cases[k], [hex(int(q)) for q in got[k, 0]], [hex(int(q)) for q in want[k, 0]],
                    int(bad.any(axis=(1, 2)).sum())))
    return failures[:20]


# ---- IEEE edge values ----------------------------------------------------------------------------------------------------------
def _fused_bits(kind, a, x, y):
    """RNE of the EXACT a * x + y of three finite reals given as bit patterns: what one fused multiply-add would store"""
    u, m, e = AB.FORMATS[kind]

    def frac(bits):
        bits = int(bits)
        sign, expo, mant = bits >> (m + e), (bits >> m) & ((1 << e) - 1), bits & ((1 << m) - 1)
        bias = (1 << (e - 1)) - 1
        v = Fraction(mant, 1 << m) * Fraction(2) ** (1 - bias) if expo == 0 else (1 + Fraction(mant, 1 << m)) * Fraction(2) ** (expo - bias)
        return -v if sign else v

    exact = frac(a) * frac(x) + frac(y)
    # exact_bits takes a float: the exact sum of these cases has at most 2m + 3 significant bits, which a double holds for every type
    # but fp64 -- there the integer arithmetic below rounds the fraction itself
    if kind != "fp64":
        return exact_bits(kind, float(exact))
    ex = exact.numerator.bit_length() - exact.denominator.bit_length()
    ulp = Fraction(2) ** (ex - m)
    while exact / ulp >= (2 << m):
        ulp *= 2
    while exact / ulp < (1 << m):
        ulp /= 2
    q = exact / ulp
    k, rem = q.numerator // q.denominator, q - q.numerator // q.denominator
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
        k += 1
    return int(np.float64(float(Fraction(k) * ulp)).view(np.uint64))


def edge_values(rank, nranks, args):
    """all pairs of the type's edge table as (x, y) -- infinities of both signs, signed zeros, subnormals, the largest finite value,
    NaN -- with coefficient pairs that are edge values themselves, the four operations, both forms; complex types pair the table with
    a rotation of itself, and complex inf * 0 gives NaN; and, per real type, a = x = 1 + ulp, y = 1 - ulp / 2: the separately rounded
    a * x + y is 2, the fused one 2 + ulp -- the library stores 2."""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype in AB.ALL_TYPES:
        kind, nc, es = AB.kind_of(dtype), AB.TYPES[dtype][1], AB.element_bytes(dtype)
        u, m, e = AB.FORMATS[kind]
        bias = (1 << (e - 1)) - 1
        table = AB.edge_table(kind)
        K = len(table)
        tab_x = np.stack([table, np.roll(table, 7)][:nc], axis=-1)
        tab_y = np.stack([np.roll(table, 3), np.roll(table, 11)][:nc], axis=-1)
        x = np.ascontiguousarray(np.broadcast_to(tab_x[None, :, :], (K, K, nc)))
        y = np.ascontiguousarray(np.broadcast_to(tab_y[:, None, :], (K, K, nc)))
        pitch = (K * es + 15) // 16 * 16 // es

        def image(cells):
            img = np.zeros((K, pitch, nc), dtype=u)
            img[:, :K] = cells
            return img.view(np.uint8).reshape(-1).copy()

        dev_x, src_y = torch.from_numpy(image(x)).cuda(), torch.from_numpy(image(y)).cuda()
        big, tiny = 2.0 ** bias * (2 - 2.0 ** -m), 2.0 ** (1 - bias - m)
        for a_pair, b_pair in (((1.0, 0.0), (1.0, 0.0)), ((-1.0, 0.5), (0.5, -2.0)), ((0.0, -0.0), (-0.0, 0.0)),
                               ((float("inf"), 1.0), (1.0, float("-inf"))), ((big, tiny), (tiny, -big)), ((NAN, 1.0), (2.0, NAN))):
            co = Coefs(nc, [a_pair], None, [b_pair], None)
            a, b = co.bits(dtype)
            for op, force in itertools.product(OPS, (0, 1)):
                dev = src_y.clone()
                cd.cudecompExtCombine3D(dev.data_ptr(), dev_x.data_ptr(), dtype, op, (K, K, 1), (1, pitch, pitch * K), 0, 0, force=force,
                                        stream=stream, **co.kwargs())
                name = cd.cudecompExtLastKernelName()
                got = dev.cpu().numpy().view(u).reshape(K, pitch, nc)[:, :K]
                want = combine_reference(dtype, op, x, y, a, b)
                bad = AB.mismatches(kind, got, want)
                if bad.any():
                    at = tuple(np.argwhere(bad)[0])
                    failures.append("%s %s a %s b %s force %d (%s): x %s y %s gave %#x want %#x (%d of %d wrong)" % (
                        AB.NAMES[dtype], OP_NAMES[op], a_pair, b_pair, force, name, [hex(int(q)) for q in x[at[0], at[1]]],
                        [hex(int(q)) for q in y[at[0], at[1]]], int(got[at]), int(want[at]), int(bad.sum()), bad.size))
        if nc == 2:  # complex inf * 0: x = (inf, 0), a = (1, 0): (1 * inf - 0 * 0, 1 * 0 + 0 * inf) = (inf, NaN)
            xi = bits_from_exact(dtype, np.array([[float("inf"), 0.0]] * 3))
            one = bits_from_exact(dtype, np.array([1.0, 0.0]))
            want = combine_reference(dtype, cd.COMBINE_AX, xi, xi, one, None)
            cls = AB.classes(kind, want)
            if not (cls["nan"][:, 1].all() and not cls["nan"][:, 0].any()):
                failures.append("%s: the reference does not give (inf, NaN) for 1 * (inf, 0)" % AB.NAMES[dtype])
            dx = torch.from_numpy(np.ascontiguousarray(xi).view(np.uint8).reshape(-1).copy()).cuda()
            co = Coefs(nc, [(1.0, 0.0)], None, None, None)
            for force in (0, 1):
                dy = torch.zeros(3 * es, dtype=torch.uint8, device="cuda")
                cd.cudecompExtCombine3D(dy.data_ptr(), dx.data_ptr(), dtype, cd.COMBINE_AX, (3, 1, 1), (1, 3, 3), 0, 0, force=force,
                                        stream=stream, **co.kwargs())
                if AB.mismatches(kind, dy.cpu().numpy().view(u).reshape(3, 2), want).any():
                    failures.append("%s force %d: 1 * (inf, 0) gave %s" % (AB.NAMES[dtype], force, dy.cpu().numpy().view(u).tolist()))
            continue
        # fused against unfused, real types: a = x = 1 + 2^-m, y = 1 - 2^-m
        ax = bits_from_exact(dtype, np.array([1.0 + 2.0 ** -m]))
        yy = bits_from_exact(dtype, np.array([1.0 - 2.0 ** -m]))
        cells_x, cells_y = np.tile(ax, 9).reshape(9, 1), np.tile(yy, 9).reshape(9, 1)
        want = combine_reference(dtype, cd.COMBINE_AXPY, cells_x, cells_y, ax, None)
        fused = _fused_bits(kind, ax[0], ax[0], yy[0])
        two = int(bits_from_exact(dtype, np.array([2.0]))[0])
        if int(want[0, 0]) != two or fused != two + 1:
            failures.append("%s: the reference gives %#x unfused and %#x fused, not 2 and 2 + ulp" % (AB.NAMES[dtype], int(want[0, 0]), fused))
        co = Coefs(nc, [(1.0 + 2.0 ** -m, NAN)], None, [(1.0, NAN)], None)
        dx = torch.from_numpy(np.ascontiguousarray(cells_x).view(np.uint8).reshape(-1).copy()).cuda()
        for op, force in itertools.product((cd.COMBINE_AXPY, cd.COMBINE_AXPBY), (0, 1)):  # (AXPBY with b = 1: the same sum)
            dy = torch.from_numpy(np.ascontiguousarray(cells_y).view(np.uint8).reshape(-1).copy()).cuda()
            cd.cudecompExtCombine3D(dy.data_ptr(), dx.data_ptr(), dtype, op, (9, 1, 1), (1, 9, 9), 0, 0, force=force, stream=stream,
                                    **co.kwargs())
            got = dy.cpu().numpy().view(u)
            if not (got == two).all():
                failures.append("%s %s force %d: (1 + ulp)^2 + (1 - ulp / 2) gave %s, unfused %#x, fused %#x" % (
                    AB.NAMES[dtype], OP_NAMES[op], force, [hex(int(q)) for q in got[:3]], two, fused))
    return failures[:20]


# ---- one CG step -----------------------------------------------------------------------------------------------------------------
def cg_step(rank, nranks, args):
    """p = r (AX), r.r and p.Ap (two DOTs), x += alpha p, r -= alpha Ap (two AXPYs with a_num = rr, a_den = pAp, the second with
    a_scale = -1), r.r again, p = r + beta p (XPBY with b_num = rr_new, b_den = rr): eight calls on one stream, no synchronisation and
    no host read in between.  Small integers, and Ap = 4 p + d with p . d = 0: alpha = 1/4 and every dot product is exact in fp64,
    so numpy's x, r and p hold bit for bit."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype, axis in itertools.product((cd.DOUBLE, cd.FLOAT), range(3)):
        p_info = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p_info, 1)
        n = int(np.prod(shape[:3]))
        r0 = integers(n, 1, 3 + axis).reshape(-1)
        x0 = integers(n, 1, 30 + axis).reshape(-1)
        d = np.zeros(n, dtype=np.int64)
        d[0:n - n % 2:2], d[1:n - n % 2:2] = r0[1:n - n % 2:2], -r0[0:n - n % 2:2]
        Ap = 4 * r0 + d
        real = AB.TYPES[dtype][0]
        fields = {}
        for name, vals in (("x", x0), ("r", r0), ("p", integers(n, 1, 77).reshape(-1)), ("Ap", Ap)):
            img, inside = pencil_with_nan_ghosts(p_info, dtype, bits_from_exact(dtype, vals.reshape(shape)))
            fields[name] = (img, torch.from_numpy(img).cuda())
        ptr = {k: [v[1].data_ptr() + SLACK] for k, v in fields.items()}
        res = {k: Scratch(1) for k in ("rr", "pAp", "rr_new")}
        dot = lambda u, v, sc: cd.cudecompAmdReduceInterior(axis, h, gd, ptr[u], ptr[v], cd.REDUCE_DOT, sc.results.data_ptr(),  # noqa: E731
                                                             sc.work.data_ptr(), dtype, halo, padding, stream)
        comb = lambda yk, xk, op, **kw: cd.cudecompAmdCombineInterior(axis, h, gd, ptr[yk], ptr[xk], op, dtype, halo, padding,  # noqa: E731
                                                                       stream=stream, **kw)
        torch.cuda.synchronize()
        comb("p", "r", cd.COMBINE_AX)                                                                    # p = r
        dot("r", "r", res["rr"])
        dot("p", "Ap", res["pAp"])
        comb("x", "p", cd.COMBINE_AXPY, a_num=res["rr"].results.data_ptr(), a_den=res["pAp"].results.data_ptr())
        comb("r", "Ap", cd.COMBINE_AXPY, a_num=res["rr"].results.data_ptr(), a_den=res["pAp"].results.data_ptr(), a_scale=-1.0)
        dot("r", "r", res["rr_new"])
        comb("p", "r", cd.COMBINE_XPBY, b_num=res["rr_new"].results.data_ptr(), b_den=res["rr"].results.data_ptr())
        torch.cuda.synchronize()
        # numpy, in the real type, every product and sum rounded on its own
        r, p, x, A = r0.astype(real), r0.astype(real), x0.astype(real), Ap.astype(real)
        rr, pAp = np.float64(np.sum(r0 * r0)), np.float64(np.sum(r0 * Ap))
        alpha, minus = real(rr / pAp), real((np.float64(-1.0) * rr) / pAp)
        x1 = x + alpha * p
        r1 = r + minus * A
        rr_new = np.float64(np.sum(r1.astype(np.float64) ** 2))  # multiples of 1/4, small: exact in any order
        beta = real(rr_new / rr)
        p1 = r1 + beta * p
        what = "%s axis %d" % (AB.NAMES[dtype], axis)
        for key, want in (("rr", rr), ("pAp", pAp), ("rr_new", rr_new)):
            got = res[key].results.cpu().numpy()
            if not same_bits(got, [want, 0.0]):
                failures.append("%s: %s is %s, want %r" % (what, key, got.tolist(), float(want)))
        if alpha != real(0.25) or not np.all(r1 == (-0.25 * d).astype(real)):
            failures.append("%s: the reference's alpha is %r" % (what, float(alpha)))
        u = AB.FORMATS[AB.kind_of(dtype)][0]
        for key, want in (("x", x1), ("r", r1), ("p", p1), ("Ap", A)):
            img = image_after(p_info, dtype, fields[key][0], np.ascontiguousarray(want).view(u).reshape(shape))
            if not np.array_equal(fields[key][1].cpu().numpy(), img):
                failures.append("%s: %s differs from numpy, %s" % (what, key, _first_bad(fields[key][1].cpu().numpy(), img, AB.element_bytes(dtype))))
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:10]


# ---- several ranks -------------------------------------------------------------------------------------------------------------
def ranks_sweep(rank, nranks, args):
    """every rank combines its slabs of two closed forms of the global index, y <- 2 x - y with both coefficients ratios in device
    memory: every owned cell equals the closed form, ghost bytes are unchanged; a rank whose interior is empty makes no launch and
    changes nothing.  [failures, {case: [cells, launches]}]"""
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
        vx, vy = np.stack([sa, sb][:nc], axis=-1), np.stack([sb, sa][:nc], axis=-1)
        img_x, _ = pencil_with_nan_ghosts(p, dtype, bits_from_exact(dtype, vx))
        img_y, inside = pencil_with_nan_ghosts(p, dtype, bits_from_exact(dtype, vy))
        dev_x, dev = torch.from_numpy(img_x).cuda(), torch.from_numpy(img_y).cuda()
        cells = int(np.prod(shape[:3]))
        co = Coefs(nc, [(6.0, 0.0)], [(3.0, 0.0)], [(5.0, 0.0)], [(-5.0, 0.0)])  # a = 2, b = -1
        torch.cuda.synchronize()
        before = cd.cudecompExtDataLaunchCount()
        cd.cudecompAmdCombineInterior(axis, h, gd, [dev.data_ptr() + SLACK], [dev_x.data_ptr() + SLACK], cd.COMBINE_AXPBY, dtype, halo,
                                      padding, stream=stream, **co.kwargs())
        launches = cd.cudecompExtDataLaunchCount() - before
        got = dev.cpu().numpy()
        want = img_y
        if cells:
            ref = combine_reference(dtype, cd.COMBINE_AXPBY, bits_from_exact(dtype, vx), bits_from_exact(dtype, vy), *co.bits(dtype))
            if not np.array_equal(ref, bits_from_exact(dtype, 2 * vx - vy)):  # (small integers: exact in every type)
                failures.append("rank %d axis %d halo %s %s: the reference is not the closed form 2 x - y" % (rank, axis, halo, AB.NAMES[dtype]))
            want = image_after(p, dtype, img_y, ref)
        if not np.array_equal(got, want) or launches != (1 if cells else 0) or not np.array_equal(dev_x.cpu().numpy(), img_x):
            where = "a ghost byte was written" if (got != want)[~inside].any() else "owned cells or x"
            failures.append("rank %d axis %d halo %s %s: %s; %d launches for %d cells" % (rank, axis, halo, AB.NAMES[dtype], where, launches, cells))
        mine["%d %s" % (axis, tuple(halo))] = [cells, launches]
    cd.cudecompGridDescDestroy(h, gd)
    return [failures, mine]


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def graph_replay(rank, nranks, args):
    """one AXPBY captured; a replay equals the eager call; the CONTENTS of a_num and a_den are rewritten, a replay equals an eager call
    with the new ratio, without re-capture"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype = args.get("axis", 0), args.get("dtype", cd.DOUBLE)
    halo, padding = args["halo"], args.get("padding", (0, 0, 0))
    nc = AB.TYPES[dtype][1]
    p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
    shape = interior_shape(p, nc)
    x = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), nc, 5).reshape(shape))
    y = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), nc, 6).reshape(shape))
    img_x, _ = pencil_with_nan_ghosts(p, dtype, x)
    img_y, inside = pencil_with_nan_ghosts(p, dtype, y)
    dev_x, src = torch.from_numpy(img_x).cuda(), torch.from_numpy(img_y).cuda()
    failures = []
    contents = [((3.0, -1.5), 2.0), ((-5.0, 0.25), 8.0)]
    co = Coefs(nc, [contents[0][0]], [(contents[0][1], 0.0)], [(0.5, 2.0)], None, 1.0, -1.0)
    field, eager = src.clone(), src.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())

    def call(t, sptr):
        cd.cudecompAmdCombineInterior(axis, h, gd, [t.data_ptr() + SLACK], [dev_x.data_ptr() + SLACK], cd.COMBINE_AXPBY, dtype, halo, padding,
                                      stream=sptr, **co.kwargs())

    with torch.cuda.stream(stream):
        call(field, stream.cuda_stream)  # warm-up
        stream.synchronize()
    if not cd.cudecompExtLastKernelName().startswith("combine_rows_kernel"):
        failures.append("kernel %s" % cd.cudecompExtLastKernelName())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        call(field, torch.cuda.current_stream().cuda_stream)
    seen = []
    for it in (0, 1):
        num, den = contents[it]
        new_num = torch.tensor([num[0], num[1] if nc == 2 else NAN], dtype=torch.float64).cuda()
        new_den = torch.tensor([den, NAN], dtype=torch.float64).cuda()
        with torch.cuda.stream(stream):
            co.dev["a_num"].copy_(new_num)  # the contents change on the stream; the pointers, and the graph, stay
            co.dev["a_den"].copy_(new_den)
            field.copy_(src)
            eager.copy_(src)
            graph.replay()
            call(eager, stream.cuda_stream)
            stream.synchronize()
        r, e = field.cpu().numpy(), eager.cpu().numpy()
        seen.append(r)
        a = coefficient_bits(dtype, num, [den], 1.0)
        b = coefficient_bits(dtype, (0.5, 2.0), None, -1.0)
        want = image_after(p, dtype, img_y, combine_reference(dtype, cd.COMBINE_AXPBY, x, y, a, b))
        if not np.array_equal(r, e) or not np.array_equal(r, want):
            failures.append("replay %d: equals eager %s, equals numpy %s" % (it, np.array_equal(r, e), np.array_equal(r, want)))
    if np.array_equal(seen[0], seen[1]):
        failures.append("the two ratios give one result")
    del graph
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """a long run of kernels is enqueued on a stream, then combinations: the calls return while that work is still running (an event
    recorded behind them has not completed), and the cells are right once it has"""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding, dtype = args["halo"], (0, 0, 0), cd.DOUBLE
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo, padding)
    shape = interior_shape(p, 1)
    x = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), 1, 3).reshape(shape))
    y = bits_from_exact(dtype, integers(int(np.prod(shape[:3])), 1, 4).reshape(shape))
    img_x, _ = pencil_with_nan_ghosts(p, dtype, x)
    img_y, inside = pencil_with_nan_ghosts(p, dtype, y)
    dev_x, src = torch.from_numpy(img_x).cuda(), torch.from_numpy(img_y).cuda()
    dev = src.clone()
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    co = some_coefs(1, 0)
    ops = (cd.COMBINE_AXPY, cd.COMBINE_XPBY, cd.COMBINE_AXPBY)

    def calls():
        for op in ops:
            cd.cudecompAmdCombineInterior(0, h, gd, [dev.data_ptr() + SLACK], [dev_x.data_ptr() + SLACK], op, dtype, halo, padding,
                                          stream=stream.cuda_stream, **co.kwargs())

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
    a, b = co.bits(dtype)
    want_bits = y
    for op in ops:
        want_bits = combine_reference(dtype, op, x, want_bits, a, b)
    failures = [] if np.array_equal(dev.cpu().numpy(), image_after(p, dtype, img_y, want_bits)) else ["the cells differ from numpy's"]
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": failures, "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3, "host_ms": (t2 - t1) * 1e3,
            "total_ms": (t3 - t0) * 1e3}
