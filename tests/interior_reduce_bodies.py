"""Bodies of tests/test_gpu_interior_reduce.py: every function runs on a rank launched by tests/mp.py (the pytest process never
opens the GPU) and returns a list of failure strings, or a dict that holds one.

The reference is numpy on INTEGER data wherever a test asks for bit-exact results: integers in [-8, 8] are exact in all seven
element types, every product and every partial sum of them is exact in fp64, so the result does not depend on the order of the
additions and must equal numpy's integer sum, converted to fp64, bit for bit."""
import itertools
import math

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB

SLACK = 64      # bytes of poison on either side of every test buffer
POISON = 0xFF   # every 2-, 4- and 8-byte real made of these bytes is a NaN
ARITH = {cd.HALF: "_Float16", cd.HALF_COMPLEX: "_Float16", cd.BFLOAT16: "__bf16", cd.FLOAT: "float", cd.FLOAT_COMPLEX: "float",
         cd.DOUBLE: "double", cd.DOUBLE_COMPLEX: "double"}
OPS = (cd.REDUCE_SUM, cd.REDUCE_DOT, cd.REDUCE_MAX_ABS)
LENGTHS = (1, 2, 3, 7, 8, 9, 17, 33, 130)


# ---- the definition in numpy -----------------------------------------------------------------------------------------------------
def reference(op, a, b=None):
    """(results[2f], results[2f + 1]) as float64 for cells a (and b): arrays of shape (cells, reals per element), integer or float64;
    float64 inputs are summed by numpy in some order -- callers that want bits pass integers"""
    a = np.asarray(a)
    nc = a.shape[1]
    zero = a.dtype.type(0)
    if op == cd.REDUCE_SUM:
        out = [a[:, 0].sum(), a[:, 1].sum() if nc == 2 else zero]
    elif op == cd.REDUCE_DOT:
        b = np.asarray(b)
        if nc == 1:
            out = [(a[:, 0] * b[:, 0]).sum(), zero]
        else:  # conj(a) * b
            out = [(a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).sum(), (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]).sum()]
    else:
        out = [np.abs(a[:, 0]).max() if a.shape[0] else zero, (np.abs(a[:, 1]).max() if a.shape[0] else zero) if nc == 2 else zero]
    return np.array([float(x) for x in out], dtype=np.float64) + 0.0  # (+0.0: an integer zero is +0.0)


def same_bits(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


def integers(cells, nc, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(cells, nc)).astype(np.int64)


def cell_bytes(dtype, values):
    """uint8 (cells, es) of float64 / integer `values` (cells, nc), exact in the type (a NaN: the type's own)"""
    values = np.asarray(values)
    if values.shape[0] == 0:
        return np.empty((0, AB.element_bytes(dtype)), dtype=np.uint8)
    if values.dtype.kind == "f" and np.isnan(values).any():
        return np.ascontiguousarray(values.astype(AB.TYPES[dtype][0])).view(np.uint8).reshape(values.shape[0], -1)
    return AB.to_bytes(values, dtype).reshape(values.shape[0], -1)


def name_of(dtype, op, rows):
    return "%s<%s,%d>" % ("reduce_rows_kernel" if rows else "reduce_elements_kernel", ARITH[dtype], op)


class Scratch:
    """workspace and results of one field on the device, results pre-set to a NaN the call must overwrite"""

    def __init__(self, n_fields=1):
        import torch
        self.torch = torch
        self.n = n_fields
        self.work = torch.full((cd.cudecompAmdReduceInteriorWorkspaceBytes(n_fields),), POISON, dtype=torch.uint8, device="cuda")
        self.results = torch.full((2 * n_fields,), float("nan"), dtype=torch.float64, device="cuda")

    def take(self):
        """the results on the host (synchronises); resets them to NaN"""
        out = self.results.cpu().numpy().copy()
        self.results.fill_(float("nan"))
        return out


# ---- kernel parity through cudecompExtReduce3D ---------------------------------------------------------------------------------
def _box_case(dtype, extent, strides, phase, seed):
    """host image of a poisoned buffer with the box `phase` bytes past SLACK, for a and b, and the integer cells"""
    es = AB.element_bytes(dtype)
    nc = AB.TYPES[dtype][1]
    cells = np.array([i * strides[0] + j * strides[1] + k * strides[2]
                      for k in range(extent[2]) for j in range(extent[1]) for i in range(extent[0])], dtype=np.int64)
    span = (int(cells.max()) + 1) * es if cells.size else 0
    nbytes = 2 * SLACK + phase + span
    ia, ib = integers(cells.size, nc, seed), integers(cells.size, nc, seed + 1)
    images = []
    for vals in (ia, ib):
        img = np.full(nbytes, POISON, dtype=np.uint8)
        body = img[SLACK + phase:SLACK + phase + span].reshape(-1, es)
        body[cells] = cell_bytes(dtype, vals)
        images.append(img)
    return images, ia, ib, span


def kernel_parity(rank, nranks, args):
    """the sweep of tests/test_interior_reduce_plan.py on the device, for one data type: every row length, pitch and phase of the
    16-byte grid, three operations, both kernels; the box inside NaN poison; results bit for bit, and the kernel's name"""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    dtype = args["dtype"]
    rs, es, nc = AB.real_bytes(dtype), AB.element_bytes(dtype), AB.TYPES[dtype][1]
    stream = torch.cuda.current_stream().cuda_stream
    sc = Scratch()
    failures, n = [], 0
    for length, extra, (rows, planes) in itertools.product(LENGTHS, (0, 3), ((1, 1), (3, 2), (5, 1))):
        pitch = length + extra
        extent, strides = (length, rows, planes), (1, pitch, pitch * rows + 5)
        for phase in range(0, 16, rs):
            (img_a, img_b), ia, ib, span = _box_case(dtype, extent, strides, phase, n)
            da, db = torch.from_numpy(img_a).cuda(), torch.from_numpy(img_b).cuda()
            if da.data_ptr() % 16 or db.data_ptr() % 16:
                return ["device buffers are not 16-byte aligned"]
            pa, pb = da.data_ptr() + SLACK + phase, db.data_ptr() + SLACK + phase
            # both kernels with nothing readable around the box and with 16 bytes (the poison allows 64): with nothing, the row
            # kernel reads the first and the last vector of a box off the 16-byte grid real by real, for a and for b.  Non-temporal
            # loads (force bit 1) on two of the lengths.
            forces = (0, 1, 2, 3) if length in (7, 130) else (0, 1)
            for op, force, readable in itertools.product(OPS, forces, (0, 16)):
                n += 1
                cls = cd.cudecompExtReduce3D(pa, pb if op == cd.REDUCE_DOT else None, dtype, op, extent, strides, readable, readable,
                                             sc.work.data_ptr(), sc.results.data_ptr(), force, stream)
                name = cd.cudecompExtLastKernelName()
                got, want = sc.take(), reference(op, ia, ib)
                rows_kernel = not (force & 1) and not (op == cd.REDUCE_DOT and nc == 2 and pa % es)
                what = "%s op %d force %d extent %s strides %s phase %d readable %d" % (AB.NAMES[dtype], op, force, extent, strides,
                                                                                       phase, readable)
                if not same_bits(got, want):
                    failures.append("%s: got %s want %s (%s)" % (what, got.tolist(), want.tolist(), name))
                if name != name_of(dtype, op, rows_kernel) or cls != (0 if rows_kernel else 2):
                    failures.append("%s: kernel %s class %d" % (what, name, cls))
            if not (np.array_equal(da.cpu().numpy(), img_a) and np.array_equal(db.cpu().numpy(), img_b)):
                failures.append("%s %s: a field was written" % (AB.NAMES[dtype], extent))
        if len(failures) > 20:
            break
    return failures[:20]


def workgroups_and_partials(rank, nranks, args):
    """more row tiles than the cap on workgroups (the stride loop takes a second pass), more partials than stage two has lanes, a
    long single row that is cut, and rows of 2^k bytes on and off the 16-byte grid (one slot more than whole tile columns, so
    more than one column); integer data inside NaN, bit for bit, both kernels"""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    stream = torch.cuda.current_stream().cuda_stream
    sc = Scratch()
    failures = []
    for dtype, extent, strides, first, blocks in ((cd.DOUBLE, (256, 4, 2049), (1, 258, 258 * 6), 0, cd.REDUCE_MAX_BLOCKS),
                                                  (cd.FLOAT_COMPLEX, (256, 4, 257), (1, 258, 258 * 6), 0, 257),
                                                  (cd.HALF, (1 << 20, 1, 1), (1, 1 << 20, 1 << 20), 0, 129),
                                                  (cd.DOUBLE, (300, 300, 1), (1, 300, 90000), 0, 45),
                                                  (cd.DOUBLE, (512, 9, 3), (1, 514, 514 * 11), 515, 18),
                                                  (cd.DOUBLE, (512, 9, 3), (1, 514, 514 * 11), 516, 18),
                                                  (cd.FLOAT, (1024, 5, 2), (1, 1027, 1027 * 6), 3, 8),
                                                  (cd.HALF_COMPLEX, (2048, 6, 1), (1, 2050, 2050 * 6), 1, 6)):
        nc, real = AB.TYPES[dtype][1], AB.TYPES[dtype][0]
        rng = np.random.default_rng(extent[2] + first)
        k, j, i = np.meshgrid(np.arange(extent[2]), np.arange(extent[1]), np.arange(extent[0]), indexing="ij")
        cells = (first + i * strides[0] + j * strides[1] + k * strides[2]).reshape(-1)
        ia, ib = (rng.integers(-8, 9, size=(cells.size, nc)) for _ in range(2))
        devs = []
        for vals in (ia, ib):
            full = np.full((int(cells.max()) + 1, nc), np.nan)  # NaN before the box and between its rows
            full[cells] = vals
            devs.append(torch.from_numpy(full.astype(real).reshape(-1).view(np.uint8)).cuda())
        es = AB.element_bytes(dtype)
        pa, pb = devs[0].data_ptr() + first * es, devs[1].data_ptr() + first * es
        d = cd.cudecompExtDescribeReduce3D(pa, pb, dtype, cd.REDUCE_DOT, extent, strides, first * es, 0)
        if d["blocks"] != blocks:
            failures.append("%s: %d workgroups, expected %d" % (extent, d["blocks"], blocks))
        for op, force in itertools.product(OPS, (0, 1)):
            cd.cudecompExtReduce3D(pa, pb, dtype, op, extent, strides, first * es, 0, sc.work.data_ptr(), sc.results.data_ptr(), force,
                                   stream)
            name = cd.cudecompExtLastKernelName()
            got, want = sc.take(), reference(op, ia, ib)
            if not same_bits(got, want) or name != name_of(dtype, op, not force):
                failures.append("%s %s first %d op %d force %d: got %s want %s (%s)" % (AB.NAMES[dtype], extent, first, op, force,
                                                                                       got.tolist(), want.tolist(), name))
    return failures


# ---- pencils -------------------------------------------------------------------------------------------------------------------
def interior_index(p):
    """index of the interior in AB.pencil3's view (numpy axis 2 - k is memory position k)"""
    idx = [None] * 3
    for k in range(3):
        ga = int(p.order[k])
        idx[2 - k] = slice(int(p.halo_extents[ga]), int(p.shape[k]) - int(p.halo_extents[ga]) - int(p.padding[ga]))
    return tuple(idx)


def pencil_image(p, dtype, interior_values, ghost_bytes):
    """uint8 image of a pencil with SLACK bytes of poison on either side: `ghost_bytes` (one element) in every ghost and padding cell,
    `interior_values` (shape of the interior + (nc,)) in the interior"""
    es = AB.element_bytes(dtype)
    cells = np.empty((int(p.size), es), dtype=np.uint8)
    cells[:] = np.frombuffer(bytes(ghost_bytes), dtype=np.uint8)
    view = AB.pencil3(p, cells)
    inner = view[interior_index(p)]
    inner[...] = cell_bytes(dtype, interior_values.reshape(-1, interior_values.shape[-1])).reshape(inner.shape)
    img = np.full(2 * SLACK + cells.size, POISON, dtype=np.uint8)
    img[SLACK:SLACK + cells.size] = cells.reshape(-1)
    return img


def interior_shape(p, nc):
    return tuple(max(s.stop - s.start, 0) for s in interior_index(p)) + (nc,)


def _reduce(axis, h, gd, ptrs_a, ptrs_b, op, sc, dtype, halo, padding, stream):
    cd.cudecompAmdReduceInterior(axis, h, gd, ptrs_a, ptrs_b if op == cd.REDUCE_DOT else None, op, sc.results.data_ptr(),
                                 sc.work.data_ptr(), dtype, halo, padding, stream)
    return sc.take()


def ghost_independence(rank, nranks, args):
    """ghosts and padding as zeros, as 0xFF bytes and as infinities: the results are bit-identical and numpy's over the interior"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    sc = Scratch()
    failures = []
    for dtype, axis in itertools.product(AB.ALL_TYPES, range(3)):
        es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p, nc)
        ia, ib = integers(int(np.prod(shape[:3])), nc, dtype + 10).reshape(shape), integers(int(np.prod(shape[:3])), nc, dtype + 50).reshape(shape)
        ghosts = (bytes(es), bytes([POISON]) * es, bytes(AB.to_bytes(np.full(nc, np.inf), dtype)))
        for op in OPS:
            seen = []
            for ghost in ghosts:
                da = torch.from_numpy(pencil_image(p, dtype, ia, ghost)).cuda()
                db = torch.from_numpy(pencil_image(p, dtype, ib, ghost)).cuda()
                seen.append(_reduce(axis, h, gd, [da.data_ptr() + SLACK], [db.data_ptr() + SLACK], op, sc, dtype, halo, padding, stream))
            want = reference(op, ia.reshape(-1, nc), ib.reshape(-1, nc))
            if not all(same_bits(s, want) for s in seen):
                failures.append("%s axis %d op %d: %s want %s" % (AB.NAMES[dtype], axis, op, [s.tolist() for s in seen], want.tolist()))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def single_rank_sweep(rank, nranks, args):
    """shapes x memory orders x axes x halos x paddings, the seven types in turn, three operations; integer data, bit for bit"""
    import torch
    from tests import gpu_bodies as B
    stream = torch.cuda.current_stream().cuda_stream
    sc = Scratch()
    failures, n = [], 0
    for gdims, order in itertools.product(args["shapes"], itertools.permutations(range(3))):
        h, gd, g = B._setup(rank, nranks, {"gdims": gdims, "pdims": (1, 1), "mem_order": (order,) * 3})
        for axis, halo, padding in itertools.product(range(3), args["halos"], args["paddings"]):
            dtype = AB.ALL_TYPES[n % 7]
            n += 1
            nc = AB.TYPES[dtype][1]
            p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
            shape = interior_shape(p, nc)
            ia, ib = integers(int(np.prod(shape[:3])), nc, n).reshape(shape), integers(int(np.prod(shape[:3])), nc, n + 1000).reshape(shape)
            ghost = bytes([POISON]) * AB.element_bytes(dtype)
            da = torch.from_numpy(pencil_image(p, dtype, ia, ghost)).cuda()
            db = torch.from_numpy(pencil_image(p, dtype, ib, ghost)).cuda()
            for op in OPS:
                got = _reduce(axis, h, gd, [da.data_ptr() + SLACK], [db.data_ptr() + SLACK], op, sc, dtype, halo, padding, stream)
                want = reference(op, ia.reshape(-1, nc), ib.reshape(-1, nc))
                if not same_bits(got, want):
                    failures.append("gdims %s order %s axis %d halo %s padding %s %s op %d: got %s want %s (%s)" % (
                        gdims, order, axis, halo, padding, AB.NAMES[dtype], op, got.tolist(), want.tolist(), cd.cudecompExtLastKernelName()))
        cd.cudecompGridDescDestroy(h, gd)
    return failures[:20]


def _random_reals(shape, seed, real):
    """finite reals with exponents over 2^-30 .. 2^30, both signs, exact in `real`"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(1.0, 2.0, size=shape) * np.exp2(rng.integers(-30, 31, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(real).astype(np.float64)


def multi_field(rank, nranks, args):
    """1, 2, 5 and 32 fields with distinct data of any magnitude: every field's pair is bit-identical to its single-field call"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    one, failures = Scratch(1), []
    for dtype, axis in ((cd.FLOAT, 0), (cd.DOUBLE_COMPLEX, 1), (cd.HALF, 2), (cd.DOUBLE, 0)):
        nc, real = AB.TYPES[dtype][1], AB.TYPES[dtype][0]
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p, nc)
        fields = []
        for f in range(32):
            vals = _random_reals(shape, 100 * (dtype + 10) + f, real) if dtype != cd.HALF else integers(int(np.prod(shape[:3])), nc, f).reshape(shape) / 4.0
            fields.append(torch.from_numpy(pencil_image(p, dtype, vals, bytes([POISON]) * AB.element_bytes(dtype))).cuda())
        ptrs = [t.data_ptr() + SLACK for t in fields]
        if any(q % 16 for q in ptrs):
            return ["fields are not 16-byte aligned"]
        for op, same in itertools.product(OPS, (False, True)):
            if same and op != cd.REDUCE_DOT:
                continue
            others = ptrs if same else ptrs[1:] + ptrs[:1]  # DOT with a[f] == b[f], and with another field
            single = [_reduce(axis, h, gd, [ptrs[f]], [others[f]], op, one, dtype, halo, padding, stream) for f in range(32)]
            if op == cd.REDUCE_DOT and same and not all(s[0] > 0 for s in single):
                failures.append("%s: a squared norm that is not positive" % AB.NAMES[dtype])
            for n in (1, 2, 5, 32):
                sc = Scratch(n)
                got = _reduce(axis, h, gd, ptrs[:n], others[:n], op, sc, dtype, halo, padding, stream)
                if not same_bits(got, np.concatenate(single[:n])):
                    failures.append("%s op %d same %s, %d fields: %s, alone %s" % (AB.NAMES[dtype], op, same, n, got.tolist(),
                                                                                 np.concatenate(single[:n]).tolist()))
            if op != cd.REDUCE_MAX_ABS and len({s.tobytes() for s in single}) < 2:  # (small integers share their largest magnitude, and some their sums)
                failures.append("%s op %d: the fields do not differ" % (AB.NAMES[dtype], op))
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:20]


def accuracy(rank, nranks, args):
    """random fp64 and fp32 data with exponents over 2^+-30, about 10^5 cells: SUM and DOT against the exactly rounded sum of the
    exact terms (math.fsum; the fp64 products through fractions), held to n * 2^-53 * sum |term|; three runs, bit-identical"""
    from fractions import Fraction

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], (0, 0, 0)
    stream = torch.cuda.current_stream().cuda_stream
    sc, failures, figures = Scratch(), [], []
    for dtype in (cd.DOUBLE, cd.FLOAT):
        real = AB.TYPES[dtype][0]
        p = cd.cudecompGetPencilInfo(h, gd, 0, halo, padding)
        shape = interior_shape(p, 1)
        n = int(np.prod(shape))
        a, b = _random_reals(shape, 1, real), _random_reals(shape, 2, real)
        ghost = bytes([POISON]) * AB.element_bytes(dtype)
        da, db = torch.from_numpy(pencil_image(p, dtype, a, ghost)).cuda(), torch.from_numpy(pencil_image(p, dtype, b, ghost)).cuda()
        for op in (cd.REDUCE_SUM, cd.REDUCE_DOT):
            if op == cd.REDUCE_SUM:
                exact = Fraction(math.fsum(a.reshape(-1)))  # (exactly rounded: within 2^-53 of the true sum, relative)
                scale = math.fsum(np.abs(a).reshape(-1))
            elif dtype == cd.FLOAT:  # products of fp32 reals are exact in fp64
                exact = Fraction(math.fsum((a * b).reshape(-1)))
                scale = math.fsum(np.abs(a * b).reshape(-1))
            else:
                terms = [Fraction(x) * Fraction(y) for x, y in zip(a.reshape(-1).tolist(), b.reshape(-1).tolist())]
                exact = sum(terms, Fraction(0))
                scale = float(sum((abs(t) for t in terms), Fraction(0)))
            runs = [_reduce(0, h, gd, [da.data_ptr() + SLACK], [db.data_ptr() + SLACK], op, sc, dtype, halo, padding, stream) for _ in range(3)]
            err, bound = abs(Fraction(float(runs[0][0])) - exact), Fraction(n) * Fraction(1, 2 ** 53) * Fraction(scale)
            figures.append("%s op %d: n %d error %.3e bound %.3e" % (AB.NAMES[dtype], op, n, float(err), float(bound)))
            print(figures[-1])
            if not (err <= bound) or runs[0][1] != 0.0:
                failures.append(figures[-1] + " got %s" % runs[0].tolist())
            if not (same_bits(runs[0], runs[1]) and same_bits(runs[0], runs[2])):
                failures.append("%s op %d: three runs differ: %s" % (AB.NAMES[dtype], op, [r.tolist() for r in runs]))
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": failures, "figures": figures}


def edge_values(rank, nranks, args):
    """MAX_ABS with -0, subnormals, the largest finite value, +-inf and a NaN in one interior cell; SUM of +inf and -inf"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    sc, failures = Scratch(), []
    for dtype in (cd.DOUBLE, cd.FLOAT, cd.HALF, cd.DOUBLE_COMPLEX):
        nc, real = AB.TYPES[dtype][1], AB.TYPES[dtype][0]
        info = np.finfo(real)
        tiny, huge = float(info.smallest_subnormal), float(info.max)
        p = cd.cudecompGetPencilInfo(h, gd, 0, halo, padding)
        shape = interior_shape(p, nc)
        cells = int(np.prod(shape[:3]))
        ghost = bytes([POISON]) * AB.element_bytes(dtype)

        def run(op, special, where=7):
            vals = np.zeros(shape)
            flat = vals.reshape(-1, nc)
            flat[:, 0] = -0.0
            for i, x in enumerate(special):
                flat[(where + 37 * i) % cells, 0] = x
            if nc == 2:
                flat[:, 1] = 0.25
            d = torch.from_numpy(pencil_image(p, dtype, vals, ghost)).cuda()
            return _reduce(0, h, gd, [d.data_ptr() + SLACK], None, op, sc, dtype, halo, padding, stream)

        im = 0.25 if nc == 2 else 0.0
        for special, want in (((), 0.0), ((-tiny,), tiny), ((tiny, -huge), huge), ((huge, -np.inf), np.inf), ((np.inf, 1.0), np.inf)):
            got = run(cd.REDUCE_MAX_ABS, special)
            if not same_bits(got, [want, im]):
                failures.append("%s max-abs of %s: %s" % (AB.NAMES[dtype], special, got.tolist()))
        for where in (0, 7, cells - 1):  # the NaN in the first, some and the last interior cell
            got = run(cd.REDUCE_MAX_ABS, (np.nan, np.inf), where)
            if not (np.isnan(got[0]) and same_bits(got[1:], [im])):
                failures.append("%s max-abs with a NaN at %d: %s" % (AB.NAMES[dtype], where, got.tolist()))
        got = run(cd.REDUCE_SUM, (np.inf, -np.inf, 1.0))
        if not (np.isnan(got[0]) and same_bits(got[1:], [im * cells])):
            failures.append("%s sum of +inf and -inf: %s" % (AB.NAMES[dtype], got.tolist()))
        got = run(cd.REDUCE_SUM, (np.inf, 1.0))
        if not same_bits(got, [np.inf, im * cells]):
            failures.append("%s sum with +inf: %s" % (AB.NAMES[dtype], got.tolist()))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


# ---- several ranks -------------------------------------------------------------------------------------------------------------
def closed_form(gdims):
    """integer field of the global index, numpy axes (z, y, x): values in [-8, 8]"""
    z, y, x = np.meshgrid(np.arange(gdims[2]), np.arange(gdims[1]), np.arange(gdims[0]), indexing="ij")
    return (3 * x + 5 * y + 7 * z) % 17 - 8, (x * y + 2 * z) % 17 - 8


def rank_slab(p, world):
    """this rank's interior of a global array with numpy axes (z, y, x), in the layout of AB.pencil3's interior"""
    sl = [None] * 3
    for k in range(3):
        sl[2 - int(p.order[k])] = slice(int(p.lo[k]), int(p.hi[k]) + 1)
    slab = world[tuple(sl)]  # axes (z, y, x) -> numpy axis 2 - k is memory position k
    return np.ascontiguousarray(np.transpose(slab, [2 - int(p.order[2 - i]) for i in range(3)]))


def ranks_sweep(rank, nranks, args):
    """every rank reduces its slab of a closed form of the global index: [failures, {case: results}]; also serves the grid on which a
    rank owns nothing (its results are zeros, and written)"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    stream = torch.cuda.current_stream().cuda_stream
    sc, failures, mine = Scratch(2), [], {}
    wa, wb = closed_form(args["gdims"])
    n = 0
    for axis, halo in itertools.product(range(3), args["halos"]):
        dtype = AB.ALL_TYPES[n % 7] if not args.get("dtype") else args["dtype"]
        n += 1
        nc = AB.TYPES[dtype][1]
        padding = (0, 1, 0)
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        if g.pencil_info(rank, axis, halo, padding).as_dict() != p.as_dict():
            failures.append("rank %d axis %d: pencil info differs from the oracle" % (rank, axis))
            continue
        sa, sb = rank_slab(p, wa), rank_slab(p, wb)
        shape = interior_shape(p, nc)
        if sa.shape != shape[:3]:
            failures.append("rank %d axis %d halo %s: slab %s, interior %s" % (rank, axis, halo, sa.shape, shape))
            continue
        ia, ib = np.stack([sa, sb][:nc] if nc == 2 else [sa], axis=-1), np.stack([sb, sa][:nc] if nc == 2 else [sb], axis=-1)
        ghost = bytes([POISON]) * AB.element_bytes(dtype)
        fa = [torch.from_numpy(pencil_image(p, dtype, v, ghost)).cuda() for v in (ia, ib)]
        ptrs = [t.data_ptr() + SLACK for t in fa]
        for op in OPS:
            got = _reduce(axis, h, gd, ptrs, ptrs[::-1], op, sc, dtype, halo, padding, stream)  # two fields: (a, b) and (b, a)
            want = np.concatenate([reference(op, ia.reshape(-1, nc), ib.reshape(-1, nc)), reference(op, ib.reshape(-1, nc), ia.reshape(-1, nc))])
            if not same_bits(got, want):
                failures.append("rank %d axis %d halo %s %s op %d: got %s want %s" % (rank, axis, halo, AB.NAMES[dtype], op, got.tolist(),
                                                                                     want.tolist()))
            mine["%d %s %d" % (axis, tuple(halo), op)] = [got.tolist(), dtype, int(np.prod(shape[:3]))]
    cd.cudecompGridDescDestroy(h, gd)
    return [failures, mine]


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def graph_replay(rank, nranks, args):
    """one call captured, replayed, the field changed, replayed again: each replay bit-identical to an eager call on the same data"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    axis, dtype, op = args.get("axis", 0), args.get("dtype", cd.DOUBLE), args.get("op", cd.REDUCE_DOT)
    halo, padding = args["halo"], args.get("padding", (0, 0, 0))
    nc, real = AB.TYPES[dtype][1], AB.TYPES[dtype][0]
    p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
    shape = interior_shape(p, nc)
    ghost = bytes([POISON]) * AB.element_bytes(dtype)
    images = [torch.from_numpy(pencil_image(p, dtype, _random_reals(shape, s, real), ghost)).cuda() for s in (1, 2, 3)]
    field, other = images[0].clone(), images[2]
    eager_sc, graph_sc = Scratch(), Scratch()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    failures = []

    def call(sc, sptr):
        cd.cudecompAmdReduceInterior(axis, h, gd, [field.data_ptr() + SLACK], [other.data_ptr() + SLACK], op, sc.results.data_ptr(),
                                     sc.work.data_ptr(), dtype, halo, padding, sptr)

    with torch.cuda.stream(stream):
        call(graph_sc, stream.cuda_stream)  # warm-up
        stream.synchronize()
        graph_sc.take()
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        call(graph_sc, torch.cuda.current_stream().cuda_stream)
    seen = []
    for it in (0, 1):
        with torch.cuda.stream(stream):
            field.copy_(images[it])  # the contents change on the stream; the pointers, and the graph, stay
            graph.replay()
            stream.synchronize()
            replayed = graph_sc.take()
            call(eager_sc, stream.cuda_stream)
            stream.synchronize()
            eager = eager_sc.take()
        seen.append(replayed)
        if np.isnan(replayed).any() or not same_bits(replayed, eager):
            failures.append("replay %d: %s, eager %s" % (it, replayed.tolist(), eager.tolist()))
    if same_bits(seen[0], seen[1]):
        failures.append("the two contents give one result")
    del graph
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """a long run of kernels is enqueued on a stream, then reductions: the calls return while that work is still running (an event
    recorded behind them has not completed), and the results are right once it has"""
    import time

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding, dtype = args["halo"], (0, 0, 0), cd.DOUBLE
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo, padding)
    shape = interior_shape(p, 1)
    ia = integers(int(np.prod(shape[:3])), 1, 3).reshape(shape)
    dev = torch.from_numpy(pencil_image(p, dtype, ia, bytes([POISON]) * 8)).cuda()
    sc = Scratch()
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def calls():
        for op in OPS:
            cd.cudecompAmdReduceInterior(0, h, gd, [dev.data_ptr() + SLACK], [dev.data_ptr() + SLACK], op, sc.results.data_ptr(),
                                         sc.work.data_ptr(), dtype, halo, padding, stream.cuda_stream)

    calls()  # warm-up: first-use work happens before the timed part
    torch.cuda.synchronize()
    sc.take()
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
    got, want = sc.take(), reference(cd.REDUCE_MAX_ABS, ia.reshape(-1, 1))
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": [] if same_bits(got, want) else ["got %s want %s" % (got.tolist(), want.tolist())],
            "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3, "host_ms": (t2 - t1) * 1e3, "total_ms": (t3 - t0) * 1e3}
