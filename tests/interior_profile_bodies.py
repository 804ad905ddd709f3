"""Bodies of tests/test_gpu_interior_profile.py: every function runs on a rank launched by tests/mp.py (the pytest process never
opens the GPU) and returns a list of failure strings, or a dict that holds one.

The reference is tests/interior_reduce_bodies.py's `reference`, applied plane by plane: numpy on INTEGER data in [-8, 8] wherever a
test asks for bit-exact results (exact in all seven element types and in any order of the additions)."""
import itertools
import math

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests.interior_reduce_bodies import (ARITH, LENGTHS, OPS, POISON, SLACK, Scratch, _random_reals, cell_bytes, closed_form, integers,
                                          interior_shape, pencil_image, rank_slab, reference, same_bits)

FORMS = ("profile_rows_kernel", "profile_columns_kernel", "profile_elements_kernel")


# ---- the definition in numpy -----------------------------------------------------------------------------------------------------
def profile_reference(op, a, b, axis):
    """(L, 2) float64: interior_reduce_bodies.reference over every plane of a (and b), arrays of shape (e2, e1, e0, nc), kept along
    numpy axis `axis`; the same definitions, vectorised over the planes"""
    nc = a.shape[-1]
    a = np.moveaxis(a, axis, 0).reshape(a.shape[axis], -1, nc)
    b = None if b is None else np.moveaxis(b, axis, 0).reshape(a.shape[0], -1, nc)
    out = np.zeros((a.shape[0], 2), dtype=np.float64)
    if a.shape[1] == 0:
        return out
    if op == cd.REDUCE_SUM:
        out[:, :nc] = a.sum(axis=1)
    elif op == cd.REDUCE_DOT and nc == 1:
        out[:, 0] = (a[:, :, 0] * b[:, :, 0]).sum(axis=1)
    elif op == cd.REDUCE_DOT:  # conj(a) * b
        out[:, 0] = (a[:, :, 0] * b[:, :, 0] + a[:, :, 1] * b[:, :, 1]).sum(axis=1)
        out[:, 1] = (a[:, :, 0] * b[:, :, 1] - a[:, :, 1] * b[:, :, 0]).sum(axis=1)
    else:
        out[:, :nc] = np.abs(a).max(axis=1)
    return out + 0.0  # (an integer zero is +0.0)


def name_of(dtype, op, form):
    return "%s<%s,%d>" % (FORMS[form], ARITH[dtype], op)


def pitches(length, es):
    """the row pitches of the parity sweep, in elements: the row itself, + 3 elements (off the 16-byte grid unless an element is 16
    bytes), and the next multiple of 16 bytes beyond the row"""
    per = 16 // math.gcd(16, es)
    return (length, length + 3, (length // per + 1) * per)


def expected_form(dtype, op, keep, extent, strides, address, force):
    """planProfile's rules: 0 rows, 1 columns, 2 element-wise"""
    es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
    if force & 1 or (op == cd.REDUCE_DOT and nc == 2 and address % es):
        return 2
    c = None  # the contiguous dim: of stride 1, and of several such the one longer than a cell
    for d in range(3):
        if strides[d] == 1 and (c is None or (extent[c] == 1 and extent[d] > 1)):
            c = d
    if keep != c:
        return 0
    others = [d for d in range(3) if d != keep and extent[d] > 1]
    return 1 if all((strides[d] * es) % 16 == 0 for d in others) else 2


class Results:
    """a device array of pairs pre-set to NaN, handed out slice by slice; one copy to the host serves many calls"""

    def __init__(self, pairs):
        import torch
        self.buf = torch.full((2 * pairs,), float("nan"), dtype=torch.float64, device="cuda")
        self.used = 0

    def take(self, pairs):
        at = self.used
        self.used += pairs
        assert 2 * self.used <= self.buf.numel()
        return self.buf.data_ptr() + 16 * at, at

    def host(self):
        """(pairs, 2) on the host (synchronises); the device array is NaN again, and empty"""
        out = self.buf.cpu().numpy().copy().reshape(-1, 2)
        self.buf.fill_(float("nan"))
        self.used = 0
        return out


def _workspace(n_fields, length):
    import torch
    return torch.full((cd.cudecompAmdProfileInteriorWorkspaceBytes(n_fields, length),), POISON, dtype=torch.uint8, device="cuda")


def _box_arrays(dtype, extent, strides, first, seed):
    """integer cells (e2, e1, e0, nc) of a and b and their device buffers: the box `first` elements into a buffer of NaN reals"""
    import torch
    nc, real = AB.TYPES[dtype][1], AB.TYPES[dtype][0]
    rng = np.random.default_rng(seed)
    k, j, i = np.meshgrid(np.arange(extent[2]), np.arange(extent[1]), np.arange(extent[0]), indexing="ij")
    cells = (first + i * strides[0] + j * strides[1] + k * strides[2]).reshape(-1)
    shape = (extent[2], extent[1], extent[0], nc)
    ia, ib = (rng.integers(-8, 9, size=shape) for _ in range(2))
    devs = []
    for vals in (ia, ib):
        full = np.full((int(cells.max()) + 1, nc), np.nan)  # NaN before the box and between its rows
        full[cells] = vals.reshape(-1, nc)
        devs.append(torch.from_numpy(full.astype(real).reshape(-1).view(np.uint8)).cuda())
    return ia, ib, devs


# ---- kernel parity through cudecompExtProfile3D --------------------------------------------------------------------------------
def kernel_parity(rank, nranks, args):
    """for one data type: every row length, three pitches, every phase of the 16-byte grid, the kept dim at each of the three
    positions, three operations, the fast form and the forced element form, nothing and 16 bytes readable around the box,
    non-temporal loads on two lengths; the box inside NaN poison; every pair bit for bit, the kernel's name and class, the fields
    unwritten"""
    import torch
    from tests import gpu_bodies as B
    from tests.interior_reduce_bodies import _box_case
    B._handle(rank)
    dtype = args["dtype"]
    rs, es = AB.real_bytes(dtype), AB.element_bytes(dtype)
    stream = torch.cuda.current_stream().cuda_stream
    work, res = _workspace(1, max(LENGTHS)), Results(3 * 3 * 4 * 2 * max(LENGTHS))
    failures, n, seen = [], 0, set()
    for length, (rows, planes) in itertools.product(LENGTHS, ((1, 1), (3, 2), (5, 1))):
        for which, pitch in enumerate(pitches(length, es)):
            # the pitch of whole 16 bytes keeps the planes on the grid too; the other two put them 5 elements off
            extent, strides = (length, rows, planes), (1, pitch, pitch * (rows + 1) if which == 2 else pitch * rows + 5)
            for phase in range(0, 16, rs):
                (img_a, img_b), ia, ib, span = _box_case(dtype, extent, strides, phase, n)
                shape = (planes, rows, length, ia.shape[1])
                ia, ib = ia.reshape(shape), ib.reshape(shape)
                da, db = torch.from_numpy(img_a).cuda(), torch.from_numpy(img_b).cuda()
                if da.data_ptr() % 16 or db.data_ptr() % 16:
                    return ["device buffers are not 16-byte aligned"]
                pa, pb = da.data_ptr() + SLACK + phase, db.data_ptr() + SLACK + phase
                forces = (0, 1, 2, 3) if length in (7, 130) else (0, 1)
                calls = []
                for keep, op, force, readable in itertools.product(range(3), OPS, forces, (0, 16)):
                    n += 1
                    ptr, at = res.take(extent[keep])
                    cls = cd.cudecompExtProfile3D(pa, pb if op == cd.REDUCE_DOT else None, dtype, op, keep, extent, strides, readable,
                                                  readable, work.data_ptr(), ptr, extent[keep], force, stream)
                    name = cd.cudecompExtLastKernelName()
                    form = expected_form(dtype, op, keep, extent, strides, pa, force)
                    seen.add(form)
                    what = "%s op %d keep %d force %d extent %s strides %s phase %d readable %d" % (
                        AB.NAMES[dtype], op, keep, force, extent, strides, phase, readable)
                    if name != name_of(dtype, op, form) or cls != (2 if form == 2 else 0):
                        failures.append("%s: kernel %s class %d, expected %s" % (what, name, cls, name_of(dtype, op, form)))
                    calls.append((at, keep, op, what, name))
                got = res.host()
                wants = {(keep, op): profile_reference(op, ia, ib, 2 - keep) for keep in range(3) for op in OPS}
                for at, keep, op, what, name in calls:
                    want = wants[keep, op]
                    if not same_bits(got[at:at + extent[keep]], want):
                        failures.append("%s: got %s want %s (%s)" % (what, got[at:at + extent[keep]].tolist(), want.tolist(), name))
                if not (np.array_equal(da.cpu().numpy(), img_a) and np.array_equal(db.cpu().numpy(), img_b)):
                    failures.append("%s %s: a field was written" % (AB.NAMES[dtype], extent))
            if len(failures) > 20:
                return failures[:20]
    if seen != {0, 1, 2}:
        failures.append("forms seen: %s" % sorted(seen))
    return failures[:20]


def sizes(rank, nranks, args):
    """more entries than workgroups in flight, more parts per entry than the final stage has lanes per entry, a kept extent of 1
    against the scalar reduction, rows of 2^k bytes on and off the 16-byte grid; integer data inside NaN, bit for bit, fast and
    element form; and ld > L: the pairs beyond L keep their NaN"""
    import torch
    from tests import gpu_bodies as B
    B._handle(rank)
    stream = torch.cuda.current_stream().cuda_stream
    scalar = Scratch()
    failures = []
    cases = ((cd.DOUBLE, (64, 3, 2049), (1, 66, 66 * 3 + 2), 0, 2, None),       # more entries than workgroups in flight
             (cd.FLOAT, (2049, 3, 5), (1, 2052, 2052 * 4), 0, 0, None),         # columns: many tile columns
             (cd.DOUBLE, (2, 600, 200), (1, 2, 1200), 0, 0, True),               # columns: more parts than the final stage has lanes
             (cd.FLOAT_COMPLEX, (4, 20000, 1), (1, 6, 6 * 20000), 0, 2, True),   # rows: kept extent 1, more parts than lanes
             (cd.DOUBLE, (300, 300, 1), (1, 300, 90000), 0, 2, True),           # kept extent 1
             (cd.HALF, (1, 70, 300), (1, 8, 560), 0, 0, None),                   # columns, kept extent 1: one real of every row
             (cd.DOUBLE, (512, 9, 3), (1, 514, 514 * 11), 515, 1, None), (cd.DOUBLE, (512, 9, 3), (1, 514, 514 * 11), 516, 2, None),
             (cd.DOUBLE, (512, 9, 3), (1, 514, 514 * 10), 516, 0, None), (cd.FLOAT, (1024, 5, 2), (1, 1028, 1028 * 6), 3, 0, None),
             (cd.FLOAT, (1024, 5, 2), (1, 1027, 1027 * 6), 3, 1, None), (cd.HALF_COMPLEX, (2048, 6, 1), (1, 2052, 2052 * 6), 1, 0, None))
    for dtype, extent, strides, first, keep, parts in cases:
        es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
        ia, ib, devs = _box_arrays(dtype, extent, strides, first, extent[2] + first)
        pa, pb = devs[0].data_ptr() + first * es, devs[1].data_ptr() + first * es
        L, ld = extent[keep], extent[keep] + 3
        d = cd.cudecompExtDescribeProfile3D(pa, pb, dtype, cd.REDUCE_DOT, keep, extent, strides, first * es, 0)
        if parts and d["parts"] <= d["final_lanes"]:
            failures.append("%s keep %d: %s, expected more parts than the final stage has lanes per entry" % (extent, keep, d))
        work, res = _workspace(1, L), Results(6 * ld)
        calls = []
        for op, force in itertools.product(OPS, (0, 1)):
            ptr, at = res.take(ld)
            cd.cudecompExtProfile3D(pa, pb, dtype, op, keep, extent, strides, first * es, 0, work.data_ptr(), ptr, ld, force, stream)
            name = cd.cudecompExtLastKernelName()
            if name != name_of(dtype, op, expected_form(dtype, op, keep, extent, strides, pa, force)):
                failures.append("%s keep %d op %d force %d: kernel %s" % (extent, keep, op, force, name))
            calls.append((at, op, force, name))
        got = res.host()
        for at, op, force, name in calls:
            want = profile_reference(op, ia, ib, 2 - keep)
            if not same_bits(got[at:at + L], want) or not np.isnan(got[at + L:at + ld]).all():
                bad = np.flatnonzero((got[at:at + L].view(np.uint64) != want.view(np.uint64)).any(axis=1))[:4]
                failures.append("%s %s first %d keep %d op %d force %d: entries %s got %s want %s; beyond L %s (%s)" % (
                    AB.NAMES[dtype], extent, first, keep, op, force, bad.tolist(), got[at:at + L][bad].tolist(), want[bad].tolist(),
                    got[at + L:at + ld].tolist(), name))
            if L == 1 and op != cd.REDUCE_MAX_ABS:  # the sum over k equals the scalar reduction of the box, bit for bit
                cd.cudecompExtReduce3D(pa, pb, dtype, op, extent, strides, first * es, 0, scalar.work.data_ptr(),
                                       scalar.results.data_ptr(), 0, stream)
                whole = scalar.take()
                if not same_bits(got[at:at + L].sum(axis=0) + 0.0, whole):
                    failures.append("%s keep %d op %d: profile %s, scalar reduction %s" % (extent, keep, op, got[at].tolist(), whole.tolist()))
    return failures[:20]


# ---- pencils -------------------------------------------------------------------------------------------------------------------
def _position(p, dim):
    """memory position of global dim `dim` in the pencil"""
    return [int(x) for x in p.order].index(dim)


def _profile(axis, h, gd, ptrs_a, ptrs_b, op, dim, L, dtype, halo, padding, stream, ld=None, work=None):
    """(n_fields, ld, 2) on the host: the call into a NaN array, which it must overwrite up to L and leave alone beyond"""
    n, ld = len(ptrs_a), L if ld is None else ld
    res = Results(max(n * ld, 1))
    work = _workspace(n, L) if work is None else work
    cd.cudecompAmdProfileInterior(axis, h, gd, ptrs_a, ptrs_b if op == cd.REDUCE_DOT else None, op, dim, res.buf.data_ptr(), ld,
                                  work.data_ptr(), dtype, halo, padding, stream)
    return res.host().reshape(n, ld, 2) if n * ld else np.zeros((n, 0, 2))


def ghost_independence(rank, nranks, args):
    """ghosts and padding as zeros and as 0xFF bytes (NaN): the profiles are bit-identical and numpy's over the interior; ld > L and
    two fields: the pairs beyond L and between the fields keep their NaN"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype, axis, dim in itertools.product(AB.ALL_TYPES, range(3), range(3)):
        es, nc = AB.element_bytes(dtype), AB.TYPES[dtype][1]
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p, nc)
        npax = 2 - _position(p, dim)
        L = shape[npax]
        ia, ib = integers(int(np.prod(shape[:3])), nc, dtype + 10).reshape(shape), integers(int(np.prod(shape[:3])), nc, dtype + 50).reshape(shape)
        for op in OPS:
            seen = []
            for ghost in (bytes(es), bytes([POISON]) * es):
                da = torch.from_numpy(pencil_image(p, dtype, ia, ghost)).cuda()
                db = torch.from_numpy(pencil_image(p, dtype, ib, ghost)).cuda()
                pa, pb = da.data_ptr() + SLACK, db.data_ptr() + SLACK
                seen.append(_profile(axis, h, gd, [pa, pb], [pb, pa], op, dim, L, dtype, halo, padding, stream, ld=L + 2))
            want = np.stack([profile_reference(op, ia, ib, npax), profile_reference(op, ib, ia, npax)])
            for s in seen:
                if not same_bits(s[:, :L], want) or not np.isnan(s[:, L:]).all():
                    failures.append("%s axis %d dim %d op %d: %s want %s (%s)" % (AB.NAMES[dtype], axis, dim, op, s.tolist(), want.tolist(),
                                                                                 cd.cudecompExtLastKernelName()))
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:10]


def single_rank_sweep(rank, nranks, args):
    """shapes x memory orders x axes x halos x paddings x dims, the seven types in turn, three operations; integer data, bit for
    bit; and the sum over k of each SUM / DOT profile equals the scalar cudecompAmdReduceInterior result"""
    import torch
    from tests import gpu_bodies as B
    stream = torch.cuda.current_stream().cuda_stream
    sc = Scratch()
    failures, n, names = [], 0, set()
    for gdims, order in itertools.product(args["shapes"], args["orders"]):
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
            pa, pb = [da.data_ptr() + SLACK], [db.data_ptr() + SLACK]
            work = _workspace(1, max(shape[:3]))
            for op, dim in itertools.product(OPS, range(3)):
                npax = 2 - _position(p, dim)
                got = _profile(axis, h, gd, pa, pb, op, dim, shape[npax], dtype, halo, padding, stream, work=work)[0]
                names.add(cd.cudecompExtLastKernelName().split("<")[0])
                want = profile_reference(op, ia, ib, npax)
                what = "gdims %s order %s axis %d halo %s padding %s %s op %d dim %d" % (gdims, order, axis, halo, padding, AB.NAMES[dtype], op, dim)
                if not same_bits(got, want):
                    failures.append("%s: got %s want %s (%s)" % (what, got.tolist(), want.tolist(), cd.cudecompExtLastKernelName()))
                if op != cd.REDUCE_MAX_ABS:
                    cd.cudecompAmdReduceInterior(axis, h, gd, pa, pb if op == cd.REDUCE_DOT else None, op, sc.results.data_ptr(),
                                                 sc.work.data_ptr(), dtype, halo, padding, stream)
                    whole = sc.take()
                    if not same_bits(got.sum(axis=0) + 0.0, whole):
                        failures.append("%s: the profile adds up to %s, the scalar reduction gives %s" % (what, got.sum(axis=0).tolist(), whole.tolist()))
        cd.cudecompGridDescDestroy(h, gd)
    if not {"profile_rows_kernel", "profile_columns_kernel", "profile_elements_kernel"} <= names:
        failures.append("kernels seen: %s" % sorted(names))
    return failures[:20]


def multi_field(rank, nranks, args):
    """3 and 32 fields with distinct data of any magnitude: every field's profile is bit-identical to its single-field call"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype, axis in ((cd.FLOAT, 0), (cd.DOUBLE_COMPLEX, 1), (cd.DOUBLE, 2)):
        nc, real = AB.TYPES[dtype][1], AB.TYPES[dtype][0]
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        shape = interior_shape(p, nc)
        ghost = bytes([POISON]) * AB.element_bytes(dtype)
        fields = [torch.from_numpy(pencil_image(p, dtype, _random_reals(shape, 100 * (dtype + 10) + f, real), ghost)).cuda() for f in range(32)]
        ptrs = [t.data_ptr() + SLACK for t in fields]
        if any(q % 16 for q in ptrs):
            return ["fields are not 16-byte aligned"]
        others = ptrs[1:] + ptrs[:1]
        for op, dim in itertools.product(OPS, range(3)):
            L = shape[2 - _position(p, dim)]
            single = np.concatenate([_profile(axis, h, gd, [ptrs[f]], [others[f]], op, dim, L, dtype, halo, padding, stream) for f in range(32)])
            for n in (3, 32):
                got = _profile(axis, h, gd, ptrs[:n], others[:n], op, dim, L, dtype, halo, padding, stream)
                if not same_bits(got, single[:n]):
                    failures.append("%s op %d dim %d, %d fields differ from their single calls" % (AB.NAMES[dtype], op, dim, n))
            if np.isnan(single).any() or len({single[f].tobytes() for f in range(32)}) < 2:
                failures.append("%s op %d dim %d: NaN in a result, or the fields do not differ" % (AB.NAMES[dtype], op, dim))
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:20]


def accuracy(rank, nranks, args):
    """random fp64 data with exponents over 2^+-30: every entry of the SUM and DOT profiles along every dim against the exactly rounded
    sum of the exact terms (math.fsum; the products through fractions), held to n_k * 2^-53 * sum |term|; two runs, bit-identical"""
    from fractions import Fraction

    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding, dtype = args["halo"], (0, 0, 0), cd.DOUBLE
    stream = torch.cuda.current_stream().cuda_stream
    failures, figures = [], []
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo, padding)
    shape = interior_shape(p, 1)
    a, b = _random_reals(shape, 1, np.float64), _random_reals(shape, 2, np.float64)
    ghost = bytes([POISON]) * 8
    da, db = torch.from_numpy(pencil_image(p, dtype, a, ghost)).cuda(), torch.from_numpy(pencil_image(p, dtype, b, ghost)).cuda()
    fa = np.vectorize(Fraction, otypes=[object])(a[..., 0])
    prod = fa * np.vectorize(Fraction, otypes=[object])(b[..., 0])  # exact products
    for op, dim in itertools.product((cd.REDUCE_SUM, cd.REDUCE_DOT), range(3)):
        npax = 2 - _position(p, dim)
        L = shape[npax]
        runs = [_profile(0, h, gd, [da.data_ptr() + SLACK], [db.data_ptr() + SLACK], op, dim, L, dtype, halo, padding, stream)[0] for _ in range(2)]
        name = cd.cudecompExtLastKernelName()
        worst = 0.0
        for k in range(L):
            if op == cd.REDUCE_SUM:
                terms = np.moveaxis(a[..., 0], npax, 0)[k].reshape(-1)
                exact, scale = Fraction(math.fsum(terms)), math.fsum(np.abs(terms))
            else:
                terms = np.moveaxis(prod, npax, 0)[k].reshape(-1)
                exact, scale = sum(terms, Fraction(0)), float(sum((abs(t) for t in terms), Fraction(0)))
            err, bound = abs(Fraction(float(runs[0][k, 0])) - exact), Fraction(terms.size) * Fraction(1, 2 ** 53) * Fraction(scale)
            worst = max(worst, float(err / bound))
            if not (err <= bound) or runs[0][k, 1] != 0.0:
                failures.append("op %d dim %d entry %d: error %.3e bound %.3e got %s" % (op, dim, k, float(err), float(bound), runs[0][k].tolist()))
        figures.append("op %d dim %d (%s): %d entries of %d cells, worst error / bound %.3e" % (op, dim, name, L, a.size // L, worst))
        print(figures[-1])
        if not same_bits(runs[0], runs[1]):
            failures.append("op %d dim %d: two runs differ" % (op, dim))
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": failures[:10], "figures": figures}


def edge_values(rank, nranks, args):
    """a NaN in one plane makes only that entry NaN for MAX_ABS; zeros of either sign give +0.0; an infinity stays in its plane"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, padding = args["halo"], args["padding"]
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for dtype, dim in itertools.product((cd.DOUBLE, cd.HALF, cd.FLOAT_COMPLEX), range(3)):
        nc = AB.TYPES[dtype][1]
        p = cd.cudecompGetPencilInfo(h, gd, 0, halo, padding)
        shape = interior_shape(p, nc)
        npax = 2 - _position(p, dim)
        L = shape[npax]
        ghost = bytes([POISON]) * AB.element_bytes(dtype)
        at = tuple(min(1, s - 1) for s in shape[:3])  # a cell of plane min(1, L - 1)
        hit = at[npax]
        im = 0.25 if nc == 2 else 0.0

        def run(op, special, fill):
            vals = np.full(shape, fill)
            if nc == 2:
                vals[..., 1] = 0.25
            if special is not None:
                vals[at + (0,)] = special
            d = torch.from_numpy(pencil_image(p, dtype, vals, ghost)).cuda()
            return _profile(0, h, gd, [d.data_ptr() + SLACK], None, op, dim, L, dtype, halo, padding, stream)[0]

        plane = int(np.prod(shape[:3])) // L
        others = [k for k in range(L) if k != hit]
        got = run(cd.REDUCE_MAX_ABS, np.nan, 1.0)
        if not (np.isnan(got[hit, 0]) and same_bits(got[others], [[1.0, im]] * len(others)) and same_bits(got[hit, 1], im)):
            failures.append("%s dim %d max-abs with a NaN in plane %d: %s" % (AB.NAMES[dtype], dim, hit, got.tolist()))
        for op, fill in itertools.product(OPS[::2], (0.0, -0.0)):
            got = run(op, None, fill)
            if not same_bits(got, [[0.0, im * (plane if op == cd.REDUCE_SUM else 1)]] * L):
                failures.append("%s dim %d op %d of zeros %s: %s" % (AB.NAMES[dtype], dim, op, fill, got.tolist()))
        for op in OPS[::2]:
            got = run(op, -np.inf, 1.0)
            rest = [float(plane) if op == cd.REDUCE_SUM else 1.0, im * (plane if op == cd.REDUCE_SUM else 1)]
            want = np.array([rest] * L)
            want[hit, 0] = -np.inf if op == cd.REDUCE_SUM else np.inf
            if not same_bits(got, want):
                failures.append("%s dim %d op %d with an infinity in plane %d: %s" % (AB.NAMES[dtype], dim, op, hit, got.tolist()))
    cd.cudecompGridDescDestroy(h, gd)
    return failures[:10]


# ---- several ranks -------------------------------------------------------------------------------------------------------------
def ranks_sweep(rank, nranks, args):
    """every rank places the profiles of its slab of a closed form of the global index at lo[dim] of a zeroed global array (the
    header's recipe, ld = the global extent): [failures, {case: [array, dtype, L, cells]}].  Also serves the grid on which a rank
    owns nothing: where L == 0 nothing is written -- the array is pre-set to a sentinel there instead of zeros."""
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
        nc = AB.TYPES[dtype][1]
        padding = (0, 1, 0)
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        sa, sb = rank_slab(p, wa), rank_slab(p, wb)
        shape = interior_shape(p, nc)
        if sa.shape != shape[:3]:
            failures.append("rank %d axis %d halo %s: slab %s, interior %s" % (rank, axis, halo, sa.shape, shape))
            continue
        ia, ib = np.stack([sa, sb][:nc] if nc == 2 else [sa], axis=-1), np.stack([sb, sa][:nc] if nc == 2 else [sb], axis=-1)
        ghost = bytes([POISON]) * AB.element_bytes(dtype)
        fa = [torch.from_numpy(pencil_image(p, dtype, v, ghost)).cuda() for v in (ia, ib)]
        ptrs = [t.data_ptr() + SLACK for t in fa]
        cells = int(np.prod(shape[:3]))
        for op, dim in itertools.product(OPS, range(3)):
            pos = _position(p, dim)
            L, N, lo = shape[2 - pos], gdims[dim], int(p.lo[pos])
            sentinel = 0.0 if L else -777.0
            glob = torch.full((2, N, 2), sentinel, dtype=torch.float64, device="cuda")
            work = _workspace(2, L)
            cd.cudecompAmdProfileInterior(axis, h, gd, ptrs, ptrs[::-1] if op == cd.REDUCE_DOT else None, op, dim,
                                          glob.data_ptr() + 16 * lo, N, work.data_ptr(), dtype, halo, padding, stream)
            got = glob.cpu().numpy()
            want = np.full((2, N, 2), sentinel)
            if cells:
                want[0, lo:lo + L], want[1, lo:lo + L] = profile_reference(op, ia, ib, 2 - pos), profile_reference(op, ib, ia, 2 - pos)
            elif L:
                want[:, lo:lo + L] = 0.0
            if not same_bits(got, want):
                failures.append("rank %d axis %d halo %s %s op %d dim %d: got %s want %s" % (rank, axis, halo, AB.NAMES[dtype], op, dim,
                                                                                            got.tolist(), want.tolist()))
            mine["%d %s %d %d" % (axis, tuple(halo), op, dim)] = [got.tolist(), dtype, L, cells]
    cd.cudecompGridDescDestroy(h, gd)
    return [failures, mine]


# ---- hipGraph, asynchrony ------------------------------------------------------------------------------------------------------
def graph_replay(rank, nranks, args):
    """one call per kept position captured, replayed, the field changed, replayed again: each replay bit-identical to an eager call"""
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
    failures, names = [], set()
    for pos in range(3):
        dim, L = int(p.order[pos]), shape[2 - pos]
        eager, replayed = Results(L), Results(L)
        works = [_workspace(1, L), _workspace(1, L)]
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())

        def call(res, work, sptr):
            cd.cudecompAmdProfileInterior(axis, h, gd, [field.data_ptr() + SLACK], [other.data_ptr() + SLACK], op, dim,
                                          res.buf.data_ptr(), L, work.data_ptr(), dtype, halo, padding, sptr)

        with torch.cuda.stream(stream):
            call(replayed, works[1], stream.cuda_stream)  # warm-up
            stream.synchronize()
            replayed.host()
            stream.synchronize()
        names.add(cd.cudecompExtLastKernelName().split("<")[0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
            call(replayed, works[1], torch.cuda.current_stream().cuda_stream)
        seen = []
        for it in (0, 1):
            with torch.cuda.stream(stream):
                field.copy_(images[it])  # the contents change on the stream; the pointers, and the graph, stay
                graph.replay()
                stream.synchronize()
                r = replayed.host()
                stream.synchronize()
                call(eager, works[0], stream.cuda_stream)
                stream.synchronize()
                e = eager.host()
                stream.synchronize()
            seen.append(r)
            if np.isnan(r).any() or not same_bits(r, e):
                failures.append("position %d replay %d differs from the eager call" % (pos, it))
        if same_bits(seen[0], seen[1]):
            failures.append("position %d: the two contents give one result" % pos)
        del graph
    if len(names) != 2:  # rows for positions 1 and 2, columns or element-wise for position 0
        failures.append("kernels seen: %s" % sorted(names))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def returns_before_the_gpu_is_done(rank, nranks, args):
    """a long run of kernels is enqueued on a stream, then profiles: the calls return while that work is still running (an event
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
    big = torch.zeros(1 << 28, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    dims = [int(p.order[pos]) for pos in range(3)]
    res = [Results(shape[2 - pos]) for pos in range(3)]
    work = _workspace(1, max(shape[:3]))

    def calls():
        for pos in range(3):
            cd.cudecompAmdProfileInterior(0, h, gd, [dev.data_ptr() + SLACK], None, cd.REDUCE_SUM, dims[pos], res[pos].buf.data_ptr(),
                                          shape[2 - pos], work.data_ptr(), dtype, halo, padding, stream.cuda_stream)

    calls()  # warm-up: first-use work happens before the timed part
    torch.cuda.synchronize()
    for r in res:
        r.host()
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
    failures = []
    for pos in range(3):
        got, want = res[pos].host(), profile_reference(cd.REDUCE_SUM, ia, None, 2 - pos)
        if not same_bits(got, want):
            failures.append("position %d: got %s want %s" % (pos, got.tolist(), want.tolist()))
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": failures, "pending_after_the_calls": pending, "enqueue_ms": (t1 - t0) * 1e3, "host_ms": (t2 - t1) * 1e3,
            "total_ms": (t3 - t0) * 1e3}
