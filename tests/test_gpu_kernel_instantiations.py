"""Every instantiation of the row and element-wise kernels a single process can reach, launched through the harness entries
cudecompExtRunMoves (modes 0 ... 10), cudecompExtRunFieldMoves and cudecompExtRunFieldMovesOp (modes 0, 1, 3, 4; three fields):
every real type of the seven data types, every lane width that type reaches (16 / 8 / 4 / 2 bytes by the row length and, for
2-byte elements, by a base at 2 mod 4), cached and streaming access, plain and TAKE, plain and sign-flipped, the mirror as the row
index and as the plane index.  tests/test_gpu_kernel_names.py and the parity suites reach a sample of these; the kernels share one
workgroup decode (csrc/kernels_walk.h), so every one of them is held to it here.  (The remote-store forms of the copies --
rows_kernel<VB,3>, rows_shifted_kernel<VB,3>, generic_kernel<ES,true> -- need no other process's memory: destination bases reach
them on local buffers, tests/test_gpu_tiled_kernel_instantiations.py, beside every instantiation of the LDS-tiled kernels.)

Shapes: the smallest at which every division of the row decode and both of its guards are live.
  wide rows   300 lane vectors x 9 rows x 3 planes, padded pitches on both sides: p0 = 8, two tile columns (the second partial),
              three row tiles of four rows (the last holds one row), three planes.  A lane narrower than 16 bytes needs an odd
              number of vectors (an even one would make the next width): 301 there.
  short rows  7 vectors x 9 rows x 5 planes: p0 = 3, one workgroup per plane, column guard and row guard.
  (rows_shifted_kernel takes rows of 256 bytes and more only: its short rows are the shortest it takes, p0 = 5, 6, 7.)
  element-wise  7 x 9 x 5 elements (315: two workgroups striding), no unit stride along the rows on either side; once with a
              destination-fast dim (the lanes run along it) and once without (along dim 0; reflections and folds: the longest).
Every instantiation runs three launches: each shape alone, then both as a two-move list -- ONE interleaved launch whose filler
workgroups pass through locate() (field-moves: through locateFieldMove) -- with the mirrors swapped.  After every launch EVERY
byte of every buffer, sources included (the take modes clear them), is compared with numpy applying the moves one at a time,
and cudecompExtLastKernelName() with the spelled-out name.  The cells of an addition hold small integers: every sum is exact in
every type.  The largest buffer is below 1 MiB."""
import numpy as np
import pytest
import torch

import cudecomp_amd as cd
from tests.move_lists import cells

pytestmark = pytest.mark.gpu

GENERIC, STREAMING, ALWAYS = 1, 2, 4  # flags of cudecompExtRunMoves; force bits 0 and 1 of the field-move calls
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
# data type -> (real type as the kernel templates spell it, bytes per real, reals per element)
TYPES = {cd.HALF: ("_Float16", 2, 1), cd.BFLOAT16: ("__bf16", 2, 1), cd.HALF_COMPLEX: ("_Float16", 2, 2), cd.FLOAT: ("float", 4, 1),
         cd.FLOAT_COMPLEX: ("float", 4, 2), cd.DOUBLE: ("double", 8, 1), cd.DOUBLE_COMPLEX: ("double", 8, 2)}
H = 9  # rows per plane of every shape
FRONT = 256  # bytes in front of the first region and behind the last one of every buffer (never written: compared)


def encode(values, real):
    """bit patterns of float64 values that the real type holds exactly"""
    if real == "__bf16":
        return (values.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    f = {"_Float16": np.float16, "float": np.float32, "double": np.float64}[real]
    return values.astype(f).view(UINT[np.dtype(f).itemsize])


def decode(bits, real):
    if real == "__bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    f = {"_Float16": np.float16, "float": np.float32, "double": np.float64}[real]
    return bits.view(f).astype(np.float64)


class Op:
    """what a launch does to the cells of its moves"""

    def __init__(self, add=False, take=False, neg=False, fill=None):
        self.add, self.take, self.neg, self.fill = add, take, neg, fill


def layout(es, real):
    """a buffer of `es`-byte elements as a 2-D array: (unsigned type of one real, reals per element)"""
    rb = {"_Float16": 2, "__bf16": 2, "float": 4, "double": 8}[real] if real else min(es, 8)
    return UINT[rb], es // rb


def apply(op, real, src, dst, sc, dc):
    """numpy execution of ONE move on (elements, reals) arrays of bit patterns"""
    if op.fill is not None:
        dst[dc] = op.fill
        return
    x = src[sc].copy()
    if op.neg:
        x ^= x.dtype.type(1 << (8 * x.dtype.itemsize - 1))
    dst[dc] = encode(decode(dst[dc], real) + decode(x, real), real) if op.add else x
    if op.take:
        src[sc] = 0


def rows(nvec, planes, vb, es, mirror=None, off=0):
    """(extent, ss, ds, src_off, dst_off, source span, destination span) of rows of nvec lanes of vb bytes; mirror: 1 the source
    runs backwards along the row index, 2 along the plane index; off: both bases that many elements up"""
    w = nvec * vb // es
    sp, dp = w + 4 + (w & 1), w + 8 + (w & 1)  # (even pitches: 2-byte rows stay dword-aligned unless the base says otherwise)
    ss, ds = [1, sp, sp * (H + 1)], [1, dp, dp * (H + 2)]
    extent = (w, H, planes)
    return place(extent, ss, ds, mirror, off, off)


def place(extent, ss, ds, mirror, soff, doff):
    span = lambda s: sum((e - 1) * abs(x) for e, x in zip(extent, s)) + 1
    if mirror is not None:
        soff += (extent[mirror] - 1) * ss[mirror]
        ss = [(-x if i == mirror else x) for i, x in enumerate(ss)]
    return extent, tuple(ss), tuple(ds), soff, doff, span(ss) + 2, span(ds) + 2


def elementwise(dst_fast, mirror=None):
    """7 x 9 x 5 elements, rows one element thick on both sides"""
    ss = [2, 17, 170]
    ds = [11, 1, 82] if dst_fast else [3, 23, 230]
    return place((7, 9, 5), ss, ds, mirror, 0, 0)


class Buffers:
    """regions for a list of moves, one behind the other, in `count` buffers of which a move reads `src` and writes `dst`"""

    def __init__(self, specs, es, real, seed, src=0, dst=1, count=2, typed=False):
        self.es, self.real = es, real
        u, nc = layout(es, real)
        n = [FRONT // es] * count
        self.moves, self.cells = [], []
        up = lambda k: -(-k // 8) * 8  # (every region starts on a multiple of 8 elements: the base offsets alone misalign)
        for extent, ss, ds, soff, doff, sspan, dspan in specs:
            s0 = n[src] + soff
            n[src] = up(n[src] + sspan + 3)
            d0 = n[dst] + doff
            n[dst] = up(n[dst] + dspan + 3)
            self.moves.append(cd.make_move(extent, ss, ds, s0, d0, src, dst))
            self.cells.append((cells(extent, ss, s0), cells(extent, ds, d0)))
        rng = np.random.default_rng(seed)
        self.host = [rng.integers(0, 256, (k + FRONT // es) * es, dtype=np.uint8).view(u).reshape(-1, nc) for k in n]
        if typed:  # small integers in the cells an addition reads
            for sc, dc in self.cells:
                self.host[src][sc] = encode(rng.integers(0, 8, (sc.size, nc)).astype(np.float64), real)
                self.host[dst][dc] = encode(rng.integers(0, 8, (dc.size, nc)).astype(np.float64), real)
        assert all(h.nbytes < 1 << 20 for h in self.host)
        self.src, self.dst = src, dst

    def expected(self, op):
        exp = [h.copy() for h in self.host]
        for sc, dc in self.cells:
            apply(op, self.real, exp[self.src], exp[self.dst], sc, dc)
        return exp


def check(name, what, dev, exp):
    torch.cuda.synchronize()
    for i, (d, e) in enumerate(zip(dev, exp)):
        bad = np.flatnonzero(d.cpu().numpy() != e.view(np.uint8).ravel())
        assert bad.size == 0, (name, what, "buffer %d: %d bytes differ, first at %d" % (i, bad.size, bad[0]))
    assert cd.cudecompExtLastKernelName() == name, what


def run_moves(name, specs, es, mode, dtype, op, flags, typed, seed):
    real = TYPES[dtype][0] if dtype else None
    b = Buffers(specs, es, real, seed, typed=typed)
    dev = [torch.from_numpy(h.view(np.uint8).ravel().copy()).cuda() for h in b.host]
    value = None if op.fill is None else op.fill.tobytes()
    _, _, total = cd.cudecompExtRunMoves(b.moves, [t.data_ptr() for t in dev] + [None], es, mode, dtype, value, flags, None,
                                         torch.cuda.current_stream().cuda_stream)
    assert total == 1, (name, "launches", total)
    check(name, (es, mode, dtype, flags, len(specs)), dev, b.expected(op))


def run_fields(name, specs, es, mode, dtype, op, force, typed, seed):
    """three fields, source and destination regions in each field's own buffer; mode None: cudecompExtRunFieldMoves"""
    real = TYPES[dtype][0] if dtype else None
    fields = [Buffers(specs, es, real, seed + f, src=0, dst=0, count=1, typed=typed) for f in range(3)]
    dev = [torch.from_numpy(b.host[0].view(np.uint8).ravel().copy()).cuda() for b in fields]
    ptrs, stream = [t.data_ptr() for t in dev], torch.cuda.current_stream().cuda_stream
    if mode is None:
        total = cd.cudecompExtRunFieldMoves(fields[0].moves, ptrs, None, 0, es, force, stream)
    else:
        total = cd.cudecompExtRunFieldMovesOp(fields[0].moves, ptrs, None, 0, es, mode, dtype, force, stream)
    assert total == 1, (name, "launches", total)
    check(name, (es, mode, dtype, force, len(specs)), dev, [b.expected(op)[0] for b in fields])


def lane_cases(es):
    """(lane bytes, vectors of a wide row, base offset in elements) an element size reaches"""
    out = [(vb, 300 if vb == 16 else 301, 0) for vb in (16, 8, 4, 2) if vb >= es]
    if es == 2:
        out.append((2, 300, 1))  # rows of whole 16-byte vectors at 2 mod 4: 2-byte lanes
    return out


def three_launches(run, specs_of):
    """each shape alone, then both as one list with the mirrors swapped (specs_of(swap) -> [wide, short])"""
    wide, short = specs_of(False)
    run([wide], 1)
    run([short], 2)
    run(specs_of(True), 3)


def row_family(run, name_of, es, dtype, mode, op, typed, mirrors=(None, None), flag=0):
    """every lane width of the element size, cached and streaming: name_of(vb, s) is the kernel's name"""
    for vb, nvec, off in lane_cases(es):
        for s in (0, 1):
            specs_of = lambda swap: [rows(nvec, 3, vb, es, mirrors[swap], off), rows(7, 5, vb, es, mirrors[not swap], off)]
            three_launches(lambda specs, k: run(name_of(vb, s), specs, es, mode, dtype, op, flag | (STREAMING if s else 0), typed,
                                                1000 * vb + 10 * s + k), specs_of)


def elementwise_family(run, name, es, dtype, mode, op, typed, mirrors=(None, None), flag=0):
    specs_of = lambda swap: [elementwise(True, mirrors[swap]), elementwise(False, mirrors[not swap])]
    three_launches(lambda specs, k: run(name, specs, es, mode, dtype, op, flag, typed, 77 + k), specs_of)


ELEMENT_SIZES = (2, 4, 8, 16)
DTYPES = sorted(TYPES, key=lambda d: (TYPES[d][1], TYPES[d][2], d))
ids = lambda d: {cd.HALF: "half", cd.BFLOAT16: "bfloat16", cd.HALF_COMPLEX: "half_complex", cd.FLOAT: "float",
                 cd.FLOAT_COMPLEX: "float_complex", cd.DOUBLE: "double", cd.DOUBLE_COMPLEX: "double_complex"}[d]
tf = lambda b: "true" if b else "false"


@pytest.mark.parametrize("es", ELEMENT_SIZES)
def test_copies(es):
    row_family(run_moves, lambda vb, s: "rows_kernel<%d,%d>" % (vb, s), es, 0, cd.MOVES_COPY, Op(), False)
    elementwise_family(run_moves, "generic_kernel<%d,false>" % es, es, 0, cd.MOVES_COPY, Op(), False)


@pytest.mark.parametrize("vb,es,short", [(16, 8, 17), (8, 8, 33), (4, 4, 65)])
def test_shifted_row_copies(vb, es, short):
    """destination rows one element off the 64-byte grid; a row of `short` vectors is the shortest the kernel takes"""
    for s in (0, 1):
        nvec = 300 if vb == 16 else 301
        wide, low = rows(nvec, 3, vb, es), rows(short, 5, vb, es)
        shift = lambda spec: spec[:4] + (spec[4] + 1,) + spec[5:]
        for k, specs in enumerate(([shift(wide)], [shift(low)], [shift(wide), shift(low)])):
            run_moves("rows_shifted_kernel<%d,%d>" % (vb, s), specs, es, cd.MOVES_COPY, 0, Op(), ALWAYS | (STREAMING if s else 0), False, k)


@pytest.mark.parametrize("es", ELEMENT_SIZES)
def test_fills(es):
    value = np.random.default_rng(es).integers(0, 256, es, dtype=np.uint8).view(layout(es, None)[0])
    for off in ((0, 1) if es == 2 else (0,)):
        for s in (0, 1):
            specs_of = lambda swap: [rows(300, 3, 16, es, None, off), rows(7, 5, 16, es, None, off)]
            three_launches(lambda specs, k: run_moves("rows_fill_kernel<16,%d>" % s, specs, es, cd.MOVES_FILL, 0, Op(fill=value),
                                                      STREAMING if s else 0, False, 10 * s + k), specs_of)
    # (a fill has no source: the destination-fast shape alone would be rows of nine elements)
    elementwise_family(run_moves, "generic_fill_kernel<%d>" % es, es, 0, cd.MOVES_FILL, Op(fill=value), False, flag=GENERIC)


@pytest.mark.parametrize("es", ELEMENT_SIZES)
def test_takes(es):
    row_family(run_moves, lambda vb, s: "rows_take_kernel<%d,%d>" % (vb, s), es, 0, cd.MOVES_TAKE, Op(take=True), False)
    elementwise_family(run_moves, "generic_take_kernel<%d>" % es, es, 0, cd.MOVES_TAKE, Op(take=True), False)


@pytest.mark.parametrize("take", (False, True), ids=("add", "add_take"))
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_additions(dtype, take):
    real, rb, nc = TYPES[dtype]
    mode, stem = (cd.MOVES_ADD_TAKE, "accumulate_take") if take else (cd.MOVES_ADD, "accumulate")
    row_family(run_moves, lambda vb, s: "rows_%s_kernel<%s,%d,%d>" % (stem, real, vb, s), rb * nc, dtype, mode, Op(add=True, take=take), True)
    elementwise_family(run_moves, "generic_%s_kernel<%s,%d>" % (stem, real, nc), rb * nc, dtype, mode, Op(add=True, take=take), True)


@pytest.mark.parametrize("es", ELEMENT_SIZES)
def test_reflections(es):
    row_family(run_moves, lambda vb, s: "rows_reflect_kernel<%d,%d,false>" % (vb, s), es, 0, cd.MOVES_REFLECT, Op(), False, (1, 2))
    elementwise_family(run_moves, "generic_reflect_kernel<%d,false>" % es, es, 0, cd.MOVES_REFLECT, Op(), False, (0, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_reflections_that_flip_signs(dtype):
    real, rb, nc = TYPES[dtype]
    row_family(run_moves, lambda vb, s: "rows_reflect_kernel<%d,%d,true>" % (vb, s), rb * nc, dtype, cd.MOVES_REFLECT_NEGATE, Op(neg=True),
               True, (2, 1))
    elementwise_family(run_moves, "generic_reflect_kernel<%d,true>" % (rb * nc), rb * nc, dtype, cd.MOVES_REFLECT_NEGATE, Op(neg=True), True, (2, 0))


@pytest.mark.parametrize("mode", (cd.MOVES_FOLD, cd.MOVES_FOLD_NEGATE, cd.MOVES_FOLD_TAKE, cd.MOVES_FOLD_NEGATE_TAKE),
                         ids=("fold", "negate", "take", "negate_take"))
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_folds(dtype, mode):
    """plain and sign-flipped share an instantiation: the wide rows mirror their row index in the plain modes and their plane
    index in the flipping ones, the short rows the other way round, and the list swaps them -- every instantiation meets both
    mirrors with both signs"""
    real, rb, nc = TYPES[dtype]
    neg, take = mode in (cd.MOVES_FOLD_NEGATE, cd.MOVES_FOLD_NEGATE_TAKE), mode in (cd.MOVES_FOLD_TAKE, cd.MOVES_FOLD_NEGATE_TAKE)
    op = Op(add=True, take=take, neg=neg)
    row_family(run_moves, lambda vb, s: "rows_fold_kernel<%s,%d,%d,%s>" % (real, vb, s, tf(take)), rb * nc, dtype, mode, op, True,
               (2, 1) if neg else (1, 2))
    elementwise_family(run_moves, "generic_fold_kernel<%s,%d,%s>" % (real, nc, tf(take)), rb * nc, dtype, mode, op, True,
                       (2, 0) if neg else (0, 2))


@pytest.mark.parametrize("es", ELEMENT_SIZES)
def test_field_copies_and_takes(es):
    for mode in (None, cd.MOVES_COPY):  # cudecompExtRunFieldMoves, then cudecompExtRunFieldMovesOp
        row_family(run_fields, lambda vb, s: "rows_fields_kernel<%d,%d>" % (vb, s), es, 0, mode, Op(), False)
        elementwise_family(run_fields, "generic_fields_kernel<%d>" % es, es, 0, mode, Op(), False)
    row_family(run_fields, lambda vb, s: "rows_fields_take_kernel<%d,%d>" % (vb, s), es, 0, cd.MOVES_TAKE, Op(take=True), False)
    elementwise_family(run_fields, "generic_fields_take_kernel<%d>" % es, es, 0, cd.MOVES_TAKE, Op(take=True), False)


@pytest.mark.parametrize("take", (False, True), ids=("add", "add_take"))
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_field_additions(dtype, take):
    real, rb, nc = TYPES[dtype]
    mode, op = cd.MOVES_ADD_TAKE if take else cd.MOVES_ADD, Op(add=True, take=take)
    row_family(run_fields, lambda vb, s: "rows_fields_accumulate_kernel<%s,%d,%d,%s>" % (real, vb, s, tf(take)), rb * nc, dtype, mode, op, True)
    elementwise_family(run_fields, "generic_fields_accumulate_kernel<%s,%d,%s>" % (real, nc, tf(take)), rb * nc, dtype, mode, op, True)
