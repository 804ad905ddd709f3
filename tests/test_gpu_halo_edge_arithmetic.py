"""IEEE edge values through the adding kernels that tests/test_gpu_halo_accumulate.py and tests/test_gpu_halo_accumulate_clear.py
do not reach: kernels_fold.hip (rows_fold_kernel, generic_fold_kernel), kernels_field_mirror.hip (rows_fields_fold_kernel,
generic_fields_fold_kernel), kernels_field_accumulate.hip (rows_fields_accumulate_kernel, generic_fields_accumulate_kernel) and
every lane width, the streaming access and the complex types of kernels_wall.hip (rows_wall_kernel, generic_wall_kernel).

Operands: all 24 x 24 pairs of AB.edge_table per real format (signed zeros, subnormals, ties, overflow ties, infinities, two NaNs)
and the three dense draws of AB.dense_draws at 2^16 reals, laid out by tests/edge_arithmetic.py.  Every launch places them by the cell
lists of tests/move_lists.py: destination cell n holds a[n], the source cell the (mirrored) move pairs with it holds b[n], every
other byte of every buffer is random.  Afterwards every byte outside the destination cells is what it was -- under TAKE the source
cells are zero bytes --, and the destination cells hold EA.expected: the sign flip of the SOURCE first, then the addition of the
element type with the destination as the first operand (AB.typed_add).  Comparison rule (AB.mismatches): where the expected real is
a NaN the device real must be a NaN of the type, every other real bit for bit.  There is no tolerance.  The names of the kernels
that ran are held to the spelled-out set of instantiations of the family: an instantiation that no launch reached fails the test.
tests/test_edge_arithmetic_table.py holds the operand tables to what these tests need of them (classes present, few NaN cells, a
wrong reference is told apart) on the CPU; the two can-fail tests at the end show the same on the device's own results.

The public calls (cudecompAmdFoldHalos*, cudecompAmdFoldFieldHalos*, cudecompAmdAccumulateFieldHalos*) on pencils filled with the
same pairs, ghost cells included, run on a rank of the pool: tests/edge_arithmetic_bodies.py."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import edge_arithmetic as EA
from tests import edge_arithmetic_bodies as EB
from tests import move_lists as ML
from tests.mp import run_ranks

pytestmark = pytest.mark.gpu

SLACK = 256  # random bytes in front of and behind every device buffer (and between the fields of an arena): compared like the rest
TYPES = pytest.mark.parametrize("dtype", AB.ALL_TYPES, ids=[AB.NAMES[t] for t in AB.ALL_TYPES])
TF = {False: "false", True: "true"}
FORCES = (0, 1, 2)  # fast path, forced element-wise, forced streaming


def _format(dtype):
    """(unsigned type of one real, reals per element, element bytes)"""
    return AB.FORMATS[AB.kind_of(dtype)][0], AB.TYPES[dtype][1], AB.element_bytes(dtype)


def _random_cells(dtype, cells, seed):
    """`cells` elements of random bytes plus the slack on both sides: (cells + 2 * SLACK / es, reals per element) bit patterns"""
    u, nc, es = _format(dtype)
    rng = np.random.default_rng([seed, AB.ALL_TYPES.index(dtype)])
    return rng.integers(0, 256, 2 * SLACK + cells * es, dtype=np.uint8).view(u).reshape(-1, nc)


def _mirrored(extent, ss, mirrored):
    """(signed strides, offset of the source cell of index 0 along the mirrored dim): the source runs backwards along that dim"""
    signed = [int(s) for s in ss]
    if mirrored is None:
        return signed, 0
    signed[mirrored] = -signed[mirrored]
    return signed, (int(extent[mirrored]) - 1) * int(ss[mirrored])


def _upload(host):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(host).view(np.uint8).reshape(-1).copy()).cuda()
    assert t.data_ptr() % 256 == 0
    return t


def _compare(dtype, dev, exp, moves, where):
    """the WHOLE buffer `dev` against `exp` ((cells, nc) bit patterns).  moves: [(destination cells, a, b)] -- bit for bit outside the
    destination cells of all of them, under AB.mismatches inside; the first four wrong reals with their operands in hex.  Returns
    the device's bit patterns."""
    u, nc, _ = _format(dtype)
    kind = AB.kind_of(dtype)
    got = dev.cpu().numpy().view(u).reshape(-1, nc)
    inside = np.zeros(len(got), dtype=bool)
    for dst, _, _ in moves:
        inside[dst] = True
    off = np.flatnonzero((got != exp).any(axis=1) & ~inside)
    assert off.size == 0, where + ("%d cells outside the destination cells differ, first cell %d: %s, expected %s" % (
        off.size, off[0], [hex(int(x)) for x in got[off[0]]], [hex(int(x)) for x in exp[off[0]]]),)
    for k, (dst, a, b) in enumerate(moves):
        bad = np.argwhere(AB.mismatches(kind, got[dst], exp[dst]))
        assert bad.size == 0, where + ("field %d" % k,) + tuple("element %d real %d: %#x (+) %#x gave %#x, expected %#x" % (
            n, r, a[n, r], b[n, r], got[dst[n], r], exp[dst[n], r]) for n, r in bad[:4]) + ("%d reals wrong" % len(bad),)
    return got


def _behind(at, span):
    """an even element offset a few cells behind a block of `span` elements that begins at `at`"""
    end = at + span + 4
    return end + (end & 1)


def _strides(w, h):
    """padded, even pitches on both sides (2-byte elements keep their wide lanes; rows and planes never continue one another)"""
    sp, dp = w + 6 + (w & 1), w + 2 + (w & 1)
    return (1, sp, sp * (h + 1)), (1, dp, dp * (h + 2))


# ---- kernels_fold.hip ---------------------------------------------------------------------------------------------------------
def _fold(dtype, extent, ss, ds, mirrored, soff, doff, a, b, negate, take, force, seed=0, reference=None):
    """one fold-move through cudecompExtFold3D, source and destination in one buffer.  Returns (kernel name, device bit patterns of
    the destination cells, expected ones).  reference: another function (dtype, a, b) -> expected bits, for the can-fail tests."""
    import torch
    u, nc, es = _format(dtype)
    signed, first = _mirrored(extent, ss, mirrored)
    front = SLACK // es
    src, dst = front + ML.cells(extent, signed, soff + first), front + ML.cells(extent, ds, doff)
    both = np.concatenate([src, dst])
    assert src.min() >= front and np.unique(both).size == both.size and a.shape == b.shape == (dst.size, nc)
    init = _random_cells(dtype, int(both.max()) + 1 - front, seed)
    init[dst], init[src] = a, b
    exp = init.copy()
    exp[dst] = EA.expected(dtype, a, b, negate) if reference is None else reference(dtype, a, b)
    if take:
        exp[src] = 0
    dev = _upload(init)
    base = dev.data_ptr() + SLACK
    cls = cd.cudecompExtFold3D(base + (soff + first) * es, base + doff * es, dtype, negate, take, extent, signed, ds, force,
                               torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    where = ("fold", AB.NAMES[dtype], extent, ss, ds, mirrored, soff, doff, "negate %d take %d force %d" % (negate, take, force), cls, name)
    if reference is not None:
        got = dev.cpu().numpy().view(u).reshape(-1, nc)
        return name, got[dst], exp[dst]
    got = _compare(dtype, dev, exp, [(dst, a, b)], where)
    return name, got[dst], exp[dst]


def _fold_names(dtype):
    t, nc, widths = EA.KERNELS[dtype]
    return {"rows_fold_kernel<%s,%d,%d,%s>" % (t, vb, s, TF[take]) for vb in widths for s in (0, 1) for take in (False, True)} | \
           {"generic_fold_kernel<%s,%d,%s>" % (t, nc, TF[take]) for take in (False, True)}


@TYPES
def test_fold_kernels_on_edge_values(dtype):
    """the four shapes of 576 elements -- the mirrored dim the row index for two of them, the plane index for the others -- through
    the fast path, the forced element-wise and the forced streaming kernel, plain and sign-flipping, with and without TAKE"""
    a, b = EA.pairs(dtype)
    t, nc, widths = EA.KERNELS[dtype]
    seen = set()
    for k, (w, h, d) in enumerate(EA.SHAPES):
        ss, ds = _strides(w, h)
        span = ML.span((w, h, d), ss)
        for force, negate, take in itertools.product(FORCES, (False, True), (False, True)):
            name, _, _ = _fold(dtype, (w, h, d), ss, ds, 1 + k % 2, 4, _behind(4, span), a, b, negate, take, force, seed=k)
            assert name.startswith("generic_fold_kernel<" if force & 1 else "rows_fold_kernel<"), (name, force)
            seen.add(name)
    assert seen == _fold_names(dtype), sorted(seen ^ _fold_names(dtype))
    if AB.element_bytes(dtype) == 2:  # odd bases: 2-byte lanes whatever the row length
        ss, ds = _strides(96, 3)
        for force, negate, take in itertools.product((0, 2), (False, True), (False, True)):
            name, _, _ = _fold(dtype, (96, 3, 2), ss, ds, 1, 1, _behind(1, ML.span((96, 3, 2), ss)) + 3, a, b, negate, take, force, seed=9)
            assert name == "rows_fold_kernel<%s,2,%d,%s>" % (t, force // 2, TF[take]), name
    # the mirrored dim as the fastest one: the element-wise kernel without a force bit
    for negate, take in itertools.product((False, True), (False, True)):
        name, _, _ = _fold(dtype, (24, 6, 4), (1, 50, 50 * 7), (1, 50, 50 * 7), 0, 0, 24, a, b, negate, take, 0, seed=10)
        assert name == "generic_fold_kernel<%s,%d,%s>" % (t, nc, TF[take]), name


# ---- kernels_field_mirror.hip, kernels_field_accumulate.hip ---------------------------------------------------------------------
def _field_launch(family, dtype, extent, ss, ds, mirrored, offsets, operands, mask, take, force, seed=0):
    """ONE launch over len(offsets) fields.  family "fold": cudecompExtRunMirroredFieldMoves, all fields in one arena with slack
    around each, field f at offsets[f] elements into its region, bit f of `mask` flips the sign of field f's source.  family
    "accumulate": cudecompExtRunFieldMovesOp, every field in a buffer of its own, source and destination regions inside it.
    operands[f] = (a, b) of field f.  Returns the kernel name."""
    import torch
    u, nc, es = _format(dtype)
    n_fields = len(offsets)
    signed, first = _mirrored(extent, ss, mirrored)
    front = SLACK // es
    part = ML.span(extent, ss) + 4
    part += part & 1  # (even: 2-byte fields decide their alignment by their offsets alone)
    region = max(offsets) + part + ML.span(extent, ds) + 4
    region += -region % 16 + front  # a field's region and the slack in front of the next one
    bases = [front + f * region + offsets[f] for f in range(n_fields)]  # cell number of every field's base in the layout
    move = cd.make_move(extent, signed, ds, src_off=first, dst_off=part, src_buf=0, dst_buf=0)
    init = _random_cells(dtype, n_fields * region - front, seed)
    cells = []
    for f in range(n_fields):
        a, b = operands[f]
        src, dst = bases[f] + ML.cells(extent, signed, first), bases[f] + part + ML.cells(extent, ds, 0)
        both = np.concatenate([src, dst])
        assert np.unique(both).size == both.size and both.min() >= bases[f] and both.max() < (f + 1) * region
        assert a.shape == b.shape == (dst.size, nc)
        init[dst], init[src] = a, b
        cells.append((src, dst))
    exp = init.copy()
    for f, (src, dst) in enumerate(cells):
        exp[dst] = EA.expected(dtype, operands[f][0], operands[f][1], bool((mask >> f) & 1))
        if take:
            exp[src] = 0
    stream = torch.cuda.current_stream().cuda_stream
    if family == "fold":  # one arena
        segments, home = [(0, len(init))], [0] * n_fields
    else:  # a buffer per field: its slack, its region; the last one also takes the slack behind
        segments = [(f * region, (f + 1) * region + (front if f == n_fields - 1 else 0)) for f in range(n_fields)]
        home = list(range(n_fields))
    dev = [_upload(init[lo:hi]) for lo, hi in segments]
    ptrs = [dev[home[f]].data_ptr() + (bases[f] - segments[home[f]][0]) * es for f in range(n_fields)]
    if family == "fold":
        mode = cd.MIRROR_FOLD_TAKE if take else cd.MIRROR_FOLD
        desc = cd.cudecompExtDescribeMirroredFieldMoves([move], ptrs, es, mode, dtype, mask, force)
        launches = cd.cudecompExtRunMirroredFieldMoves([move], ptrs, es, mode, dtype, mask, force, stream)
    else:
        assert mask == 0
        mode = cd.MOVES_ADD_TAKE if take else cd.MOVES_ADD
        desc = cd.cudecompExtDescribeFieldMovesOp([move], ptrs, None, 0, es, mode, dtype, force)
        launches = cd.cudecompExtRunFieldMovesOp([move], ptrs, None, 0, es, mode, dtype, force, stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    where = ("field " + family, AB.NAMES[dtype], extent, ss, ds, mirrored, offsets, "mask %#x take %d force %d" % (mask, take, force), name, desc)
    assert launches == 1 and desc["blocks"] == n_fields * desc["blocks_per_field"], where
    for k, ((lo, hi), t) in enumerate(zip(segments, dev)):
        mine = [f for f in range(n_fields) if home[f] == k]
        _compare(dtype, t, exp[lo:hi], [(cells[f][1] - lo, operands[f][0], operands[f][1]) for f in mine], where + ("fields %s" % mine[:1],))
    return name


def _rotated(a, b, f):
    """the pairs of field f: rotated by 24 f + f, so that the fields differ and a field served from another's base is seen"""
    return np.roll(a, -(25 * f), axis=0), np.roll(b, -(25 * f), axis=0)


def _field_names(family, dtype):
    t, nc, widths = EA.KERNELS[dtype]
    return {"rows_fields_%s_kernel<%s,%d,%d,%s>" % (family, t, vb, s, TF[take]) for vb in widths for s in (0, 1) for take in (False, True)} | \
           {"generic_fields_%s_kernel<%s,%d,%s>" % (family, t, nc, TF[take]) for take in (False, True)}


def _field_family(family, dtype):
    a, b = EA.pairs(dtype)
    t, nc, widths = EA.KERNELS[dtype]
    three = [_rotated(a, b, f) for f in range(3)]
    mask = 0b010 if family == "fold" else 0
    seen = set()
    for k, (w, h, d) in enumerate(EA.SHAPES):
        ss, ds = _strides(w, h)
        mirrored = 1 + k % 2 if family == "fold" else None
        for force, take in itertools.product(FORCES, (False, True)):
            name = _field_launch(family, dtype, (w, h, d), ss, ds, mirrored, [0, 2, 4], three, mask, take, force, seed=k)
            assert name.startswith("generic_fields_" if force & 1 else "rows_fields_"), (name, force)
            seen.add(name)
    assert seen == _field_names(family, dtype), sorted(seen ^ _field_names(family, dtype))
    ss, ds = _strides(96, 3)
    mirrored = 2 if family == "fold" else None
    if family == "fold":  # 32 fields, only the last one flipped: the mask at its full width
        many = [_rotated(a, b, f) for f in range(32)]
        for force, take in itertools.product(FORCES, (False, True)):
            _field_launch(family, dtype, (96, 3, 2), ss, ds, mirrored, [2 * (f % 5) for f in range(32)], many, 1 << 31, take, force, seed=11)
    if AB.element_bytes(dtype) == 2:  # ONE field at 2 mod 4: 2-byte lanes for the whole launch
        for force, take in itertools.product((0, 2), (False, True)):
            name = _field_launch(family, dtype, (96, 3, 2), ss, ds, mirrored, [0, 3, 4], three, mask, take, force, seed=12)
            assert name == "rows_fields_%s_kernel<%s,2,%d,%s>" % (family, t, force // 2, TF[take]), name


@TYPES
def test_field_fold_kernels_on_edge_values(dtype):
    """three fields of which the middle one flips its signs, each with the pairs rotated by another amount and held to the expected
    sums of its own parity; 32 fields with only field 31 flipped; one field at an odd offset (2-byte elements)"""
    _field_family("fold", dtype)


@TYPES
def test_field_accumulate_kernels_on_edge_values(dtype):
    """three fields in buffers of their own, additions and additions that take"""
    _field_family("accumulate", dtype)


# ---- kernels_wall.hip ---------------------------------------------------------------------------------------------------------------
WALL_LENGTHS = {2: (24, 28, 26, 25), 4: (24, 26, 25), 8: (24, 25), 16: (24,)}  # element bytes -> row lengths: lanes of 16, 8, 4, 2 bytes
LAYERS = 4


def _wall(dtype, extent, ss, ds, mirrored, soff, doff, src_bits, addends, side, negate, force, seed=0):
    """one wall-value move through cudecompExtWall3D: dst = (flipped) src + the addend of the destination's layer (side 0: layer
    extent - 1 - j, side 1: layer j, j the index along the mirrored dim).  src_bits: (elements, nc) in the order of the move's
    cells; addends: (layers, nc).  Returns the kernel name."""
    import torch
    u, nc, es = _format(dtype)
    signed, first = _mirrored(extent, ss, mirrored)
    front = SLACK // es
    src, dst = front + ML.cells(extent, signed, soff + first), front + ML.cells(extent, ds, doff)
    both = np.concatenate([src, dst])
    assert src.min() >= front and np.unique(both).size == both.size and extent[mirrored] <= cd.MAX_WALL_HALO
    j = np.indices([int(e) for e in extent][::-1]).reshape(3, -1)[::-1][mirrored]  # index along the mirrored dim, in the cells' order
    layer = (int(extent[mirrored]) - 1 - j) if side == 0 else j
    init = _random_cells(dtype, int(both.max()) + 1 - front, seed)
    init[src] = src_bits
    exp = init.copy()
    exp[dst] = EA.expected_wall(dtype, src_bits, addends[layer], negate)
    dev = _upload(init)
    base = dev.data_ptr() + SLACK
    cls = cd.cudecompExtWall3D(base + (soff + first) * es, base + doff * es, dtype, negate, side, np.ascontiguousarray(addends), extent,
                               signed, ds, force, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    where = ("wall", AB.NAMES[dtype], extent, ss, ds, mirrored, soff, doff, "side %d negate %d force %d" % (side, negate, force), cls, name)
    _compare(dtype, dev, exp, [(dst, src_bits, addends[layer])], where)
    return name


@TYPES
def test_wall_kernels_on_edge_values_every_lane_width(dtype):
    """rows that hold the 24 mirror values cyclically, four layers along the row index whose addends are four table entries; six
    launches walk the table, so that every (mirror, addend) pair of reals meets every lane width, both accesses and both parities.
    Complex types: the two reals of an element -- of the source and of the addend -- come from different rows of the table."""
    u, nc, es = _format(dtype)
    t, _, widths = EA.KERNELS[dtype]
    table = AB.edge_table(AB.kind_of(dtype))
    names = {"rows_wall_kernel<%s,%d,%d,%s>" % (t, vb, s, TF[neg]) for vb in widths for s in (0, 1) for neg in (False, True)} | \
            {"generic_wall_kernel<%s,%d,%s>" % (t, es, TF[neg]) for neg in (False, True)}
    seen = set()
    assert LAYERS <= cd.MAX_WALL_HALO
    for length in WALL_LENGTHS[es]:
        extent = (length, LAYERS, 1)
        pitch = length + 2 + (length & 1)
        ss = ds = (1, pitch, pitch * LAYERS)
        i, r = np.meshgrid(np.arange(length), np.arange(LAYERS))  # the cells' order: dim 0 fastest
        i, r = i.reshape(-1), r.reshape(-1)
        src_bits = np.stack([table[(i + 5 * r + 11 * c) % 24] for c in range(nc)], axis=1)  # (every row holds all 24, each shifted)
        met = [set() for _ in range(nc)]
        for q, negate, force in itertools.product(range(6), (False, True), FORCES):
            which = 4 * q + np.arange(LAYERS)
            addends = np.stack([table[(which + 13 * c) % 24] for c in range(nc)], axis=1)
            side = q & 1
            seen.add(_wall(dtype, extent, ss, ds, 1, 2, 2 + pitch * LAYERS + 4, src_bits, addends, side, negate, force, seed=q))
            layer = (LAYERS - 1 - r) if side == 0 else r  # (as _wall pairs them: the n-th source cell with the n-th destination cell)
            for c in range(nc):
                met[c] |= set(zip(src_bits[:, c].tolist(), addends[layer, c].tolist()))
        assert all(len(m) == 576 for m in met)  # every (mirror, addend) pair of reals, in both parts of a complex element
        if nc == 2:
            assert (src_bits[:, 0] != src_bits[:, 1]).all() and (addends[:, 0] != addends[:, 1]).all()
    assert seen == names, sorted(seen ^ names)


# ---- dense bit patterns -----------------------------------------------------------------------------------------------------------
DENSE = 1 << 16  # reals per launch


def _dense_shapes(nc):
    n = DENSE // nc
    rows = n // 1024
    return n, (512, rows, 2), (1, 520, 520 * (rows + 1)), (1, 516, 516 * (rows + 2))


@pytest.mark.parametrize("family", ["fold", "field_fold", "field_accumulate", "wall"])
@TYPES
def test_dense_bit_patterns(dtype, family):
    """2^16 reals per launch of uniformly random patterns, of nearly cancelling pairs and of subnormal operands, as one move of 512-
    element rows with padded pitches on both sides, through the three paths.  Two halves: plain (fold, field fold, wall; the field
    accumulation takes) and sign-flipping (fold and field fold take; the field accumulation does not).  The field families give each
    of two fields half of the move's rows (the launch as a whole carries the 2^16 reals); of the field fold's two fields one flips its
    signs, the other one in the other half.  The wall takes the a side as the mirror and two elements of the b side as the addends
    of its two layers.  The draws contain what they are for: tests/test_edge_arithmetic_table.py."""
    u, nc, es = _format(dtype)
    n, extent, ss, ds = _dense_shapes(nc)
    doff = _behind(0, ML.span(extent, ss))
    plain, for_a_flip = EA.draws(dtype, DENSE, False), EA.draws(dtype, DENSE, True)  # (the second: b with its sign bits flipped)
    for flipped in (False, True):
        for (name, (a, b)), (_, (_, b_flipped)), force in ((p, m, f) for p, m in zip(plain.items(), for_a_flip.items()) for f in FORCES):
            if family == "fold":
                kernel, _, _ = _fold(dtype, extent, ss, ds, 1 if flipped else 2, 0, doff, a, b_flipped if flipped else b, flipped, flipped, force)
                assert kernel.startswith("generic_fold_" if force & 1 else "rows_fold_kernel<%s,16,%d," % (EA.KERNELS[dtype][0], force // 2)), kernel
            elif family == "wall":  # the mirror is the a side; the addends of the two layers (planes) come from the b side
                addends = (b_flipped if flipped else b)[[3, n // 2 + 5]]
                kernel = _wall(dtype, extent, ss, ds, 2, 0, doff, a, addends, int(flipped), flipped, force)
                assert kernel.startswith("generic_wall_" if force & 1 else "rows_wall_kernel<%s,16,%d," % (EA.KERNELS[dtype][0], force // 2)), kernel
            else:  # two fields, half of the draw each
                half = (extent[0], extent[1] // 2, extent[2])
                if family == "field_fold":  # the flipped field changes with the half, and takes b with its sign bits flipped
                    mask = 0b01 if flipped else 0b10
                    operands = [(a[f * (n // 2):(f + 1) * (n // 2)], (b_flipped if (mask >> f) & 1 else b)[f * (n // 2):(f + 1) * (n // 2)]) for f in range(2)]
                    kernel = _field_launch("fold", dtype, half, ss, ds, 1 if flipped else 2, [0, 2], operands, mask, flipped, force)
                else:
                    operands = [(a[f * (n // 2):(f + 1) * (n // 2)], b[f * (n // 2):(f + 1) * (n // 2)]) for f in range(2)]
                    kernel = _field_launch("accumulate", dtype, half, ss, ds, None, [0, 2], operands, 0, not flipped, force)
                assert kernel.startswith("generic_fields_" if force & 1 else "rows_fields_"), kernel


# ---- the comparison can fail ----------------------------------------------------------------------------------------------------
def test_comparison_can_fail_flip_order():
    """one sign-flipping fold of the bf16 pairs: right against EA.expected, and WRONG -- in reals that are not NaN -- against the
    restatements that flip after the addition or flip the destination (only the numpy side is mutated)"""
    dtype = cd.BFLOAT16
    a, b = EA.pairs(dtype)
    ss, ds = _strides(96, 3)
    doff = _behind(4, ML.span((96, 3, 2), ss))
    _, got, want = _fold(dtype, (96, 3, 2), ss, ds, 1, 4, doff, a, b, True, False, 0)
    assert not AB.mismatches("bf16", got, want).any()
    for wrong in (EA.flip_after_the_addition, EA.flip_the_destination):
        _, got, mutated = _fold(dtype, (96, 3, 2), ss, ds, 1, 4, doff, a, b, True, False, 0, reference=wrong)
        told = int(EA.wrong_outside_nan(dtype, got, mutated).sum())
        print(wrong.__name__, "reals told apart:", told)
        # (as many as numpy's own expected sums differ from the mutated ones in: several hundred of the 576)
        assert told == int(EA.wrong_outside_nan(dtype, want, mutated).sum()) > 0, wrong.__name__


def test_comparison_can_fail_flush():
    """one fold of the fp16 pairs against the expected sums with their subnormals flushed to zero: the 30 subnormal results differ"""
    dtype = cd.HALF
    a, b = EA.pairs(dtype)
    ss, ds = _strides(96, 3)
    flushed = lambda dt, x, y: EA.flush_subnormal_results(dt, EA.expected(dt, x, y, False))  # noqa: E731
    _, got, mutated = _fold(dtype, (96, 3, 2), ss, ds, 1, 4, _behind(4, ML.span((96, 3, 2), ss)), a, b, False, False, 0, reference=flushed)
    told = int(EA.wrong_outside_nan(dtype, got, mutated).sum())
    print("subnormal results flushed, reals told apart:", told)
    assert told == int(AB.classes("fp16", EA.expected(dtype, a, b, False))["subnormal"].sum()) > 0


# ---- the public calls on pencils of edge values -------------------------------------------------------------------------------------
PENCILS, ORDERS = EB.PENCILS, EB.ORDERS


@pytest.mark.parametrize("layout", list(ORDERS))
@pytest.mark.parametrize("call", ["fold", "fold_fields", "accumulate_fields"])
def test_public_calls_on_edge_valued_pencils(call, layout):
    """cudecompAmdFoldHalos*, cudecompAmdFoldFieldHalos* and cudecompAmdAccumulateFieldHalos* on pencils whose every cell, ghost
    cells included, walks the 576 pairs: whole buffers with their slack against the numpy restatements; no NaN or infinity of a
    ghost cell lands anywhere but where the contract adds it"""
    out = run_ranks(1, "tests.edge_arithmetic_bodies", call, dict(PENCILS, mem_order=ORDERS[layout]), timeout=300, fresh=False)[0]
    assert out["failures"] == [], out["failures"][:10]
    assert out["launching"] > 0 and out["compared"] >= out["launching"], out
