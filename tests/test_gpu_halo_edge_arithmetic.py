"""IEEE edge values through the adding kernels that tests/test_gpu_halo_accumulate.py and tests/test_gpu_halo_accumulate_clear.py
do not reach: kernels_fold.hip (rows_fold_kernel, generic_fold_kernel), kernels_field_mirror.hip (rows_fields_fold_kernel,
generic_fields_fold_kernel), kernels_field_accumulate.hip (rows_fields_accumulate_kernel, generic_fields_accumulate_kernel),
every lane width, the streaming access and the complex types of kernels_wall.hip (rows_wall_kernel, generic_wall_kernel), and
the same of kernels_field_wall.hip (rows_fields_wall_kernel, generic_fields_wall_kernel: per-field signs, the addend table up to
its last entry and at its odd half-words) and kernels_wall_plane.hip (rows_wall_plane_kernel, generic_wall_plane_kernel: the plane
a third operand with pitches of its own, eight plane operands in one launch).

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

The wall kernels have no destination operand: the source cell holds a[n], the addend -- of the layer, or the plane entry of the
destination cell -- b[n], and the destination holds EA.expected_wall, the flipped mirror first.

The public calls (cudecompAmdFoldHalos*, cudecompAmdFoldFieldHalos*, cudecompAmdAccumulateFieldHalos*, cudecompAmdSetWallHalos*,
cudecompAmdSetWallFieldHalos*, cudecompAmdSetWallPlaneHalos*) on pencils filled with the same pairs, ghost cells included, run on
a rank of the pool: tests/edge_arithmetic_bodies.py."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import edge_arithmetic as EA
from tests import edge_arithmetic_bodies as EB
from tests import move_lists as ML
from tests import wall_planes_bodies as WPB
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


# ---- kernels_wall_plane.hip -----------------------------------------------------------------------------------------------------
def _up8(n):
    return -(-int(n) // 8) * 8


def _plane_strides(w, h):
    """(pencil source, pencil destination, plane): three different padded pitches, each a multiple of 8 elements -- the lanes of a
    wall-plane move divide every base and stride of its three operands, so with these only the row length narrows them"""
    sp, dp, pp = _up8(w) + 16, _up8(w) + 8, _up8(w) + 24
    return (1, sp, sp * (h + 1)), (1, dp, dp * (h + 2)), (1, pp, pp * (h + 3))


def _wall_plane(dtype, extent, ss, ds, ps, mirrored, soff, doff, poff, a, b, negate, side, force, seed=0, reference=None):
    """one wall-plane move through cudecompExtWallPlane3D: source and destination in one buffer, the plane in a second one, mirrored
    along `mirrored` on the low side (0) as the source always is.  Source cell n holds a[n], the plane entry of destination cell n
    holds b[n]; dst = (flipped) a + b.  The plane buffer must stay as it is.  Returns (kernel name, device bit patterns of the
    destination cells, expected ones); reference: as for _fold."""
    import torch
    u, nc, es = _format(dtype)
    signed, first = _mirrored(extent, ss, mirrored)
    psigned, pfirst = _mirrored(extent, ps, mirrored if side == 0 else None)
    front = SLACK // es
    src, dst = front + ML.cells(extent, signed, soff + first), front + ML.cells(extent, ds, doff)
    pc = front + ML.cells(extent, psigned, poff + pfirst)
    both = np.concatenate([src, dst])
    assert src.min() >= front and np.unique(both).size == both.size and a.shape == b.shape == (dst.size, nc)
    assert pc.min() >= front and np.unique(pc).size == pc.size
    init = _random_cells(dtype, int(both.max()) + 1 - front, seed)
    pinit = _random_cells(dtype, int(pc.max()) + 1 - front, seed + 1000)
    init[src], pinit[pc] = a, b
    exp = init.copy()
    exp[dst] = EA.expected_wall(dtype, a, b, negate) if reference is None else reference(dtype, a, b)
    dev, pdev = _upload(init), _upload(pinit)
    base, pbase = dev.data_ptr() + SLACK, pdev.data_ptr() + SLACK
    cls = cd.cudecompExtWallPlane3D(base + (soff + first) * es, base + doff * es, pbase + (poff + pfirst) * es, dtype, negate, extent,
                                    signed, ds, psigned, force, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    where = ("wall plane", AB.NAMES[dtype], extent, ss, ds, ps, mirrored, soff, doff, poff,
             "side %d negate %d force %d" % (side, negate, force), cls, name)
    assert np.array_equal(pdev.cpu().numpy().view(u).reshape(-1, nc), pinit), where + ("the plane buffer was written",)
    if reference is not None:
        got = dev.cpu().numpy().view(u).reshape(-1, nc)
        return name, got[dst], exp[dst]
    got = _compare(dtype, dev, exp, [(dst, a, b)], where)
    return name, got[dst], exp[dst]


@TYPES
def test_wall_plane_kernels_on_edge_values(dtype):
    """the four shapes of 576 elements -- the mirrored dim the row index for two of them, the plane index for the others -- through
    the fast path, the forced element-wise and the forced streaming kernel, plain and sign-flipping, from a low and from a high
    plane whose pitches are not the pencil's; 2-byte elements at odd bases of the pencil, and of the plane alone"""
    a, b = EA.pairs(dtype)
    t, nc, widths = EA.KERNELS[dtype]
    es = AB.element_bytes(dtype)
    seen = set()
    for k, (w, h, d) in enumerate(EA.SHAPES):
        ss, ds, ps = _plane_strides(w, h)
        assert len({ss[1], ds[1], ps[1]}) == 3 and not (ss[1] | ds[1] | ps[1] | ss[2] | ds[2] | ps[2]) & 1
        doff = _up8(8 + ML.span((w, h, d), ss) + 4)
        vb = max(v for v in widths if (w * es) % v == 0)
        for force, negate, side in itertools.product(FORCES, (False, True), (0, 1)):
            name, _, _ = _wall_plane(dtype, (w, h, d), ss, ds, ps, 1 + k % 2, 8, doff, 16, a, b, negate, side, force, seed=k)
            assert name == ("generic_wall_plane_kernel<%s,%d,%s>" % (t, es, TF[negate]) if force & 1 else
                            "rows_wall_plane_kernel<%s,%d,%d,%s>" % (t, vb, force // 2, TF[negate])), (name, force)
            seen.add(name)
    assert seen == EA.wall_plane_names(dtype), sorted(seen ^ EA.wall_plane_names(dtype))
    if es == 2:  # 2-byte lanes whatever the row length: (a) the pencil's bases odd, (b) ONLY the plane's base odd
        ss, ds, ps = _plane_strides(96, 3)
        doff = _up8(8 + ML.span((96, 3, 2), ss) + 4)
        for (soff, at, poff), force, negate, side in itertools.product(((1, doff + 3, 16), (8, doff, 17)), (0, 2), (False, True), (0, 1)):
            name, _, _ = _wall_plane(dtype, (96, 3, 2), ss, ds, ps, 1, soff, at, poff, a, b, negate, side, force, seed=9)
            assert name == "rows_wall_plane_kernel<%s,2,%d,%s>" % (t, force // 2, TF[negate]), (name, soff, poff)
    # the mirrored dim as the fastest one: the element-wise kernel without a force bit
    for negate, side in itertools.product((False, True), (0, 1)):
        name, _, _ = _wall_plane(dtype, (24, 6, 4), (1, 50, 50 * 7), (1, 50, 50 * 7), (1, 32, 32 * 8), 0, 0, 24, 2, a, b, negate, side, 0, seed=10)
        assert name == "generic_wall_plane_kernel<%s,%d,%s>" % (t, es, TF[negate]), name


@TYPES
def test_wall_plane_lists_on_edge_values(dtype):
    """eight wall-plane moves of one kernel choice in ONE launch of cudecompExtRunMoves, the PlaneOperands of all eight in use: move
    i carries the pairs rotated by 25 i, the sides alternate, every move reads its plane at another offset, and every destination is
    held to ITS plane entries; the fast path and the element-wise flag, plain and sign-flipping"""
    import torch
    u, nc, es = _format(dtype)
    a, b = EA.pairs(dtype)
    t = EA.KERNELS[dtype][0]
    extent, front = (96, 3, 2), SLACK // es
    ss, _, ps = _plane_strides(96, 3)
    span, pspan = ML.span(extent, ss), ML.span(extent, ps)
    pairs, at = [], 8
    for i in range(8):
        doff = _up8(at + span + 4)
        pairs.append(WPB.plane_move(extent, ss, 1 + (i // 2) % 2, at, doff, i & 1, ps, poff=8 * (i + 1) + (i // 2) * _up8(pspan + 8)))
        at = _up8(doff + span + 4)
    moves, operands = [m for m, _ in pairs], [o for _, o in pairs]
    src = [front + ML.cells(m.extent, m.ss, m.src_off) for m in moves]
    dst = [front + ML.cells(m.extent, m.ds, m.dst_off) for m in moves]
    pcs = [front + ML.cells(m.extent, pstr, poff) for m, (poff, pstr) in pairs]
    everything = np.concatenate(src + dst)
    assert everything.min() >= front and np.unique(everything).size == everything.size
    assert len({poff for poff, _ in operands}) == 8 and [m.peer for m in moves] == [0, 1] * 4
    for side in (0, 1):
        mine = np.concatenate([c for m, c in zip(moves, pcs) if m.peer == side])
        assert mine.min() >= front and np.unique(mine).size == mine.size
    rotated = [_rotated(a, b, i) for i in range(8)]
    for negate, flags in itertools.product((False, True), (0, 1)):
        init = _random_cells(dtype, int(everything.max()) + 1 - front, 20 + flags)
        pinit = [_random_cells(dtype, max(int(c.max()) for c in pcs) + 1 - front, 30 + side) for side in (0, 1)]
        for m, s, c, (x, y) in zip(moves, src, pcs, rotated):
            init[s], pinit[m.peer][c] = x, y
        exp = init.copy()
        for d, (x, y) in zip(dst, rotated):
            exp[d] = EA.expected_wall(dtype, x, y, negate)
        dev, pdev = _upload(init), [_upload(x) for x in pinit]
        ptrs = [dev.data_ptr() + SLACK, pdev[0].data_ptr() + SLACK, pdev[1].data_ptr() + SLACK]
        mode = cd.MOVES_WALL_PLANE_NEGATE if negate else cd.MOVES_WALL_PLANE
        described = cd.cudecompExtDescribeMoves(moves, ptrs, es, mode, dtype, flags, planes=operands)
        launches, elements, total = cd.cudecompExtRunMoves(moves, ptrs, es, mode, dtype, None, flags, None,
                                                           torch.cuda.current_stream().cuda_stream, planes=operands)
        torch.cuda.synchronize()
        name = cd.cudecompExtLastKernelName()
        where = ("wall plane list", AB.NAMES[dtype], "negate %d flags %d" % (negate, flags), name)
        assert total == len(described) == 1 and described[0]["n"] == 8 and sorted(described[0]["index"]) == list(range(8)), where + (described,)
        assert sum(elements) == 8 * 576 and launches[2 if flags else 0] == 1, where + (launches, elements)
        assert name == ("generic_wall_plane_kernel<%s,%d,%s>" % (t, es, TF[negate]) if flags else
                        "rows_wall_plane_kernel<%s,16,0,%s>" % (t, TF[negate])), where
        _compare(dtype, dev, exp, [(d, x, y) for d, (x, y) in zip(dst, rotated)], where)
        for side in (0, 1):
            assert np.array_equal(pdev[side].cpu().numpy().view(u).reshape(-1, nc), pinit[side]), where + ("plane %d was written" % side,)


# ---- kernels_field_wall.hip -------------------------------------------------------------------------------------------------------
def _field_wall_launch(dtype, extent, strides, mirrored, offsets, mirrors, addends, mask, side_list, force, seed=0):
    """ONE call of cudecompExtRunWallFieldMoves over len(offsets) fields: all fields in one arena with slack around each, field f
    at offsets[f] elements into its region, which holds a source and a destination block per side of `side_list` (0 low, 1 high):
    one move per side, for every field.  mirrors[f]: (elements, nc), what field f's source cells hold, in the order of the move's
    cells, on every side; addends[f][side]: (layers, nc), ghost layer k counted from the wall outward -- destination index extent
    - 1 - k along the mirrored dim on the low side, k on the high side; bit f of `mask` flips the signs of field f's source.
    Returns (kernel name, the launches cudecompExtDescribeWallFieldMoves lists)."""
    import torch
    u, nc, es = _format(dtype)
    n_fields, layers = len(offsets), int(extent[mirrored])
    signed, first = _mirrored(extent, strides, mirrored)
    front = SLACK // es
    part = ML.span(extent, strides) + 4
    part += part & 1  # (even: 2-byte fields decide their alignment by their offsets alone)
    region = max(offsets) + 2 * len(side_list) * part
    region += -region % 16 + front  # a field's region and the slack in front of the next one
    bases = [front + f * region + offsets[f] for f in range(n_fields)]
    j = np.indices([int(e) for e in extent][::-1]).reshape(3, -1)[::-1][mirrored]  # index along the mirrored dim, in the cells' order
    rng = np.random.default_rng([seed, 5])
    raw = rng.integers(0, 256, (n_fields, 2, cd.MAX_WALL_HALO, es), dtype=np.uint8)  # (a side or layer no move has: never read)
    moves, blocks = [], []
    for i, side in enumerate(side_list):
        m = cd.make_move(extent, signed, strides, src_off=2 * i * part + first, dst_off=(2 * i + 1) * part, src_buf=0, dst_buf=0)
        m.peer = side
        moves.append(m)
        blocks.append((side, ML.cells(extent, signed, 2 * i * part + first), ML.cells(extent, strides, (2 * i + 1) * part)))
    init = _random_cells(dtype, n_fields * region - front, seed)
    for f in range(n_fields):
        assert mirrors[f].shape == (j.size, nc) and layers <= cd.MAX_WALL_HALO
        for side, src, dst in blocks:
            both = bases[f] + np.concatenate([src, dst])
            assert both.min() >= bases[f] and both.max() < (f + 1) * region
            init[bases[f] + src] = mirrors[f]
            assert addends[f][side].shape == (layers, nc)
            raw[f, side, :layers] = np.ascontiguousarray(addends[f][side]).view(np.uint8).reshape(layers, es)
    everything = np.concatenate([bases[f] + c for f in range(n_fields) for _, s, d in blocks for c in (s, d)])
    assert np.unique(everything).size == everything.size
    exp, held = init.copy(), []
    for f in range(n_fields):
        for side, src, dst in blocks:
            per_cell = addends[f][side][(layers - 1 - j) if side == 0 else j]
            exp[bases[f] + dst] = EA.expected_wall(dtype, mirrors[f], per_cell, bool((mask >> f) & 1))
            held.append((bases[f] + dst, mirrors[f], per_cell))
    dev = _upload(init)
    ptrs = [dev.data_ptr() + bases[f] * es for f in range(n_fields)]
    desc = cd.cudecompExtDescribeWallFieldMoves(moves, ptrs, dtype, raw.tobytes(), mask, force)
    launches = cd.cudecompExtRunWallFieldMoves(moves, ptrs, dtype, raw.tobytes(), mask, force, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    name = cd.cudecompExtLastKernelName()
    where = ("field wall", AB.NAMES[dtype], extent, strides, mirrored, offsets, "mask %#x sides %s force %d" % (mask, side_list, force), name)
    assert launches == len(desc), where + (launches, desc)
    _compare(dtype, dev, exp, held, where)
    return name, desc


def _table_entry(desc, es, u, index):
    """entry `index` of the addend table of a described launch, as the reals' bit patterns"""
    return desc["table"][index * es:(index + 1) * es].view(u)


def _field_wall_pass(dtype, length, as_rows, seen):
    """the launches of one row length with the layers as the row index (extent (length, 4, 1)) or as the plane index ((length, 3, 4),
    mirrored dim 2): three fields of which the middle one flips its signs, six launches that walk the table x FORCES x one side and
    both sides.  Every (mirror, addend) pair of reals must have met in every field and part of an element, on a single side and in
    the SECOND move of a launch of two"""
    u, nc, es = _format(dtype)
    table = AB.edge_table(AB.kind_of(dtype))
    pitch = length + 2 + (length & 1)
    if as_rows:
        extent, strides, mirrored = (length, LAYERS, 1), (1, pitch, pitch * LAYERS), 1
    else:
        extent, strides, mirrored = (length, 3, LAYERS), (1, pitch, pitch * 4), 2
    k = np.indices(extent[::-1]).reshape(3, -1)[::-1]  # the cells' order: dim 0 fastest
    i, r = k[0] + 7 * k[3 - mirrored], k[mirrored]  # (layers as planes: the three rows of a plane begin at different entries)
    mirrors = [np.stack([table[(i + 25 * f + 5 * r + 11 * c) % 24] for c in range(nc)], axis=1) for f in range(3)]
    met = {(f, c, second): set() for f in range(3) for c in range(nc) for second in (False, True)}
    for q, force, side_list in itertools.product(range(6), FORCES, (None, (0, 1))):
        side_list = (q & 1,) if side_list is None else side_list
        which = 4 * q + np.arange(LAYERS)
        second = 12 * (len(side_list) - 1)  # (the high side of a launch of both takes other entries than the low side)
        addends = [[np.stack([table[(which + 13 * c + 7 * f + second * side) % 24] for c in range(nc)], axis=1) for side in (0, 1)]
                   for f in range(3)]
        name, desc = _field_wall_launch(dtype, extent, strides, mirrored, [0, 2, 4], mirrors, addends, 0b010, side_list, force, seed=q)
        assert name.startswith("generic_fields_wall_kernel<" if force & 1 else "rows_fields_wall_kernel<") and len(desc) == 1, (name, force, desc)
        seen.add(name)
        for n, side in enumerate(side_list):
            layer = (LAYERS - 1 - r) if side == 0 else r
            for f, c in itertools.product(range(3), range(nc)):
                if len(side_list) == 1 or n == 1:
                    met[(f, c, n == 1)] |= set(zip(mirrors[f][:, c].tolist(), addends[f][side][layer, c].tolist()))
        if nc == 2:
            assert all((addends[f][side][:, 0] != addends[f][side][:, 1]).all() for f in range(3) for side in (0, 1))
    # every (mirror, addend) pair of reals: in the flipped field (1) and in the others, in both parts of a complex element
    assert all(len(m) == 576 for m in met.values()), {key: len(m) for key, m in met.items()}
    if nc == 2:
        assert all((m[:, 0] != m[:, 1]).all() for m in mirrors)


@TYPES
def test_field_wall_kernels_on_edge_values(dtype):
    """every lane width of the type (WALL_LENGTHS), the layers as rows and as planes, three fields with per-field signs and addends,
    one and two moves per launch; 32 fields that fill the addend table; for 2-byte elements one field at 2 mod 4, and addends at the
    odd half-words of the table"""
    u, nc, es = _format(dtype)
    t = EA.KERNELS[dtype][0]
    table = AB.edge_table(AB.kind_of(dtype))
    assert LAYERS <= cd.MAX_WALL_HALO
    seen = set()
    for length in WALL_LENGTHS[es]:
        for as_rows in (True, False):
            _field_wall_pass(dtype, length, as_rows, seen)
    assert seen == EA.field_wall_names(dtype), sorted(seen ^ EA.field_wall_names(dtype))
    # 32 fields, one side, only field 31 flipped: for 16-byte elements 32 x 4 entries are the whole table
    length = WALL_LENGTHS[es][0]
    pitch = length + 2
    k = np.indices((length, LAYERS, 1)[::-1]).reshape(3, -1)[::-1]
    mirrors = [np.stack([table[(k[0] + 25 * f + 5 * k[1] + 11 * c) % 24] for c in range(nc)], axis=1) for f in range(32)]
    for q, force in itertools.product(range(6), FORCES):
        which = 4 * q + np.arange(LAYERS)
        addends = [[np.stack([table[(which + 13 * c + 7 * f) % 24] for c in range(nc)], axis=1)] * 2 for f in range(32)]
        side = q & 1
        name, desc = _field_wall_launch(dtype, (length, LAYERS, 1), (1, pitch, pitch * LAYERS), 1, [2 * (f % 5) for f in range(32)], mirrors,
                                        addends, 1 << 31, (side,), force, seed=11)
        assert len(desc) == 1 and desc[0]["fields"] == 32, desc  # (one launch for every element size: 32 x 4 x 16 bytes fit)
        last = (31 * LAYERS + LAYERS - 1)
        assert es < 16 or (last + 1) * es == cd.WALL_FIELD_TABLE_BYTES
        # the table holds destination layers: the last entry is field 31's outermost ghost layer on the high side, its innermost on the low
        assert np.array_equal(_table_entry(desc[0], es, u, last), addends[31][side][LAYERS - 1 if side else 0])
    if es == 2:  # ONE field at 2 mod 4: 2-byte lanes for the whole launch; three layers, so that field 1's entries begin at an odd half-word
        k = np.indices((24, 3, 1)[::-1]).reshape(3, -1)[::-1]
        mirrors = [table[(k[0] + 25 * f + 5 * k[1]) % 24].reshape(-1, 1) for f in range(3)]
        for q, force in itertools.product(range(8), (0, 2)):
            which = 3 * q + np.arange(3)
            addends = [[table[(which + 7 * f + 12 * side) % 24].reshape(-1, 1) for side in (0, 1)] for f in range(3)]
            side_list = (0, 1) if q & 1 else (1,)
            name, desc = _field_wall_launch(dtype, (24, 3, 1), (1, 26, 26 * 3), 1, [0, 3, 4], mirrors, addends, 0b010, side_list, force, seed=12)
            assert name == "rows_fields_wall_kernel<%s,2,%d>" % (t, force // 2), name
            odd = 0
            for n, side in enumerate(side_list):
                for f, j in itertools.product(range(3), range(3)):
                    index = (n * 3 + f) * 3 + j  # (move, field, destination layer), in elements of 2 bytes
                    assert np.array_equal(_table_entry(desc[0], es, u, index), addends[f][side][2 - j if side == 0 else j])
                    odd += (index * es) & 2 != 0
            assert odd == (9 if len(side_list) == 2 else 4)  # (entries 1, 3, ... of 18 or of 9: each an edge value, each checked)


# ---- dense bit patterns -----------------------------------------------------------------------------------------------------------
DENSE = 1 << 16  # reals per launch


def _dense_shapes(nc):
    n = DENSE // nc
    rows = n // 1024
    return n, (512, rows, 2), (1, 520, 520 * (rows + 1)), (1, 516, 516 * (rows + 2))


@pytest.mark.parametrize("family", ["fold", "field_fold", "field_accumulate", "wall", "wall_plane", "field_wall"])
@TYPES
def test_dense_bit_patterns(dtype, family):
    """2^16 reals per launch of uniformly random patterns, of nearly cancelling pairs and of subnormal operands, as one move of 512-
    element rows with padded pitches on both sides, through the three paths.  Two halves: plain (fold, field fold, wall; the field
    accumulation takes) and sign-flipping (fold and field fold take; the field accumulation does not).  The field families give each
    of two fields half of the move's rows (the launch as a whole carries the 2^16 reals); of the field fold's two fields one flips its
    signs, the other one in the other half.  The wall takes the a side as the mirror and two elements of the b side as the addends
    of its two layers.  The wall plane takes the a side as the mirror and the b side as the plane, pair by pair, so every pair of
    the draw is an addition.  The field wall gives each of two fields half of the rows, one flipped and the other not, swapped in
    the second half, the addends of the two layers from the b side.  The draws contain what they are for:
    tests/test_edge_arithmetic_table.py."""
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
            elif family == "wall_plane":  # the mirror is the a side, the plane the b side, pair by pair: every pair an addition
                ps = (1, 528, 528 * (extent[1] + 3))
                kernel, _, _ = _wall_plane(dtype, extent, ss, ds, ps, 1 if flipped else 2, 0, doff, 8, a, b_flipped if flipped else b, flipped,
                                           int(flipped), force)
                assert kernel.startswith("generic_wall_plane_" if force & 1 else "rows_wall_plane_kernel<%s," % EA.KERNELS[dtype][0]), kernel
                assert force & 1 or kernel.endswith(",%d,%s>" % (force // 2, TF[flipped])), kernel
            elif family == "field_wall":  # two fields, half of the rows each, one of them flipped; both planes of a field are layers
                half = (extent[0], extent[1] // 2, extent[2])
                mask = 0b01 if flipped else 0b10
                mirrors = [a[f * (n // 2):(f + 1) * (n // 2)] for f in range(2)]
                addends = [[(b_flipped if (mask >> f) & 1 else b)[[f * (n // 2) + 3 + side, f * (n // 2) + n // 4 + 5 + side]] for side in (0, 1)]
                           for f in range(2)]
                kernel, _ = _field_wall_launch(dtype, half, ss, 2, [0, 2], mirrors, addends, mask, (int(flipped),), force)
                assert kernel.startswith("generic_fields_wall_" if force & 1 else "rows_fields_wall_kernel<%s,16,%d>" % (EA.KERNELS[dtype][0], force // 2)), kernel
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


def test_comparison_can_fail_wall_plane_flip():
    """one sign-flipping wall-plane move of the bf16 pairs: right against EA.expected_wall, and WRONG -- in reals that are not NaN --
    against the restatements that flip the plane entry instead of the mirror, or the sum (only the numpy side is mutated)"""
    dtype = cd.BFLOAT16
    a, b = EA.pairs(dtype)
    ss, ds, ps = _plane_strides(96, 3)
    doff = _up8(8 + ML.span((96, 3, 2), ss) + 4)
    _, got, want = _wall_plane(dtype, (96, 3, 2), ss, ds, ps, 1, 8, doff, 16, a, b, True, 0, 0)
    assert not AB.mismatches("bf16", got, want).any()
    for wrong in (EA.flip_the_addend, EA.flip_after_the_addition):
        _, got, mutated = _wall_plane(dtype, (96, 3, 2), ss, ds, ps, 1, 8, doff, 16, a, b, True, 0, 0, reference=wrong)
        told = int(EA.wrong_outside_nan(dtype, got, mutated).sum())
        print(wrong.__name__, "reals told apart:", told)
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
@pytest.mark.parametrize("call", ["fold", "fold_fields", "accumulate_fields", "wall_values", "wall_fields", "wall_planes"])
def test_public_calls_on_edge_valued_pencils(call, layout):
    """cudecompAmdFoldHalos*, cudecompAmdFoldFieldHalos*, cudecompAmdAccumulateFieldHalos*, cudecompAmdSetWallHalos*,
    cudecompAmdSetWallFieldHalos* and cudecompAmdSetWallPlaneHalos* on pencils whose every cell, ghost cells included, walks the 576
    pairs (the wall planes too; the wall values are table entries): whole buffers with their slack against the numpy restatements; no
    NaN or infinity of a ghost cell, a mirror cell, an addend or a plane lands anywhere but where the contract puts it"""
    out = run_ranks(1, "tests.edge_arithmetic_bodies", call, dict(PENCILS, mem_order=ORDERS[layout]), timeout=300, fresh=False)[0]
    assert out["failures"] == [], out["failures"][:10]
    assert out["launching"] > 0 and out["compared"] >= out["launching"], out
