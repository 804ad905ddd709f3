"""The CHOICES of the kernel layer over a seeded sweep of about 5,000 moves: cudecompExtDescribeMove (no GPU, no memory) must
answer, move by move, what tests/golden/kernel_choice_sweep.json.gz records -- the ten values class, variant, tile, tile counts,
batch, run, walk bits, access mode.  tests/test_kernel_choice_pins.py pins the moves of the benchmarked configurations; this
sweep covers the space around them: every element size, row-like moves, transposes onto either other dim, moves without a unit
stride, small extents and extents that cross the 1 MiB and 32 MiB thresholds, aligned and misaligned bases, pencils with halos
of 1 and 2, the tuning flags and the planner's row pitch.

The fixture is a record of what the classifier DID, to be regenerated only for a deliberate change of a choice: check out the
commit whose choices are the reference, build it, run  python tests/test_kernel_choice_sweep.py --regen  there with this file,
and commit the result.  A refactoring of csrc/kernels.cc never regenerates it."""
import gzip
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_choice_sweep.json.gz")
KEYS = ("cls", "variant", "tile_i", "tile_j", "tiles_i", "tiles_j", "batch", "run", "walk", "access")
SRC, DST = 1 << 32, 1 << 36  # line-aligned "addresses"
N_MOVES = 5000
# cudecompExtDescribeMove flags: 2 streaming access, 4 shifted / window kernels whatever the size, 8 never rewrite the cells
# between rows, 64 / 128 walk i / j first, 256 whole destination rows
FLAGS = (0, 0, 0, 2, 4, 8, 64, 128, 256, 2 | 4, 256 | 4, 256 | 2, 256 | 4 | 2, 256 | 8, 64 | 2, 128 | 2, 256 | 4 | 64)
DST_ORDERS = {"rows": ((0, 1, 2), (0, 2, 1)), "dim1": ((1, 0, 2), (1, 2, 0)), "dim2": ((2, 0, 1), (2, 1, 0))}


def _extent(rng, big):
    r = rng.random()
    if big and r < 0.6:
        return rng.choice([256, 512, 1000, 1024, 1026, 2048])
    if r < 0.8:
        return rng.randint(1, 300)
    return rng.choice([1, 4, 8, 16, 32, 64, 128, 192, 256])


def _layout(ext, order, halo):
    """Strides (elements) of a pencil that holds the logical dims in memory order `order`, with `halo` cells on both sides of
    its two fastest dims, and the offset of its first interior cell."""
    shape = [ext[p] for p in order]
    mem = [1, shape[0] + 2 * halo, (shape[0] + 2 * halo) * (shape[1] + 2 * halo)]
    strides = [0, 0, 0]
    for i, p in enumerate(order):
        strides[p] = mem[i]
    return strides, halo * (1 + mem[1] + mem[2]), mem[1]


def moves():
    """The sweep: (src address, dst address, es, extent, ss, ds, flags, row_pitch) per move, the same on every run."""
    rng = random.Random(20240601)
    out = []
    while len(out) < N_MOVES:
        es = rng.choice([2, 4, 8, 16])
        big = rng.random() < 0.35
        ext = [_extent(rng, big) for _ in range(3)]
        if ext[0] * ext[1] * ext[2] > 1 << 32:
            continue
        shape = rng.choice(["rows", "rows", "dim1", "dim1", "dim1", "dim2", "dim2", "dim2", "none"])
        shalo, dhalo = rng.choice([0, 0, 1, 2]), rng.choice([0, 1, 1, 2])
        cycle = shape in ("dim1", "dim2") and rng.random() < 0.3
        if cycle:  # the hops of an axis-contiguous cycle: line-aligned extents and bases, rows dense or padded by a line
            ext = [rng.choice([64, 128, 192, 256, 320, 512, 1024]) for _ in range(3)]
            shalo, dhalo = 0, rng.choice([0, 0, 64 // es])
        ss, soff, _ = _layout(ext, (0, 1, 2), shalo)
        ds, doff, pitch = _layout(ext, rng.choice(DST_ORDERS.get(shape, DST_ORDERS["dim1"] + DST_ORDERS["dim2"])), dhalo)
        if shape == "none":  # every other cell of the source and / or every third of the destination: no unit stride
            k = rng.choice([(2, 1), (1, 3), (2, 3)])
            ss, ds = [s * k[0] for s in ss], [d * k[1] for d in ds]
        # bases: aligned, one element on, an odd number of elements on, the first interior cell of the halo pencil
        soff = rng.choice([0, 0, 1, rng.choice([3, 5, 7, 9]), soff])
        doff = rng.choice([0, 1, rng.choice([3, 5, 7, 9]), doff, doff])
        flags = rng.choice(FLAGS)
        if cycle:
            soff, doff, flags = 0, 0, rng.choice([0, 2, 2, 2, 64 | 2, 128 | 2])
        row_pitch = pitch if dhalo and rng.random() < 0.25 else 0  # the planner's word instead of (or besides) flag 256
        out.append((SRC + soff * es, DST + doff * es, es, ext, ss, ds, flags, row_pitch))
    return out


def describe(move):
    src, dst, es, ext, ss, ds, flags, row_pitch = move
    d = cd.cudecompExtDescribeMove(src, dst, es, ext, ss, ds, flags=flags, row_pitch=row_pitch)
    return [d[k] for k in KEYS]


def _recorded():
    with gzip.open(FIXTURE, "rt") as f:
        columns = json.load(f)
    return [list(row) for row in zip(*[columns[k] for k in KEYS])]


def test_every_move_of_the_sweep_is_classified_as_recorded():
    sweep, recorded = moves(), _recorded()
    assert len(sweep) == len(recorded) == N_MOVES
    diffs = []
    for move, want in zip(sweep, recorded):
        got = describe(move)
        if got != want:
            diffs.append("move (src, dst, es, extent, ss, ds, flags, row_pitch) = %s\n  recorded %s\n  now      %s"
                         % (move, dict(zip(KEYS, want)), dict(zip(KEYS, got))))
    assert not diffs, "%d of %d choices differ from %s:\n%s" % (len(diffs), N_MOVES, FIXTURE, "\n".join(diffs[:20]))


def test_the_sweep_reaches_every_kind_of_choice():
    """The record is not vacuous: every kernel family, every variant, both run walks and the three local access modes occur at
    least 20 times.  The ten values do not name the window kernel; it and the plain kernel are counted by the signatures only
    they have (4-byte elements: 64 x 128 tiles without the 300 of the plain kernel's; plain: the longer tiles, 2-byte elements,
    64 x 64 tiles of 4-byte elements, access mode 2), which undercounts both."""
    rows = [dict(zip(KEYS, r), es=m[2]) for m, r in zip(moves(), _recorded())]
    count = lambda pred: sum(1 for r in rows if pred(r))
    tiled = lambda r: r["cls"] == 1 and not r["walk"] & (8 | 16)
    seen = {
        "rows plain": count(lambda r: r["cls"] == 0 and r["tile_i"] == 0),
        "rows shifted": count(lambda r: r["cls"] == 0 and r["tile_i"] == 1),
        "rows dense": count(lambda r: r["cls"] == 0 and r["tile_i"] == 2),
        "transpose plain": count(lambda r: tiled(r) and (r["variant"] >= 300 or r["es"] == 2 or r["access"] == 2
                                                         or (r["es"] == 4 and r["tile_j"] == 64))),
        "transpose window": count(lambda r: tiled(r) and r["es"] == 4 and r["tile_j"] == 128 and r["variant"] < 300),
        "transpose lines": count(lambda r: r["cls"] == 1 and r["walk"] & 8),
        "transpose rowlines": count(lambda r: r["cls"] == 1 and r["walk"] & 16),
        "generic": count(lambda r: r["cls"] == 2),
        "run along j": count(lambda r: tiled(r) and r["run"] > 1 and not r["walk"] & 4),
        "run over planes": count(lambda r: tiled(r) and r["run"] > 1 and r["walk"] & 4),
    }
    for v in (1, 2, 4, 8, 301, 302, 304):
        seen["variant %d" % v] = count(lambda r: r["cls"] == 1 and r["variant"] == v)
    for a in (0, 2, 4):
        seen["access %d" % a] = count(lambda r: r["access"] == a)
    assert all(n >= 20 for n in seen.values()), seen


if __name__ == "__main__" and "--regen" in sys.argv:
    table = [describe(m) for m in moves()]
    columns = {k: [row[i] for row in table] for i, k in enumerate(KEYS)}  # (column-wise: it compresses to half the size)
    with open(FIXTURE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:
        f.write(json.dumps(columns, separators=(",", ":")).encode())
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
