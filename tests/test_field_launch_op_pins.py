"""The answers of the field-move list planner for the lists that are no plain copies, pinned (no GPU): adding and taking lists
(cudecompExtDescribeFieldMovesOp), mirrored lists with a sign per field (cudecompExtDescribeMirroredFieldMoves), wall lists with
their launches and addend tables (cudecompExtDescribeWallFieldMoves), and the result code of a few lists each entry refuses.
tests/golden/field_launch_pins.json (tests/test_halo_fields_plan.py) holds the plain copies; the cases here come from the same
generator."""
import hashlib
import itertools
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import cudecomp_amd as cd  # noqa: E402
from tests.test_halo_fields_plan import _pin_cases  # noqa: E402
from tests.test_halo_wall_value_fields_plan import _moves as wall_moves  # noqa: E402

PINS = os.path.join(ROOT, "tests", "golden", "field_launch_op_pins.json")
DTYPE = {2: cd.HALF, 4: cd.FLOAT, 8: cd.DOUBLE, 16: cd.DOUBLE_COMPLEX}
KEYS = ("kind", "vec", "access", "blocks_per_field", "blocks")


def _answer(call):
    try:
        d = call()
    except cd.CudecompError as e:
        return {"error": e.code}
    if isinstance(d, dict):
        return [d[k] for k in KEYS]
    # wall lists: per launch the seven integers and a short hash of the table bytes
    return [[l[k] for k in ("kind", "vec", "access", "blocks", "blocks_per_field", "first_field", "fields")] +
            [hashlib.sha1(l["table"].tobytes()).hexdigest()[:12]] for l in d]


def _mirror(move, dim):
    """the move with its source running backwards along `dim`: the stride negated, src_off at the source cell of index 0"""
    m = cd.make_move(list(move.extent), list(move.ss), list(move.ds), move.src_off, move.dst_off, move.src_buf, move.dst_buf)
    m.peer = move.peer
    m.src_off += max(m.extent[dim] - 1, 0) * m.ss[dim]
    m.ss[dim] = -m.ss[dim]
    return m


def _op_cases():
    """every third case of the generator, the modes 1 (add), 3 (take) and 4 (add and take) in turn: 160 cases"""
    for i, (key, moves, bases, stride, es, force) in enumerate(_pin_cases()):
        if i % 3 == 0:
            mode = (1, 3, 4)[(i // 3) % 3]
            yield "op mode %d, %s" % (mode, key), (moves, bases, 1 << 44, stride, es, mode, DTYPE[es], force)


def _mirrored_cases():
    """the generator's field-to-field cases, mirrored: mode (0 reflect, 1 fold, 4 fold and take) x signs (none, field 0, all) x the
    mirrored dim (0, the fastest, 1, 2) in turn: 160 cases"""
    combos = list(itertools.product((0, 1, 4), ("none", "first", "all"), (0, 1, 2)))
    j = 0
    for key, moves, bases, stride, es, force in _pin_cases():
        if ", field to field," not in key:
            continue
        mode, signs, dim = combos[j % len(combos)]
        j += 1
        neg = {"none": 0, "first": 1, "all": (1 << len(bases)) - 1}[signs]
        yield ("mirrored mode %d, signs %s, dim %d, %s" % (mode, signs, dim, key),
               ([_mirror(m, dim) for m in moves], bases, es, mode, DTYPE[es], neg, force))


def _wall_addends(n_fields, es):
    return np.random.RandomState(4000 + 100 * n_fields + es).randint(0, 256, n_fields * 2 * cd.MAX_WALL_HALO * es).astype(np.uint8).tobytes()


def _wall_cases():
    """fields x element size x layers x sides x mirrored dim x force: the rule F = min(32, 2048 / (S * h * es)) on both sides: 192 cases"""
    for n, es, h, sides, dim, force in itertools.product((1, 2, 5, 32), (2, 16), (1, 8), (1, 3), (0, 1, 2), (0, 1)):
        moves, cells = wall_moves(h, sides, mirrored=dim)
        fields = [0x7f0000000000 + f * (cells * es + 256) for f in range(n)]
        neg = 0xAAAAAAAA & ((1 << n) - 1)
        yield ("wall %d fields, es %d, %d layers, sides %d, dim %d, force %d" % (n, es, h, sides, dim, force),
               (moves, fields, DTYPE[es], _wall_addends(n, es), neg, force))


def _refused_cases():
    """lists each entry refuses: the result code (and one that looks refusable and is not)"""
    row = cd.make_move((64, 5, 3), (1, 66, 732), (1, 66, 732), 0, 2000, 0, 1)
    bases = [(f + 1) << 36 for f in range(33)]
    for n in (0, 33):
        yield "refused op: %d fields" % n, "op", ([row], bases[:n], 1 << 44, 960, 8, 1, cd.DOUBLE, 0)
        yield "refused mirrored: %d fields" % n, "mirrored", ([_mirror(row, 1)], bases[:n], 8, 0, cd.DOUBLE, 0, 0)
        moves, _ = wall_moves(2, 3)
        yield "refused wall: %d fields" % n, "wall", (moves, bases[:n], cd.DOUBLE, _wall_addends(n, 8), 0, 0)
    yield "refused op: mode 2", "op", ([row], bases[:3], 1 << 44, 960, 8, 2, cd.DOUBLE, 0)
    yield "refused op: mode 1, element size against the type", "op", ([row], bases[:3], 1 << 44, 960, 4, 1, cd.DOUBLE, 0)
    yield "refused op: add onto the workspace", "op", ([cd.make_move((64, 5, 3), (1, 66, 732), (1, 64, 320), 0, 0, 0, 2)], bases[:3], 1 << 44, 960,
                                                       8, 1, cd.DOUBLE, 0)
    yield "refused mirrored: mode 3", "mirrored", ([_mirror(row, 1)], bases[:3], 8, 3, cd.DOUBLE, 0, 0)
    yield "refused mirrored: sign bit 3 of 3 fields", "mirrored", ([_mirror(row, 1)], bases[:3], 8, 0, cd.DOUBLE, 8, 0)
    yield "accepted mirrored: no mirrored dim (a fold along nothing)", "mirrored", ([row], bases[:3], 8, 1, cd.DOUBLE, 0, 0)
    yield "refused mirrored: two mirrored dims", "mirrored", ([_mirror(_mirror(row, 1), 2)], bases[:3], 8, 1, cd.DOUBLE, 0, 0)
    moves, _ = wall_moves(2, 3)
    yield "refused wall: sign bit 2 of 2 fields", "wall", (moves, bases[:2], cd.DOUBLE, _wall_addends(2, 8), 4, 0)
    yield "refused wall: two mirrored dims", "wall", ([_mirror(moves[0], 2), moves[1]], bases[:2], cd.DOUBLE, _wall_addends(2, 8), 0, 0)
    yield "refused wall: no mirrored dim", "wall", ([_mirror(moves[0], 1), moves[1]], bases[:2], cd.DOUBLE, _wall_addends(2, 8), 0, 0)
    moves, _ = wall_moves(9, 3)
    yield "refused wall: nine layers", "wall", (moves, bases[:2], cd.DOUBLE, _wall_addends(2, 8), 0, 0)


ENTRY = {"op": lambda a: cd.cudecompExtDescribeFieldMovesOp(*a), "mirrored": lambda a: cd.cudecompExtDescribeMirroredFieldMoves(*a),
         "wall": lambda a: cd.cudecompExtDescribeWallFieldMoves(*a)}


def op_launches():
    table = {}
    for key, args in _op_cases():
        table[key] = _answer(lambda: ENTRY["op"](args))
    for key, args in _mirrored_cases():
        table[key] = _answer(lambda: ENTRY["mirrored"](args))
    for key, args in _wall_cases():
        table[key] = _answer(lambda: ENTRY["wall"](args))
    for key, entry, args in _refused_cases():
        table[key] = _answer(lambda: ENTRY[entry](args))
    return table


def test_field_launches_with_an_operation_are_the_pinned_ones(capfd):
    """tests/golden/field_launch_op_pins.json: [kind, lane bytes, access, workgroups per field, workgroups] of the one launch of an
    adding, taking or mirrored list; per launch of a wall list [kind, lane bytes, access, workgroups, workgroups per field, first
    field, fields, hash of the addend table]; or the error code.  Recorded before the planner took one request record; a mismatch
    is a finding about the planner, not a reason to regenerate (python tests/test_field_launch_op_pins.py --regen rewrites the file
    from whatever library is built)."""
    with open(PINS) as f:
        pinned = json.load(f)
    now = op_launches()
    capfd.readouterr()  # (the refused lists speak on stderr)
    assert sorted(now) == sorted(pinned) and len(now) == 160 + 160 + 192 + 17
    diffs = ["%s: pinned %s, now %s" % (k, pinned[k], now[k]) for k in sorted(now) if now[k] != pinned[k]]
    assert not diffs, "field launches differ from tests/golden/field_launch_op_pins.json:\n" + "\n".join(diffs[:40])
    # a few readable facts of the table
    assert all(isinstance(v, dict) for k, v in pinned.items() if k.startswith("refused"))
    assert pinned["refused mirrored: mode 3"] == pinned["refused wall: 33 fields"] == {"error": cd.RESULT_INVALID_USAGE}
    kinds = lambda prefix: {v[0] for k, v in pinned.items() if k.startswith(prefix) and isinstance(v, list)}  # noqa: E731
    assert kinds("op mode 1,") == {-1, 25, 26} and kinds("op mode 3,") == {-1, 27, 28} and kinds("op mode 4,") == {-1, 29, 30}
    assert kinds("mirrored mode 0,") == {-1, 31, 32} and kinds("mirrored mode 1,") == {-1, 33, 34} and kinds("mirrored mode 4,") == {-1, 35, 36}
    # the mirrored dim as the fastest one is never a row kernel's
    assert all(v[0] in (-1, 32, 34, 36) for k, v in pinned.items() if k.startswith("mirrored") and ", dim 0," in k and isinstance(v, list))
    # wall lists: ceil(n / F) launches with F = min(32, 2048 / (S * h * es)); one field runs as the single call (kinds 37 / 38)
    for k, v in pinned.items():
        if k.startswith("wall"):
            n, es, h, sides = [int(x) for x in re.match(r"wall (\d+) fields, es (\d+), (\d+) layers, sides (\d+),", k).groups()]
            per = min(32, 2048 // (bin(sides).count("1") * h * es))
            assert len(v) == -(-n // per) and [l[5] for l in v] == list(range(0, n, per)) and sum(l[6] for l in v) == n, (k, v)
            assert all(l[0] in ((37, 38) if n == 1 else (39, 40)) for l in v), (k, v)
    assert len(pinned["wall 32 fields, es 16, 8 layers, sides 3, dim 1, force 0"]) == 4


if __name__ == "__main__" and "--regen" in sys.argv:
    with open(PINS, "w") as f:
        table = op_launches()
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)) + "\n}\n")
    print("wrote", PINS)
