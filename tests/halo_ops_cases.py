"""Case lines of the halo-extension test programs, tests/native/halo_ops_test.cpp and tests/fortran/halo_ops_test.f90 (the same lines,
the Fortran twin with one-based --ax, --dim and --mem_order): shared by tests/test_gpu_native_halo_ops.py and tests/test_fortran.py.

The 16 x 20 x 18 grid of tests/test_gpu_native.py::_halo_lines (ragged slabs on 1 x 4 and 4 x 1); every case is accepted by the library
(h + centering <= the narrowest slab of 4 cells, halos no wider than a slab): a refused case in a positive list fails the list."""
import itertools

OPS = ("accumulate", "fill", "accumulate_clear", "reflect")
COMMUNICATING = ("accumulate", "accumulate_clear")
LOCAL = ("fill", "reflect")
# (halo, periods, padding); the third has a halo in every dim -- the reflection refuses h == 0 only with a bad parity, see the refusals
SETS = [((1, 1, 1), (1, 1, 1), (0, 0, 0)), ((2, 1, 2), (1, 0, 1), (1, 0, 2)), ((1, 2, 1), (0, 0, 0), (0, 1, 0))]
MIRRORS = [(1, 0), (-1, 0), (1, 1), (-1, 1)]  # (parity, centering)
GRID = "--gx 16 --gy 20 --gz 18"


class Forms:
    """What varies from case to case beside the geometry: the reflection cycles through the four mirrors, the fill alternates between
    value = NULL and a value, padding = NULL is passed every other time the padding is zero (`stream`: the Fortran twin alternates
    between its own stream and none; the native program ignores the option)."""

    def __init__(self, base=0, stream=False):
        self.n = {"mirror": 0, "value": 0, "nullpad": 0, "stream": 0}
        self.base, self.stream = base, stream

    def _tick(self, what):
        self.n[what] += 1
        return self.n[what] - 1

    def line(self, op, pdims, backend, ax, ac, halo, per, pad, grid=GRID, more=""):
        text = "--op %s --pr %d --pc %d %s --backend %d --ax %d --ac %d --hex %d --hey %d --hez %d --hpx %d --hpy %d --hpz %d " \
               "--pdx %d --pdy %d --pdz %d" % ((op,) + tuple(pdims) + (grid, backend, ax + self.base, ac) + tuple(halo) + tuple(per) + tuple(pad))
        if op == "reflect":
            text += " --parity %+d --centering %d" % MIRRORS[self._tick("mirror") % 4]
        if op == "fill" and self._tick("value") % 2:
            text += " --value 37"
        if not any(pad) and self._tick("nullpad") % 2:
            text += " --nullpad"
        if self.stream and self._tick("stream") % 3 != 1:
            text += " --stream"
        return text + more


def single_rank_lines(forms, backend=3, ops=OPS, more=""):
    return [forms.line(op, (1, 1), backend, ax, ac, h, per, pad, more=more)
            for op, ax, ac, (h, per, pad) in itertools.product(ops, (0, 1, 2), (0, 1), SETS)]


def mem_order_lines(forms, backend=3):
    """the six memory orders of the tested pencil on 12 x 14 x 10: dims 0 and 2 periodic (accumulate, fill), dim 1 not (reflect)"""
    return [forms.line(op, (1, 1), backend, ax, 0, (1, 2, 1), (1, 0, 1), (0, 1, 0), grid="--gx 12 --gy 14 --gz 10",
                       more=" --mem_order %d %d %d" % tuple(x + forms.base for x in perm))
            for op, ax, perm in itertools.product(OPS, (0, 1, 2), itertools.permutations((0, 1, 2)))]


def four_rank_lines(forms, pdims_list, backends, ops, diagonal=False):
    """per (process grid, backend, operation): the three pencil axes x the three (halo, periods, padding) sets, axis-contiguous
    layout every other case.  `diagonal`: three cases of the nine, every axis and every set once, another pairing per combination."""
    lines = []
    for n, (pdims, b, op) in enumerate(itertools.product(pdims_list, backends, ops)):
        for i, (ax, (h, per, pad)) in enumerate(itertools.product((0, 1, 2), SETS)):
            if diagonal and (i % 3) != (ax + n) % 3:
                continue
            lines.append(forms.line(op, pdims, b, ax, (i + ax + n) % 2, h, per, pad))
    return lines


def refusal_lines(forms, backend=3):
    """(lines, how many of them are refusals).  Every refusal happens on the host before any launch; the result code is the
    headers' CUDECOMP_RESULT_INVALID_USAGE, the pencil stays byte-identical, and a valid case follows each of them.
    cudecomp_amd_reflect.h refuses a bad parity or centering "also when h == 0" and otherwise lets h == 0 succeed with nothing to do
    (tests/test_halo_reflect_plan.py pins that), so the reflection with halo_extents[dim] = 0 is refused for its parity."""
    b = forms.base
    head = "--pr 1 --pc 1 %s --backend %d --ac 0 --hpx 0 --hpy 1 --hpz 1 --pdx 0 --pdy 1 --pdz 0 --expect-refusal" % (GRID, backend)
    refused = ["--op %s --ax %d --dim %d %s" % (op, ax + b, 3 + b, head) for ax, op in enumerate(OPS[:3])]
    refused += ["--op reflect --ax %d --dim %d %s" % (0 + b, 3 + b, head),
                "--op reflect --ax %d --dim %d --parity 0 --centering 0 %s" % (1 + b, 0 + b, head),
                "--op reflect --ax %d --dim %d --parity -1 --centering 2 %s" % (2 + b, 0 + b, head),
                "--op reflect --ax %d --dim %d --parity 0 --centering 1 --hex 0 %s" % (0 + b, 0 + b, head),
                # a halo wider than the rank's interior along a periodic dim: 4 > 3
                "--op accumulate --ax %d --dim %d --hey 4 %s" % (0 + b, 1 + b, head.replace("--gy 20", "--gy 3")),
                "--op accumulate_clear --ax %d --dim %d --hez 4 %s" % (1 + b, 2 + b, head.replace("--gz 18", "--gz 3"))]
    valid = single_rank_lines(forms, backend)
    lines = []
    for i, r in enumerate(refused):
        lines += [r, valid[(7 * i) % len(valid)]]
    return lines, len(refused)
