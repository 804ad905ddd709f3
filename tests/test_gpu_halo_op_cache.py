"""One descriptor, one plan cache, every halo family: a descriptor caches the plans of all eight families of halo call in ONE map
keyed by (axis, dim, halos, padding, periods, packed) AND the operation, and a plan cached for one family must never be served
to another.  Here every family is called with the SAME (axis, dim, halo, periods, padding) on one descriptor, once in a fixed order
and once in the reverse order (so that each family both fills the cache before and finds it filled by every other family), and
each result is compared bit for bit -- the slack around the pencil included -- with the numpy definition the family's own GPU test
uses (tests/*_bodies.py).

Global grid 12 x 10 x 8 on one rank, X pencils, halos (2, 1, 1), periods (True, False, True), no padding: along dims 0 and 2 the
rank is its own neighbour (update, accumulation, fill have cells to write; reflection and folding have none), along dim 1 it has no
neighbour (the other way round).  Every refusal condition of the planners holds with room to spare: h + c <= n - 2h is 3 <= 8
along dim 0, and no halo is wider than the interior.  Payloads are finite, so there is no tolerance anywhere."""
import itertools

import numpy as np
import pytest

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import accumulate_clear_bodies as ACB
from tests import fill_bodies as FLB
from tests import fold_bodies as FB
from tests import reflect_bodies as RB

pytestmark = pytest.mark.gpu

GDIMS, AXIS, HALO, PERIODS, PADDING = (12, 10, 8), 0, (2, 1, 1), (True, False, True), (0, 0, 0)
DTYPES = (cd.FLOAT, cd.DOUBLE_COMPLEX)
SLACK = FB.SLACK


class _Ctx:
    pass


def _families(c):
    """[(name, number of pencils, call(pointers, dim), definition(pencil bits, dim) in place)] in the order of the calls"""
    common = (c.dtype, HALO, PERIODS)
    one = [c.info]
    out = [
        ("update", 1, lambda p, d: cd.cudecompUpdateHalos(AXIS, c.h, c.gd, p[0], c.work, *common, d, PADDING, c.stream),
         lambda b, d: AB.update_reference(c.g, AXIS, HALO, PERIODS, d, one, [b])),
        ("accumulate", 1, lambda p, d: cd.cudecompAccumulateHalos(AXIS, c.h, c.gd, p[0], c.work, *common, d, PADDING, c.stream),
         lambda b, d: AB.accumulate_reference(c.g, AXIS, HALO, PERIODS, d, one, [b], c.add)),
        ("accumulate and clear", 1,
         lambda p, d: cd.cudecompAccumulateAndClearHalos(AXIS, c.h, c.gd, p[0], c.work, *common, d, PADDING, c.stream),
         lambda b, d: ACB.fused_reference(c.g, AXIS, HALO, PERIODS, d, one, [b], c.add)),
        ("fill", 1, lambda p, d: cd.cudecompFillHalos(AXIS, c.h, c.gd, p[0], *common, d, PADDING, c.value, c.stream),
         lambda b, d: FLB.fill_reference(c.g, 0, AXIS, HALO, PERIODS, d, c.info, b.view(np.uint8).reshape(-1, c.es), c.value)),
    ]
    for parity, centering in itertools.product((1, -1), (0, 1)):
        out.append(("reflect parity %+d centering %d" % (parity, centering), 1,
                    lambda p, d, s=parity, k=centering: cd.cudecompReflectHalos(AXIS, c.h, c.gd, p[0], c.dtype, s, k, HALO, PERIODS, d,
                                                                                PADDING, c.stream),
                    lambda b, d, s=parity, k=centering: RB.reflect_reference(c.info, b.view(np.uint8).reshape(-1, c.es), HALO, d, c.nb[d],
                                                                             s, k, AB.real_bytes(c.dtype))))
    for parity, centering, clear in itertools.product((1, -1), (0, 1), (0, 1)):
        out.append(("fold parity %+d centering %d clear %d" % (parity, centering, clear), 1,
                    lambda p, d, s=parity, k=centering, z=clear: cd.cudecompFoldHalos(AXIS, c.h, c.gd, p[0], c.dtype, s, k, z, HALO,
                                                                                      PERIODS, d, PADDING, c.stream),
                    lambda b, d, s=parity, k=centering, z=clear: FB.fold_reference(c.info, b, HALO, d, c.nb[d], s, k, z, c.dtype)))
    for n in (2, 3):
        out.append(("update of %d fields" % n, n,
                    lambda p, d: cd.cudecompUpdateFieldHalos(AXIS, c.h, c.gd, p, c.work, *common, d, PADDING, c.stream), out[0][3]))
    for clear in (0, 1):
        out.append(("accumulation of 2 fields clear %d" % clear, 2,
                    lambda p, d, z=clear: cd.cudecompAccumulateFieldHalos(AXIS, c.h, c.gd, p, c.work, *common, d, PADDING, bool(z),
                                                                          c.stream), out[1 + clear][3]))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=[AB.NAMES[t] for t in DTYPES])
def test_every_family_with_the_same_key_in_both_orders(dtype):
    import torch
    from tests import gpu_bodies as B
    c = _Ctx()
    c.h, c.gd, c.g = B._setup(0, 1, {"gdims": GDIMS, "pdims": (1, 1)})
    c.dtype, c.es = dtype, AB.element_bytes(dtype)
    c.info = c.g.pencil_info(0, AXIS, HALO, PADDING)
    assert c.info.as_dict() == cd.cudecompGetPencilInfo(c.h, c.gd, AXIS, HALO, PADDING).as_dict()
    c.nb = FB.neighbours_of(c.g, 0, AXIS, PERIODS)
    assert c.nb == [[True, True], [False, False], [True, True]]
    c.add = lambda x, y: AB.typed_add(dtype, x, y)  # noqa: E731  (bit patterns in, bit patterns out)
    c.value = FLB.value_bytes(c.es)
    c.stream = torch.cuda.current_stream().cuda_stream
    wsz = max(cd.cudecompGetHaloWorkspaceSize(c.h, c.gd, AXIS, HALO), 1)
    c.work = cd.cudecompMalloc(c.h, c.gd, 3 * wsz * c.es)  # (three fields at the most)
    start = [FB.start_pencil(c.info, dtype, 21 + f) for f in range(3)]
    families = _families(c)
    assert len(families) == 20
    calls = [(dim, i) for dim in range(3) for i in range(len(families))]
    want, failures = {}, []  # (the definitions: computed once, shared by both orders)
    for order, sequence in (("forward", calls), ("reversed", calls[::-1])):
        for dim, i in sequence:
            name, n, call, definition = families[i]
            if (dim, i) not in want:
                want[dim, i] = [b.copy() for b in start[:n]]
                for b in want[dim, i]:
                    definition(b, dim)
            dev = [torch.from_numpy(FB.guarded(b)).cuda() for b in start[:n]]
            call([t.data_ptr() + SLACK for t in dev], dim)
            kernel = cd.cudecompExtLastKernelName()
            torch.cuda.synchronize()
            for f in range(n):
                diff = FB.first_difference(dev[f].cpu().numpy(), FB.guarded(want[dim, i][f]), c.es)
                if diff:
                    failures.append("%s, %s order, dim %d, %s, field %d: %s; last kernel %s" % (AB.NAMES[dtype], order, dim, name, f, diff,
                                                                                               kernel))
    # the cases are not all no-ops of one another: the definitions of different families differ somewhere along every dim
    for dim in range(3):
        distinct = {want[dim, i][0].tobytes() for i in range(len(families))}
        assert len(distinct) >= 5, (dim, len(distinct))
    cd.cudecompFree(c.h, c.gd, c.work)
    cd.cudecompGridDescDestroy(c.h, c.gd)
    assert failures == []
