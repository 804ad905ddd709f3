"""Halo accumulation (cudecomp_amd.h: cudecompAmdAccumulateHalos{X,Y,Z}) without a GPU: the product's planner
(cudecompExtPlanHaloAccumulate, the buildHaloAccumulatePlan the executor runs) is asked for the plan of EVERY rank of randomly
drawn decompositions, the plans are executed on host arrays with numpy (add-moves add, the exchange is simulated by copying
the send slots into the neighbours' receive slots) and compared with the contract restated in tests/accumulate_bodies.py.

A note on "halo cells are only read".  The slabs of one call along `dim` span the other two dims INCLUDING their halos (that
is what folds edges and corners when dims 2, 1, 0 are called in turn), so the two faces a call adds into contain cells that
are halo cells of the OTHER dims, and those change.  What a call must leave alone is checked here after every call: every cell
outside its two faces -- all halo cells along `dim`, all padding cells, everything else; after the whole 2-1-0 sequence every
padding cell and every cell of the outermost halo layers no face ever covers hold what they held before (both follow from
the whole-pencil comparison with the restatement, and are asserted separately)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import cudecomp_amd as cd
from oracle import oracle as orc
from tests import accumulate_bodies as AB
from tests.half_bodies import global_index, halo_source_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMS = list(itertools.permutations((0, 1, 2)))
INVALID_USAGE, NOT_SUPPORTED = 1, 2
POISON = -10 ** 9


@st.composite
def decompositions(draw, max_ranks=12):
    # (the strategy of tests/test_plan_sim.py)
    pdims = draw(st.sampled_from([(a, b) for a in range(1, 7) for b in range(1, 7) if a * b <= max_ranks]))
    lo = max(pdims)  # no empty pencils: that case has its own test
    gdims = tuple(draw(st.integers(lo, lo + 9)) for _ in range(3))
    if draw(st.booleans()):
        mem_order = tuple(draw(st.sampled_from(PERMS)) for _ in range(3))
    else:
        ac = tuple(draw(st.booleans()) for _ in range(3))
        mem_order = tuple(tuple((ax + i) % 3 if ac[ax] else i for i in range(3)) for ax in range(3))
    gdims_dist = None
    if draw(st.booleans()):
        gdims_dist = tuple(draw(st.integers(max(lo, g - 3), g)) for g in gdims)
    return {"gdims": gdims, "pdims": pdims, "mem_order": mem_order, "gdims_dist": gdims_dist,
            "col_major": draw(st.booleans())}


small3 = st.tuples(st.integers(0, 2), st.integers(0, 2), st.integers(0, 2))


def _grids(d):
    spec = cd.make_grid_spec(d["gdims"], d["pdims"], d["mem_order"], d["gdims_dist"], d["col_major"])
    g = orc.Grid(d["gdims"], d["pdims"], gdims_dist=d["gdims_dist"], rank_order=2 if d["col_major"] else 1,
                 mem_order=d["mem_order"])
    return spec, g


def _view(buf, off, extent, strides):
    shape = tuple(int(e) for e in extent)[::-1]
    st_ = tuple(int(s) * buf.itemsize for s in strides)[::-1]
    return np.lib.stride_tricks.as_strided(buf[off:], shape=shape, strides=st_)


def _cells(m, off_key, st_key):
    k = np.indices(list(m.extent)).reshape(3, -1)
    s = list(getattr(m, st_key))
    return getattr(m, off_key) + k[0] * s[0] + k[1] * s[1] + k[2] * s[2]


def run_moves(moves, n, add_bits, bufs, ordered):
    """numpy execution of a plan's move list; add_bits: bit i = move i adds.  Two add-moves whose destinations share a cell
    must be marked `ordered` (the executor then launches them one by one, in list order -- which is what this loop does)."""
    live = [moves[i] for i in range(n) if 0 not in list(moves[i].extent)]
    if len(live) == 2 and live[0].dst_buf == live[1].dst_buf:
        shared = np.intersect1d(_cells(live[0], "dst_off", "ds"), _cells(live[1], "dst_off", "ds")).size
        assert shared == 0 or ordered, "two moves of one phase write the same cells and the plan does not say so"
    for i in range(n):
        m = moves[i]
        if 0 in list(m.extent):
            continue
        src = _view(bufs[m.src_buf], m.src_off, m.extent, m.ss).copy()
        dst = _view(bufs[m.dst_buf], m.dst_off, m.extent, m.ds)
        if (add_bits >> i) & 1:
            assert m.dst_buf == 0 and m.row_pitch == 0, "an add-move targets the pencil and never claims the cells between rows"
            dst[...] += src
        else:
            dst[...] = src


def execute(plans, data, work, wsz):
    """every rank's plan: pre, the flights of the exchange (send slot i -> neighbour i's receive slot 1 - i), post"""
    n = len(plans)
    for r in range(n):
        p = plans[r]
        assert p.kind in (0, 1, 2), "accumulation plans are never direct"
        if p.kind == 0:
            assert p.n_pre == 0 and p.n_post == 0
            continue
        assert p.reserved & 1, "not marked as an accumulation plan"
        if p.kind == 1:
            assert p.n_pre == 2 and p.n_post == 0 and (p.reserved >> 4) & 3 == 3, "wrap onto myself: two add-moves"
        else:
            assert (p.reserved >> 4) & 3 == 0 and (p.reserved >> 6) & 3 == (1 << p.n_post) - 1, "packs copy, what arrived is added"
            assert p.xbuf == 2, "accumulation always exchanges through the workspace"
            for i in range(2):  # workspace bounds (cudecompGetHaloWorkspaceSize covers four aligned faces)
                assert 0 <= p.send_off[i] and p.send_off[i] + p.face_elements <= wsz[r]
                assert 0 <= p.recv_off[i] and p.recv_off[i] + p.face_elements <= wsz[r]
        run_moves(p.pre, p.n_pre, (p.reserved >> 4) & 3, [data[r], data[r], work[r]], bool(p.reserved & 2))
    flights = []
    for r in range(n):
        p = plans[r]
        if p.kind != 2:
            continue
        for i in range(2):
            nb = p.neighbor[i]
            if nb < 0:
                continue
            q = plans[nb]
            assert q.kind == 2 and q.neighbor[1 - i] == r and q.face_elements == p.face_elements
            flights.append((nb, q.recv_off[1 - i], work[r][p.send_off[i]:p.send_off[i] + p.face_elements].copy()))
    for nb, off, face in flights:
        assert not (face == POISON).any(), "a send slot travels with cells nobody packed"
        work[nb][off:off + face.size] = face
    for r in range(n):
        p = plans[r]
        if p.kind == 2:
            run_moves(p.post, p.n_post, (p.reserved >> 6) & 3, [data[r], data[r], work[r]], bool(p.reserved & 2))


def simulate_accumulate(d, axis, halo, periods, padding, force_packed, seed):
    """dims 2, 1, 0 in turn on every rank; None if the planner refuses the configuration (INVALID_USAGE / NOT_SUPPORTED)"""
    spec, g = _grids(d)
    n = g.nranks
    infos = [g.pencil_info(r, axis, halo, padding) for r in range(n)]
    wsz = [max(g.halo_workspace_size(r, axis, halo), 1) for r in range(n)]
    for r in range(n):
        assert cd.cudecompExtWorkspaceSizes(spec, r, axis, halo)[1] == g.halo_workspace_size(r, axis, halo)
    init = [AB.initial_cells(seed, r, axis, infos[r].size, 1).reshape(-1) for r in range(n)]  # 0..7 in EVERY cell
    data = [a.copy() for a in init]
    want = [a.copy().reshape(-1, 1) for a in init]
    for dim in (2, 1, 0):
        try:
            plans = [cd.cudecompExtPlanHaloAccumulate(spec, r, axis, halo, periods, dim, padding, force_packed) for r in range(n)]
        except cd.CudecompError as e:
            assert e.code in (INVALID_USAGE, NOT_SUPPORTED), e.code
            return None
        before = [a.copy() for a in data]
        work = [np.full(wsz[r], POISON, dtype=np.int64) for r in range(n)]  # poisoned for every call
        execute(plans, data, work, wsz)
        AB.accumulate_reference(g, axis, halo, periods, dim, infos, want)
        for r in range(n):
            assert np.array_equal(data[r], want[r].reshape(-1)), "rank %d differs from the restatement after dim %d" % (r, dim)
            # (b) per call: every cell outside the call's two faces holds what it held
            faces = np.zeros(int(infos[r].size), dtype=bool)
            if halo[dim]:
                for which in ("LF", "HF"):
                    AB.pencil3(infos[r], faces)[AB.slab(infos[r], dim, which, halo[dim])] = True
            assert np.array_equal(data[r][~faces], before[r][~faces]), "rank %d dim %d: a cell outside the two faces changed" % (r, dim)
    # (a) interior cells: own value + the values of all ghost cells, on any rank, that the updates along 0, 1, 2 fill from them
    ncells = d["gdims"][0] * d["gdims"][1] * d["gdims"][2]
    total = np.zeros(ncells, dtype=np.int64)
    for r in range(n):
        src = halo_source_index(infos[r], d["gdims"], periods)
        ghost = (src >= 0) & (global_index(infos[r], d["gdims"]) < 0)
        np.add.at(total, src[ghost], init[r][ghost])
    for r in range(n):
        gi = global_index(infos[r], d["gdims"])
        inside = gi >= 0
        assert np.array_equal(data[r][inside], init[r][inside] + total[gi[inside]]), "rank %d: interior closed form" % r
        # (b) after the sequence: padding cells, and the cells no face of any call covers
        p = infos[r]
        shape, never = [int(x) for x in p.shape], np.ones(int(p.size), dtype=bool)
        pad = np.zeros(int(p.size), dtype=bool)
        l = np.arange(int(p.size))
        for k in range(3):
            o = int(p.order[k])
            lk = l // int(np.prod(shape[:k], dtype=np.int64)) % shape[k]
            pad |= lk >= shape[k] - int(p.padding[o])
        for dim in range(3):
            if halo[dim]:
                for which in ("LF", "HF"):
                    AB.pencil3(p, never)[AB.slab(p, dim, which, halo[dim])] = False
        assert np.array_equal(data[r][pad], init[r][pad]), "rank %d: a padding cell changed" % r
        assert np.array_equal(data[r][never], init[r][never]), "rank %d: a cell outside every face changed" % r
    adjoint_identity(d, spec, g, axis, halo, periods, padding, force_packed, infos, wsz, seed)
    return True


def adjoint_identity(d, spec, g, axis, halo, periods, padding, force_packed, infos, wsz, seed):
    """(c) <U x, y> over all cells == <x, A y> over interior cells, x zero outside the interior, U = the product's own UPDATE
    plans (cudecompExtPlanHalo) along 0, 1, 2 executed the same way, A = the accumulation plans along 2, 1, 0"""
    n = g.nranks
    rng = np.random.default_rng([seed, 99])
    inside = [global_index(infos[r], d["gdims"]) >= 0 for r in range(n)]
    x = [np.where(inside[r], rng.integers(1, 8, size=int(infos[r].size)), 0).astype(np.int64) for r in range(n)]
    y = [rng.integers(0, 8, size=int(infos[r].size)).astype(np.int64) for r in range(n)]
    ux, ay = [a.copy() for a in x], [a.copy() for a in y]
    for dim in (0, 1, 2):
        plans = [cd.cudecompExtPlanHalo(spec, r, axis, halo, periods, dim, padding, force_packed) for r in range(n)]
        work = [np.full(wsz[r], POISON, dtype=np.int64) for r in range(n)]
        for r in range(n):
            if plans[r].kind != 0:
                run_moves(plans[r].pre, plans[r].n_pre, 0, [ux[r], ux[r], work[r]], True)
        flights = []
        for r in range(n):
            p = plans[r]
            if p.kind in (0, 1):
                continue
            src = [ux[r], ux[r], work[r]][p.xbuf]
            for i in range(2):
                nb = p.neighbor[i]
                if nb >= 0:
                    q = plans[nb]
                    flights.append((nb, q.xbuf, q.recv_off[1 - i], src[p.send_off[i]:p.send_off[i] + p.face_elements].copy()))
        for nb, xbuf, off, face in flights:
            [ux[nb], ux[nb], work[nb]][xbuf][off:off + face.size] = face
        for r in range(n):
            if plans[r].kind != 0:
                run_moves(plans[r].post, plans[r].n_post, 0, [ux[r], ux[r], work[r]], True)
    for dim in (2, 1, 0):
        plans = [cd.cudecompExtPlanHaloAccumulate(spec, r, axis, halo, periods, dim, padding, force_packed) for r in range(n)]
        work = [np.full(wsz[r], POISON, dtype=np.int64) for r in range(n)]
        execute(plans, ay, work, wsz)
    lhs = sum(int(np.dot(ux[r], y[r])) for r in range(n))
    rhs = sum(int(np.dot(x[r][inside[r]], ay[r][inside[r]])) for r in range(n))
    assert lhs == rhs, "<U x, y> = %d but <x, A y> = %d" % (lhs, rhs)


def test_accumulate_plans_random_decompositions():
    """Plans of every rank, dims 2, 1, 0, poisoned workspaces, 0..7 in every cell: (a) the interior closed form, (b) what must
    not change does not, (c) the adjoint identity against the product's update plans.  A drawn configuration is dropped only
    when the planner refuses it (INVALID_USAGE / NOT_SUPPORTED); more than a third dropped fails the test."""
    seen = {"examples": 0, "dropped": 0}

    @settings(max_examples=200, deadline=None, suppress_health_check=list(HealthCheck), database=None)
    @given(d=decompositions(), axis=st.integers(0, 2), halo=small3, periods=st.tuples(st.booleans(), st.booleans(), st.booleans()),
           padding=small3, force_packed=st.booleans(), seed=st.integers(0, 2 ** 31))
    def run(d, axis, halo, periods, padding, force_packed, seed):
        seen["examples"] += 1
        if simulate_accumulate(d, axis, halo, periods, padding, force_packed, seed) is None:
            seen["dropped"] += 1

    run()
    print("halo accumulation plans: %d examples, %d refused by the planner" % (seen["examples"], seen["dropped"]))
    assert seen["examples"] >= 100
    assert 3 * seen["dropped"] <= seen["examples"], seen


def test_small_interiors_keep_the_stated_order():
    # interior narrower than two halos: the faces overlap, the plan says so, low face first
    d = {"gdims": (3, 5, 4), "pdims": (1, 1), "mem_order": ((0, 1, 2),) * 3, "gdims_dist": None, "col_major": False}
    spec, _ = _grids(d)
    p = cd.cudecompExtPlanHaloAccumulate(spec, 0, 0, (2, 2, 2), (True, True, True), 0, None, False)
    assert p.kind == 1 and p.reserved & 2
    p = cd.cudecompExtPlanHaloAccumulate(spec, 0, 0, (1, 2, 2), (True, True, True), 0, None, False)
    assert p.kind == 1 and not p.reserved & 2
    assert simulate_accumulate(d, 0, (2, 2, 2), (True, True, True), (1, 0, 2), False, 3) is True
    d4 = dict(d, gdims=(6, 6, 6), pdims=(2, 2))
    assert simulate_accumulate(d4, 1, (2, 2, 2), (True, False, True), (0, 1, 0), True, 4) is True


def test_refusals_and_empty_plans():
    order = ((0, 1, 2),) * 3
    one = cd.make_grid_spec((4, 6, 6), (1, 1), order)

    def code(call):
        with pytest.raises(cd.CudecompError) as e:
            call()
        return e.value.code

    # wider than my own interior along a dim that wraps onto myself
    assert code(lambda: cd.cudecompExtPlanHaloAccumulate(one, 0, 0, (5, 0, 0), (True, True, True), 0)) == INVALID_USAGE
    assert cd.cudecompExtPlanHaloAccumulate(one, 0, 0, (4, 0, 0), (True, True, True), 0).kind == 1
    # wider than a neighbour's slab (the update's message and code)
    four = cd.make_grid_spec((4, 4, 4), (2, 2), order)
    assert code(lambda: cd.cudecompExtPlanHaloAccumulate(four, 0, 0, (0, 3, 0), (True, True, True), 1)) == INVALID_USAGE
    assert cd.cudecompExtPlanHaloAccumulate(four, 0, 0, (0, 2, 0), (True, True, True), 1).kind == 2
    uneven = cd.make_grid_spec((4, 7, 4), (3, 1), order)  # Y split 3 + 2 + 2 for X pencils
    assert code(lambda: cd.cudecompExtPlanHaloAccumulate(uneven, 0, 0, (0, 3, 0), (False, False, False), 1)) == INVALID_USAGE
    # empty pencils
    empty = cd.make_grid_spec((3, 8, 8), (4, 1), order)
    assert code(lambda: cd.cudecompExtPlanHaloAccumulate(empty, 0, 1, (1, 1, 1), (True, True, True), 0)) == NOT_SUPPORTED
    # nothing to do: h == 0, no neighbour at all
    assert cd.cudecompExtPlanHaloAccumulate(four, 0, 0, (1, 0, 1), (True, True, True), 1).kind == 0
    assert cd.cudecompExtPlanHaloAccumulate(one, 0, 0, (1, 1, 1), (False, False, False), 2).kind == 0
    p = cd.cudecompExtPlanHaloAccumulate(four, 0, 0, (1, 1, 1), (False, False, False), 1)  # an edge rank: one side only
    assert p.kind == 2 and sorted(p.neighbor) [0] == -1 and p.n_pre == 1 and p.n_post == 1
    # update plans are untouched: no accumulation marks
    assert cd.cudecompExtPlanHalo(four, 0, 0, (1, 1, 1), (True, True, True), 1).reserved == 0


def test_entry_points_check_their_arguments_like_the_updates():
    L = cd.lib()
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((9, 10, 11), (1, 1)))
    i3 = (C.c_int32 * 3)
    for name in cd.AMD_SYMBOLS:
        fn, up = getattr(L, name), getattr(L, name.replace("AmdAccumulate", "Update"))
        for args in ((h, gd, 1, 1, cd.FLOAT, None, None, 0, None, None), (h, gd, None, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),
                     (h, gd, 1, None, cd.FLOAT, i3(1, 1, 1), None, 0, None, None), (h, gd, 1, 1, cd.FLOAT, i3(1, 1, 1), None, 3, None, None),
                     (h, gd, 1, 1, 99, i3(1, 1, 1), None, 0, None, None), (h, None, 1, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None),
                     (h, gd, None, None, cd.FLOAT, i3(0, 0, 0), None, 0, None, None),
                     (h, gd, 1, 1, cd.FLOAT, i3(1, 1, 1), None, 0, None, None)):  # (non-periodic single rank: nothing to do)
            assert fn(*args) == up(*args), (name, args)
    # wider than the interior: refused before any device work
    assert L.cudecompAmdAccumulateHalosX(h, gd, 8, 8, cd.DOUBLE, i3(10, 0, 0), (C.c_bool * 3)(True, True, True), 0, None, None) == cd.RESULT_INVALID_USAGE
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


def test_header_declares_and_library_exports_the_symbols():
    src = open(os.path.join(ROOT, "include", "cudecomp_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cudecomp\w+)\s*\(", src))
    assert declared == set(cd.AMD_SYMBOLS) == {"cudecompAmdAccumulateHalos" + a for a in "XYZ"}
    L = cd.lib()
    for name in sorted(declared) + ["cudecompExtPlanHaloAccumulate", "cudecompExtAccumulate3D"]:
        assert hasattr(L, name), name
    ext = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cudecomp_ext.h")).read(), flags=re.S)
    assert "cudecompExtPlanHaloAccumulate" in ext and "cudecompExtAccumulate3D" in ext


def test_arguments_are_checked_in_the_stated_order(capfd):
    from tests import halo_check_order
    halo_check_order.check("accumulate", capfd)
