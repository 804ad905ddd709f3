"""Multi-field halo accumulation (cudecomp_halo_accumulate_fields.h: cudecompAmdAccumulateFieldHalos{X,Y,Z}): the per-rank bodies of
tests/test_gpu_halo_accumulate_fields.py and the gloo body of tests/test_halo_accumulate_fields_plan.py.  The oracle of the pencil
tests is the single call: every field after the fields call against a clone of it after cudecompAmdAccumulateHalos{X,Y,Z} (clear
== 0) or cudecompAmdAccumulateAndClearHalos{X,Y,Z} (clear == 1) with the same remaining arguments.  Whole buffers, byte for byte;
there is no tolerance anywhere.

Payload of the pencil tests (the "bit arm"): finite non-integer reals of the element type in every cell (AB.typed_cells: every sum
rounds), with -0, subnormals and +infinity sprinkled in and no NaN -- infinities of ONE sign only, because inf + -inf would make a
NaN and which NaN comes out is unspecified by cudecomp_amd.h."""
import ctypes as C
import itertools

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests.fields_bodies import _Work

PRE_ADD, POST_ADD, PRE_TAKE, ORDERED = 16, 64, 1024, 2  # bits of the plans' `reserved` word (cudecomp_ext.h)


def field_bytes(p, dtype, seed):
    """uint8 (cells * es): the bit arm's payload for one field"""
    nc = AB.TYPES[dtype][1]
    kind = AB.kind_of(dtype)
    u, m, e = AB.FORMATS[kind]
    bits = AB.bits_of(dtype, AB.typed_cells(dtype, seed, 0, 0, int(p.size), nc)).copy().reshape(-1)
    rng = np.random.default_rng([int(seed), 91])
    pick = rng.integers(0, 16, bits.size)
    sign = u(1 << (m + e))
    special = {0: sign, 1: u(1), 2: u((1 << m) - 1) | sign, 3: u(((1 << e) - 1) << m)}  # -0, smallest subnormal, -largest subnormal, +inf
    for k, pattern in special.items():
        bits[pick == k] = pattern
    assert not AB.classes(kind, bits)["nan"].any()
    return bits.view(np.uint8).reshape(-1)


def _fields(p, dtype, n, seed):
    import torch
    return [torch.from_numpy(field_bytes(p, dtype, seed * 1009 + f * 7919 + 1)).cuda() for f in range(n)]


def _single(clear, axis, h, gd, ptr, work, dtype, halo, periods, dim, padding, stream):
    (cd.cudecompAccumulateAndClearHalos if clear else cd.cudecompAccumulateHalos)(axis, h, gd, ptr, work, dtype, halo, periods, dim,
                                                                                   padding, stream)


def fields_sweep(rank, nranks, args):
    """cudecompAmdAccumulateFieldHalos for every axis of args["axes"], type of args["dtypes"], field count of args["n_fields"], both
    values of `clear` and every dim (args["all_dims"]: also dims 2, 1, 0 in turn on one set of fields: edges and corners) against
    single calls on clones.  args["guard"]: the workspace holds exactly n x the queried size inside a poisoned buffer, and nothing
    outside it changes.  args["launches"]: {"self": a, "packed": b} -- the data-movement launches one fields call makes, by the kind
    of its plan; one more where the plan is ordered.  args["expect_ordered"]: some plan of the sweep must be ordered."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    stream = torch.cuda.current_stream().cuda_stream
    spec = cd.make_grid_spec(args["gdims"], args["pdims"], [[int(x) for x in g.pencil_info(rank, a).order] for a in range(3)],
                             gdims_dist=args.get("gdims_dist"))
    self_exchange = bool(args.get("self_exchange"))
    failures = []
    seen_kernels, ordered_seen = set(), False
    for axis in args.get("axes", [0, 1, 2]):
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        info = g.pencil_info(rank, axis, halo, padding)
        if info.as_dict() != p.as_dict():
            failures.append("rank %d axis %d: pencil info differs from the oracle" % (rank, axis))
            continue
        wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
        for dtype in args.get("dtypes", [cd.DOUBLE]):
            es = AB.element_bytes(dtype)
            single = _Work(h, gd, wsz * es, False)
            for n, clear in itertools.product(args.get("n_fields", [3]), args.get("clear", [0, 1])):
                work = _Work(h, gd, n * wsz * es, bool(args.get("guard")))
                for dims in [(0,), (1,), (2,)] + ([(2, 1, 0)] if args.get("all_dims") else []):
                    got = _fields(info, dtype, n, (rank * 3 + axis) * 64 + n)
                    want = [t.clone() for t in got]
                    for dim in dims:
                        before = cd.cudecompExtDataLaunchCount()
                        cd.cudecompAccumulateFieldHalos(axis, h, gd, [t.data_ptr() for t in got], work.ptr, dtype, halo, periods, dim,
                                                        padding, clear, stream)
                        made = cd.cudecompExtDataLaunchCount() - before
                        name = cd.cudecompExtLastKernelName()
                        plan = cd.cudecompExtPlanHaloAccumulateFields(spec, rank, axis, halo, periods, dim, padding, n, clear, self_exchange)
                        ordered = bool(plan.reserved & ORDERED)
                        ordered_seen = ordered_seen or (ordered and plan.kind != 0)
                        if plan.kind != 0 and n >= 2:
                            seen_kernels.add(name.split("<")[0])
                            if "_fields_accumulate_kernel<" not in name:  # (the last launch of a call always adds)
                                failures.append("rank %d axis %d dim %d n %d: the last kernel was %s" % (rank, axis, dim, n, name))
                            if not name.endswith(",true>" if clear and plan.kind == 1 else ",false>"):
                                failures.append("rank %d axis %d dim %d n %d clear %d kind %d: the last kernel was %s" %
                                                (rank, axis, dim, n, clear, plan.kind, name))
                        if args.get("launches") and plan.kind != 0 and n >= 2:
                            expect = args["launches"]["self" if plan.kind == 1 else "packed"] + (1 if ordered else 0)
                            if made != expect:
                                failures.append("rank %d axis %d dim %d n %d clear %d: %d data-movement launches, expected %d" %
                                                (rank, axis, dim, n, clear, made, expect))
                        for t in want:
                            _single(clear, axis, h, gd, t.data_ptr(), single.ptr, dtype, halo, periods, dim, padding, stream)
                    torch.cuda.synchronize()
                    for f in range(n):
                        if not torch.equal(got[f], want[f]):
                            bad = torch.nonzero(got[f] != want[f]).reshape(-1)
                            failures.append("rank %d axis %d %s halo %s periods %s padding %s dims %s n %d clear %d field %d: %d bytes "
                                            "differ, first in cell %d" % (rank, axis, AB.NAMES[dtype], tuple(halo), tuple(periods),
                                                                          tuple(padding), dims, n, clear, f, bad.numel(), int(bad[0]) // es))
                    if not work.outside_untouched():
                        failures.append("rank %d axis %d dims %s n %d: bytes outside the workspace changed" % (rank, axis, dims, n))
                work.free()
            single.free()
    if args.get("expect_kernels") and not seen_kernels:
        failures.append("rank %d: no accumulating fields kernel ran at all" % rank)
    if args.get("expect_ordered") and not ordered_seen:
        failures.append("rank %d: no plan of the sweep was ordered" % rank)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def one_field_is_the_single_call(rank, nranks, args):
    """n_fields = 1: the same bytes, the same last kernel and the same number of launches as the single call"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for axis in range(3):
        info = g.pencil_info(rank, axis, halo, padding)
        for dtype in args.get("dtypes", [cd.DOUBLE]):
            es = AB.element_bytes(dtype)
            work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * es)
            for dim, clear in itertools.product(range(3), (0, 1)):
                got = _fields(info, dtype, 1, axis)[0]
                want = got.clone()
                c0 = cd.cudecompExtDataLaunchCount()
                cd.cudecompAccumulateFieldHalos(axis, h, gd, [got.data_ptr()], work, dtype, halo, periods, dim, padding, clear, stream)
                a, c1 = cd.cudecompExtLastKernelName(), cd.cudecompExtDataLaunchCount()
                _single(clear, axis, h, gd, want.data_ptr(), work, dtype, halo, periods, dim, padding, stream)
                b, c2 = cd.cudecompExtLastKernelName(), cd.cudecompExtDataLaunchCount()
                torch.cuda.synchronize()
                if a != b or "_fields_" in a or c1 - c0 != c2 - c1 or not torch.equal(got, want):
                    failures.append("axis %d %s dim %d clear %d: kernels %s / %s, launches %d / %d, equal bytes: %s" %
                                    (axis, AB.NAMES[dtype], dim, clear, a, b, c1 - c0, c2 - c1, torch.equal(got, want)))
            cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def adjoint(rank, nranks, args):
    """single rank, periodic: sum over ALL cells of (U x) * y == sum over INTERIOR cells of x * (A y), field by field, x zero outside
    the interior, U = the multi-field update along 0, 1, 2, A = this call along 2, 1, 0; small integers, exact in fp64"""
    import torch
    from tests import gpu_bodies as B
    from tests.half_bodies import global_index
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding, n = args["halo"], args["periods"], args.get("padding", (0, 0, 0)), args.get("n", 3)
    stream = torch.cuda.current_stream().cuda_stream
    failures = []
    for axis in range(3):
        p = g.pencil_info(rank, axis, halo, padding)
        inside = global_index(p, g.gdims) >= 0
        rng = np.random.default_rng(11 + axis)
        xs = [np.where(inside, rng.integers(1, 8, size=int(p.size)), 0).astype(np.float64) for _ in range(n)]
        ys = [rng.integers(0, 8, size=int(p.size)).astype(np.float64) for _ in range(n)]
        work = cd.cudecompMalloc(h, gd, n * max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1) * 8)
        ux, ay = [torch.from_numpy(x).cuda() for x in xs], [torch.from_numpy(y).cuda() for y in ys]
        for dim in (0, 1, 2):
            cd.cudecompUpdateFieldHalos(axis, h, gd, [t.data_ptr() for t in ux], work, cd.DOUBLE, halo, periods, dim, padding, stream)
        for dim in (2, 1, 0):
            cd.cudecompAccumulateFieldHalos(axis, h, gd, [t.data_ptr() for t in ay], work, cd.DOUBLE, halo, periods, dim, padding, 0, stream)
        torch.cuda.synchronize()
        for f in range(n):
            lhs = float(np.dot(ux[f].cpu().numpy(), ys[f]))
            rhs = float(np.dot(xs[f][inside], ay[f].cpu().numpy()[inside]))
            if lhs != rhs or lhs == 0.0:
                failures.append("axis %d field %d: <U x, y> = %r but <x, A y> = %r" % (axis, f, lhs, rhs))
        cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def graph_replay(rank, nranks, args):
    """One fields call with three fields captured on a side stream after an eager warm-up (the host array of pointers is a
    temporary that is gone before the replay); two replays on refilled fields at the same addresses, each against single calls"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    axis, dim, dtype, n, clear = args.get("axis", 0), args.get("dim", 1), args.get("dtype", cd.DOUBLE), 3, int(args.get("clear", 0))
    es = AB.element_bytes(dtype)
    info = g.pencil_info(rank, axis, halo, padding)
    wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
    work = cd.cudecompMalloc(h, gd, n * wsz * es)
    single = cd.cudecompMalloc(h, gd, wsz * es)
    fn = getattr(cd.lib(), "cudecompAmdAccumulateFieldHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    fields = _fields(info, dtype, n, 5)

    def call(sptr):
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in fields])
        rc = fn(h, gd, ptrs, n, work, dtype, i3(*halo), b3(*[bool(x) for x in periods]), dim, i3(*padding), clear, sptr)
        assert rc == cd.RESULT_SUCCESS, rc
        for i in range(n):
            ptrs[i] = None  # the caller's array changes after the call

    failures = []
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call(stream.cuda_stream)  # warm-up
        stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream, capture_error_mode="thread_local"):
        call(torch.cuda.current_stream().cuda_stream)
    for it in range(2):
        fresh = _fields(info, dtype, n, 100 + it)
        want = [t.clone() for t in fresh]
        with torch.cuda.stream(stream):
            for t, src in zip(fields, fresh):
                t.copy_(src)
            graph.replay()
            for t in want:
                _single(clear, axis, h, gd, t.data_ptr(), single, dtype, halo, periods, dim, padding, stream.cuda_stream)
            stream.synchronize()
        for f in range(n):
            if not torch.equal(fields[f], want[f]) or torch.equal(fields[f], fresh[f]):
                failures.append("replay %d field %d differs from the single call (or nothing changed)" % (it, f))
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompFree(h, gd, single)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


# ---- numpy execution of the plans (no GPU) ---------------------------------------------------------------------------------------
def run_phase(moves, n, add_bits, take_bits, bufs):
    """the moves of one phase in list order: dst = src or dst += src (bit i of add_bits), then src = 0 (bit i of take_bits)"""
    from tests.bodies import _view
    for i in range(n):
        m = moves[i]
        if 0 in list(m.extent):
            continue
        src = _view(bufs[m.src_buf], m.src_off, m.extent, m.ss)
        dst = _view(bufs[m.dst_buf], m.dst_off, m.extent, m.ds)
        held = src.copy()
        if add_bits >> i & 1:
            dst[...] += held
        else:
            dst[...] = held
        if take_bits >> i & 1:
            src[...] = 0


def _run_plan_phase(plan, post, field, work, shift):
    """the pre (post) moves of field 0 carried out for the field whose pieces lie `shift` elements further into the workspace"""
    r = plan.reserved
    if post:
        run_phase(plan.post, plan.n_post, r // POST_ADD & 3, 0, [field, field, work[shift:]])
    else:
        run_phase(plan.pre, plan.n_pre, r // PRE_ADD & 3, r // PRE_TAKE & 3, [field, field, work[shift:]])


def plan_gloo(rank, nranks, args):
    """The stateless plan (cudecompExtPlanHaloAccumulateFields) executed with numpy block moves and a real multi-process exchange
    over gloo -- ONE message of n slabs per direction -- against the single plans (cudecompExtPlanHaloAccumulate /
    cudecompExtPlanHaloAccumulateClear) executed field by field with their own exchanges.  int16 payload of small integers; every
    axis, dims 2, 1, 0 in sequence on one set of fields, both values of `clear`; no GPU."""
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=nranks)
    gdims, pdims, padding = args["gdims"], args["pdims"], args["padding"]
    from oracle import oracle as orc
    g = orc.Grid(gdims, pdims)
    spec = cd.make_grid_spec(gdims, pdims, [[int(x) for x in g.pencil_info(rank, a).order] for a in range(3)])
    failures = []
    ran = 0

    def exchange(plan, work, count):
        """send slot i -> neighbour i's receive slot 1 - i, `count` elements; the tag names the receiving slot"""
        reqs, landing = [], []
        for i in range(2):
            if plan.neighbor[i] < 0:
                continue
            t = torch.zeros(count, dtype=torch.int16)
            reqs.append(dist.irecv(t, plan.neighbor[i], tag=i))
            landing.append((t, plan.recv_off[i]))
        for i in range(2):
            if plan.neighbor[i] < 0:
                continue
            s = torch.from_numpy(work[plan.send_off[i]:plan.send_off[i] + count].copy())
            reqs.append(dist.isend(s, plan.neighbor[i], tag=1 - i))
        for r in reqs:
            r.wait()
        for t, off in landing:
            work[off:off + count] = t.numpy()

    for halo, periods, clear in itertools.product(args["halos"], args["periods"], (0, 1)):
        single_planner = cd.cudecompExtPlanHaloAccumulateClear if clear else cd.cudecompExtPlanHaloAccumulate
        for axis, n in itertools.product(range(3), args["n_fields"]):
            info = g.pencil_info(rank, axis, halo, padding)
            ws = max(cd.cudecompExtWorkspaceSizes(spec, rank, axis, halo)[1], 1)
            rng = np.random.RandomState(1000 * rank + 10 * axis + n)
            got = [rng.randint(-8, 9, size=int(info.size)).astype(np.int16) for _ in range(n)]
            want = [a.copy() for a in got]
            work = np.full(n * ws, 0x5EAD, dtype=np.int16)
            single_work = np.full(ws, 0x3EEF, dtype=np.int16)
            for dim in (2, 1, 0):
                # a refusal concerns some ranks only: every rank works that out for all ranks, and all of them leave the dim out
                refused = []
                for r in range(nranks):
                    codes = []
                    for planner, more in ((single_planner, (True,)), (cd.cudecompExtPlanHaloAccumulateFields, (n, clear))):
                        try:
                            planner(spec, r, axis, halo, periods, dim, padding, *more)
                            codes.append(0)
                        except cd.CudecompError as e:
                            codes.append(e.code)
                    if codes[0] != codes[1]:
                        failures.append("rank %d axis %d dim %d n %d: single plan result %d, fields plan result %d" % ((r, axis, dim, n) + tuple(codes)))
                    refused.append(codes[0] != 0 or codes[1] != 0)
                if any(refused):
                    continue
                fp = cd.cudecompExtPlanHaloAccumulateFields(spec, rank, axis, halo, periods, dim, padding, n, clear)
                sp = single_planner(spec, rank, axis, halo, periods, dim, padding, True)
                if fp.kind not in (0, 1, 2):
                    failures.append("fields plan of kind %d" % fp.kind)
                if fp.kind != 0:
                    ran += 1
                    for f in range(n):
                        _run_plan_phase(fp, False, got[f], work, f * fp.face_elements)
                    if fp.kind == 2:
                        exchange(fp, work, n * fp.face_elements)
                        for f in range(n):
                            _run_plan_phase(fp, True, got[f], work, f * fp.face_elements)
                if sp.kind != 0:
                    for f in range(n):
                        _run_plan_phase(sp, False, want[f], single_work, 0)
                        if sp.kind == 2:
                            exchange(sp, single_work, sp.face_elements)
                            _run_plan_phase(sp, True, want[f], single_work, 0)
                for f in range(n):
                    if not np.array_equal(got[f], want[f]):
                        failures.append("rank %d halo %s periods %s clear %d axis %d n %d dim %d field %d: %d cells differ" %
                                        (rank, halo, periods, clear, axis, n, dim, f, int((got[f] != want[f]).sum())))
    if ran == 0:
        failures.append("rank %d: no plan had anything to do" % rank)
    dist.destroy_process_group()
    return failures


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out
