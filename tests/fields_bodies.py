"""Multi-field halo updates (cudecomp_halo_fields.h: cudecompAmdUpdateFieldHalos{X,Y,Z}): the per-rank bodies of
tests/test_gpu_halo_fields.py.  The oracle is the single call: every field after the fields call against a clone of it after
cudecompUpdateHalos{X,Y,Z} with the same remaining arguments.  Whole buffers, byte for byte; there is no tolerance anywhere.

Payload: every byte of every field drawn at random (another seed per field, rank and axis: a face that lands in the wrong field
or the wrong rank shows), the poison byte in the padding cells."""
import ctypes as C
import itertools

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB

POISON = 0x5C
GUARD = 256  # poison bytes before and after a workspace that is allocated at exactly its size


def field_bytes(p, es, seed):
    """uint8 (cells * es): random bytes, the poison in the padding cells of pencil `p`"""
    rng = np.random.RandomState(seed % (1 << 31))
    cells = rng.randint(0, 256, size=(int(p.size), es)).astype(np.uint8)
    inside = np.zeros(int(p.size), dtype=bool)
    AB.pencil3(p, inside)[tuple(slice(0, int(p.shape[k]) - int(p.padding[int(p.order[k])])) for k in (2, 1, 0))] = True
    cells[~inside] = POISON
    return cells.reshape(-1)


def _fields(p, es, n, seed):
    import torch
    return [torch.from_numpy(field_bytes(p, es, seed * 1009 + f * 7919 + 1)).cuda() for f in range(n)]


class _Work:
    """n single workspaces: from cudecompMalloc, or (guard) at exactly that size inside a larger poisoned torch buffer"""

    def __init__(self, h, gd, nbytes, guard):
        import torch
        self.h, self.gd, self.guard, self.nbytes = h, gd, guard, nbytes
        if guard:
            self.buf = torch.full((nbytes + 2 * GUARD,), POISON, dtype=torch.uint8, device="cuda")
            self.ptr = self.buf.data_ptr() + GUARD
        else:
            self.ptr = cd.cudecompMalloc(h, gd, nbytes)

    def outside_untouched(self):
        import torch
        if not self.guard:
            return True
        return bool(torch.all(self.buf[:GUARD] == POISON)) and bool(torch.all(self.buf[GUARD + self.nbytes:] == POISON))

    def free(self):
        if not self.guard:
            cd.cudecompFree(self.h, self.gd, self.ptr)


def fields_sweep(rank, nranks, args):
    """cudecompAmdUpdateFieldHalos for every axis of args["axes"], type of args["dtypes"], field count of args["n_fields"] and dim
    (args["all_dims"]: also dims 0, 1, 2 in turn on one set of fields: edges and corners) against single calls on clones.
    args["guard"]: the workspace holds exactly n x the queried size inside a poisoned buffer, and nothing outside it changes.
    args["launches"]: {"self": a, "packed": b} -- the data-movement launches one fields call makes, by the kind of its plan."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    stream = torch.cuda.current_stream().cuda_stream
    spec = cd.make_grid_spec(args["gdims"], args["pdims"], [[int(x) for x in g.pencil_info(rank, a).order] for a in range(3)],
                             gdims_dist=args.get("gdims_dist"))
    failures = []
    seen_kernels = set()
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
            for n in args.get("n_fields", [3]):
                work = _Work(h, gd, n * wsz * es, bool(args.get("guard")))
                for dims in [(0,), (1,), (2,)] + ([(0, 1, 2)] if args.get("all_dims") else []):
                    got = _fields(info, es, n, (rank * 3 + axis) * 64 + n)
                    want = [t.clone() for t in got]
                    for dim in dims:
                        before = cd.cudecompExtDataLaunchCount()
                        cd.cudecompUpdateFieldHalos(axis, h, gd, [t.data_ptr() for t in got], work.ptr, dtype, halo, periods, dim,
                                                    padding, stream)
                        made = cd.cudecompExtDataLaunchCount() - before
                        name = cd.cudecompExtLastKernelName()
                        plan = cd.cudecompExtPlanHaloFields(spec, rank, axis, halo, periods, dim, padding, n)
                        if plan.kind != 0 and n >= 2:
                            seen_kernels.add(name.split("<")[0])
                            if "_fields_kernel<" not in name:
                                failures.append("rank %d axis %d dim %d n %d: the last kernel was %s" % (rank, axis, dim, n, name))
                        if args.get("launches") and plan.kind != 0 and n >= 2:
                            expect = args["launches"]["self" if plan.kind == 1 else "packed"]
                            if made != expect:
                                failures.append("rank %d axis %d dim %d n %d: %d data-movement launches, expected %d" %
                                                (rank, axis, dim, n, made, expect))
                        for t in want:
                            cd.cudecompUpdateHalos(axis, h, gd, t.data_ptr(), single.ptr, dtype, halo, periods, dim, padding, stream)
                    torch.cuda.synchronize()
                    for f in range(n):
                        if not torch.equal(got[f], want[f]):
                            bad = torch.nonzero(got[f] != want[f]).reshape(-1)
                            failures.append("rank %d axis %d %s halo %s periods %s padding %s dims %s n %d field %d: %d bytes differ, "
                                            "first in cell %d" % (rank, axis, AB.NAMES[dtype], tuple(halo), tuple(periods), tuple(padding),
                                                                  dims, n, f, bad.numel(), int(bad[0]) // es))
                    if not work.outside_untouched():
                        failures.append("rank %d axis %d dims %s n %d: bytes outside the workspace changed" % (rank, axis, dims, n))
                work.free()
            single.free()
    if args.get("expect_kernels") and not seen_kernels:
        failures.append("rank %d: no fields kernel ran at all" % rank)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def one_field_is_the_single_call(rank, nranks, args):
    """n_fields = 1: the same bytes and the same last kernel as cudecompUpdateHalos"""
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
            for dim in range(3):
                got = _fields(info, es, 1, axis)[0]
                want = got.clone()
                cd.cudecompUpdateFieldHalos(axis, h, gd, [got.data_ptr()], work, dtype, halo, periods, dim, padding, stream)
                a = cd.cudecompExtLastKernelName()
                cd.cudecompUpdateHalos(axis, h, gd, want.data_ptr(), work, dtype, halo, periods, dim, padding, stream)
                b = cd.cudecompExtLastKernelName()
                torch.cuda.synchronize()
                if a != b or "_fields_" in a or not torch.equal(got, want):
                    failures.append("axis %d %s dim %d: kernels %s / %s, equal bytes: %s" % (axis, AB.NAMES[dtype], dim, a, b,
                                                                                             torch.equal(got, want)))
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
    axis, dim, dtype, n = args.get("axis", 0), args.get("dim", 1), args.get("dtype", cd.DOUBLE), 3
    es = AB.element_bytes(dtype)
    info = g.pencil_info(rank, axis, halo, padding)
    wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
    work = cd.cudecompMalloc(h, gd, n * wsz * es)
    single = cd.cudecompMalloc(h, gd, wsz * es)
    fn = getattr(cd.lib(), "cudecompAmdUpdateFieldHalos" + "XYZ"[axis])
    i3, b3 = (C.c_int32 * 3), (C.c_bool * 3)
    fields = _fields(info, es, n, 5)

    def call(sptr):
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in fields])
        rc = fn(h, gd, ptrs, n, work, dtype, i3(*halo), b3(*[bool(x) for x in periods]), dim, i3(*padding), sptr)
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
        fresh = _fields(info, es, n, 100 + it)
        want = [t.clone() for t in fresh]
        with torch.cuda.stream(stream):
            for t, src in zip(fields, fresh):
                t.copy_(src)
            graph.replay()
            for t in want:
                cd.cudecompUpdateHalos(axis, h, gd, t.data_ptr(), single, dtype, halo, periods, dim, padding, stream.cuda_stream)
            stream.synchronize()
        for f in range(n):
            if not torch.equal(fields[f], want[f]) or torch.equal(fields[f], fresh[f]):
                failures.append("replay %d field %d differs from the single call (or nothing changed)" % (it, f))
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompFree(h, gd, single)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def _run_field_moves(moves, n, field, work, shift):
    """the moves of field 0 carried out for the field whose pieces lie `shift` elements further into the workspace"""
    from tests.bodies import run_moves
    run_moves(moves, n, [field, field, work[shift:]])


def plan_fields_gloo(rank, nranks, args):
    """The stateless fields plan (cudecompExtPlanHaloFields) executed with numpy block moves and a real multi-process exchange over
    gloo -- ONE message of n faces per direction -- against the single plan (cudecompExtPlanHalo, packed) executed field by field
    with its own exchanges.  uint16 payload; every axis, dims 0, 1, 2 in sequence on one set of fields; no GPU."""
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=nranks)
    gdims, pdims, padding = args["gdims"], args["pdims"], args["padding"]
    from oracle import oracle as orc
    g = orc.Grid(gdims, pdims)
    spec = cd.make_grid_spec(gdims, pdims, [[int(x) for x in g.pencil_info(rank, a).order] for a in range(3)])
    failures = []

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
            s = torch.from_numpy(work[plan.send_off[i]:plan.send_off[i] + count].view(np.int16).copy())
            reqs.append(dist.isend(s, plan.neighbor[i], tag=1 - i))
        for r in reqs:
            r.wait()
        for t, off in landing:
            work[off:off + count] = t.numpy().view(np.uint16)

    for halo, periods in itertools.product(args["halos"], args["periods"]):
        for axis, n in itertools.product(range(3), args["n_fields"]):
            info = g.pencil_info(rank, axis, halo, padding)
            ws = max(cd.cudecompExtWorkspaceSizes(spec, rank, axis, halo)[1], 1)
            rng = np.random.RandomState(1000 * rank + 10 * axis + n)
            got = [rng.randint(0, 1 << 16, size=int(info.size)).astype(np.uint16) for _ in range(n)]
            want = [a.copy() for a in got]
            work = np.full(n * ws, 0xDEAD, dtype=np.uint16)
            single_work = np.full(ws, 0xBEEF, dtype=np.uint16)
            for dim in range(3):
                # a halo wider than some neighbour's slab is refused, on the ranks it concerns, by both planners alike: every
                # rank works that out for all ranks, and all of them leave the dim out
                refused = []
                for r in range(nranks):
                    codes = []
                    for planner, more in ((cd.cudecompExtPlanHalo, (True,)), (cd.cudecompExtPlanHaloFields, (n,))):
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
                fp = cd.cudecompExtPlanHaloFields(spec, rank, axis, halo, periods, dim, padding, n)
                sp = cd.cudecompExtPlanHalo(spec, rank, axis, halo, periods, dim, padding, True)
                if fp.kind == 3 and n >= 2:
                    failures.append("direct fields plan")
                if fp.kind not in (0, 3):
                    for f in range(n):
                        _run_field_moves(fp.pre, fp.n_pre, got[f], work, f * fp.face_elements)
                    if fp.kind == 2:
                        exchange(fp, work, n * fp.face_elements)
                        for f in range(n):
                            _run_field_moves(fp.post, fp.n_post, got[f], work, f * fp.face_elements)
                if sp.kind != 0:
                    for f in range(n):
                        _run_field_moves(sp.pre, sp.n_pre, want[f], single_work, 0)
                        if sp.kind == 2:
                            exchange(sp, single_work, sp.face_elements)
                            _run_field_moves(sp.post, sp.n_post, want[f], single_work, 0)
                for f in range(n):
                    if not np.array_equal(got[f], want[f]):
                        failures.append("rank %d halo %s periods %s axis %d n %d dim %d field %d: %d cells differ" %
                                        (rank, halo, periods, axis, n, dim, f, int((got[f] != want[f]).sum())))
    dist.destroy_process_group()
    return failures


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out
