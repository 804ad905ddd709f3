"""Multi-field transposes (cudecomp_transpose_fields.h: cudecompAmdTransposeFields{XToY,YToZ,ZToY,YToX}): the per-rank bodies of
tests/test_gpu_transpose_fields.py and the gloo body of tests/test_transpose_fields_plan.py.  The oracle is the single call: every
field after the fields call against a clone after cudecompTranspose* with the same remaining arguments.  Whole buffers -- halo and
padding cells of the outputs included -- byte for byte; there is no tolerance anywhere.

Payload: every byte of every field drawn at random (another seed per field, rank and op: a chunk that lands in the wrong field or
the wrong rank shows), the poison byte in the padding cells of the first pencil, as tests/fields_bodies.py does."""
import ctypes as C

import numpy as np

import cudecomp_amd as cd
from tests import accumulate_bodies as AB
from tests import fields_bodies as FB

POISON = FB.POISON
OP_AXES = {"XToY": (0, 1), "YToZ": (1, 2), "ZToY": (2, 1), "YToX": (1, 0)}


def _buffer(info, es, nel, seed):
    """uint8 (nel * es) on the device: the pencil `info` of random bytes (poison in its padding cells), poison behind it"""
    import torch
    a = np.full(nel * es, POISON, dtype=np.uint8)
    a[:int(info.size) * es] = FB.field_bytes(info, es, seed)
    return torch.from_numpy(a).cuda()


def _noise(nel, es, seed):
    import torch
    return torch.from_numpy(np.random.RandomState(seed % (1 << 31)).randint(0, 256, size=nel * es).astype(np.uint8)).cuda()


def _spec(g, rank, args):
    return cd.make_grid_spec(args["gdims"], args["pdims"], [[int(x) for x in g.pencil_info(rank, a).order] for a in range(3)],
                             gdims_dist=args.get("gdims_dist"))


def predicted_launches(spec, rank, op, halos, pads, inplace, symmetric, n, ins, outs, work, es):
    """the data-movement launches planFieldMoveLaunches predicts for the fields plan of this call (real addresses)"""
    ai, ao = OP_AXES[op]
    p, ps, us = cd.cudecompExtPlanTransposeFields(spec, rank, op, halos[ai], halos[ao], pads[ai], pads[ao], inplace, False, symmetric,
                                                  0, n)
    if p.noop:
        return 0, 1
    total = 0
    for moves, cnt, steps in ((p.pack, p.n_pack, ps), (p.unpack, p.n_unpack, us)):
        if cnt:
            total += len(cd.cudecompExtDescribeFieldMoveList([moves[i] for i in range(cnt)], steps, ins, outs, work, es))
    return total, (p.nranks if p.exchange else 1)


def h_self_exchange():
    import os
    return os.environ.get("CUDECOMP_TEST_SELF_EXCHANGE") == "1"


def fields_cycle(rank, nranks, args):
    """args["ops"] (default the full cycle X->Y->Z->Y->X) of n fields for every n of args["n_fields"], type of args["dtypes"] and
    both of args["out_of_place"], against single calls on clones after every hop.  halos / pads: one triple per axis.
    args["guard"]: the workspace holds exactly n x the queried size inside a poisoned buffer, and nothing outside it changes.
    args["launches"]: "predict" -- every call makes exactly the launches planFieldMoveLaunches predicts for its plan -- or an
    integer every exchanging call must make.  The count is that of cudecompExtDataLaunchCount, which also sees the chunk copies
    the one-sided transport makes with the row-copy kernel between ranks that share a GPU: the tests that pass "launches" over a
    one-sided enum pin its copies to the copy engines (CUDECOMP_PEER_COPY_ENGINE=sdma), so every launch counted is the call's own.
    args["local_launches"]: single rank: 1 out of place, 2 in place with differing
    layouts, 0 for the no-op, the same for every n."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halos, pads = args.get("halos", [(0, 0, 0)] * 3), args.get("pads", [(0, 0, 0)] * 3)
    stream = torch.cuda.current_stream().cuda_stream
    spec = _spec(g, rank, args)
    backend = cd.cudecompGetGridDescConfig(h, gd).transpose_comm_backend
    symmetric = backend not in (cd.TRANSPOSE_COMM_NCCL, cd.TRANSPOSE_COMM_NCCL_PL)  # (every other enum: the one-sided transport)
    infos = [g.pencil_info(rank, ax, halos[ax], pads[ax]) for ax in range(3)]
    failures = []
    for ax in range(3):
        if cd.cudecompGetPencilInfo(h, gd, ax, halos[ax], pads[ax]).as_dict() != infos[ax].as_dict():
            failures.append("rank %d axis %d: pencil info differs from the oracle" % (rank, ax))
    nel = max(int(p.size) for p in infos)
    wsz = max(cd.cudecompGetTransposeWorkspaceSize(h, gd), 1)
    ops = args.get("ops", list(cd.OPS))
    seen = set()
    for dtype in args.get("dtypes", [cd.DOUBLE]):
        es = AB.element_bytes(dtype)
        single = FB._Work(h, gd, wsz * es, False)
        for n in args.get("n_fields", [3]):
            work = FB._Work(h, gd, n * wsz * es, bool(args.get("guard")))
            for oop in args.get("out_of_place", [True, False]):
                first = OP_AXES[ops[0]][0]
                cur = [_buffer(infos[first], es, nel, (rank * 4 + first) * 1009 + f * 7919 + n) for f in range(n)]
                nxt = [_noise(nel, es, 31 * f + rank + 5) for f in range(n)] if oop else cur
                wcur = [t.clone() for t in cur]
                wnxt = [t.clone() for t in nxt] if oop else wcur
                for op in ops:
                    ai, ao = OP_AXES[op]
                    ins, outs = [t.data_ptr() for t in cur], [t.data_ptr() for t in nxt]
                    before = cd.cudecompExtDataLaunchCount()
                    cd.cudecompTransposeFields(op, h, gd, ins, outs, work.ptr, dtype, halos[ai], halos[ao], pads[ai], pads[ao], stream)
                    made = cd.cudecompExtDataLaunchCount() - before
                    name = cd.cudecompExtLastKernelName()
                    for a, b in zip(wcur, wnxt):
                        cd.cudecompTranspose(op, h, gd, a.data_ptr(), b.data_ptr(), single.ptr, dtype, halos[ai], halos[ao], pads[ai],
                                             pads[ao], stream)
                    torch.cuda.synchronize()
                    what = "rank %d %s %s n %d oop %s halos %s pads %s" % (rank, AB.NAMES[dtype], op, n, oop, halos, pads)
                    if made and n >= 2:
                        seen.add(name.split("<")[0])
                        if "_fields_kernel<" not in name:
                            failures.append("%s: the last kernel was %s" % (what, name))
                    if n >= 2 and args.get("launches") is not None:
                        expect, members = predicted_launches(spec, rank, op, halos, pads, not oop, symmetric, n, ins, outs, work.ptr, es)
                        if args["launches"] != "predict" and members > 1:
                            expect = args["launches"]
                        elif args["launches"] != "predict" and h_self_exchange():
                            expect = args["launches"]
                        if made != expect:
                            failures.append("%s: %d data-movement launches, expected %d" % (what, made, expect))
                    if n >= 2 and args.get("local_launches"):
                        p1 = cd.cudecompExtPlanTranspose(spec, rank, op, halos[ai], halos[ao], pads[ai], pads[ao], not oop)
                        expect = 0 if p1.noop else (1 if oop else 2)
                        if made != expect:
                            failures.append("%s: %d data-movement launches, expected %d" % (what, made, expect))
                    for f in range(n):
                        for which, got, want in (("output", nxt[f], wnxt[f]), ("input", cur[f], wcur[f])):
                            if not torch.equal(got, want):
                                bad = torch.nonzero(got != want).reshape(-1)
                                failures.append("%s field %d %s: %d bytes differ, first in cell %d" %
                                                (what, f, which, bad.numel(), int(bad[0]) // es))
                    if not work.outside_untouched():
                        failures.append("%s: bytes outside the workspace changed" % what)
                    if oop:
                        cur, nxt, wcur, wnxt = nxt, cur, wnxt, wcur
                    if len(failures) > 20:
                        break
            work.free()
        single.free()
    if args.get("expect_kernels") and not seen:
        failures.append("rank %d: no fields kernel ran at all" % rank)
    if args.get("expect_path"):
        counters = cd.cudecompExtGetCounters(h, gd)
        for name in args["expect_path"]:
            if counters[name] <= 0:
                failures.append("executor path %r did not run: %r" % (name, counters))
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def one_field_is_the_single_call(rank, nranks, args):
    """n_fields = 1: the same bytes and the same last kernel as cudecompTranspose*"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halos, pads = args.get("halos", [(0, 0, 0)] * 3), args.get("pads", [(0, 0, 0)] * 3)
    stream = torch.cuda.current_stream().cuda_stream
    infos = [g.pencil_info(rank, ax, halos[ax], pads[ax]) for ax in range(3)]
    nel = max(int(p.size) for p in infos)
    wsz = max(cd.cudecompGetTransposeWorkspaceSize(h, gd), 1)
    failures = []
    for dtype in args.get("dtypes", [cd.DOUBLE]):
        es = AB.element_bytes(dtype)
        work = cd.cudecompMalloc(h, gd, wsz * es)
        for op in cd.OPS:
            ai, ao = OP_AXES[op]
            for oop in (True, False):
                a = _buffer(infos[ai], es, nel, 77 + ai)
                b = _noise(nel, es, 3) if oop else a
                wa = a.clone()
                wb = b.clone() if oop else wa
                cd.cudecompTransposeFields(op, h, gd, [a.data_ptr()], [b.data_ptr()], work, dtype, halos[ai], halos[ao], pads[ai],
                                           pads[ao], stream)
                k1 = cd.cudecompExtLastKernelName()
                cd.cudecompTranspose(op, h, gd, wa.data_ptr(), wb.data_ptr(), work, dtype, halos[ai], halos[ao], pads[ai], pads[ao], stream)
                k2 = cd.cudecompExtLastKernelName()
                torch.cuda.synchronize()
                if k1 != k2 or "_fields_" in k1 or not torch.equal(b, wb) or not torch.equal(a, wa):
                    failures.append("%s %s oop %s: kernels %s / %s, equal bytes: %s" % (AB.NAMES[dtype], op, oop, k1, k2, torch.equal(b, wb)))
        cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def graph_replay(rank, nranks, args):
    """One fields call with three fields captured on a side stream after an eager warm-up (the host arrays of pointers are
    temporaries that are gone before the replay); two replays on refilled fields at the same addresses, each against single calls"""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    halos, pads = args.get("halos", [(0, 0, 0)] * 3), args.get("pads", [(0, 0, 0)] * 3)
    op, dtype, n = args.get("op", "XToY"), args.get("dtype", cd.DOUBLE), 3
    ai, ao = OP_AXES[op]
    es = AB.element_bytes(dtype)
    infos = [g.pencil_info(rank, ax, halos[ax], pads[ax]) for ax in range(3)]
    nel = max(int(p.size) for p in infos)
    wsz = max(cd.cudecompGetTransposeWorkspaceSize(h, gd), 1)
    work = cd.cudecompMalloc(h, gd, n * wsz * es)
    single = cd.cudecompMalloc(h, gd, wsz * es)
    fn = getattr(cd.lib(), "cudecompAmdTransposeFields" + op)
    i3 = C.c_int32 * 3
    ins = [_buffer(infos[ai], es, nel, 5 + f) for f in range(n)]
    outs = [_noise(nel, es, 50 + f) for f in range(n)]

    def call(sptr):
        pi = (C.c_void_p * n)(*[t.data_ptr() for t in ins])
        po = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
        rc = fn(h, gd, pi, po, n, work, dtype, i3(*halos[ai]), i3(*halos[ao]), i3(*pads[ai]), i3(*pads[ao]), sptr)
        assert rc == cd.RESULT_SUCCESS, rc
        for i in range(n):
            pi[i] = None  # the caller's arrays change after the call
            po[i] = None

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
        fresh = [_buffer(infos[ai], es, nel, 100 + 10 * it + f) for f in range(n)]
        noise = [_noise(nel, es, 200 + 10 * it + f) for f in range(n)]
        want = [t.clone() for t in noise]
        with torch.cuda.stream(stream):
            for t, src in zip(ins, fresh):
                t.copy_(src)
            for t, src in zip(outs, noise):
                t.copy_(src)
            graph.replay()
            for a, b in zip(fresh, want):
                cd.cudecompTranspose(op, h, gd, a.data_ptr(), b.data_ptr(), single, dtype, halos[ai], halos[ao], pads[ai], pads[ao],
                                     stream.cuda_stream)
            stream.synchronize()
        for f in range(n):
            if not torch.equal(outs[f], want[f]) or torch.equal(outs[f], noise[f]) or not torch.equal(ins[f], fresh[f]):
                failures.append("replay %d field %d differs from the single call (or nothing changed)" % (it, f))
    del graph
    cd.cudecompFree(h, gd, work)
    cd.cudecompFree(h, gd, single)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def plan_fields_gloo(rank, nranks, args):
    """The stateless fields plans (cudecompExtPlanTransposeFields) executed with numpy block moves and a real all-to-all over gloo
    -- ONE message per peer that holds all fields' chunks -- through a full X->Y->Z->Y->X cycle, against the single plans
    (cudecompExtPlanTranspose) executed field by field with their own exchanges.  uint16 payload; no GPU."""
    import torch
    import torch.distributed as dist
    from oracle import oracle as orc
    from tests.bodies import run_moves
    dist.init_process_group("gloo", rank=rank, world_size=nranks)
    gdims, pdims, n = args["gdims"], args["pdims"], args["n_fields"]
    g = orc.Grid(gdims, pdims)
    spec = cd.make_grid_spec(gdims, pdims, [[int(x) for x in g.pencil_info(rank, a).order] for a in range(3)])
    failures = []

    def exchange(p, send, recv):
        """member d gets send[send_base + send_off[d] ...] and it lands at the receiver's recv_base + recv_off[me]"""
        reqs, landing = [], []
        me = p.comm_rank
        for s in range(p.nranks):
            if s == me:
                continue
            t = torch.zeros(int(p.recv_cnt[s]), dtype=torch.int16)
            reqs.append(dist.irecv(t, int(p.member_global_rank[s])))
            landing.append((t, p.recv_base + p.recv_off[s]))
        chunks = [send[p.send_base + p.send_off[d]:p.send_base + p.send_off[d] + p.send_cnt[d]].copy() for d in range(p.nranks)]
        for d in range(p.nranks):
            if d != me:
                reqs.append(dist.isend(torch.from_numpy(chunks[d].view(np.int16)), int(p.member_global_rank[d])))
        for r in reqs:
            r.wait()
        recv[p.recv_base + p.recv_off[me]:p.recv_base + p.recv_off[me] + chunks[me].size] = chunks[me]
        for t, off in landing:
            recv[off:off + t.numel()] = t.numpy().view(np.uint16)

    for halos, pads, inplace, symmetric in args["cases"]:
        infos = [g.pencil_info(rank, ax, halos[ax], pads[ax]) for ax in range(3)]
        nel = max(int(p.size) for p in infos)
        ws = max(cd.cudecompExtWorkspaceSizes(spec, rank, 0, (0, 0, 0))[0], 1)
        rng = np.random.RandomState(1000 * rank + 7)
        cur = [rng.randint(0, 1 << 16, size=nel).astype(np.uint16) for _ in range(n)]
        nxt = cur if inplace else [rng.randint(0, 1 << 16, size=nel).astype(np.uint16) for _ in range(n)]
        wcur = [a.copy() for a in cur]
        wnxt = wcur if inplace else [a.copy() for a in nxt]
        work = np.full(n * ws, 0xDEAD, dtype=np.uint16)
        single_work = np.full(ws, 0xBEEF, dtype=np.uint16)
        for op in cd.OPS:
            ai, ao = OP_AXES[op]
            fp, ps, us = cd.cudecompExtPlanTransposeFields(spec, rank, op, halos[ai], halos[ao], pads[ai], pads[ao], inplace, False,
                                                           symmetric, 0, n)
            sp = cd.cudecompExtPlanTranspose(spec, rank, op, halos[ai], halos[ao], pads[ai], pads[ao], inplace, False, symmetric, 0)
            if not fp.noop:
                for f in range(n):
                    for i in range(fp.n_pack):  # the move of field 0, its workspace end f * step further
                        run_moves([fp.pack[i]], 1, [cur[f], nxt[f], work[f * ps[i]:]])
                if fp.exchange:
                    if fp.send_buf != 2 or fp.recv_buf != 2:
                        failures.append("%s: a fields plan that does not exchange through the workspace" % op)
                    exchange(fp, work, work)
                for f in range(n):
                    for i in range(fp.n_unpack):
                        run_moves([fp.unpack[i]], 1, [cur[f], nxt[f], work[f * us[i]:]])
            if not sp.noop:
                for f in range(n):
                    bufs = [wcur[f], wnxt[f], single_work]
                    run_moves(sp.pack, sp.n_pack, bufs)
                    if sp.exchange:
                        exchange(sp, bufs[sp.send_buf], bufs[sp.recv_buf])
                    run_moves(sp.unpack, sp.n_unpack, bufs)
            for f in range(n):
                if not np.array_equal(nxt[f], wnxt[f]) or not np.array_equal(cur[f], wcur[f]):
                    failures.append("rank %d halos %s pads %s inplace %s %s field %d: %d cells differ" %
                                    (rank, halos, pads, inplace, op, f, int((nxt[f] != wnxt[f]).sum())))
            if not inplace:
                cur, nxt, wcur, wnxt = nxt, cur, wnxt, wcur
    dist.destroy_process_group()
    return failures


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group; returns all failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out
