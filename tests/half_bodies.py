"""2-byte element types (cudecomp_amd.h: CUDECOMP_AMD_HALF, CUDECOMP_AMD_BFLOAT16) and complex-fp16: payloads, expected
values and the per-rank bodies of tests/test_half_types.py and tests/test_gpu_half_types.py.

The analytic oracle knows the four reference types only, so the expected values here are closed forms of the global
linear index g = x + nx * (y + ny * z) of every interior cell.  A 16-bit element cannot hold g above 65,535 cells, so a
grid is checked in passes: pass `shift` stores payload((g >> shift) & 0xffff); the low pass (shift 0) and, for larger
grids, the high pass (shift 16) identify every cell.  The payload is a fixed permutation of the 65,536 bit patterns that
puts fp16 / bf16 infinities, NaNs with payloads, -0 and subnormals first, so every grid of a few dozen cells moves them
(data movement is bit-exact: nothing may be converted).  Complex-fp16 elements (4 bytes) carry both halves of g at once."""
import os

import numpy as np

import cudecomp_amd as cd
from oracle import oracle as orc

HALF_TYPES = {cd.HALF: 2, cd.BFLOAT16: 2, cd.HALF_COMPLEX: 4}

SPECIALS = [0x7c00, 0xfc00, 0x7e00, 0x7c01, 0x7fff, 0xfe01, 0x8000, 0x0000, 0x0001, 0x03ff, 0x8001, 0x83ff,  # fp16
            0x7f80, 0xff80, 0x7fc0, 0x7f81, 0xffc1, 0x007f, 0x807f, 0x0080]  # bf16
_rest = np.setdiff1d(np.arange(65536), SPECIALS)
PERM = np.concatenate([np.array(SPECIALS), _rest]).astype(np.uint16)
assert np.unique(PERM).size == 65536


def word_dtype(es):
    return {2: np.uint16, 4: np.uint32}[es]


def payload(g, es, shift=0):
    """values of the cells with global indices g (int64 array, all >= 0)"""
    if es == 2:
        return PERM[(g >> shift) & 0xffff]
    lo = PERM[g & 0xffff].astype(np.uint32)
    hi = PERM[(g >> 16) & 0xffff].astype(np.uint32)
    return lo | (hi << 16)


def _coords(p):
    shape = [int(x) for x in p.shape]
    i = np.arange(int(p.size), dtype=np.int64)
    return shape, [i % shape[0], i // shape[0] % shape[1], i // (shape[0] * shape[1])]


def global_index(p, gdims):
    """global linear index of every cell of pencil `p` (pencil info), -1 outside the interior (halo, padding)"""
    shape, l = _coords(p)
    inside = np.ones(int(p.size), dtype=bool)
    gl = [None] * 3
    for k in range(3):
        o = p.order[k]
        inside &= (l[k] >= p.halo_extents[o]) & (l[k] < shape[k] - p.halo_extents[o] - p.padding[o])
        gl[o] = l[k] + p.lo[k] - p.halo_extents[o]
    g = gl[0] + gdims[0] * (gl[1] + gl[2] * gdims[1])
    return np.where(inside, g, -1)


def halo_source_index(p, gdims, periods):
    """after UpdateHalos along dims 0, 1, 2 in turn: the global index whose value each cell holds, -1 where the cell keeps
    what it held (padding, non-periodic edges); the oracle's fill_halo_reference as indices"""
    shape, l = _coords(p)
    unset = np.zeros(int(p.size), dtype=bool)
    gl = [None] * 3
    for k in range(3):
        o = p.order[k]
        gl[o] = l[k] + p.lo[k] - p.halo_extents[o]
        unset |= l[k] >= shape[k] - p.padding[o]
    for d in range(3):
        out = (gl[d] < 0) | (gl[d] >= gdims[d])
        if periods[d]:
            gl[d] = gl[d] % gdims[d]
        else:
            unset |= out
    g = gl[0] + gdims[0] * (gl[1] + gl[2] * gdims[1])
    return np.where(unset, -1, g)


def first_difference(got, want):
    bad = np.nonzero(got != want)[0]
    return None if bad.size == 0 else (int(bad.size), int(bad[0]), int(want[bad[0]]), int(got[bad[0]]))


# ---- host execution of the product's plans over gloo (no GPU) --------------------------------------------------------------
def plan_transpose_gloo(rank, nranks, args):
    """The product's transpose plans (cudecompExtGetTransposePlan) for a uint16 payload, executed with numpy block moves and a
    gloo exchange, X->Y->Z->Y->X in and out of place; every interior cell compared with the closed form after every hop."""
    import torch
    import torch.distributed as dist
    from tests.bodies import run_moves
    dist.init_process_group("gloo", rank=rank, world_size=nranks)
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config(args["gdims"], args["pdims"], axis_contiguous=args.get("ac", (0, 0, 0))))
    halos, pads = args.get("halos", [(0, 0, 0)] * 3), args.get("pads", [(0, 0, 0)] * 3)
    pin = [cd.cudecompGetPencilInfo(h, gd, ax, halos[ax], pads[ax]) for ax in range(3)]
    wsz = cd.cudecompGetTransposeWorkspaceSize(h, gd)
    nel = max(p.size for p in pin)
    failures = []
    gdims = args["gdims"]
    if cd.cudecompGetDataTypeSize(args.get("dtype", cd.HALF)) != 2:
        return ["the library's size of dtype %d is not 2" % args.get("dtype", cd.HALF)]
    for backend in args["backends"]:
        for oop in (True, False):
            a = np.full(nel, 0xdead, dtype=np.uint16)
            b = np.full(nel, 0xbeef, dtype=np.uint16) if oop else a
            gi = global_index(pin[0], gdims)
            a[:pin[0].size][gi >= 0] = payload(gi[gi >= 0], 2)
            cur, nxt = a, b
            for op in cd.OPS:
                ai, ao = orc.OP_AXES[op]
                plan = cd.cudecompExtGetTransposePlan(h, gd, op, halos[ai], halos[ao], pads[ai], pads[ao], inplace=not oop,
                                                      backend_override=backend)
                bufs = [cur, nxt, np.zeros(wsz, dtype=np.uint16)]
                if not plan.noop:
                    run_moves(plan.pack, plan.n_pack, bufs)
                    if plan.exchange:
                        sendb, recvb = bufs[plan.send_buf], bufs[plan.recv_buf]
                        reqs, stage = [], {}
                        for d in range(plan.nranks):
                            gr = plan.member_global_rank[d]
                            so, sc = plan.send_base + plan.send_off[d], plan.send_cnt[d]
                            ro, rc = plan.recv_base + plan.recv_off[d], plan.recv_cnt[d]
                            if gr == rank:
                                recvb[ro:ro + rc] = sendb[so:so + sc].copy()
                                continue
                            stage[d] = (torch.zeros(rc, dtype=torch.int16), ro, rc)
                            if sc:
                                reqs.append(dist.isend(torch.from_numpy(sendb[so:so + sc].view(np.int16).copy()), gr))
                            if rc:
                                reqs.append(dist.irecv(stage[d][0], gr))
                        for q in reqs:
                            q.wait()
                        for d, (t, ro, rc) in stage.items():
                            recvb[ro:ro + rc] = t.numpy().view(np.uint16)
                    run_moves(plan.unpack, plan.n_unpack, bufs)
                gi = global_index(pin[ao], gdims)
                got = nxt[:pin[ao].size][gi >= 0]
                diff = first_difference(got, payload(gi[gi >= 0], 2))
                if diff:
                    failures.append("backend %d oop %s %s: %d cells differ, first at %d (want %#x got %#x)" %
                                    ((backend, oop, op) + diff))
                    break
                if oop:
                    cur, nxt = nxt, cur
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)
    dist.destroy_process_group()
    return failures


# ---- GPU bodies ------------------------------------------------------------------------------------------------------------
def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8)).cuda()


def _host(t, es):
    return t.cpu().numpy().view(word_dtype(es))


def half_cycle(rank, nranks, args):
    """X->Y->Z->Y->X in dtype args["dtype"] (a cudecomp_amd.h type), out of place and in place, one pass per args["shifts"].
    Out of place EVERY cell of the destination buffer is compared after every hop: the interior with the closed form,
    halo / padding cells and the buffer's tail with what they held before the call.  In place (the output overwrites the
    input's buffer) the interior is compared.  args["data_alloc"] == "malloc": pencils from cudecompMalloc (NVSHMEM_SM then
    puts directly into the peers' output pencils)."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    dtype = args["dtype"]
    es = HALF_TYPES[dtype]
    wd = word_dtype(es)
    gdims = args["gdims"]
    halos, pads = args.get("halos", [(0, 0, 0)] * 3), args.get("pads", [(0, 0, 0)] * 3)
    pin = [cd.cudecompGetPencilInfo(h, gd, ax, halos[ax], pads[ax]) for ax in range(3)]
    failures = ["rank %d: pencil info axis %d differs from the oracle" % (rank, ax)
                for ax in range(3) if pin[ax].as_dict() != g.pencil_info(rank, ax, halos[ax], pads[ax]).as_dict()]
    gidx = [global_index(p, gdims) for p in pin]
    nel = max(p.size for p in pin) + 64
    wsz = cd.cudecompGetTransposeWorkspaceSize(h, gd)
    work_ptr = cd.cudecompMalloc(h, gd, max(wsz, 1) * es)
    rng = np.random.default_rng(77 + rank)
    to_free = []
    for oop in args.get("out_of_place", [True, False]):
        for shift in args.get("shifts", [0]):
            if args.get("data_alloc") == "malloc":
                from tests import gpu_util as G
                a, pa = G.library_bytes(cd, h, gd, nel * es)
                b, pb = G.library_bytes(cd, h, gd, nel * es) if oop else (a, None)
                to_free += [p for p in (pa, pb) if p]
                a.copy_(_dev(rng.integers(0, 256, nel * es, dtype=np.uint8)))
                if oop:
                    b.copy_(_dev(rng.integers(0, 256, nel * es, dtype=np.uint8)))
            else:
                a = _dev(rng.integers(0, 256, nel * es, dtype=np.uint8))
                b = _dev(rng.integers(0, 256, nel * es, dtype=np.uint8)) if oop else a
            init = _host(a, es).copy()
            gi = gidx[0]
            init[:pin[0].size][gi >= 0] = payload(gi[gi >= 0], es, shift)
            a.copy_(_dev(init))
            cur, nxt = a, b
            for op in cd.OPS:
                ai, ao = orc.OP_AXES[op]
                before = _host(nxt, es).copy()
                cd.cudecompTranspose(op, h, gd, cur.data_ptr(), nxt.data_ptr(), work_ptr, dtype, halos[ai], halos[ao],
                                     pads[ai], pads[ao], torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got = _host(nxt, es)
                gi = gidx[ao]
                exp = payload(gi[gi >= 0], es, shift)
                if oop:
                    want = before.copy()
                    want[:pin[ao].size][gi >= 0] = exp
                    diff = first_difference(got, want)
                else:
                    diff = first_difference(got[:pin[ao].size][gi >= 0], exp)
                if diff:
                    failures.append("rank %d dtype %d oop=%s shift %d %s: %d cells differ, first at %d (want %#x got %#x); "
                                    "last kernel %s" % ((rank, dtype, oop, shift, op) + diff + (cd.cudecompExtLastKernelName(),)))
                    break
                if oop:
                    cur, nxt = nxt, cur
    counters = cd.cudecompExtGetCounters(h, gd)
    for name, want in (args.get("expect_counts") or {}).items():
        if counters[name] != want:
            failures.append("rank %d: executor path %r ran %d times, expected %d" % (rank, name, counters[name], want))
    for name in args.get("expect_path", []):
        if counters[name] <= 0:
            failures.append("rank %d: executor path %r did not run: %r" % (rank, name, counters))
    torch.cuda.synchronize()
    for p in to_free:
        cd.cudecompFree(h, gd, p)
    cd.cudecompFree(h, gd, work_ptr)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def half_halo(rank, nranks, args):
    """UpdateHalos{X,Y,Z} (args["axes"]) along dims 0, 1, 2 in turn on a halo-carrying, padded pencil of 2-byte elements;
    the whole pencil compared: every cell a halo update fills holds its source cell's closed form, all others what they
    held before."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    dtype = args["dtype"]
    es = HALF_TYPES[dtype]
    gdims = args["gdims"]
    halo, periods, padding = args["halo"], args["periods"], args.get("padding", (0, 0, 0))
    failures = []
    for axis in args.get("axes", [0, 1, 2]):
        p = cd.cudecompGetPencilInfo(h, gd, axis, halo, padding)
        wsz = max(cd.cudecompGetHaloWorkspaceSize(h, gd, axis, halo), 1)
        work_ptr = cd.cudecompMalloc(h, gd, wsz * es)
        # (one value in every cell outside the interior, on every rank: the updates copy whole slabs, halo corners of the
        # non-periodic edges included, so such cells may receive another rank's unset cells -- as in the reference's test)
        init = np.full(int(p.size), 0xdeadbeef & ((1 << (8 * es)) - 1), dtype=word_dtype(es))
        gi = global_index(p, gdims)
        init[gi >= 0] = payload(gi[gi >= 0], es)
        data = _dev(init)
        for dim in range(3):
            cd.cudecompUpdateHalos(axis, h, gd, data.data_ptr(), work_ptr, dtype, halo, periods, dim, padding,
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        src = halo_source_index(p, gdims, periods)
        want = init.copy()
        want[src >= 0] = payload(src[src >= 0], es)
        diff = first_difference(_host(data, es), want)
        if diff:
            failures.append("rank %d axis %d halo %s periods %s: %d cells differ, first at %d (want %#x got %#x)" %
                            ((rank, axis, tuple(halo), tuple(periods)) + diff))
        cd.cudecompFree(h, gd, work_ptr)
    cd.cudecompGridDescDestroy(h, gd)
    return failures


def autotune_half(rank, nranks, args):
    """Grid + backend autotuning with options.dtype = CUDECOMP_AMD_HALF (transpose or halo grid mode), then a checked fp16
    cycle and halo update on what was picked."""
    from tests import gpu_bodies as B
    h = B._handle(rank)
    cfg = cd.make_config(args["gdims"], (0, 0), axis_contiguous=args.get("ac", (0, 0, 0)))
    opt = cd.cudecompGridDescAutotuneOptionsSetDefaults()
    opt.n_warmup_trials, opt.n_trials = 1, 1
    opt.dtype = cd.HALF
    opt.autotune_transpose_backend = True
    opt.autotune_halo_backend = True
    opt.disable_nccl_backends = True
    for i in range(3):
        opt.halo_extents[i] = 1
        opt.halo_periods[i] = True
    if args.get("grid_mode_halo"):
        opt.grid_mode = cd.AUTOTUNE_GRID_HALO
    gd = cd.cudecompGridDescCreate(h, cfg, opt)
    picked = {"pdims": [cfg.pdims[0], cfg.pdims[1]], "tb": cfg.transpose_comm_backend, "hb": cfg.halo_comm_backend}
    cd.cudecompGridDescDestroy(h, gd)
    a = {"gdims": args["gdims"], "pdims": picked["pdims"], "ac": args.get("ac", (0, 0, 0)), "dtype": cd.HALF,
         "transpose_backend": picked["tb"], "halo_backend": picked["hb"], "out_of_place": [True]}
    fails = half_cycle(rank, nranks, a)
    fails += half_halo(rank, nranks, dict(a, halo=(1, 1, 1), periods=(1, 1, 1), axes=[0]))
    return {"picked": picked, "failures": fails}


def many(rank, nranks, args):
    """Run a list of {"fn": name, "args": {...}} jobs in this process group (one launch of fresh processes); returns all
    failures."""
    out = []
    for job in args["jobs"]:
        fails = globals()[job["fn"]](rank, nranks, job["args"])
        out.extend("%s: %s" % (job.get("id", job["fn"]), f) for f in fails)
    return out


def full_size_cycle(rank, nranks, args):
    """The 2048 x 2048 x 1024 fp16 axis-contiguous cycle (2^32 elements, 8 GiB per pencil) on a 1 x 1 grid, out of place,
    in two passes (low and high 16 bits of the global index): after every hop every cell of the output pencil is compared
    on the device with the closed form, in chunks."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, dict(args, pdims=(1, 1)))
    gdims = args["gdims"]
    pin = [cd.cudecompGetPencilInfo(h, gd, ax) for ax in range(3)]
    n = int(pin[0].size)
    perm = torch.from_numpy(PERM.view(np.int16).copy()).cuda()
    wsz = cd.cudecompGetTransposeWorkspaceSize(h, gd)
    work_ptr = cd.cudecompMalloc(h, gd, max(wsz, 1) * 2)
    a = torch.empty(n, dtype=torch.int16, device="cuda")
    b = torch.empty(n, dtype=torch.int16, device="cuda")
    chunk = 1 << 28
    failures, kernels = [], []

    def expected(p, lo, hi, shift):
        # local position -> global index -> payload, for the cells [lo, hi) of pencil p (no halos: every cell is interior)
        i = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
        s0, s1 = int(p.shape[0]), int(p.shape[1])
        l = [i % s0, (i // s0) % s1, i // (s0 * s1)]
        gl = [None] * 3
        for k in range(3):
            gl[p.order[k]] = l[k] + int(p.lo[k])
        gi = gl[0] + gdims[0] * (gl[1] + gl[2] * gdims[1])
        return perm[(gi >> shift) & 0xffff]

    for shift in (0, 16):
        for lo in range(0, n, chunk):
            a[lo:lo + chunk] = expected(pin[0], lo, min(n, lo + chunk), shift)
        b.fill_(0x5a5a)
        cur, nxt = a, b
        for op in cd.OPS:
            ai, ao = orc.OP_AXES[op]
            cd.cudecompTranspose(op, h, gd, cur.data_ptr(), nxt.data_ptr(), work_ptr, cd.HALF, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            kernels.append(cd.cudecompExtLastKernelName())
            for lo in range(0, n, chunk):
                hi = min(n, lo + chunk)
                bad = (nxt[lo:hi] != expected(pin[ao], lo, hi, shift)).nonzero()
                if bad.numel():
                    failures.append("shift %d %s: %d cells differ in [%d, %d), first at %d; kernel %s" %
                                    (shift, op, bad.numel(), lo, hi, lo + int(bad[0]), kernels[-1]))
                    break
            if failures:
                break
            cur, nxt = nxt, cur
        if failures:
            break
    torch.cuda.synchronize()
    del a, b
    cd.cudecompFree(h, gd, work_ptr)
    cd.cudecompGridDescDestroy(h, gd)
    return {"failures": failures, "kernels": kernels}


def perf_report_half(rank, nranks, args):
    """fp16, bf16 and complex-fp16 transposes and halo updates with the performance report on (the caller's environment);
    returns the report files the descriptor's destruction wrote."""
    import torch
    from tests import gpu_bodies as B
    h, gd, g = B._setup(rank, nranks, args)
    pin = [cd.cudecompGetPencilInfo(h, gd, ax) for ax in range(3)]
    hp = cd.cudecompGetPencilInfo(h, gd, 0, (1, 1, 1))
    nel = max([p.size for p in pin] + [hp.size])
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetTransposeWorkspaceSize(h, gd), 1) * 4)
    hwork = cd.cudecompMalloc(h, gd, max(cd.cudecompGetHaloWorkspaceSize(h, gd, 0, (1, 1, 1)), 1) * 4)
    a = torch.zeros(nel * 4, dtype=torch.uint8, device="cuda")
    b = torch.zeros(nel * 4, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for dtype in (cd.HALF, cd.BFLOAT16, cd.HALF_COMPLEX):
        for _ in range(3):
            for op in cd.OPS:
                cd.cudecompTranspose(op, h, gd, a.data_ptr(), b.data_ptr(), work, dtype, stream=stream)
            cd.cudecompUpdateHalos(0, h, gd, a.data_ptr(), hwork, dtype, (1, 1, 1), (1, 1, 1), 0, stream=stream)
    torch.cuda.synchronize()
    cd.cudecompFree(h, gd, work)
    cd.cudecompFree(h, gd, hwork)
    cd.cudecompGridDescDestroy(h, gd)
    d = os.environ["CUDECOMP_PERFORMANCE_REPORT_WRITE_DIR"]
    return {"files": {f: open(os.path.join(d, f)).read() for f in os.listdir(d)}} if rank == 0 else {"files": {}}
