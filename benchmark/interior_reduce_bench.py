#!/usr/bin/env python3
"""Interior reductions next to the row copy of the same box (single rank, one GPU).

    python benchmark/interior_reduce_bench.py [--n 512] [--reps 5] [--calls 10] [--json profiles/interior_reduce_bench.json]

An X pencil of n^3 fp64 cells with halos (1, 1, 1) and with halos (0, 0, 0).  For each, cudecompAmdReduceInteriorX with SUM (one
field) and DOT (two distinct fields) is timed against the existing row copy of the interior box into a compact buffer
(cudecompExtMove3D): the copy reads the bytes a SUM reads and writes as many again, which is also what a DOT of two fields reads, so
a reduction should not take longer than the copy.  No ratio is fixed in advance.  The two are timed interleaved in one process --
copy, reduction, reduction, copy -- `reps` repetitions of `calls` calls each, between HIP events; reported: every repetition, min /
median / max, GB/s of the median against the algorithmic bytes, the ratio of the medians and the kernels' names.  The results are
checked once against torch on the same data.  One JSON line on stdout, and in --json FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps, calls):
    import torch
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def _record(ms, alg_bytes):
    s = sorted(ms)
    med = s[len(s) // 2]
    return {"ms": [round(x, 4) for x in ms], "min_ms": round(s[0], 4), "median_ms": round(med, 4), "max_ms": round(s[-1], 4),
            "GBps": round(alg_bytes / med / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512, help="cells along every dim")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--json", metavar="FILE", default=None, help="also write the result line to FILE")
    a = ap.parse_args()

    import torch

    import cudecomp_amd as cd
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")
    n, es = a.n, 8
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((n, n, n), (1, 1)))
    st = torch.cuda.current_stream().cuda_stream
    work = torch.empty(cd.cudecompAmdReduceInteriorWorkspaceBytes(1), dtype=torch.uint8, device="cuda")
    results = torch.zeros(2, dtype=torch.float64, device="cuda")
    compact = torch.empty(n * n * n, dtype=torch.float64, device="cuda")
    box_bytes = n * n * n * es
    res = {}
    for halo in ((1, 1, 1), (0, 0, 0)):
        p = cd.cudecompGetPencilInfo(h, gd, 0, halo)
        shape = [int(x) for x in p.shape]
        # small integers: every sum is exact, so the check below is an equality
        fields = [((torch.arange(int(p.size), device="cuda") * m) % 17 - 8).to(torch.float64) for m in (3, 5)]
        first = halo[0] + shape[0] * (halo[1] + shape[1] * halo[2])
        ss, ds = (1, shape[0], shape[0] * shape[1]), (1, n, n * n)

        def copy():
            cd.cudecompExtMove3D(fields[0].data_ptr() + first * es, compact.data_ptr(), es, (n, n, n), ss, ds, stream=st)

        def reduce_sum():
            cd.cudecompAmdReduceInterior(0, h, gd, [fields[0].data_ptr()], None, cd.REDUCE_SUM, results.data_ptr(), work.data_ptr(),
                                         cd.DOUBLE, halo, None, st)

        def reduce_dot():
            cd.cudecompAmdReduceInterior(0, h, gd, [fields[0].data_ptr()], [fields[1].data_ptr()], cd.REDUCE_DOT, results.data_ptr(),
                                         work.data_ptr(), cd.DOUBLE, halo, None, st)

        out = {}
        views = [f.view(shape[2], shape[1], shape[0])[halo[2]:shape[2] - halo[2], halo[1]:shape[1] - halo[1], halo[0]:shape[0] - halo[0]]
                 for f in fields]
        for name, fn, alg in (("sum", reduce_sum, box_bytes), ("dot", reduce_dot, 2 * box_bytes)):
            runs, kernels = {"copy": [], name: []}, {}
            for which, f in (("copy", copy), (name, fn), (name, fn), ("copy", copy)):
                runs[which] += _time(f, a.reps, a.calls)
                kernels[which] = cd.cudecompExtLastKernelName()
            out[name] = {"copy": _record(runs["copy"], 2 * box_bytes), "reduce": _record(runs[name], alg),
                         "copy_kernel": kernels["copy"], "reduce_kernel": kernels[name]}
            out[name]["reduce_over_copy"] = round(out[name]["reduce"]["median_ms"] / out[name]["copy"]["median_ms"], 3)
            fn()
            torch.cuda.synchronize()
            want = views[0].sum() if name == "sum" else (views[0] * views[1]).sum()
            out[name]["matches_torch"] = bool(results[0].item() == want.item() and results[1].item() == 0.0)
        copy()
        torch.cuda.synchronize()
        out["copy_matches_torch"] = bool(torch.equal(compact.view(n, n, n), views[0]))
        res["halo_%d%d%d" % halo] = out
        del fields, views
    line = json.dumps({"workload": "X pencil %d^3 fp64, single rank, halos (1,1,1) and (0,0,0): cudecompAmdReduceInteriorX SUM (one field) and "
                                   "DOT (two fields) next to the row copy of the interior box into a compact buffer, interleaved copy, "
                                   "reduction, reduction, copy; %d repetitions of %d calls" % (n, a.reps, a.calls),
                       "device": torch.cuda.get_device_name(0), "result": res})
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


if __name__ == "__main__":
    main()
