#!/usr/bin/env python3
"""Interior combinations next to the row copy of the same interior box and to torch.add over the whole allocation (single rank, one GPU).

    python benchmark/interior_combine_bench.py [--n 512] [--reps 5] [--calls 10] [--json profiles/interior_combine_bench.json]

An X pencil of n^3 cells with halos (1, 1, 1).  cudecompAmdCombineInteriorX with AXPY, XPBY, AXPBY and AX, for fp64 and fp32, on one
pair of fields and on three, both coefficients ratios of doubles in device memory, is timed against two yardsticks in the same
process: the row copy of the same interior boxes into a compact buffer (cudecompExtMove3D, as benchmark/interior_reduce_bench.py times
it; one copy per field) -- one read and one write of the box, where AX makes the same two passes and the other three operations make
three -- and torch.add(y, x, alpha=...) in place over the WHOLE allocation, ghost cells and all, which is what a caller without this
call does once the coefficient is on the host.  No ratio is fixed in advance.  All arms of a data type and field count are timed
interleaved -- copy, torch.add, the four operations, then the same backwards -- `reps` repetitions of `calls` calls each, between HIP
events; reported: every repetition, min / median / max, GB/s of the median against the algorithmic bytes, the ratios of the medians to
both yardsticks, the copy's own min-max spread, and the kernels' names.  After the timing every case is run once on fresh integer data
and compared with torch.  One JSON line on stdout, and in --json FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark.interior_reduce_bench import _record, _time  # noqa: E402

OPS = ("axpy", "xpby", "axpby", "ax")


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
    n, halo, nmax = a.n, (1, 1, 1), 3
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((n, n, n), (1, 1)))
    st = torch.cuda.current_stream().cuda_stream
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo)
    shape = [int(x) for x in p.shape]
    assert [int(x) for x in p.order] == [0, 1, 2]
    first = halo[0] + shape[0] * (halo[1] + shape[1] * halo[2])
    ss, ds = (1, shape[0], shape[0] * shape[1]), (1, n, n * n)
    nan = float("nan")
    # a = (1 * 1) / 2 and b = (-1 * 1) / -2: both 1/2, so that repeated updates stay bounded
    a_num, a_den = torch.tensor([1.0, nan], dtype=torch.float64).cuda(), torch.tensor([2.0, nan], dtype=torch.float64).cuda()
    b_num, b_den = torch.tensor([1.0, nan], dtype=torch.float64).cuda(), torch.tensor([-2.0, nan], dtype=torch.float64).cuda()
    kw = dict(a_num=a_num.data_ptr(), a_den=a_den.data_ptr(), a_scale=1.0, b_num=b_num.data_ptr(), b_den=b_den.data_ptr(), b_scale=-1.0)
    res = {}
    for name, dtype, tt, es in (("fp64", cd.DOUBLE, torch.float64, 8), ("fp32", cd.FLOAT, torch.float32, 4)):
        box_bytes = n * n * n * es

        def fresh(m):
            return ((torch.arange(int(p.size), device="cuda") * m) % 17 - 8).to(tt)

        ys, xs = [fresh(m) for m in (3, 5, 7)], [fresh(m) for m in (11, 13, 15)]
        compact = torch.empty(n * n * n, dtype=tt, device="cuda")
        for nf in (1, nmax):
            py, px = [f.data_ptr() for f in ys[:nf]], [f.data_ptr() for f in xs[:nf]]

            def copy():
                for q in px:
                    cd.cudecompExtMove3D(q + first * es, compact.data_ptr(), es, (n, n, n), ss, ds, stream=st)

            def torch_add():
                for y, x in zip(ys[:nf], xs[:nf]):
                    torch.add(y, x, alpha=0.5, out=y)

            def combine(op):
                return lambda: cd.cudecompAmdCombineInterior(0, h, gd, py, px, op, dtype, halo, None, stream=st, **kw)

            arms = [("copy", copy), ("torch_add", torch_add)] + [(OPS[op], combine(op)) for op in range(4)]
            runs = {arm: [] for arm, _ in arms}
            for arm, fn in arms + arms[::-1]:
                runs[arm] += _time(fn, a.reps, a.calls)
                if arm == "copy":
                    copy_kernel = cd.cudecompExtLastKernelName()
            out = {"copy": _record(runs["copy"], 2 * nf * box_bytes), "copy_kernel": copy_kernel,
                   "torch_add": _record(runs["torch_add"], 3 * nf * int(p.size) * es)}
            spread = out["copy"]["max_ms"] - out["copy"]["min_ms"]
            out["copy"]["spread_ms"] = round(spread, 4)
            for op, (arm, fn) in enumerate(arms[2:]):
                rec = _record(runs[arm], (2 if arm == "ax" else 3) * nf * box_bytes)
                # one call on fresh data against torch (small integers and halves: exact, fused or not)
                for f, m in zip(ys[:nf] + xs[:nf], (3, 5, 7)[:nf] + (11, 13, 15)[:nf]):
                    f.copy_(fresh(m))
                before = [f.clone() for f in ys[:nf]]
                fn()
                rec["kernel"] = cd.cudecompExtLastKernelName()
                torch.cuda.synchronize()
                ok = True
                for f, b, x in zip(ys[:nf], before, xs[:nf]):
                    want = b.clone()
                    inner = want.view(shape[2], shape[1], shape[0])[1:-1, 1:-1, 1:-1]
                    xi = x.view(shape[2], shape[1], shape[0])[1:-1, 1:-1, 1:-1]
                    inner.copy_((inner + 0.5 * xi, xi + 0.5 * inner, 0.5 * xi + 0.5 * inner, 0.5 * xi)[op])
                    ok = ok and bool(torch.equal(f, want))
                rec["matches_torch"] = ok
                rec["over_copy"] = round(rec["median_ms"] / out["copy"]["median_ms"], 3)
                rec["over_torch_add"] = round(rec["median_ms"] / out["torch_add"]["median_ms"], 3)
                rec["slower_than_copy_by_more_than_its_spread"] = bool(rec["median_ms"] > out["copy"]["median_ms"] + spread)
                out[arm] = rec
            res["%s_%d_field%s" % (name, nf, "s" if nf > 1 else "")] = out
        del ys, xs, compact
        torch.cuda.empty_cache()
    line = json.dumps({"workload": "X pencil %d^3, single rank, halos (1,1,1): cudecompAmdCombineInteriorX AXPY, XPBY, AXPBY and AX for fp64 and "
                                   "fp32 on 1 and 3 pairs of fields next to the row copy of the same interior boxes and to torch.add over the "
                                   "whole allocations, interleaved; %d repetitions of %d calls, twice per arm" % (n, a.reps, a.calls),
                       "device": torch.cuda.get_device_name(0), "result": res})
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


if __name__ == "__main__":
    main()
