#!/usr/bin/env python3
"""Interior profiles next to the scalar interior reduction and the row copy of the same box (single rank, one GPU).

    python benchmark/interior_profile_bench.py [--n 512] [--reps 5] [--calls 10] [--json profiles/interior_profile_bench.json]

An X pencil of n^3 fp64 cells with halos (1, 1, 1), default memory order, so global dim d sits at memory position d: position 0 is
served by the column kernel (or element by element where the row pitch is no multiple of 16 bytes), positions 1 and 2 by the row
kernel.  cudecompAmdProfileInteriorX with SUM and DOT, on one field and on three, kept along each of the three dims, is timed against
two yardsticks: cudecompAmdReduceInteriorX with the same operation on the same fields, and the row copy of the interior box of one
field into a compact buffer (cudecompExtMove3D).  No ratio is fixed in advance.  All arms are timed interleaved in one process -- copy,
scalar, dims 0 1 2, dims 2 1 0, scalar, copy -- `reps` repetitions of `calls` calls each, between HIP events; reported: every
repetition, min / median / max, GB/s of the median against the algorithmic bytes, the ratios of the medians and the kernels' names.
Every profile is checked once against torch on the same integer data.  One JSON line on stdout, and in --json FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchmark.interior_reduce_bench import _record, _time  # noqa: E402


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
    n, es, halo, nmax = a.n, 8, (1, 1, 1), 3
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((n, n, n), (1, 1)))
    st = torch.cuda.current_stream().cuda_stream
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo)
    shape = [int(x) for x in p.shape]
    assert [int(x) for x in p.order] == [0, 1, 2]
    work_p = torch.empty(cd.cudecompAmdProfileInteriorWorkspaceBytes(nmax, n), dtype=torch.uint8, device="cuda")
    work_r = torch.empty(cd.cudecompAmdReduceInteriorWorkspaceBytes(nmax), dtype=torch.uint8, device="cuda")
    prof = torch.zeros(nmax * n * 2, dtype=torch.float64, device="cuda")
    scal = torch.zeros(nmax * 2, dtype=torch.float64, device="cuda")
    compact = torch.empty(n * n * n, dtype=torch.float64, device="cuda")
    box_bytes = n * n * n * es
    # small integers: every sum is exact, so the checks below are equalities
    fa = [((torch.arange(int(p.size), device="cuda") * m) % 17 - 8).to(torch.float64) for m in (3, 5, 7)]
    fb = [((torch.arange(int(p.size), device="cuda") * m) % 13 - 6).to(torch.float64) for m in (2, 9, 11)]
    first = halo[0] + shape[0] * (halo[1] + shape[1] * halo[2])
    ss, ds = (1, shape[0], shape[0] * shape[1]), (1, n, n * n)
    view = lambda f: f.view(shape[2], shape[1], shape[0])[1:-1, 1:-1, 1:-1]  # noqa: E731

    def copy():
        cd.cudecompExtMove3D(fa[0].data_ptr() + first * es, compact.data_ptr(), es, (n, n, n), ss, ds, stream=st)

    res = {}
    for op, opname in ((cd.REDUCE_SUM, "sum"), (cd.REDUCE_DOT, "dot")):
        for nf in (1, nmax):
            pa, pb = [f.data_ptr() for f in fa[:nf]], ([f.data_ptr() for f in fb[:nf]] if op == cd.REDUCE_DOT else None)
            alg = nf * box_bytes * (2 if op == cd.REDUCE_DOT else 1)

            def scalar():
                cd.cudecompAmdReduceInterior(0, h, gd, pa, pb, op, scal.data_ptr(), work_r.data_ptr(), cd.DOUBLE, halo, None, st)

            def profile(dim):
                return lambda: cd.cudecompAmdProfileInterior(0, h, gd, pa, pb, op, dim, prof.data_ptr(), n, work_p.data_ptr(), cd.DOUBLE,
                                                             halo, None, st)

            arms = [("copy", copy), ("scalar", scalar)] + [("dim%d" % d, profile(d)) for d in range(3)]
            runs, kernels = {name: [] for name, _ in arms}, {}
            for name, fn in arms + arms[::-1]:
                runs[name] += _time(fn, a.reps, a.calls)
                kernels[name] = cd.cudecompExtLastKernelName() if name in ("copy", "scalar") else None
            out = {"copy": _record(runs["copy"], 2 * box_bytes), "scalar": _record(runs["scalar"], alg), "copy_kernel": kernels["copy"]}
            for d in range(3):
                name = "dim%d" % d
                rec = _record(runs[name], alg)
                profile(d)()
                rec["kernel"] = cd.cudecompExtLastKernelName()  # (the final stage does not change the name)
                torch.cuda.synchronize()
                got = prof.view(nmax, n, 2)[:nf]
                ok = True
                for f in range(nf):
                    cells = view(fa[f]) if op == cd.REDUCE_SUM else view(fa[f]) * view(fb[f])
                    want = cells.sum(dim=[x for x in range(3) if x != 2 - d])  # (numpy axis 2 - d is memory position d)
                    ok = ok and bool(torch.equal(got[f, :, 0], want)) and bool((got[f, :, 1] == 0).all())
                rec["matches_torch"] = ok
                rec["over_scalar"] = round(rec["median_ms"] / out["scalar"]["median_ms"], 3)
                rec["over_copy"] = round(rec["median_ms"] / out["copy"]["median_ms"], 3)
                out[name] = rec
            res["%s_%d_field%s" % (opname, nf, "s" if nf > 1 else "")] = out
    line = json.dumps({"workload": "X pencil %d^3 fp64, single rank, halos (1,1,1): cudecompAmdProfileInteriorX SUM and DOT on 1 and 3 "
                                   "fields kept along each dim (memory position = dim) next to cudecompAmdReduceInteriorX on the same fields "
                                   "and the row copy of one field's interior box, interleaved; %d repetitions of %d calls, twice per arm"
                                   % (n, a.reps, a.calls),
                       "device": torch.cuda.get_device_name(0), "result": res})
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


if __name__ == "__main__":
    main()
