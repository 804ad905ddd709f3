#!/usr/bin/env python3
"""Interior plane updates next to the row copy of the same interior box (single rank, one GPU).

    python benchmark/interior_planes_bench.py [--n 512] [--reps 5] [--calls 10] [--json profiles/interior_planes_bench.json]

An X pencil of n^3 cells with halos (1, 1, 1), default memory order, so global dim d sits at memory position d: position 0 is served by
the column kernel, positions 1 and 2 by the row kernel.  cudecompAmdApplyPlanesInteriorX with ADD and MUL, for fp64, fp32 and
complex64, along each of the three dims, on one field and on three, is timed against the row copy of the same interior boxes into a
compact buffer (cudecompExtMove3D, as benchmark/interior_reduce_bench.py times it; one copy per field): the update reads and writes
the bytes the copy reads and writes.  No ratio is fixed in advance.  All arms of a data type and field count are timed interleaved in
one process -- copy, ADD dims 0 1 2, MUL dims 0 1 2, then the same backwards -- `reps` repetitions of `calls` calls each, between HIP
events; reported: every repetition, min / median / max, GB/s of the median against the algorithmic bytes, the ratio of the medians,
the copy's own min-max spread in that run, whether the update's median lies above the copy's median by more than that spread, and
the kernels' names.  After the timing every case is run once on fresh integer data and compared with torch.  One JSON line on stdout,
and in --json FILE."""
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
    n, halo, nmax = a.n, (1, 1, 1), 3
    h = cd.cudecompInit()
    gd = cd.cudecompGridDescCreate(h, cd.make_config((n, n, n), (1, 1)))
    st = torch.cuda.current_stream().cuda_stream
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo)
    shape = [int(x) for x in p.shape]
    assert [int(x) for x in p.order] == [0, 1, 2]
    first = halo[0] + shape[0] * (halo[1] + shape[1] * halo[2])
    ss, ds = (1, shape[0], shape[0] * shape[1]), (1, n, n * n)
    k = torch.arange(n, device="cuda")
    # coefficients that keep repeated updates bounded: ADD +-1 in turn along the dim, MUL a sign (complex: a power of i)
    add_c = torch.stack([(1 - 2 * (k % 2)).double(), (2 * (k % 2) - 1).double()], dim=1)
    mul_c = torch.stack([torch.tensor([1.0, 0.0, -1.0, 0.0], device="cuda")[k % 4].double(),
                         torch.tensor([0.0, 1.0, 0.0, -1.0], device="cuda")[k % 4].double()], dim=1)
    mul_r = torch.stack([(1 - 2 * (k % 2)).double(), torch.full((n,), float("nan"), device="cuda", dtype=torch.float64)], dim=1)
    res = {}
    for name, dtype, tt, es in (("fp64", cd.DOUBLE, torch.float64, 8), ("fp32", cd.FLOAT, torch.float32, 4),
                                ("complex64", cd.FLOAT_COMPLEX, torch.complex64, 8)):
        cplx = tt.is_complex
        box_bytes = n * n * n * es

        def fresh(m):
            v = ((torch.arange(int(p.size), device="cuda") * m) % 17 - 8).to(torch.float32)
            return torch.complex(v, -v + 1).contiguous() if cplx else v.to(tt)

        fields = [fresh(m) for m in (3, 5, 7)]
        compact = torch.empty(n * n * n, dtype=tt, device="cuda")
        coefs = {cd.PLANES_ADD: add_c.contiguous(), cd.PLANES_MUL: (mul_c if cplx else mul_r).contiguous()}
        for nf in (1, nmax):
            ptrs = [f.data_ptr() for f in fields[:nf]]

            def copy():
                for q in ptrs:
                    cd.cudecompExtMove3D(q + first * es, compact.data_ptr(), es, (n, n, n), ss, ds, stream=st)

            def update(op, dim):
                return lambda: cd.cudecompAmdApplyPlanesInterior(0, h, gd, ptrs, op, dim, coefs[op].data_ptr(), 0, 1.0, dtype, halo, None, st)

            arms = [("copy", copy)] + [("%s_dim%d" % (("add", "mul")[op], d), update(op, d)) for op in (0, 1) for d in range(3)]
            runs = {arm: [] for arm, _ in arms}
            for arm, fn in arms + arms[::-1]:
                runs[arm] += _time(fn, a.reps, a.calls)
                if arm == "copy":
                    copy_kernel = cd.cudecompExtLastKernelName()
            out = {"copy": _record(runs["copy"], 2 * nf * box_bytes), "copy_kernel": copy_kernel}
            spread = out["copy"]["max_ms"] - out["copy"]["min_ms"]
            out["copy"]["spread_ms"] = round(spread, 4)
            for arm, fn in arms[1:]:
                rec = _record(runs[arm], 2 * nf * box_bytes)
                op, d = (0 if arm.startswith("add") else 1), int(arm[-1])
                # one call on fresh data against torch
                for f, m in zip(fields[:nf], (3, 5, 7)):
                    f.copy_(fresh(m))
                before = [f.clone() for f in fields[:nf]]
                fn()
                rec["kernel"] = cd.cudecompExtLastKernelName()
                torch.cuda.synchronize()
                c = coefs[op]
                cv = torch.complex(c[:, 0], c[:, 1]).to(tt) if cplx else c[:, 0].to(tt)
                cshape = [1, 1, 1]
                cshape[2 - d] = n  # (numpy axis 2 - d is memory position d)
                ok = True
                for f, b in zip(fields[:nf], before):
                    want = b.clone()
                    inner = want.view(shape[2], shape[1], shape[0])[1:-1, 1:-1, 1:-1]
                    inner.copy_(inner + cv.view(cshape) if op == 0 else inner * cv.view(cshape))
                    ok = ok and bool(torch.equal(torch.view_as_real(f) if cplx else f, torch.view_as_real(want) if cplx else want))
                rec["matches_torch"] = ok
                rec["over_copy"] = round(rec["median_ms"] / out["copy"]["median_ms"], 3)
                rec["slower_than_copy_by_more_than_its_spread"] = bool(rec["median_ms"] > out["copy"]["median_ms"] + spread)
                out[arm] = rec
            res["%s_%d_field%s" % (name, nf, "s" if nf > 1 else "")] = out
        del fields, compact
        torch.cuda.empty_cache()
    line = json.dumps({"workload": "X pencil %d^3, single rank, halos (1,1,1): cudecompAmdApplyPlanesInteriorX ADD and MUL for fp64, fp32 and "
                                   "complex64 along each dim (memory position = dim) on 1 and 3 fields next to the row copy of the same "
                                   "interior boxes, interleaved; %d repetitions of %d calls, twice per arm" % (n, a.reps, a.calls),
                       "device": torch.cuda.get_device_name(0), "result": res})
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    cd.cudecompGridDescDestroy(h, gd)
    cd.cudecompFinalize(h)


if __name__ == "__main__":
    main()
