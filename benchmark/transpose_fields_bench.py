#!/usr/bin/env python3
"""Multi-field transpose timing on one rank: an out-of-place X -> Y -> Z -> Y -> X cycle of --fields N fp64 pencils of an n^3
grid (default layout) through cudecompAmdTransposeFields* (cudecomp_transpose_fields.h: one launch per hop for all N fields) and,
beside it on the same buffers, through N single cudecompTranspose* cycles (N launches per hop).  Per size: `--reps` repetitions of
`--calls` back-to-back cycles each, ms per cycle of every repetition, their min / median / max.  After the timing every field is
compared on the device with a clone moved by single calls.

--single-only times the N single cycles alone and touches nothing but cudecompTranspose*: that is the form to run on the PARENT
commit (whose library has no fields call), and the figure the fields cycle is held against -- never this tree's own single path.
The result is one JSON line; --json FILE also writes it to FILE."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ("XToY", "YToZ", "ZToY", "YToX")


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


def _record(ms):
    s = sorted(ms)
    return {"ms": [round(x, 4) for x in ms], "min_ms": round(s[0], 4), "median_ms": round(s[len(s) // 2], 4), "max_ms": round(s[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256, 512], help="edge lengths n of the n^3 grids")
    ap.add_argument("--fields", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--single-only", action="store_true", help="time the single cycles only (the form to run on the parent commit)")
    ap.add_argument("--json", metavar="FILE", default=None, help="also write the result line to FILE")
    a = ap.parse_args()
    import torch

    import cudecomp_amd as cd
    torch.cuda.set_device(0)
    h = cd.cudecompInit()
    st = torch.cuda.current_stream().cuda_stream
    n, res, differ = a.fields, {}, 0
    for size in a.sizes:
        gd = cd.cudecompGridDescCreate(h, cd.make_config((size,) * 3, (1, 1)))
        nel = max(cd.cudecompGetPencilInfo(h, gd, ax).size for ax in range(3))
        ws = max(cd.cudecompGetTransposeWorkspaceSize(h, gd), 1)
        bufs = [[torch.randn(nel, dtype=torch.float64, device="cuda") for _ in range(n)] for _ in range(2)]
        ptrs = [[t.data_ptr() for t in side] for side in bufs]
        work = cd.cudecompMalloc(h, gd, n * ws * 8)

        def single_cycle():
            for f in range(n):
                cur = 0
                for op in OPS:
                    cd.cudecompTranspose(op, h, gd, ptrs[cur][f], ptrs[1 - cur][f], work, cd.DOUBLE, stream=st)
                    cur = 1 - cur

        def fields_cycle():
            cur = 0
            for op in OPS:
                cd.cudecompTransposeFields(op, h, gd, ptrs[cur], ptrs[1 - cur], work, cd.DOUBLE, stream=st)
                cur = 1 - cur

        rec = {"pencil_MiB": round(nel * 8 / 2**20, 3), "single": _record(_time(single_cycle, a.reps, a.calls))}
        rec["single_kernel"] = cd.cudecompExtLastKernelName()
        if not a.single_only:
            rec["fields"] = _record(_time(fields_cycle, a.reps, a.calls))
            rec["fields_kernel"] = cd.cudecompExtLastKernelName()
            rec["fields_over_own_single"] = round(rec["fields"]["median_ms"] / rec["single"]["median_ms"], 3)  # (orientation only)
            # after the timing: fresh payloads, one cycle by the fields calls against single calls on clones, on the device
            for side in bufs:
                for t in side:
                    t.normal_()
            clones = [[t.clone() for t in side] for side in bufs]
            cur = 0
            for op in OPS:
                cd.cudecompTransposeFields(op, h, gd, ptrs[cur], ptrs[1 - cur], work, cd.DOUBLE, stream=st)
                for f in range(n):
                    cd.cudecompTranspose(op, h, gd, clones[cur][f].data_ptr(), clones[1 - cur][f].data_ptr(), work, cd.DOUBLE, stream=st)
                torch.cuda.synchronize()
                for side, cside in zip(bufs, clones):
                    for t, c in zip(side, cside):
                        differ += int(torch.count_nonzero(t.view(torch.int64) != c.view(torch.int64)))
                cur = 1 - cur
        res[str(size)] = rec
        cd.cudecompFree(h, gd, work)
        cd.cudecompGridDescDestroy(h, gd)
        del bufs
    line = json.dumps({"workload": "single rank, out of place, X->Y->Z->Y->X cycle of %d fp64 fields, default layout; %d repetitions of "
                                   "%d cycles; ms per cycle of all fields" % (n, a.reps, a.calls),
                       "single_only": bool(a.single_only), "device": torch.cuda.get_device_name(0), "result": res,
                       "cells_that_differ_from_single_calls": differ})
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    cd.cudecompFinalize(h)
    if differ:
        sys.exit("transpose_fields_bench.py: after a fields cycle %d cells differ from single calls on clones" % differ)


if __name__ == "__main__":
    main()
