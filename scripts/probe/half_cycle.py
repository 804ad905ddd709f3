"""fp16 against fp32 at the same bytes: X->Y->Z->Y->X of an 8-GiB pencil on a 1x1 grid, out of place, both layouts, 2 warm-up + 5
timed cycles with HIP events around every transpose (the method of bench.dtype_table).  Per hop: median ms, GB/s = 2 x pencil
bytes / ms, fraction of the 8 TB/s HBM peak, the kernel the library launched.  Two more fp16 cases without a target: an
odd-extent pencil and a halo-1 axis-contiguous pencil (rows at 2 mod 4 bytes: element-wise lanes).  One JSON line per case,
then one line with the fp16 / fp32 GB/s ratio per hop:
    python scripts/probe/half_cycle.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import torch  # noqa: E402

import bench  # noqa: E402
import cudecomp_amd as cd  # noqa: E402

CASES = [("fp16", cd.HALF, 2, (2048, 2048, 1024), None), ("fp32", cd.FLOAT, 4, (2048, 1024, 1024), None),
         ("fp16_odd", cd.HALF, 2, (2047, 2049, 1023), None), ("fp16_halo1", cd.HALF, 2, (2046, 2046, 1022), (1, 1, 1))]


def run(h, stream, name, dt, es, gdims, halo, layout, ac):
    row = {"case": name, "element_bytes": es, "gdims": list(gdims), "halo": halo, "layout": layout}
    gd = cd.cudecompGridDescCreate(h, cd.make_config(gdims, (1, 1), axis_contiguous=ac))
    pins = [cd.cudecompGetPencilInfo(h, gd, ax, halo) for ax in range(3)]
    nbytes = max(p.size for p in pins) * es
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    a = torch.randint(-2**62, 2**62, ((nbytes + 7) // 8,), dtype=torch.int64, device="cuda", generator=gen)
    keep = a.clone()
    b = torch.zeros_like(a)
    work = cd.cudecompMalloc(h, gd, max(cd.cudecompGetTransposeWorkspaceSize(h, gd), 1) * es)
    ms = {op: [] for op in cd.OPS}
    kernels = {}
    for it in range(2 + 5):
        cur, nxt = a, b
        for op in cd.OPS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cd.cudecompTranspose(op, h, gd, cur.data_ptr(), nxt.data_ptr(), work, dt, halo, halo, stream=stream)
            e1.record()
            kernels[op] = cd.cudecompExtLastKernelName()
            torch.cuda.synchronize()
            if it >= 2:
                ms[op].append(e0.elapsed_time(e1))
            cur, nxt = nxt, cur
    interior = gdims[0] * gdims[1] * gdims[2] * es
    row["round_trip_ok"] = bool(torch.equal(a, keep)) if halo is None else None  # (halo cells of the output: not written)
    row["per_op"] = []
    for op in cd.OPS:
        med = sorted(ms[op])[len(ms[op]) // 2]
        gbps = 2 * interior / (med * 1e-3) / 1e9
        row["per_op"].append({"op": op, "ms": round(med, 4), "ms_min": round(min(ms[op]), 4), "ms_max": round(max(ms[op]), 4),
                              "GBps": round(gbps, 1), "frac": round(gbps / bench.HBM_PEAK_GBPS, 4), "kernel": kernels[op]})
    row["cycle_ms"] = round(sum(o["ms"] for o in row["per_op"]), 4)
    del a, b, keep
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    torch.cuda.empty_cache()
    return row


def main():
    torch.zeros(1, device="cuda")
    h = cd.cudecompInit()
    stream = torch.cuda.current_stream().cuda_stream
    rows = {}
    for layout, ac in (("contiguous", (1, 1, 1)), ("default", (0, 0, 0))):
        for name, dt, es, gdims, halo in CASES:
            if name in ("fp16_odd", "fp16_halo1") and layout == "default" and halo:
                continue
            row = run(h, stream, name, dt, es, gdims, halo, layout, ac)
            rows[(name, layout)] = row
            print(json.dumps(row), flush=True)
    for layout in ("contiguous", "default"):
        h16, h32 = rows[("fp16", layout)]["per_op"], rows[("fp32", layout)]["per_op"]
        ratio = {a["op"]: round(a["GBps"] / b["GBps"], 3) for a, b in zip(h16, h32)}
        print(json.dumps({"layout": layout, "fp16_over_fp32_GBps": ratio, "target": 0.9,
                          "met": all(v >= 0.9 for v in ratio.values())}), flush=True)
    cd.cudecompFinalize(h)


if __name__ == "__main__":
    main()
