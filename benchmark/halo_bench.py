#!/usr/bin/env python3
"""Halo timing on one rank: the per-rank X pencil of BASELINE config 5 (2048 x 2048 x 1024 fp64 on a
2x4 grid -> 2048 x 1024 x 256 per rank) treated as a periodic single-rank grid, so every dim exercises the
face kernels: cudecompUpdateHalosX (periodic self copy; reference include/internal/halo.h:165-193) and, beside
it on the same pencil, cudecompAmdAccumulateHalosX (cudecomp_amd.h: the two face additions) and, with --fill,
cudecompAmdFillHalosX (cudecomp_amd_fill.h: the two halos set to zero) and, with --accumulate-clear,
cudecompAmdAccumulateAndClearHalosX (cudecomp_amd_fill.h: both in the accumulation's launches) and, with --reflect,
cudecompAmdReflectHalosX (cudecomp_amd_reflect.h) on the same pencil as a NON-periodic single rank: the odd mirror, centering 0 --
per dim the cells the periodic update writes, as many cells read, the same two sibling moves in one launch (4 * face bytes) and, with
--fold / --fold-clear, cudecompAmdFoldHalosX (cudecomp_halo_fold.h), the reflection's transpose, on the same non-periodic single rank
with parity -1, centering 0 and clear 0 / 1: the reflection's two sibling moves the other way round, the destinations read as well
(6 * face bytes), the ghost cells zeroed as well (8 * face bytes) and, with --fields N, cudecompAmdUpdateFieldHalosX
(cudecomp_halo_fields.h) on N such pencils, periodic: the update's two wrap copies for all N in one launch (N * 4 * face bytes) and,
with --accumulate --fields N / --accumulate-clear --fields N, cudecompAmdAccumulateFieldHalosX (cudecomp_halo_accumulate_fields.h) with
clear 0 / 1 on N such pencils: the two wrap additions for all N in one launch (N * 6 / N * 8 * face bytes) and, with --wall-fields N,
cudecompAmdReflectFieldHalosX and cudecompAmdFoldFieldHalosX (cudecomp_halo_wall_fields.h; centering 0, clear 0, parities -1, +1, -1, ...)
on N such pencils as a NON-periodic single rank: one call for all N against N single calls with the same parities, the two arms
timed alternately in both orders (fields first, then singles; singles first, then fields) with every shape warmed up before and, with
--wall-values, cudecompAmdSetWallHalosX (cudecomp_halo_wall_values.h; parity -1, centering 0, both sides, one addend per layer) next to
cudecompAmdReflectHalosX with parity -1 on the same pencil, walls along dims 1 and 2 (dim 0 periodic), for fp64 and for fp16: the
reflection's two sibling moves plus one addition per element (4 * face bytes), the two calls timed in the order reflection, wall
values, wall values, reflection and, with --wall-value-fields N, cudecompAmdSetWallFieldHalosX (cudecomp_halo_wall_value_fields.h;
parities -1, +1, -1, ..., centering 0, both sides, addends of its own for every field) on N such pencils next to N single
cudecompAmdSetWallHalosX calls with the same parities and addends, walls along dims 1 and 2, for fp64 and for fp16, timed in the order
singles, fields, fields, singles; afterwards every cell of every field against the single calls on clones and, with --wall-planes,
cudecompAmdSetWallPlaneHalosX (cudecomp_halo_wall_planes.h; parity -1, centering 0, both sides, two device planes whose entries differ
from cell to cell) next to cudecompAmdSetWallHalosX on the same non-periodic pencil, walls along dims 0, 1 and 2, for fp64 and for
fp16: the wall values' two sibling moves plus one plane read per element (6 * face bytes against 4), timed in the order values,
planes, planes, values; dim 0 is the fastest memory axis, where both calls run element by element.
Per dim: `--reps` repetitions of `--calls` back-to-back calls each, ms per call of every repetition, their
min / median / max, and GB/s of the median against the algorithmic bytes (update: 2 faces read + written,
4 * face bytes; accumulation: 2 faces read, 2 destinations read and written, 6 * face bytes; fill: 2 halos written, 2 * face
bytes; accumulate-and-clear: the sum of the last two, 8 * face bytes).  --fill also checks on the device that afterwards no ghost cell holds anything but zero and no interior cell changed,
and times one contiguous 64 MiB fill with cached and with non-temporal stores (the store policy of the fill kernels)."""
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
    ap.add_argument("--halo", type=int, default=1, help="halo width along every dim")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--update-only", action="store_true", help="time cudecompUpdateHalosX only")
    ap.add_argument("--fill", action="store_true", help="also time cudecompAmdFillHalosX (value zero), after the other passes")
    ap.add_argument("--accumulate-clear", action="store_true",
                    help="also time cudecompAmdAccumulateAndClearHalosX, after the other passes")
    ap.add_argument("--reflect", action="store_true",
                    help="also time cudecompAmdReflectHalosX (non-periodic, parity -1, centering 0), after the other passes")
    ap.add_argument("--fold", action="store_true",
                    help="also time cudecompAmdFoldHalosX (non-periodic, parity -1, centering 0, clear 0), after the other passes")
    ap.add_argument("--fold-clear", action="store_true", help="... and with clear 1")
    ap.add_argument("--fields", type=int, default=0, metavar="N",
                    help="also time cudecompAmdUpdateFieldHalosX on N pencils (periodic; one launch for all of them), after the other "
                         "passes, and compare every field on the device with a clone updated by single calls")
    ap.add_argument("--accumulate", action="store_true",
                    help="with --fields N: also time cudecompAmdAccumulateFieldHalosX (clear 0) on the N pencils and compare every field "
                         "on the device with a clone accumulated by single calls; with --accumulate-clear --fields N: the same with clear 1")
    ap.add_argument("--wall-fields", type=int, default=0, metavar="N",
                    help="also time cudecompAmdReflectFieldHalosX / cudecompAmdFoldFieldHalosX on N pencils (non-periodic) against N single "
                         "calls, both orders of the two arms, and compare every field on the device with a clone served by single calls")
    ap.add_argument("--wall-values", action="store_true",
                    help="also time cudecompAmdSetWallHalosX (parity -1, centering 0, both sides) next to cudecompAmdReflectHalosX with "
                         "parity -1, walls along dims 1 and 2, fp64 and fp16, after the other passes")
    ap.add_argument("--wall-planes", action="store_true",
                    help="also time cudecompAmdSetWallPlaneHalosX (parity -1, centering 0, both sides, planes whose entries differ from cell "
                         "to cell) next to cudecompAmdSetWallHalosX at the same shapes, walls along dims 0, 1 and 2 (non-periodic), fp64 and "
                         "fp16, in the order values, planes, planes, values; afterwards the low wall's ghost cells against the plane")
    ap.add_argument("--wall-value-fields", type=int, default=0, metavar="N",
                    help="also time cudecompAmdSetWallFieldHalosX on N pencils (centering 0, both sides, a parity and addends per field) next "
                         "to N single cudecompAmdSetWallHalosX calls, walls along dims 1 and 2, fp64 and fp16, in the order singles, fields, "
                         "fields, singles, and compare every field on the device with a clone served by single calls")
    ap.add_argument("--gdims", type=int, nargs=3, default=[2048, 1024, 256], metavar="N",
                    help="the pencil (default: config 5's per-rank X pencil; 64 64 64: a pencil on which fixed cost dominates)")
    ap.add_argument("--json", metavar="FILE", default=None, help="also write the result line to FILE")
    a = ap.parse_args()
    import torch

    import cudecomp_amd as cd
    torch.cuda.set_device(0)
    gdims, halo = tuple(a.gdims), (a.halo,) * 3
    h = cd.cudecompInit()
    res = {}
    gd = cd.cudecompGridDescCreate(h, cd.make_config(gdims, (1, 1)))
    p = cd.cudecompGetPencilInfo(h, gd, 0, halo)
    data = torch.zeros(p.size, dtype=torch.float64, device="cuda")
    ws = max(cd.cudecompGetHaloWorkspaceSize(h, gd, 0, halo), 1)
    work = cd.cudecompMalloc(h, gd, ws * 8)
    st = torch.cuda.current_stream().cuda_stream
    shape = list(p.shape)
    faces = [halo[dim] * (shape[(dim + 1) % 3]) * (shape[(dim + 2) % 3]) for dim in range(3)]
    # two passes: every update first, the accumulations afterwards -- the update figures are then taken exactly as with
    # --update-only (nothing else touches the pencil between their repetitions)
    for dim in range(3):
        ms = _time(lambda: cd.cudecompUpdateHalos(0, h, gd, data.data_ptr(), work, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st),
                   a.reps, a.calls)
        res["dim%d" % dim] = {"face_MiB": round(faces[dim] * 8 / 2**20, 2), "update": _record(ms, 4 * faces[dim] * 8)}
    for dim in range(3):
        if a.update_only:
            break
        rec = res["dim%d" % dim]
        ms = _time(lambda: cd.cudecompAccumulateHalos(0, h, gd, data.data_ptr(), work, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st),
                   a.reps, a.calls)
        rec["accumulate"] = _record(ms, 6 * faces[dim] * 8)
        rec["accumulate_kernel"] = cd.cudecompExtLastKernelName()
        rec["accumulate_over_update"] = round(rec["accumulate"]["median_ms"] / rec["update"]["median_ms"], 3)
    extra = {}
    if a.fill:
        data.fill_(1.0)  # the fills store zero: what they wrote, and only that, shows afterwards
        for dim in range(3):
            rec = res["dim%d" % dim]
            ms = _time(lambda: cd.cudecompFillHalos(0, h, gd, data.data_ptr(), cd.DOUBLE, halo, (1, 1, 1), dim, stream=st), a.reps, a.calls)
            rec["fill"] = _record(ms, 2 * faces[dim] * 8)
            rec["fill_kernel"] = cd.cudecompExtLastKernelName()
            rec["fill_over_update"] = round(rec["fill"]["median_ms"] / rec["update"]["median_ms"], 3)
        cells = data.view(shape[2], shape[1], shape[0])
        interior = cells[a.halo:shape[2] - a.halo, a.halo:shape[1] - a.halo, a.halo:shape[0] - a.halo]
        inside = int(torch.count_nonzero(interior))
        extra["ghost_cells_not_zero"] = int(torch.count_nonzero(cells)) - inside
        extra["interior_cells_changed"] = interior.numel() - inside
        # store policy: one contiguous 64 MiB move, cached (force bit 2) against non-temporal (what the size rule picks)
        n = (64 << 20) // 8
        policy = {}
        for name, force in (("cached", 4), ("non_temporal", 0), ("cached_again", 4), ("non_temporal_again", 0)):
            ms = _time(lambda: cd.cudecompExtFill3D(data.data_ptr(), 8, None, (n, 1, 1), (1, 0, 0), force, st), a.reps, a.calls)
            policy[name] = dict(_record(ms, n * 8), kernel=cd.cudecompExtLastKernelName())
        extra["store_policy_64MiB"] = policy
    if a.accumulate_clear:
        for dim in range(3):
            rec = res["dim%d" % dim]
            ms = _time(lambda: cd.cudecompAccumulateAndClearHalos(0, h, gd, data.data_ptr(), work, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st),
                       a.reps, a.calls)
            rec["accumulate_clear"] = _record(ms, 8 * faces[dim] * 8)
            rec["accumulate_clear_kernel"] = cd.cudecompExtLastKernelName()
            if "accumulate" in rec and "fill" in rec:  # (this tree's own two calls: for orientation, not the figure to hold it against)
                rec["accumulate_clear_over_accumulate_plus_fill"] = round(
                    rec["accumulate_clear"]["median_ms"] / (rec["accumulate"]["median_ms"] + rec["fill"]["median_ms"]), 3)
        # every call leaves the ghost cells along its dim zero: after dims 0, 1, 2 none holds anything else
        data.fill_(1.0)
        for dim in (2, 1, 0):
            cd.cudecompAccumulateAndClearHalos(0, h, gd, data.data_ptr(), work, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st)
        cells = data.view(shape[2], shape[1], shape[0])
        interior = cells[a.halo:shape[2] - a.halo, a.halo:shape[1] - a.halo, a.halo:shape[0] - a.halo]
        extra["ghost_cells_not_zero_after_accumulate_clear"] = int(torch.count_nonzero(cells)) - int(torch.count_nonzero(interior))
        extra["interior_sum_after_accumulate_clear"] = float(interior.sum())  # every cell of the pencil lands in the interior once
        extra["cells"] = int(cells.numel())
    if a.reflect:
        for dim in range(3):
            rec = res["dim%d" % dim]
            ms = _time(lambda: cd.cudecompReflectHalos(0, h, gd, data.data_ptr(), cd.DOUBLE, -1, 0, halo, (0, 0, 0), dim, stream=st),
                       a.reps, a.calls)
            rec["reflect"] = _record(ms, 4 * faces[dim] * 8)
            rec["reflect_kernel"] = cd.cudecompExtLastKernelName()
            rec["reflect_over_update"] = round(rec["reflect"]["median_ms"] / rec["update"]["median_ms"], 3)
        # the even mirror of an interior of ones over dims 0, 1, 2 leaves a one in every cell, edges and corners included
        data.zero_()
        cells = data.view(shape[2], shape[1], shape[0])
        cells[a.halo:shape[2] - a.halo, a.halo:shape[1] - a.halo, a.halo:shape[0] - a.halo] = 1.0
        for dim in range(3):
            cd.cudecompReflectHalos(0, h, gd, data.data_ptr(), cd.DOUBLE, 1, 0, halo, (0, 0, 0), dim, stream=st)
        extra["cells_not_one_after_reflect"] = int(cells.numel()) - int(torch.count_nonzero(cells == 1.0))
    if a.wall_values:
        periods = (1, 0, 0)
        for dtype, tdtype, es, label in ((cd.DOUBLE, torch.float64, 8, "fp64"), (cd.HALF, torch.float16, 2, "fp16")):
            pencil = torch.ones(p.size, dtype=tdtype, device="cuda")
            low, high = [0.5 * (k + 1) for k in range(a.halo)], [-0.25 * (k + 1) for k in range(a.halo)]
            reflect = lambda: cd.cudecompReflectHalos(0, h, gd, pencil.data_ptr(), dtype, -1, 0, halo, periods, dim, stream=st)
            wall = lambda: cd.cudecompAmdSetWallHalos(0, h, gd, pencil.data_ptr(), dtype, -1, 0, 3, low, high, halo, periods, dim, stream=st)
            for dim in (1, 2):
                rec = res["dim%d" % dim].setdefault("wall_values", {})
                runs, kernels = {"reflect": [], "wall_values": []}, {}
                for name, fn in (("reflect", reflect), ("wall_values", wall), ("wall_values", wall), ("reflect", reflect)):
                    runs[name] += _time(fn, a.reps, a.calls)
                    kernels[name] = cd.cudecompExtLastKernelName()
                out = {name: _record(ms, 4 * faces[dim] * es) for name, ms in runs.items()}
                out["reflect_kernel"], out["wall_values_kernel"] = kernels["reflect"], kernels["wall_values"]
                out["wall_values_over_reflect"] = round(out["wall_values"]["median_ms"] / out["reflect"]["median_ms"], 3)
                rec[label] = out
            # what the call wrote: from an interior of ones, parity -1 and a_k leave -1 + a_k in ghost layer k of the low wall of dim 1
            pencil.fill_(1.0)
            cd.cudecompAmdSetWallHalos(0, h, gd, pencil.data_ptr(), dtype, -1, 0, 3, low, high, halo, periods, 1, stream=st)
            cells = pencil.view(shape[2], shape[1], shape[0])
            want = torch.tensor([low[a.halo - 1 - j] - 1.0 for j in range(a.halo)], dtype=tdtype, device="cuda")
            got = cells[a.halo, :a.halo, a.halo]
            extra["wall_values_wrong_cells_" + label] = int(torch.count_nonzero(got != want))
    if a.wall_planes:
        periods = (0, 0, 0)
        for dtype, tdtype, es, label in ((cd.DOUBLE, torch.float64, 8, "fp64"), (cd.HALF, torch.float16, 2, "fp16")):
            pencil = torch.ones(p.size, dtype=tdtype, device="cuda")
            low, high = [0.5 * (k + 1) for k in range(a.halo)], [-0.25 * (k + 1) for k in range(a.halo)]
            for dim in range(3):
                # the planes of this dim: the pencil's shape with the extent along `dim` replaced by the halo; entries that differ
                # from cell to cell (multiples of 1/4 below 64: exact in fp16)
                pshape, elements = cd.wall_plane_shape(p, dim, halo)
                planes = [((torch.arange(elements, device="cuda") * (3 + side)) % 251).to(tdtype) * 0.25 for side in (0, 1)]
                values = lambda: cd.cudecompAmdSetWallHalos(0, h, gd, pencil.data_ptr(), dtype, -1, 0, 3, low, high, halo, periods, dim, stream=st)
                wall = lambda: cd.cudecompAmdSetWallPlaneHalos(0, h, gd, pencil.data_ptr(), dtype, -1, 0, 3, planes[0].data_ptr(),
                                                               planes[1].data_ptr(), halo, periods, dim, stream=st)
                rec = res["dim%d" % dim].setdefault("wall_planes", {})
                runs, kernels = {"wall_values": [], "wall_planes": []}, {}
                for name, fn in (("wall_values", values), ("wall_planes", wall), ("wall_planes", wall), ("wall_values", values)):
                    runs[name] += _time(fn, a.reps, a.calls)
                    kernels[name] = cd.cudecompExtLastKernelName()
                out = {"wall_values": _record(runs["wall_values"], 4 * faces[dim] * es), "wall_planes": _record(runs["wall_planes"], 6 * faces[dim] * es)}
                out["wall_values_kernel"], out["wall_planes_kernel"] = kernels["wall_values"], kernels["wall_planes"]
                out["wall_planes_over_wall_values"] = round(out["wall_planes"]["median_ms"] / out["wall_values"]["median_ms"], 3)
                out["fastest_memory_axis"] = int(p.order[0]) == dim
                rec[label] = out
                # what the call wrote: from an interior of ones, parity -1 leaves -1 + plane entry in every ghost cell of the low wall
                pencil.fill_(1.0)
                wall()
                cells = pencil.view(shape[2], shape[1], shape[0])
                plane = planes[0].view(pshape[2], pshape[1], pshape[0])
                at = [slice(a.halo, shape[2] - a.halo), slice(a.halo, shape[1] - a.halo), slice(a.halo, shape[0] - a.halo)]
                ax = 2 - [int(x) for x in p.order].index(dim)
                wrong = 0
                for k in range(a.halo):  # ghost layer k sits at index halo - 1 - k of the pencil, index k of the plane
                    at[ax] = a.halo - 1 - k
                    got = cells[tuple(at)]
                    at[ax] = k
                    wrong += int(torch.count_nonzero(got != plane[tuple(at)] - 1.0))
                extra["wall_planes_wrong_cells_%s_dim%d" % (label, dim)] = wrong
                pencil.fill_(1.0)
    for clear, wanted in ((0, a.fold), (1, a.fold_clear)):
        if not wanted:
            continue
        name = "fold_clear" if clear else "fold"
        data.zero_()
        for dim in range(3):
            rec = res["dim%d" % dim]
            ms = _time(lambda: cd.cudecompFoldHalos(0, h, gd, data.data_ptr(), cd.DOUBLE, -1, 0, clear, halo, (0, 0, 0), dim, stream=st),
                       a.reps, a.calls)
            rec[name] = _record(ms, (8 if clear else 6) * faces[dim] * 8)
            rec[name + "_kernel"] = cd.cudecompExtLastKernelName()
            rec[name + "_over_update"] = round(rec[name]["median_ms"] / rec["update"]["median_ms"], 3)
        # a pencil of ones folded with parity +1 and clearing along dims 2, 1, 0: an interior cell holds the number of cells of the
        # pencil that mirror onto it -- per dim one more for every wall it lies within `halo` cells of -- and every ghost cell zero
        data.fill_(1.0)
        cells = data.view(shape[2], shape[1], shape[0])
        for dim in (2, 1, 0):
            cd.cudecompFoldHalos(0, h, gd, data.data_ptr(), cd.DOUBLE, 1, 0, 1, halo, (0, 0, 0), dim, stream=st)
        count = []
        for dim in range(3):
            g = shape[dim] - 2 * a.halo
            c = torch.ones(g, dtype=torch.float64, device="cuda")
            c[:a.halo] += 1.0
            c[g - a.halo:] += 1.0
            count.append(c)
        expected = count[2][:, None, None] * count[1][None, :, None] * count[0][None, None, :]
        interior = cells[a.halo:shape[2] - a.halo, a.halo:shape[1] - a.halo, a.halo:shape[0] - a.halo]
        extra["interior_cells_with_another_count_after_" + name] = int(torch.count_nonzero(interior != expected))
        extra["ghost_cells_not_zero_after_" + name] = int(torch.count_nonzero(cells)) - int(torch.count_nonzero(interior))
    if a.fields:
        # N pencils of the same descriptor; the figure to hold against is N times the update's median of the same dim
        n = a.fields
        fields = [torch.randn(p.size, dtype=torch.float64, device="cuda") for _ in range(n)]
        fwork = cd.cudecompMalloc(h, gd, n * ws * 8)
        ptrs = [t.data_ptr() for t in fields]
        for dim in range(3):
            rec = res["dim%d" % dim]
            ms = _time(lambda: cd.cudecompUpdateFieldHalos(0, h, gd, ptrs, fwork, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st), a.reps, a.calls)
            rec["fields"] = _record(ms, n * 4 * faces[dim] * 8)
            rec["fields_kernel"] = cd.cudecompExtLastKernelName()
            rec["fields_over_n_updates"] = round(rec["fields"]["median_ms"] / (n * rec["update"]["median_ms"]), 3)
        # after the timing: fresh payloads, dims 0, 1, 2 by the fields call against single calls on clones, on the device
        differ = 0
        for t in fields:
            t.normal_()
        clones = [t.clone() for t in fields]
        for dim in range(3):
            cd.cudecompUpdateFieldHalos(0, h, gd, ptrs, fwork, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st)
            for c in clones:
                cd.cudecompUpdateHalos(0, h, gd, c.data_ptr(), work, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st)
        torch.cuda.synchronize()
        for t, c in zip(fields, clones):
            differ += int(torch.count_nonzero(t.view(torch.int64) != c.view(torch.int64)))
        extra["n_fields"] = n
        extra["field_cells_that_differ_from_single_calls"] = differ
        # the accumulation of the N pencils in one call; the figure to hold against is N times the single call's median of the same dim
        for clear, wanted in ((0, a.accumulate), (1, a.accumulate_clear)):
            if not wanted:
                continue
            name, single = ("accumulate_clear", cd.cudecompAccumulateAndClearHalos) if clear else ("accumulate", cd.cudecompAccumulateHalos)
            for t in fields:
                t.normal_()
            for dim in range(3):
                rec = res["dim%d" % dim]
                ms = _time(lambda: cd.cudecompAccumulateFieldHalos(0, h, gd, ptrs, fwork, cd.DOUBLE, halo, (1, 1, 1), dim, None, clear, st),
                           a.reps, a.calls)
                rec[name + "_fields"] = _record(ms, n * (8 if clear else 6) * faces[dim] * 8)
                rec[name + "_fields_kernel"] = cd.cudecompExtLastKernelName()
                rec[name + "_fields_over_n_singles"] = round(rec[name + "_fields"]["median_ms"] / (n * rec[name]["median_ms"]), 3)
            # after the timing: fresh payloads, dims 2, 1, 0 by the fields call against single calls on clones, on the device
            differ = 0
            for t in fields:
                t.normal_()
            clones = [t.clone() for t in fields]
            for dim in (2, 1, 0):
                cd.cudecompAccumulateFieldHalos(0, h, gd, ptrs, fwork, cd.DOUBLE, halo, (1, 1, 1), dim, None, clear, st)
                for c in clones:
                    single(0, h, gd, c.data_ptr(), work, cd.DOUBLE, halo, (1, 1, 1), dim, stream=st)
            torch.cuda.synchronize()
            for t, c in zip(fields, clones):
                differ += int(torch.count_nonzero(t.view(torch.int64) != c.view(torch.int64)))
            extra[name + "_field_cells_that_differ_from_single_calls"] = differ
        cd.cudecompFree(h, gd, fwork)
    if a.wall_fields:
        n = a.wall_fields
        wall = [torch.randn(p.size, dtype=torch.float64, device="cuda") for _ in range(n)]
        wptrs = [t.data_ptr() for t in wall]
        parities = [1 if f % 3 == 1 else -1 for f in range(n)]
        none = (0, 0, 0)

        def arms(op, dim):
            if op == "reflect":
                def many():
                    cd.cudecompReflectFieldHalos(0, h, gd, wptrs, cd.DOUBLE, parities, 0, halo, none, dim, stream=st)

                def singles():
                    for q, s in zip(wptrs, parities):
                        cd.cudecompReflectHalos(0, h, gd, q, cd.DOUBLE, s, 0, halo, none, dim, stream=st)
            else:
                def many():
                    cd.cudecompFoldFieldHalos(0, h, gd, wptrs, cd.DOUBLE, parities, 0, 0, halo, none, dim, stream=st)

                def singles():
                    for q, s in zip(wptrs, parities):
                        cd.cudecompFoldHalos(0, h, gd, q, cd.DOUBLE, s, 0, 0, halo, none, dim, stream=st)
            return many, singles

        for op, per_byte in (("reflect", 4), ("fold", 6)):
            for dim in range(3):
                rec = res["dim%d" % dim]
                many, singles = arms(op, dim)
                for t in wall:
                    t.normal_()
                out = {}
                for order in ("fields_first", "singles_first"):  # (_time warms every arm up before it times it)
                    pair = [("fields", many), ("singles", singles)]
                    for arm, fn in (pair if order == "fields_first" else pair[::-1]):
                        out[order + "_" + arm] = _record(_time(fn, a.reps, a.calls), n * per_byte * faces[dim] * 8)
                many()
                out["kernel"] = cd.cudecompExtLastKernelName()
                out["fields_over_singles"] = [round(out[o + "_fields"]["median_ms"] / out[o + "_singles"]["median_ms"], 3)
                                              for o in ("fields_first", "singles_first")]
                rec[op + "_wall_fields"] = out
        # after the timing: fresh payloads, reflection along dims 0, 1, 2 and fold along 2, 1, 0 by the field calls against single calls
        # on clones, on the device
        for t in wall:
            t.normal_()
        clones = [t.clone() for t in wall]
        for op, dims in (("reflect", (0, 1, 2)), ("fold", (2, 1, 0))):
            for dim in dims:
                many, _ = arms(op, dim)
                many()
                for c, s in zip(clones, parities):
                    if op == "reflect":
                        cd.cudecompReflectHalos(0, h, gd, c.data_ptr(), cd.DOUBLE, s, 0, halo, none, dim, stream=st)
                    else:
                        cd.cudecompFoldHalos(0, h, gd, c.data_ptr(), cd.DOUBLE, s, 0, 0, halo, none, dim, stream=st)
        torch.cuda.synchronize()
        extra["n_wall_fields"] = n
        extra["wall_field_cells_that_differ_from_single_calls"] = sum(
            int(torch.count_nonzero(t.view(torch.int64) != c.view(torch.int64))) for t, c in zip(wall, clones))
    if a.wall_value_fields:
        n = a.wall_value_fields
        periods = (1, 0, 0)
        parities = [1 if f % 3 == 1 else -1 for f in range(n)]
        # field f, ghost layer k: multiples of 1/8 that differ from field to field and layer to layer, exact in fp16
        low = [[0.5 * (k + 1) + 0.125 * f for k in range(a.halo)] for f in range(n)]
        high = [[-0.25 * (k + 1) - 0.125 * f for k in range(a.halo)] for f in range(n)]
        flat_low, flat_high = [x for v in low for x in v], [x for v in high for x in v]
        extra["n_wall_value_fields"] = n
        for dtype, tdtype, es, label in ((cd.DOUBLE, torch.float64, 8, "fp64"), (cd.HALF, torch.float16, 2, "fp16")):
            pencils = [torch.randn(p.size, dtype=torch.float64, device="cuda").to(tdtype) for _ in range(n)]
            wptrs = [t.data_ptr() for t in pencils]

            def many(dim, ptrs=wptrs):
                cd.cudecompAmdSetWallFieldHalos(0, h, gd, ptrs, dtype, parities, 0, 3, flat_low, flat_high, halo, periods, dim, stream=st)

            def singles(dim, ptrs=wptrs):
                for f, q in enumerate(ptrs):
                    cd.cudecompAmdSetWallHalos(0, h, gd, q, dtype, parities[f], 0, 3, low[f], high[f], halo, periods, dim, stream=st)

            for dim in (1, 2):
                rec = res["dim%d" % dim].setdefault("wall_value_fields", {})
                runs, kernels = {"singles": [], "fields": []}, {}
                for name, fn in (("singles", singles), ("fields", many), ("fields", many), ("singles", singles)):
                    runs[name].append(_time(lambda: fn(dim), a.reps, a.calls))
                    kernels[name] = cd.cudecompExtLastKernelName()
                out = {name: _record(ms[0] + ms[1], n * 4 * faces[dim] * es) for name, ms in runs.items()}
                first, second = (sorted(ms)[len(ms) // 2] for ms in runs["singles"])
                out["singles_kernel"], out["fields_kernel"] = kernels["singles"], kernels["fields"]
                out["singles_first_run_median_ms"], out["singles_second_run_median_ms"] = round(first, 4), round(second, 4)
                out["singles_spread"] = round(abs(first - second) / min(first, second), 3)  # between the two runs of the yardstick
                out["fields_over_singles"] = round(out["fields"]["median_ms"] / out["singles"]["median_ms"], 3)
                rec[label] = out
            # after the timing: fresh payloads, dims 0, 1, 2 by the field call against single calls on clones, on the device
            for t in pencils:
                t.copy_(torch.randn(p.size, dtype=torch.float64, device="cuda").to(tdtype))
            clones = [t.clone() for t in pencils]
            for dim in range(3):
                many(dim)
                singles(dim, [c.data_ptr() for c in clones])
            torch.cuda.synchronize()
            bits = torch.int64 if es == 8 else torch.int16
            extra["wall_value_field_cells_that_differ_from_single_calls_" + label] = sum(
                int(torch.count_nonzero(t.view(bits) != c.view(bits))) for t, c in zip(pencils, clones))
            del pencils, clones
    cd.cudecompFree(h, gd, work)
    cd.cudecompGridDescDestroy(h, gd)
    line = json.dumps(dict({"workload": "X pencil %dx%dx%d fp64 + halo %d, single rank, periodic where not said otherwise, per dim: update (self copy), "
                                        "accumulation (self add)%s; %d repetitions of %d calls"
                                        % (gdims + (a.halo,) + ((" and fill (zero)" if a.fill else "") + (" and accumulate-and-clear" if a.accumulate_clear else "")
                                           + (" and reflection (non-periodic, odd mirror, centering 0)" if a.reflect else "")
                                           + (" and fold (non-periodic, parity -1, centering 0)" if a.fold else "")
                                           + (" and fold with clear" if a.fold_clear else "")
                                           + (" and the update of %d pencils in one call" % a.fields if a.fields else "")
                                           + (" and their accumulation in one call" if a.fields and a.accumulate else "")
                                           + (" and their accumulate-and-clear in one call" if a.fields and a.accumulate_clear else "")
                                           + (" and the reflection and the fold of %d pencils in one call (non-periodic)" % a.wall_fields
                                              if a.wall_fields else "")
                                           + (" and wall values next to the reflection (walls along dims 1 and 2, fp64 and fp16)" if a.wall_values else "")
                                           + (" and the wall values of %d pencils in one call next to %d single calls (walls along dims 1 and 2, fp64 "
                                              "and fp16)" % (a.wall_value_fields, a.wall_value_fields) if a.wall_value_fields else "")
                                           + (" and wall planes next to the wall values (non-periodic, walls along dims 0, 1 and 2, fp64 and fp16)"
                                              if a.wall_planes else ""),
                                           a.reps, a.calls)),
                            "device": torch.cuda.get_device_name(0), "result": res}, **extra))
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    cd.cudecompFinalize(h)
    if extra.get("ghost_cells_not_zero_after_accumulate_clear") or extra.get("interior_sum_after_accumulate_clear", extra.get("cells")) != extra.get("cells"):
        sys.exit("halo_bench.py: after accumulate-and-clear along 2, 1, 0 %d ghost cells are not zero, the interior sums to %r of %d"
                 % (extra["ghost_cells_not_zero_after_accumulate_clear"], extra["interior_sum_after_accumulate_clear"], extra["cells"]))
    if extra.get("field_cells_that_differ_from_single_calls"):
        sys.exit("halo_bench.py: after the fields call along 0, 1, 2 %d cells differ from single calls on clones" % extra["field_cells_that_differ_from_single_calls"])
    for name in ("accumulate", "accumulate_clear"):
        if extra.get(name + "_field_cells_that_differ_from_single_calls"):
            sys.exit("halo_bench.py: after the %s fields call along 2, 1, 0 %d cells differ from single calls on clones"
                     % (name, extra[name + "_field_cells_that_differ_from_single_calls"]))
    if extra.get("wall_field_cells_that_differ_from_single_calls"):
        sys.exit("halo_bench.py: after the wall field calls %d cells differ from single calls on clones"
                 % extra["wall_field_cells_that_differ_from_single_calls"])
    for label in ("fp64", "fp16"):
        if extra.get("wall_value_field_cells_that_differ_from_single_calls_" + label):
            sys.exit("halo_bench.py: after the wall-value field calls along 0, 1, 2 %d cells differ from single calls on clones (%s)"
                     % (extra["wall_value_field_cells_that_differ_from_single_calls_" + label], label))
    for name in ("fold", "fold_clear"):
        if extra.get("interior_cells_with_another_count_after_" + name) or extra.get("ghost_cells_not_zero_after_" + name):
            sys.exit("halo_bench.py: after folding a pencil of ones along 2, 1, 0 (%s pass) %d interior cells do not hold their count and %d "
                     "ghost cells are not zero" % (name, extra["interior_cells_with_another_count_after_" + name],
                                                   extra["ghost_cells_not_zero_after_" + name]))
    for label in ("fp64", "fp16"):
        for dim in range(3):
            if extra.get("wall_planes_wrong_cells_%s_dim%d" % (label, dim)):
                sys.exit("halo_bench.py: %d ghost cells of the low wall of dim %d do not hold -1 + plane entry after the wall planes (%s)"
                         % (extra["wall_planes_wrong_cells_%s_dim%d" % (label, dim)], dim, label))
        if extra.get("wall_values_wrong_cells_" + label):
            sys.exit("halo_bench.py: %d ghost cells of the low wall do not hold -1 + a_k after the wall values (%s)"
                     % (extra["wall_values_wrong_cells_" + label], label))
    if extra.get("cells_not_one_after_reflect"):
        sys.exit("halo_bench.py: after the even mirror along 0, 1, 2 %d cells do not hold the interior's value" % extra["cells_not_one_after_reflect"])
    if extra.get("ghost_cells_not_zero") or extra.get("interior_cells_changed"):
        sys.exit("halo_bench.py: after the fills %d ghost cells are not zero and %d interior cells changed"
                 % (extra["ghost_cells_not_zero"], extra["interior_cells_changed"]))


if __name__ == "__main__":
    main()
