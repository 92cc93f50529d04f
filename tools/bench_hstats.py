#!/usr/bin/env python3
"""Horizontal statistics of level batches: mifc_hstats_levels (area and rows; the moments alone and with the extremes;
with and without a weight plane) on device-resident fields, next to the yardstick in the same process on the same tensors:
torch.sum(x, dim=..., dtype=torch.float64), plus torch.amin and torch.amax where the call computes the extremes.  Cases:
  batch    1440x720x137, 1 and 4 fields;
  level    one 4000x4000 level (the combination walks 4000 partials one after the other);
  points   a (137, 1, 2 000 000) point batch, as mifc_hinterp_levels writes it.
Per call: the kernel time of each of ROUNDS calls after a warm-up call (HIP events around the launches of the call,
measurement build: the segment launches and the combine launch; torch.cuda events around the yardstick; the calls
alternate), its median, minimum and spread (max - min), and the algorithmic bytes -- 4 B per cell and field, 8 with a minus
batch, the weight plane once -- with the rate they give.  Then per mifc call the ratio of the yardstick's time to its
time (> 1: mifc is faster).  The yardstick adds in another order, takes no weight and tests nothing: a comparison of
speed, never of results.

    python tools/bench_hstats.py [--small]   -> one JSON line per call, then one comparison line per mifc call
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIFC_LIB_PATH", os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc_measure.so"))  # mifc_timing_*

import torch  # noqa: E402

import mi_fieldcalc_amd as fc  # noqa: E402

ROUNDS = 7


def algorithmic_bytes(nx, ny, nlev, nf, weighted, minus=False):
    return 4 * nx * ny * (nlev * nf * (2 if minus else 1) + (1 if weighted else 0))


def time_alternating(ctx, calls):
    """calls: name -> (callable, is_mifc).  One warm-up each, then ROUNDS rounds in which every call is timed once, in turn."""
    for call, _ in calls.values():
        call()  # warm-up: code object, scratch, the allocator's blocks
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, (call, is_mifc) in calls.items():
            if is_mifc:
                ctx.timing_begin()
                call()
                torch.cuda.synchronize()
                ms[name].append(ctx.timing_end_ms())
            else:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call()
                t1.record()
                torch.cuda.synchronize()
                ms[name].append(t0.elapsed_time(t1))
    return ms


def stats(ts):
    return {"kernel_ms": round(float(np.median(ts)), 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_spread": round(max(ts) - min(ts), 4)}


def yardstick(x, mode, extremes):
    dims = (-2, -1) if mode == "area" else (-1,)
    out = [torch.sum(x, dim=dims, dtype=torch.float64)]
    if extremes:
        out += [torch.amin(x, dim=dims), torch.amax(x, dim=dims)]
    return out


def run_case(ctx, case, fields, weight, lines, modes=("area", "rows")):
    nf, nlev, ny, nx = fields.shape
    every = np.zeros((nf, nlev), np.int32)  # ALL_DEFINED
    calls, meta = {}, {}
    for mode in modes:
        out = torch.empty((nf, nlev, 1 if mode == "area" else ny, 8), dtype=torch.float64, device=fields.device)
        for products in (("moments",), ("moments", "extremes")):
            what = "+".join(products)
            for w in ((None, weight) if weight is not None else (None,)):
                name = "mifc %s %s%s" % (mode, what, ", weight" if w is not None else "")
                calls[name] = (lambda mode=mode, products=products, w=w, out=out: ctx.hstats_levels(fields, weight=w, mode=mode, products=products, out=out), True)
                meta[name] = (mode, len(products) == 2, w is not None)
            name = "torch %s %s" % (mode, what)
            calls[name] = (lambda mode=mode, ext=len(products) == 2: yardstick(fields, mode, ext), False)
            meta[name] = (mode, len(products) == 2, False)
        name = "mifc %s moments+extremes, ALL_DEFINED" % mode
        calls[name] = (lambda mode=mode, out=out: ctx.hstats_levels(fields, mode=mode, fdefined_in=every, out=out), True)
        meta[name] = (mode, True, False)
    ms = time_alternating(ctx, calls)
    results = {}
    for name, ts in ms.items():
        mode, ext, weighted = meta[name]
        r = {"case": case, "call": name, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **stats(ts), "algorithmic_bytes": algorithmic_bytes(nx, ny, nlev, nf, weighted)}
        r["GBps"] = round(r["algorithmic_bytes"] / r["kernel_ms"] / 1e6, 1)
        results[name] = r
        print(json.dumps(r), flush=True)
    for name, r in results.items():
        if name.startswith("mifc"):
            mode, ext, _ = meta[name]
            yard = results["torch %s %s" % (mode, "moments+extremes" if ext else "moments")]
            lines.append({"case": case, "call": name, "kernel_ms": r["kernel_ms"], "GBps": r["GBps"], "yardstick": yard["call"], "yardstick_ms": yard["kernel_ms"],
                          "yardstick_over_mifc": round(yard["kernel_ms"] / r["kernel_ms"], 3)})


def main():
    small = "--small" in sys.argv
    nx, ny, nlev = (360, 180, 24) if small else (1440, 720, 137)
    side, npts = (1000, 200000) if small else (4000, 2000000)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    lines = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        fields = torch.randn((4, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 10 + 280
        weight = torch.rand((ny, nx), generator=gen, device=dev, dtype=torch.float32) + 0.5
        for nf in (1, 4):
            run_case(ctx, "batch, %d field%s" % (nf, "s" if nf > 1 else ""), fields[:nf], weight, lines)
            print(json.dumps({"case": "batch", "nfields": nf, "launch": ctx.last_hstats_form()}), flush=True)
        del fields, weight
        level = torch.randn((1, 1, side, side), generator=gen, device=dev, dtype=torch.float32) * 10 + 280
        run_case(ctx, "level", level, None, lines)
        print(json.dumps({"case": "level", "launch": ctx.last_hstats_form()}), flush=True)
        del level
        points = torch.randn((1, nlev, 1, npts), generator=gen, device=dev, dtype=torch.float32) * 10 + 280
        run_case(ctx, "points", points, None, lines, modes=("area",))
        print(json.dumps({"case": "points", "launch": ctx.last_hstats_form()}), flush=True)
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
