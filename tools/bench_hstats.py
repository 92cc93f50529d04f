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
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc

ROUNDS = 7


def algorithmic_bytes(nx, ny, nlev, nf, weighted, minus=False):
    return 4 * nx * ny * (nlev * nf * (2 if minus else 1) + (1 if weighted else 0))


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
                calls[name] = lambda mode=mode, products=products, w=w, out=out: ctx.hstats_levels(fields, weight=w, mode=mode, products=products, out=out)
                meta[name] = (mode, len(products) == 2, w is not None)
            name = "torch %s %s" % (mode, what)
            calls[name] = (lambda mode=mode, ext=len(products) == 2: yardstick(fields, mode, ext), bk.EVENTS)
            meta[name] = (mode, len(products) == 2, False)
        name = "mifc %s moments+extremes, ALL_DEFINED" % mode
        calls[name] = lambda mode=mode, out=out: ctx.hstats_levels(fields, mode=mode, fdefined_in=every, out=out)
        meta[name] = (mode, True, False)
    _, ms = bk.alternate(ctx, calls, ROUNDS)
    results = {}
    for name, ts in ms.items():
        mode, ext, weighted = meta[name]
        r = {"case": case, "call": name, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **bk.stats(ts), "algorithmic_bytes": algorithmic_bytes(nx, ny, nlev, nf, weighted)}
        r["GBps"] = bk.rate(r["algorithmic_bytes"], r["kernel_ms"])[0]
        results[name] = r
        print(json.dumps(r), flush=True)
    for name, r in results.items():
        if name.startswith("mifc"):
            mode, ext, _ = meta[name]
            yard = results["torch %s %s" % (mode, "moments+extremes" if ext else "moments")]
            lines.append({"case": case, "call": name, "kernel_ms": r["kernel_ms"], "GBps": r["GBps"], "yardstick": yard["call"], "yardstick_ms": yard["kernel_ms"],
                          "yardstick_over_mifc": round(yard["kernel_ms"] / r["kernel_ms"], 3)})


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    side, npts = bk.shape(sys.argv, (4000, 2000000), (1000, 200000))
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
