#!/usr/bin/env python3
"""Area histograms and exact percentiles of level batches: mifc_hdist_histogram_levels and mifc_hdist_quantile_levels on
device-resident fields, next to yardsticks in the same process on the same tensors.  Cases:
  batch    1440x720x137 (--small: 360x180x24): histograms of 16, 256 and 1025 bins on 1 and 4 fields, area and rows;
           1 and 5 percentiles of one field that is smooth (a synthetic temperature), constant, or white noise;
  level    one 4000x4000 level (--small: 1000x1000): 256 bins; 5 percentiles of the smooth field.
Yardsticks, for speed only (they bin by other rules, test nothing and interpolate in float): torch.bucketize + torch.bincount
with the level folded into the index, torch.histc per level on the single level, torch.sort along a level, torch.quantile.
Per call: the kernel time of each of ROUNDS calls after a warm-up call (HIP events around every launch and memset of the
call, measurement build; torch.cuda events around a yardstick; the calls alternate), its median, minimum and spread, the
algorithmic bytes -- 4 B per cell and field for a histogram, 4 B per cell and pass for the selection, the passes as
mifc_last_hdist_form reports them plus the extent pass -- with the rate they give and its share of the 6.29 TB/s copy rate
of DESIGN.md 4.22.  Then per mifc call the ratio of the yardstick's time to its time (> 1: mifc is faster).

    python tools/bench_hdist.py [--small]   -> one JSON line per call, then one comparison line per mifc call
    MIFC_HDIST_AGGREGATE=0 python tools/bench_hdist.py   -> the same without the wave's ballot; tools/benchkit.py compare pairs the two
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import hdist

ROUNDS = 5
COPY_GBPS = 6290.0


def smooth(nlev, ny, nx, dev, gen):
    """A synthetic temperature: a wave over the level, colder with height, a little noise."""
    j = torch.arange(ny, device=dev, dtype=torch.float32).view(1, ny, 1)
    i = torch.arange(nx, device=dev, dtype=torch.float32).view(1, 1, nx)
    k = torch.arange(nlev, device=dev, dtype=torch.float32).view(nlev, 1, 1)
    t = 288.0 - 0.4 * k + 12.0 * torch.sin(2 * np.pi * i / nx) * torch.cos(np.pi * j / ny)
    return (t + 0.05 * torch.randn((nlev, ny, nx), generator=gen, device=dev)).contiguous()


def report(case, name, shape, ts, nbytes, results, extra=None):
    nf, nlev, ny, nx = shape
    r = {"case": case, "call": name, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **bk.stats(ts), "algorithmic_bytes": nbytes, **(extra or {})}
    r["GBps"] = bk.rate(nbytes, r["kernel_ms"])[0]
    r["GBps_over_copy_rate"] = round(r["GBps"] / COPY_GBPS, 3)
    results[name] = r
    print(json.dumps(r), flush=True)


def hist_case(ctx, case, fields, bins, lines, modes=("area", "rows"), histc=False):
    nf, nlev, ny, nx = fields.shape
    every = np.zeros((nf, nlev), np.int32)  # ALL_DEFINED
    lo, hi = float(fields.min()), float(fields.max())
    calls, meta = {}, {}
    for nb in bins:
        edges = np.linspace(lo, hi, nb + 1)[1:-1].astype(np.float32) if nb > 2 else np.array([(lo + hi) / 2], np.float32)
        dedges = torch.from_numpy(edges).to(fields.device)
        offsets = (torch.arange(nf * nlev, device=fields.device, dtype=torch.int64) * (edges.size + 1)).view(nf, nlev, 1, 1)
        for mode in modes:
            name = "mifc hist %s, %d bins" % (mode, edges.size + 1)
            calls[name] = lambda mode=mode, edges=edges: hdist.histogram_levels(ctx, fields, edges, mode=mode)
            meta[name] = "torch bucketize+bincount, %d bins" % (edges.size + 1)
        name = "mifc hist area, %d bins, ALL_DEFINED" % (edges.size + 1)
        calls[name] = lambda edges=edges: hdist.histogram_levels(ctx, fields, edges, fdefined_in=every)
        meta[name] = "torch bucketize+bincount, %d bins" % (edges.size + 1)
        name = "torch bucketize+bincount, %d bins" % (edges.size + 1)
        calls[name] = (lambda dedges=dedges, offsets=offsets, n=nf * nlev * (edges.size + 1): torch.bincount(
            (torch.bucketize(fields, dedges, right=True) + offsets).view(-1), minlength=n), bk.EVENTS)
        if histc:
            name = "torch histc, %d bins" % (edges.size + 1)
            calls[name] = (lambda nb=edges.size + 1: torch.histc(fields, bins=nb, min=lo, max=hi), bk.EVENTS)
    _, ms = bk.alternate(ctx, calls, ROUNDS)
    results = {}
    for name, ts in ms.items():
        report(case, name, fields.shape, ts, 4 * nf * nlev * ny * nx, results)
    for name, yard in meta.items():
        r, y = results[name], results[yard]
        lines.append({"case": case, "call": name, "kernel_ms": r["kernel_ms"], "GBps": r["GBps"], "yardstick": yard, "yardstick_ms": y["kernel_ms"],
                      "yardstick_over_mifc": round(y["kernel_ms"] / r["kernel_ms"], 3)})
    print(json.dumps({"case": case, "launch": hdist.last_hdist_form(ctx)}), flush=True)


def quant_case(ctx, case, field, lines, percentiles=((50.0,), (2.0, 25.0, 50.0, 75.0, 98.0)), quantile=True):
    nlev, ny, nx = field.shape
    flat = field.view(nlev, ny * nx)
    every = np.zeros(nlev, np.int32)
    calls, meta, forms = {}, {}, {}
    for ps in percentiles:
        for method in ("lower", "linear"):
            name = "mifc quant %s, %d percentile%s" % (method, len(ps), "s" if len(ps) > 1 else "")
            calls[name] = lambda ps=ps, method=method: hdist.quantile_levels(ctx, field, ps, method, fdefined_in=every)
            meta[name] = "torch sort"
    calls["torch sort"] = (lambda: torch.sort(flat, dim=1), bk.EVENTS)
    if quantile and ny * nx < 16000000:  # (torch.quantile refuses longer rows)
        q = torch.tensor(percentiles[-1], device=field.device) / 100.0
        calls["torch quantile, %d percentiles" % len(percentiles[-1])] = (lambda: torch.quantile(flat, q, dim=1), bk.EVENTS)
    for name in list(meta):  # the passes of each mifc call: what the selection read
        calls[name]()
        forms[name] = hdist.last_hdist_form(ctx)
    _, ms = bk.alternate(ctx, calls, ROUNDS)
    results = {}
    for name, ts in ms.items():
        passes = 1 + forms[name]["passes"] if name in forms else 1
        extra = {"passes": passes, "prefix": forms[name]["prefix"]} if name in forms else None
        report(case, name, (1,) + tuple(field.shape), ts, 4 * nlev * ny * nx * passes, results, extra)
    for name, yard in meta.items():
        r, y = results[name], results[yard]
        lines.append({"case": case, "call": name, "kernel_ms": r["kernel_ms"], "GBps": r["GBps"], "yardstick": yard, "yardstick_ms": y["kernel_ms"],
                      "yardstick_over_mifc": round(y["kernel_ms"] / r["kernel_ms"], 3)})


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    (side,) = bk.shape(sys.argv, (4000,), (1000,))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    lines = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        fields = torch.stack([smooth(nlev, ny, nx, dev, gen) + 3.0 * g for g in range(4)])
        for nf in (1, 4):
            hist_case(ctx, "batch, %d field%s" % (nf, "s" if nf > 1 else ""), fields[:nf], (16, 256, 1025), lines)
        quant_case(ctx, "batch, smooth", fields[0], lines)
        quant_case(ctx, "batch, constant", torch.full_like(fields[0], 281.25), lines, quantile=False)
        noise = torch.randn((nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32)
        quant_case(ctx, "batch, white noise", noise, lines, quantile=False)
        del fields, noise
        level = smooth(1, side, side, dev, gen)
        hist_case(ctx, "level", level.view(1, 1, side, side), (256,), lines, histc=True)
        quant_case(ctx, "level, smooth", level, lines, percentiles=((2.0, 25.0, 50.0, 75.0, 98.0),))
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
