#!/usr/bin/env python3
"""Level batches sampled at arbitrary points: mifc_hinterp_levels (nearest, bilinear, bicubic; fields flagged SOME_DEFINED,
so every value is tested, and bilinear once more with every level ALL_DEFINED) on device-resident fields, next to the
yardstick, torch.nn.functional.grid_sample (align_corners=True, bilinear and nearest, the levels as channels) in the same
process on the same data.  Two cases:
  regrid   one 1440x720x137 field to a 2000x1000 grid of rotated positions;
  section  2000 points x 137 levels x 8 fields.
Per call: the kernel time of each of ROUNDS calls after a warm-up call (HIP events around the launches of the call,
measurement build; torch.cuda events around grid_sample; the calls alternate), its median, minimum and spread (max - min),
and the algorithmic bytes -- the positions read, every output value written, and of the fields what the call cannot avoid
reading: the values the points need (1, 4 or 16 per point, level and field) or the whole fields, whichever is less -- with
the rate they give.  Then per mifc call the ratio of the yardstick's time to its time (> 1: mifc is faster).  The yardstick
is float32 arithmetic with zero padding and no undefined values: a comparison of speed, never of results.

    python tools/bench_hinterp.py [--small]   -> one JSON line per call, then one comparison line per mifc call
"""
import json
import math
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch
import torch.nn.functional as F

import mi_fieldcalc_amd as fc

ROUNDS = 9
VALUES_PER_POINT = {"nearest": 1, "bilinear": 4, "bicubic": 16}


def algorithmic_bytes(nx, ny, nlev, nf, npos, method):
    needed = VALUES_PER_POINT[method] * npos
    return 4 * (2 * npos + nf * nlev * npos + nf * nlev * min(nx * ny, needed))


def rotated_grid(nx, ny, gx, gy, dev):
    """A gx x gy grid turned by 20 degrees about the centre of the source grid, a little larger than fits: the corners leave it."""
    u = torch.linspace(-0.5 * (nx - 1), 0.5 * (nx - 1), gx, device=dev)
    v = torch.linspace(-0.5 * (ny - 1), 0.5 * (ny - 1), gy, device=dev)
    vv, uu = torch.meshgrid(v, u, indexing="ij")
    c, s = math.cos(math.radians(20)), math.sin(math.radians(20))
    x = 0.5 * (nx - 1) + 0.9 * (c * uu - s * vv)
    y = 0.5 * (ny - 1) + 0.9 * (s * uu + c * vv)
    return x.contiguous(), y.contiguous()


def run_case(ctx, case, fields, x, y, lines):
    nf, nlev, ny, nx = fields.shape
    npos = x.numel()
    out = torch.empty((nf, nlev) + tuple(x.shape), device=fields.device, dtype=torch.float32)
    every = np.zeros((nf, nlev), np.int32)  # ALL_DEFINED
    # the yardstick's view of the same data: the levels of every field as channels, the positions normalised to [-1, 1]
    image = fields.view(1, nf * nlev, ny, nx)
    grid = torch.stack([2 * x / max(nx - 1, 1) - 1, 2 * y / max(ny - 1, 1) - 1], dim=-1).view(1, -1, x.shape[-1], 2).contiguous()
    calls = {}
    for method in ("nearest", "bilinear", "bicubic"):
        calls["mifc %s" % method] = lambda method=method: ctx.hinterp_levels(fields, x, y, method, out=out)
    calls["mifc bilinear, ALL_DEFINED"] = lambda: ctx.hinterp_levels(fields, x, y, "bilinear", fdefined_in=every, out=out)
    for mode in ("nearest", "bilinear"):
        calls["grid_sample %s" % mode] = (lambda mode=mode: F.grid_sample(image, grid, mode=mode, padding_mode="zeros", align_corners=True), bk.EVENTS)
    _, ms = bk.alternate(ctx, calls, ROUNDS)
    results = {}
    for name, ts in ms.items():
        method = name.split()[1].rstrip(",")
        r = {"case": case, "call": name, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, "npos": npos, **bk.stats(ts),
             "algorithmic_bytes": algorithmic_bytes(nx, ny, nlev, nf, npos, method)}
        r["GBps"] = bk.rate(r["algorithmic_bytes"], r["kernel_ms"])[0]
        results[name] = r
        print(json.dumps(r), flush=True)
    for name, r in results.items():
        if name.startswith("mifc"):
            yard = results["grid_sample %s" % ("nearest" if "nearest" in name else "bilinear")]
            lines.append({"case": case, "call": name, "kernel_ms": r["kernel_ms"], "yardstick": yard["call"], "yardstick_ms": yard["kernel_ms"],
                          "yardstick_over_mifc": round(yard["kernel_ms"] / r["kernel_ms"], 3)})


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    gx, gy, npts, nf = bk.shape(sys.argv, (2000, 1000, 2000, 8), (500, 250, 500, 4))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    lines = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        fields = torch.randn((nf, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 10 + 280
        x, y = rotated_grid(nx, ny, gx, gy, dev)
        run_case(ctx, "regrid", fields[:1], x, y, lines)
        print(json.dumps({"case": "regrid", "launch": ctx.last_hinterp_form(), "points_outside": int(((x < 0) | (x > nx - 1) | (y < 0) | (y > ny - 1)).sum())}),
              flush=True)
        # a section line across the grid with stations scattered around it
        s = torch.linspace(0, 1, npts, device=dev)
        xs = (0.02 + 0.96 * s) * (nx - 1) + torch.randn(npts, generator=gen, device=dev)
        ys = (0.5 + 0.4 * torch.sin(6.28 * s)) * (ny - 1) + torch.randn(npts, generator=gen, device=dev)
        run_case(ctx, "section", fields, xs.clamp(0, nx - 1).contiguous(), ys.clamp(0, ny - 1).contiguous(), lines)
        print(json.dumps({"case": "section", "launch": ctx.last_hinterp_form()}), flush=True)
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
