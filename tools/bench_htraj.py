#!/usr/bin/env python3
"""Trajectories through wind level batches: mifc_htraj_levels on device-resident fields, one interval between two hourly
slices, nsub = 4 substeps with niter = 2 corrections (12 evaluations of the index velocity per particle).  Cases:
  origin   one 1440x720 level (--small: 360x180), one particle per cell: an origin map;
  batch    137 levels x 10 000 particles (--small: 24 x 1 000) on the same grid;
  chain    the origin case against the chain of existing entries, per evaluation: mifc_hinterp_levels on u and v of both
           slices and on the two map planes (six fields of one level, bilinear) at the current positions, then
           mifc_fexpr_levels for the new x and the new y -- 12 times, the positions handed on from call to call on the
           device.  The chain is a yardstick for speed only: it rounds to float at every call and knows no lost particle,
           so it does not compute the definition.
Per call: the kernel time of each of ROUNDS calls after a warm-up call (HIP events around every launch, measurement
build) and the host clock around the call and a synchronise, their median, minimum and spread; the particle evaluations
per second; the bytes the evaluations gather (24 corners of 4 B each -- from caches mostly, so the rate is a gather rate
and no share of the memory bandwidth).  Then the ratio of the chain's times to the call's (> 1: mifc_htraj_levels is faster).

    python tools/bench_htraj.py [--small]   -> one JSON line per call, then the comparison line
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import fexpr, htraj

ROUNDS = 5
NSUB, NITER = 4, 2
EVALS = NSUB * (1 + NITER)
TAU = 3600.0
MAP = 3.6e-5  # grid cells per metre on a quarter-degree grid


def winds(nlev, ny, nx, dev, gen, phase):
    """A smooth wind of +-20 m/s that differs from level to level and from slice to slice, a little noise."""
    j = torch.arange(ny, device=dev, dtype=torch.float32).view(1, ny, 1)
    i = torch.arange(nx, device=dev, dtype=torch.float32).view(1, 1, nx)
    k = torch.arange(nlev, device=dev, dtype=torch.float32).view(nlev, 1, 1)
    u = 20.0 * torch.sin(2 * np.pi * (i / nx + 0.01 * k) + phase) * torch.cos(np.pi * j / ny)
    v = 12.0 * torch.cos(4 * np.pi * i / nx + phase) * torch.sin(2 * np.pi * (j / ny + 0.02 * k))
    noise = lambda: 0.5 * torch.randn((nlev, ny, nx), generator=gen, device=dev)  # noqa: E731
    return (u + noise()).contiguous(), (v + noise()).contiguous()


def report(case, name, shape, npos, wall, kernel, extra=None):
    nlev, ny, nx = shape
    r = {"case": case, "call": name, "nx": nx, "ny": ny, "nlev": nlev, "npos": npos, "nsub": NSUB, "niter": NITER, "intervals": 1, **bk.stats(kernel),
         **bk.stats(wall, "wall_ms"), "evaluations": nlev * npos * EVALS, "algorithmic_bytes": nlev * npos * EVALS * 96, **(extra or {})}
    r["Gevals_per_s"] = round(r["evaluations"] / r["kernel_ms"] / 1e6, 3)
    r["gathered_GBps"] = bk.rate(r["algorithmic_bytes"], r["kernel_ms"])[0]
    print(json.dumps(r), flush=True)
    return r


def htraj_case(ctx, case, nlev, ny, nx, xpos, ypos, dev, gen, chain=False):
    uA, vA = winds(nlev, ny, nx, dev, gen, 0.0)
    uB, vB = winds(nlev, ny, nx, dev, gen, 0.3)
    xm = torch.full((ny, nx), MAP, device=dev) * (1.0 + 0.05 * torch.rand((ny, nx), generator=gen, device=dev))
    ym = torch.full((ny, nx), MAP, device=dev) * (1.0 + 0.05 * torch.rand((ny, nx), generator=gen, device=dev))
    every = 0  # ALL_DEFINED
    calls = {
        "mifc htraj, tested": (lambda: htraj.trajectories(ctx, [uA, uB], [vA, vB], [0.0, TAU], xm, ym, xpos, ypos, nsub=NSUB, niter=NITER), bk.WALL_KERNEL),
        "mifc htraj, ALL_DEFINED": (lambda: htraj.trajectories(ctx, [uA, uB], [vA, vB], [0.0, TAU], xm, ym, xpos, ypos, nsub=NSUB, niter=NITER,
                                                                fdefined_in=every, fdef_map=every), bk.WALL_KERNEL),
    }
    if chain:
        h, hh = TAU / NSUB, 0.5 * TAU / NSUB
        planes = [uA, uB, vA, vB, xm.view(1, ny, nx), ym.view(1, ny, nx)]
        step = fexpr.compile("x + h * ((a + w * (b - a)) * m)", fields=("x", "a", "b", "m"), level_scalars=("h", "w"))
        npos = xpos.numel()

        def chain_call(section):
            x, y = xpos.view(1, 1, npos), ypos.view(1, 1, npos)
            state = {"x": x, "y": y}
            for s in range(NSUB):
                for it in range(1 + NITER):
                    w = (s + (0 if it == 0 else 1)) / NSUB

                    def evaluation(w=w, it=it):
                        smp, _ = ctx.hinterp_levels(planes, state["x"].view(-1), state["y"].view(-1), "bilinear")
                        smp = smp.view(6, 1, 1, npos)
                        scal = [[h if it == 0 else hh], [w]]
                        state["x"], _ = fexpr.evaluate(ctx, step, [x, smp[0], smp[1], smp[4]], level_scalars=scal)
                        state["y"], _ = fexpr.evaluate(ctx, step, [y, smp[2], smp[3], smp[5]], level_scalars=scal)

                    section(evaluation)

        calls["chain of hinterp and fexpr calls"] = (chain_call, bk.WALL_SECTIONS)
    wall, kernel = bk.alternate(ctx, calls, ROUNDS)
    form = None
    results = {}
    for name in calls:
        if name.startswith("mifc"):
            calls[name][0]()
            form = htraj.last_htraj_form(ctx)
        results[name] = report(case, name, (nlev, ny, nx), xpos.numel(), wall[name], kernel[name], {"launch": form} if name.startswith("mifc") else {"launches_per_evaluation": 4})
    return results


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    (npos,) = bk.shape(sys.argv, (10000,), (1000,))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        jj, ii = torch.meshgrid(torch.arange(ny, device=dev, dtype=torch.float32), torch.arange(nx, device=dev, dtype=torch.float32), indexing="ij")
        origin = htraj_case(ctx, "origin map, one level", 1, ny, nx, ii.reshape(-1).contiguous(), jj.reshape(-1).contiguous(), dev, gen, chain=True)
        xs = (torch.rand(npos, generator=gen, device=dev) * (nx - 1)).contiguous()
        ys = (torch.rand(npos, generator=gen, device=dev) * (ny - 1)).contiguous()
        htraj_case(ctx, "batch of levels", nlev, ny, nx, xs, ys, dev, gen)
    r, y = origin["mifc htraj, tested"], origin["chain of hinterp and fexpr calls"]
    print(json.dumps({"case": "origin map, one level", "call": "mifc htraj, tested", "kernel_ms": r["kernel_ms"], "wall_ms": r["wall_ms"],
                      "yardstick": "chain of hinterp and fexpr calls", "yardstick_kernel_ms": y["kernel_ms"], "yardstick_wall_ms": y["wall_ms"],
                      "yardstick_over_mifc_kernel": round(y["kernel_ms"] / r["kernel_ms"], 3), "yardstick_over_mifc_wall": round(y["wall_ms"] / r["wall_ms"], 3)}),
          flush=True)


if __name__ == "__main__":
    main()
