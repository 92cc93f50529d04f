#!/usr/bin/env python3
"""Ertel potential vorticity of level batches: mifc_pvort_hlevels / mifc_pvort_fields / mifc_pvort_levels with both
methods on a device-resident 1440x720x137 batch (the shape of tools/bench_vderiv.py), alternating in the same process with
  (a) the chain of existing entries that computes the same field: absvort over the levels, the two gradients of theta,
      one mifc_vderiv_* call for the three fields, and the field algebra level by level (three products, a difference, a
      sum, the factor), and
  (b) mifc_vderiv_* of the three fields alone, which reads what the fused call reads and writes three batches.
Per case: the kernel time of each of ROUNDS calls after a warm-up call (HIP events around the launches of the call,
measurement build; the calls alternate), its median, minimum and spread (max - min); for the fused call the bytes of its
model (u, v, th and the coordinate read once, the halo rows of u and th once more per tile of 8 rows, PV written once),
the rate they give, its share of the 8 TB/s peak and of (b)'s rate, and whether it is not slower than the chain beyond
the two spreads.

    python tools/bench_pvort.py [--small]   -> one JSON line per case, then one comparison line per form and method
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
from mi_fieldcalc_amd import pvort  # noqa: E402

NX, NY, NLEV = 1440, 720, 137
ROUNDS = 9
PEAK_GBPS = 8000.0
KINDS = ("hybrid", "field", "levels")
METHODS = ("centred", "weighted")
TILE_ROWS = 8
SCALE = pvort.PVU_SCALE


def coord_planes(kind, nlev):
    return {"hybrid": 1, "field": nlev, "levels": 0}[kind]


def pvort_bytes(nx, ny, nlev, kind, halo=True):
    """The model: every input level once, xmapr, ymapr and f once, the output once; with halo: the rows above and below a
    tile of u and th again (they come through L2 when the neighbouring tile runs close in time)."""
    planes = 3 * nlev + coord_planes(kind, nlev) + 3 + nlev
    if halo:
        planes += 2 * nlev * 2.0 / TILE_ROWS
    return int(planes * 4 * nx * ny)


def vderiv_bytes(nx, ny, nlev, kind):
    return (3 * nlev + coord_planes(kind, nlev) + 3 * nlev) * 4 * nx * ny


def chain_bytes(nx, ny, nlev, kind):
    """absvort 2 in 1 out, two gradients 1 in 1 out, vderiv, and per level six 2-D calls of (2 in, 1 out) or (1 in, 1 out)."""
    return (3 + 2 * 2 + 17) * nlev * 4 * nx * ny + vderiv_bytes(nx, ny, nlev, kind)


def timed(ctx, call):
    """The kernel time of one call (or of a few: a timing section holds 16 launches)."""
    ctx.timing_begin()
    call()
    torch.cuda.synchronize()
    ms = ctx.timing_end_ms()
    if ms < 0:
        raise RuntimeError("a timing section with too many launches")
    return ms


def kernel_ms_alternating(ctx, calls):
    """calls: name -> callable(section), which runs its calls through section(callable) -- one timing section each -- and
    returns nothing.  One warm-up each, then ROUNDS rounds in which every call is timed once, in turn."""
    for call in calls.values():
        call(lambda part: part())  # warm-up: code object, scratch
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            parts = []
            call(lambda part: parts.append(timed(ctx, part)))  # noqa: B023
            ms[name].append(sum(parts))
    return ms


def stats(ts):
    return {"kernel_ms": round(float(np.median(ts)), 4), "kernel_ms_min": round(min(ts), 4), "kernel_ms_spread": round(max(ts) - min(ts), 4)}


def main():
    nx, ny, nlev = (360, 180, 24) if "--small" in sys.argv else (NX, NY, NLEV)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    eta = np.linspace(0.01, 1, nlev) ** 3
    alevel, blevel = (1000 * (eta - eta ** 2)).astype(np.float32), (eta ** 2).astype(np.float32)
    levels = (alevel + blevel * np.float32(1000)).astype(np.float32)
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, ny, device=dev), torch.linspace(0, 12.56, nx, device=dev), indexing="ij")
    ps = (780 + 260 * torch.sin(xx) * torch.cos(yy) + torch.randn((ny, nx), generator=gen, device=dev)).clamp(520, 1040).contiguous()
    uvt = torch.randn((3, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    u, v, th = uvt[0], uvt[1], uvt[2]
    coord = (torch.from_numpy(alevel).to(dev)[:, None, None] + torch.from_numpy(blevel).to(dev)[:, None, None] * ps[None]).contiguous()
    xm = torch.full((ny, nx), 2e-5, device=dev) + 1e-6 * torch.rand((ny, nx), generator=gen, device=dev)
    ym = torch.full((ny, nx), 2e-5, device=dev) + 1e-6 * torch.rand((ny, nx), generator=gen, device=dev)
    f = torch.full((ny, nx), 1e-4, device=dev) + 1e-5 * torch.rand((ny, nx), generator=gen, device=dev)
    out = torch.empty((nlev, ny, nx), device=dev, dtype=torch.float32)
    d3 = torch.empty((3, nlev, ny, nx), device=dev, dtype=torch.float32)
    av, gx, gy, chain_out = (torch.empty((nlev, ny, nx), device=dev, dtype=torch.float32) for _ in range(4))
    t1, t2 = (torch.empty((ny, nx), device=dev, dtype=torch.float32) for _ in range(2))
    lines = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()

        def vderiv(kind, method):
            if kind == "hybrid":
                return ctx.vderiv_hlevels(uvt, ps, alevel, blevel, method, out=d3)
            if kind == "field":
                return ctx.vderiv_fields(uvt, coord, method, out=d3)
            return ctx.vderiv_levels(uvt, levels, method, out=d3)

        def fused(kind, method):
            if kind == "hybrid":
                return pvort.pvort_hlevels(ctx, u, v, th, ps, alevel, blevel, xm, ym, f, method, SCALE, out=out)
            if kind == "field":
                return pvort.pvort_fields(ctx, u, v, th, coord, xm, ym, f, method, SCALE, out=out)
            return pvort.pvort_levels(ctx, u, v, th, levels, xm, ym, f, method, SCALE, out=out)

        def algebra(k):
            ctx.fieldOPERfield(3, av[k], d3[2, k], out=t1)
            ctx.fieldOPERfield(3, d3[1, k], gx[k], out=t2)
            ctx.fieldOPERfield(2, t1, t2, out=t1)
            ctx.fieldOPERfield(3, d3[0, k], gy[k], out=t2)
            ctx.fieldOPERfield(1, t1, t2, out=t1)
            ctx.constantOPERfield(3, SCALE, t1, out=chain_out[k])

        def chain(kind, method, section):
            section(lambda: ctx.stencil_levels("absvort", u, v, xm, ym, f, out0=av))
            section(lambda: ctx.stencil_levels("gradient1", th, None, xm, ym, out0=gx))
            section(lambda: ctx.stencil_levels("gradient2", th, None, xm, ym, out0=gy))
            section(lambda: vderiv(kind, method))
            for k in range(nlev):
                section(lambda k=k: algebra(k))

        for kind in KINDS:
            for method in METHODS:
                calls = {"pvort": lambda section: section(lambda: fused(kind, method)), "chain": lambda section: chain(kind, method, section),  # noqa: B023
                         "vderiv x3": lambda section: section(lambda: vderiv(kind, method))}  # noqa: B023
                ms = kernel_ms_alternating(ctx, calls)
                form = pvort.last_pvort_form(ctx)
                # the chain rounds every intermediate to float: the same field, not the same bits
                inner = (slice(None), slice(1, -1), slice(1, -1))
                close = (out[inner] - chain_out[inner]).abs() <= 1e-3 * out[inner].abs() + 1e-3 * out[inner].abs().mean()
                st = {name: stats(ts) for name, ts in ms.items()}
                alg = {"pvort": pvort_bytes(nx, ny, nlev, kind), "chain": chain_bytes(nx, ny, nlev, kind), "vderiv x3": vderiv_bytes(nx, ny, nlev, kind)}
                for name in calls:
                    r = {"call": name, "coordinate": kind, "method": method, "nx": nx, "ny": ny, "nlev": nlev, **st[name], "algorithmic_bytes": alg[name]}
                    r["GBps"] = round(alg[name] / r["kernel_ms"] / 1e6, 1)
                    r["share_of_8TBps"] = round(r["GBps"] / PEAK_GBPS, 3)
                    print(json.dumps(r), flush=True)
                p, c, b = st["pvort"], st["chain"], st["vderiv x3"]
                model_ms = pvort_bytes(nx, ny, nlev, kind, halo=False) / PEAK_GBPS / 1e6
                lines.append({"coordinate": kind, "method": method, "form": form, "pvort_ms": p["kernel_ms"], "chain_ms": c["kernel_ms"],
                              "speedup_over_chain": round(c["kernel_ms"] / p["kernel_ms"], 2),
                              "not_slower_than_chain_beyond_the_two_spreads": bool(p["kernel_ms_min"] <= c["kernel_ms_min"] + c["kernel_ms_spread"] + p["kernel_ms_spread"]),
                              "byte_model_ms_at_8TBps": round(model_ms, 4), "share_of_byte_model_time": round(model_ms / p["kernel_ms"], 3),
                              "GBps": round(alg["pvort"] / p["kernel_ms"] / 1e6, 1), "vderiv_x3_GBps": round(alg["vderiv x3"] / b["kernel_ms"] / 1e6, 1),
                              "share_of_vderiv_rate": round((alg["pvort"] / p["kernel_ms"]) / (alg["vderiv x3"] / b["kernel_ms"]), 3),
                              "chain_agrees": round(float(close.float().mean().item()), 4)})
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
