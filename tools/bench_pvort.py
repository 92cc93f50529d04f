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
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import pvort

ROUNDS = 9
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


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    alevel, blevel, levels, ps, make_coord = bk.hybrid_atmosphere(nx, ny, nlev, dev, gen)
    uvt = torch.randn((3, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    u, v, th = uvt[0], uvt[1], uvt[2]
    coord = make_coord()
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
                # a timing section holds 16 launches: the chain runs its calls through section(), one timing section each
                calls = {"pvort": lambda: fused(kind, method), "chain": (lambda section: chain(kind, method, section), bk.SECTIONS),  # noqa: B023
                         "vderiv x3": lambda: vderiv(kind, method)}  # noqa: B023
                _, ms = bk.alternate(ctx, calls, ROUNDS)
                form = pvort.last_pvort_form(ctx)
                # the chain rounds every intermediate to float: the same field, not the same bits
                inner = (slice(None), slice(1, -1), slice(1, -1))
                close = (out[inner] - chain_out[inner]).abs() <= 1e-3 * out[inner].abs() + 1e-3 * out[inner].abs().mean()
                st = {name: bk.stats(ts) for name, ts in ms.items()}
                alg = {"pvort": pvort_bytes(nx, ny, nlev, kind), "chain": chain_bytes(nx, ny, nlev, kind), "vderiv x3": vderiv_bytes(nx, ny, nlev, kind)}
                for name in calls:
                    r = {"call": name, "coordinate": kind, "method": method, "nx": nx, "ny": ny, "nlev": nlev, **st[name], "algorithmic_bytes": alg[name]}
                    r["GBps"], r["share_of_8TBps"] = bk.rate(alg[name], r["kernel_ms"])
                    print(json.dumps(r), flush=True)
                p, c, b = st["pvort"], st["chain"], st["vderiv x3"]
                model_ms = pvort_bytes(nx, ny, nlev, kind, halo=False) / bk.PEAK_GBPS / 1e6
                lines.append({"coordinate": kind, "method": method, "form": form, "pvort_ms": p["kernel_ms"], "chain_ms": c["kernel_ms"],
                              "speedup_over_chain": round(c["kernel_ms"] / p["kernel_ms"], 2),
                              "not_slower_than_chain_beyond_the_two_spreads": bk.not_slower(p, c),
                              "byte_model_ms_at_8TBps": round(model_ms, 4), "share_of_byte_model_time": round(model_ms / p["kernel_ms"], 3),
                              "GBps": round(alg["pvort"] / p["kernel_ms"] / 1e6, 1), "vderiv_x3_GBps": round(alg["vderiv x3"] / b["kernel_ms"] / 1e6, 1),
                              "share_of_vderiv_rate": round((alg["pvort"] / p["kernel_ms"]) / (alg["vderiv x3"] / b["kernel_ms"]), 3),
                              "chain_agrees": round(float(close.float().mean().item()), 4)})
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
