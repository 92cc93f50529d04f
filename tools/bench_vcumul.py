#!/usr/bin/env python3
"""Running vertical integrals of level batches: mifc_vcumul_hlevels / mifc_vcumul_fields / mifc_vcumul_levels with both
methods and both walk directions on 1, 4 and 8 fields of 1440x720x137 (the shape of tools/bench_vderiv.py) -- next to the
yardstick, mifc_vderiv_* (centred, derivatives only) on the same inputs in the same process: on the same shape and field
count it moves the same bytes, nf + 1 batches read (nf and ps, nf alone for the `levels` form) and nf written.

Device memory: per case the kernel time of each of ROUNDS calls after a warm-up call (HIP events around the launches of
the call, measurement build; the calls alternate), its median, minimum and spread (max - min), the algorithmic bytes per
call, the rate they give and its share of the 8 TB/s peak.  Host memory (--host, or both with --all): the wall time of the
whole call -- staging band by band, kernels, download -- over HOST_ROUNDS calls, and the same bytes over it.

    python tools/bench_vcumul.py [--small] [--host | --all]   -> one JSON line per case, then one comparison line per case
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import vcumul

NFS = (1, 4, 8)
ROUNDS, HOST_ROUNDS = 9, 3
KINDS = ("hybrid", "field", "levels")
# (name, method, from_, with start and base)
CASES = (("linear, first", "linear", "first", False), ("linear, last", "linear", "last", False), ("linear, last, start+base", "linear", "last", True),
         ("log, first", "log", "first", False), ("log, last, start+base", "log", "last", True))


def coord_planes(kind, nlev):
    return {"hybrid": 1, "field": nlev, "levels": 0}[kind]


def batch_bytes(nx, ny, nlev, nf, kind, extra_planes=0):
    """Every field level and the coordinate (or ps) read once, every output level written once; the start and base planes."""
    return (nf * nlev + coord_planes(kind, nlev) + nf * nlev + extra_planes) * 4 * nx * ny


def make_calls(ctx, kind, fields, ps, coord, alevel, blevel, levels, start, bases, out):
    """The yardstick and the cases of one coordinate form on one set of arrays (device tensors or host arrays)."""
    nf = len(fields)
    calls = {}
    if kind == "hybrid":
        calls["vderiv centred"] = lambda: ctx.vderiv_hlevels(fields, ps, alevel, blevel, "centred", out=out)
    elif kind == "field":
        calls["vderiv centred"] = lambda: ctx.vderiv_fields(fields, coord, "centred", out=out)
    else:
        calls["vderiv centred"] = lambda: ctx.vderiv_levels(fields, levels, "centred", out=out)
    for name, method, from_, full in CASES:
        kw = dict(start=start[from_], base=[bases[f] for f in range(nf)], scale=[-29.3] * nf) if full else {}
        if kind == "hybrid":
            call = lambda method=method, from_=from_, kw=kw: vcumul.vcumul_hlevels(ctx, fields, ps, alevel, blevel, method, from_, out=out, **kw)  # noqa: E731
        elif kind == "field":
            call = lambda method=method, from_=from_, kw=kw: vcumul.vcumul_fields(ctx, fields, coord, method, from_, out=out, **kw)  # noqa: E731
        else:
            call = lambda method=method, from_=from_, kw=kw: vcumul.vcumul_levels(ctx, fields, levels, method, from_, out=out, **kw)  # noqa: E731
        calls["vcumul " + name] = call
    return calls


def report(ms, key, nx, ny, nlev, nf, kind, memory, lines):
    base = bk.stats(ms["vderiv centred"], key)
    base_bytes = batch_bytes(nx, ny, nlev, nf, kind)
    base_gbps = base_bytes / base[key] / 1e6
    for name, ts in ms.items():
        extra = 1 + nf if name.endswith("start+base") else 0
        alg = batch_bytes(nx, ny, nlev, nf, kind, extra)
        r = {"call": name, "memory": memory, "coordinate": kind, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **bk.stats(ts, key), "algorithmic_bytes": alg}
        r["GBps"], r["share_of_8TBps"] = bk.rate(alg, r[key])
        print(json.dumps(r), flush=True)
        if name != "vderiv centred":
            lines.append({"call": name, "memory": memory, "coordinate": kind, "nfields": nf, "GBps": r["GBps"], "vderiv_centred_GBps": round(base_gbps, 1),
                          "ratio_to_vderiv_GBps": round(r["GBps"] / base_gbps, 3)})


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    on_device = "--host" not in sys.argv
    on_host = "--host" in sys.argv or "--all" in sys.argv
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    alevel, blevel, levels, ps, make_coord = bk.hybrid_atmosphere(nx, ny, nlev, dev, gen)
    start = {"first": torch.full((ny, nx), 0.005, device=dev), "last": (ps + 5).contiguous()}
    bases = torch.rand((max(NFS), ny, nx), generator=gen, device=dev) * 2000
    lines = []
    with fc.Context(0) as ctx:
        if on_device:
            ctx.use_torch_stream()
            all_fields = torch.randn((max(NFS), nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
            coord = make_coord()
            out_all = torch.empty((max(NFS), nlev, ny, nx), device=dev, dtype=torch.float32)
            for nf in NFS:
                for kind in KINDS:
                    calls = make_calls(ctx, kind, all_fields[:nf], ps, coord, alevel, blevel, levels, start, bases, out_all[:nf])
                    report(bk.alternate(ctx, calls, ROUNDS)[1], "kernel_ms", nx, ny, nlev, nf, kind, "device", lines)
            del all_fields, coord, out_all
            torch.cuda.empty_cache()
        if on_host:
            rng = np.random.default_rng(2024)
            h_ps = ps.cpu().numpy()
            h_start = {k: v.cpu().numpy() for k, v in start.items()}
            h_bases = bases.cpu().numpy()
            h_fields = (rng.standard_normal((max(NFS), nlev, ny, nx), dtype=np.float32) * 3 + 250).astype(np.float32)
            h_coord = (alevel[:, None, None] + blevel[:, None, None] * h_ps[None]).astype(np.float32)
            h_out = np.empty((max(NFS), nlev, ny, nx), np.float32)
            for nf in NFS:
                for kind in ("hybrid",):
                    calls = make_calls(ctx, kind, h_fields[:nf], h_ps, h_coord, alevel, blevel, levels, h_start, h_bases, h_out[:nf])
                    walled = {name: (call, bk.WALL) for name, call in calls.items()}
                    report(bk.alternate(ctx, walled, HOST_ROUNDS)[0], "wall_ms", nx, ny, nlev, nf, kind, "host", lines)
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
