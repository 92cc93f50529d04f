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
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIFC_LIB_PATH", os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc_measure.so"))  # mifc_timing_*

import torch  # noqa: E402

import mi_fieldcalc_amd as fc  # noqa: E402
from mi_fieldcalc_amd import vcumul  # noqa: E402

NX, NY, NLEV = 1440, 720, 137
NFS = (1, 4, 8)
ROUNDS, HOST_ROUNDS = 9, 3
PEAK_GBPS = 8000.0
KINDS = ("hybrid", "field", "levels")
# (name, method, from_, with start and base)
CASES = (("linear, first", "linear", "first", False), ("linear, last", "linear", "last", False), ("linear, last, start+base", "linear", "last", True),
         ("log, first", "log", "first", False), ("log, last, start+base", "log", "last", True))


def coord_planes(kind, nlev):
    return {"hybrid": 1, "field": nlev, "levels": 0}[kind]


def batch_bytes(nx, ny, nlev, nf, kind, extra_planes=0):
    """Every field level and the coordinate (or ps) read once, every output level written once; the start and base planes."""
    return (nf * nlev + coord_planes(kind, nlev) + nf * nlev + extra_planes) * 4 * nx * ny


def kernel_ms_alternating(ctx, calls):
    """calls: name -> callable.  One warm-up each, then ROUNDS rounds in which every call is timed once, in turn."""
    for call in calls.values():
        call()  # warm-up: code object, scratch
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            ctx.timing_begin()
            call()
            torch.cuda.synchronize()
            ms[name].append(ctx.timing_end_ms())
    return ms


def wall_ms_alternating(calls):
    for call in calls.values():
        call()
    ms = {name: [] for name in calls}
    for _ in range(HOST_ROUNDS):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return ms


def stats(ts, key):
    return {key: round(float(np.median(ts)), 4), key + "_min": round(min(ts), 4), key + "_spread": round(max(ts) - min(ts), 4)}


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
    base = stats(ms["vderiv centred"], key)
    base_bytes = batch_bytes(nx, ny, nlev, nf, kind)
    base_gbps = base_bytes / base[key] / 1e6
    for name, ts in ms.items():
        extra = 1 + nf if name.endswith("start+base") else 0
        alg = batch_bytes(nx, ny, nlev, nf, kind, extra)
        r = {"call": name, "memory": memory, "coordinate": kind, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **stats(ts, key), "algorithmic_bytes": alg}
        r["GBps"] = round(alg / r[key] / 1e6, 1)
        r["share_of_8TBps"] = round(r["GBps"] / PEAK_GBPS, 3)
        print(json.dumps(r), flush=True)
        if name != "vderiv centred":
            lines.append({"call": name, "memory": memory, "coordinate": kind, "nfields": nf, "GBps": r["GBps"], "vderiv_centred_GBps": round(base_gbps, 1),
                          "ratio_to_vderiv_GBps": round(r["GBps"] / base_gbps, 3)})


def main():
    nx, ny, nlev = (360, 180, 24) if "--small" in sys.argv else (NX, NY, NLEV)
    on_device = "--host" not in sys.argv
    on_host = "--host" in sys.argv or "--all" in sys.argv
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    eta = np.linspace(0.01, 1, nlev) ** 3
    alevel, blevel = (1000 * (eta - eta ** 2)).astype(np.float32), (eta ** 2).astype(np.float32)
    levels = (alevel + blevel * np.float32(1000)).astype(np.float32)
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, ny, device=dev), torch.linspace(0, 12.56, nx, device=dev), indexing="ij")
    ps = (780 + 260 * torch.sin(xx) * torch.cos(yy) + torch.randn((ny, nx), generator=gen, device=dev)).clamp(520, 1040).contiguous()
    start = {"first": torch.full((ny, nx), 0.005, device=dev), "last": (ps + 5).contiguous()}
    bases = torch.rand((max(NFS), ny, nx), generator=gen, device=dev) * 2000
    lines = []
    with fc.Context(0) as ctx:
        if on_device:
            ctx.use_torch_stream()
            all_fields = torch.randn((max(NFS), nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
            coord = (torch.from_numpy(alevel).to(dev)[:, None, None] + torch.from_numpy(blevel).to(dev)[:, None, None] * ps[None]).contiguous()
            out_all = torch.empty((max(NFS), nlev, ny, nx), device=dev, dtype=torch.float32)
            for nf in NFS:
                for kind in KINDS:
                    calls = make_calls(ctx, kind, all_fields[:nf], ps, coord, alevel, blevel, levels, start, bases, out_all[:nf])
                    report(kernel_ms_alternating(ctx, calls), "kernel_ms", nx, ny, nlev, nf, kind, "device", lines)
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
                    report(wall_ms_alternating(calls), "wall_ms", nx, ny, nlev, nf, kind, "host", lines)
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
