#!/usr/bin/env python3
"""Vertical derivatives of level batches: mifc_vderiv_hlevels / mifc_vderiv_fields / mifc_vderiv_levels with both methods,
writing the derivatives, the magnitudes alone and both, on 1, 2, 4 and 8 device-resident fields of 1440x720x137 (the
shapes of tools/bench_vinterp.py and tools/bench_vlayer.py) -- next to the yardstick, mifc_vinterp_hlevels / _fields with
ONE target on the same inputs in the same process (it reads the same levels; the `levels` form is set beside the hybrid
one).  Per case: the kernel time of each of ROUNDS calls after a warm-up call (HIP events around the launches of the
call, measurement build; the calls alternate), its median, minimum and spread (max - min), the algorithmic bytes per
call (every field level and the coordinate or ps read once, every output level written once), the rate they give and
its share of the 8 TB/s peak.  vderiv writes a full batch where vinterp writes one level, so the comparison is of the
rates, not of the times.

    python tools/bench_vderiv.py [--small]   -> one JSON line per case, then one comparison line per case
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

NX, NY, NLEV = 1440, 720, 137
NFS = (1, 2, 4, 8)
ROUNDS = 9
PEAK_GBPS = 8000.0
KINDS = ("hybrid", "field", "levels")
METHODS = ("centred", "weighted")
WHAT = {"derivatives": None, "magnitude only": "only", "both": "also"}


def coord_planes(kind, nlev):
    return {"hybrid": 1, "field": nlev, "levels": 0}[kind]


def vderiv_bytes(nx, ny, nlev, nf, kind, what):
    written = (nf if what != "magnitude only" else 0) + (nf // 2 if what != "derivatives" else 0)
    return (nf * nlev + coord_planes(kind, nlev) + written * nlev) * 4 * nx * ny


def vinterp_bytes(nx, ny, nlev, nf, nt, hybrid):
    return (nf * nlev + (0 if hybrid else nlev) + 1 + nf * nt) * 4 * nx * ny


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
    all_fields = torch.randn((max(NFS), nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    coord = (torch.from_numpy(alevel).to(dev)[:, None, None] + torch.from_numpy(blevel).to(dev)[:, None, None] * ps[None]).contiguous()
    out_all = torch.empty((max(NFS), nlev, ny, nx), device=dev, dtype=torch.float32)
    mag_all = torch.empty((max(NFS) // 2, nlev, ny, nx), device=dev, dtype=torch.float32)
    lines = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        for nf in NFS:
            fields = all_fields[:nf]
            vi_out = torch.empty((nf, 1, ny, nx), device=dev, dtype=torch.float32)
            for kind in KINDS:
                calls = {}
                if kind == "field":
                    calls["vinterp"] = lambda: ctx.vinterp_fields(fields, coord, [500.0], out=vi_out)  # noqa: B023
                else:
                    calls["vinterp"] = lambda: ctx.vinterp_hlevels(fields, ps, alevel, blevel, [500.0], out=vi_out)  # noqa: B023
                for method in METHODS:
                    for wname, magnitude in WHAT.items():
                        if magnitude is not None and nf % 2:
                            continue
                        out = {None: out_all[:nf], "only": mag_all[:nf // 2], "also": (out_all[:nf], mag_all[:nf // 2])}[magnitude]
                        if kind == "hybrid":
                            call = lambda method=method, magnitude=magnitude, out=out: ctx.vderiv_hlevels(  # noqa: B023, E731
                                fields, ps, alevel, blevel, method, magnitude, out=out)  # noqa: B023
                        elif kind == "field":
                            call = lambda method=method, magnitude=magnitude, out=out: ctx.vderiv_fields(fields, coord, method, magnitude, out=out)  # noqa: B023, E731
                        else:
                            call = lambda method=method, magnitude=magnitude, out=out: ctx.vderiv_levels(fields, levels, method, magnitude, out=out)  # noqa: B023, E731
                        calls["vderiv %s, %s" % (method, wname)] = call
                ms = kernel_ms_alternating(ctx, calls)
                base = stats(ms["vinterp"])
                base_bytes = vinterp_bytes(nx, ny, nlev, nf, 1, kind != "field")
                base_gbps = base_bytes / base["kernel_ms"] / 1e6
                base_lo = base_bytes / (base["kernel_ms_min"] + base["kernel_ms_spread"]) / 1e6  # its slowest call
                for name, ts in ms.items():
                    alg = base_bytes if name == "vinterp" else vderiv_bytes(nx, ny, nlev, nf, kind, name.split(", ")[1])
                    r = {"call": name, "coordinate": kind, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **stats(ts), "algorithmic_bytes": alg}
                    r["GBps"] = round(alg / r["kernel_ms"] / 1e6, 1)
                    r["share_of_8TBps"] = round(r["GBps"] / PEAK_GBPS, 3)
                    print(json.dumps(r), flush=True)
                    if name != "vinterp":
                        best = alg / r["kernel_ms_min"] / 1e6  # its fastest call
                        lines.append({"call": name, "coordinate": kind, "nfields": nf, "GBps": r["GBps"], "vinterp_1_target_GBps": round(base_gbps, 1),
                                      "ratio_to_vinterp_GBps": round(r["GBps"] / base_gbps, 3), "within_the_two_spreads": bool(best >= base_lo)})
            del vi_out
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
