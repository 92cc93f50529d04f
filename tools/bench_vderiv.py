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
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import torch

import mi_fieldcalc_amd as fc

NFS = (1, 2, 4, 8)
ROUNDS = 9
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


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    alevel, blevel, levels, ps, make_coord = bk.hybrid_atmosphere(nx, ny, nlev, dev, gen)
    all_fields = torch.randn((max(NFS), nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    coord = make_coord()
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
                _, ms = bk.alternate(ctx, calls, ROUNDS)
                base = bk.stats(ms["vinterp"])
                base_bytes = vinterp_bytes(nx, ny, nlev, nf, 1, kind != "field")
                base_gbps = base_bytes / base["kernel_ms"] / 1e6
                base_lo = base_bytes / (base["kernel_ms_min"] + base["kernel_ms_spread"]) / 1e6  # its slowest call
                for name, ts in ms.items():
                    alg = base_bytes if name == "vinterp" else vderiv_bytes(nx, ny, nlev, nf, kind, name.split(", ")[1])
                    r = {"call": name, "coordinate": kind, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **bk.stats(ts), "algorithmic_bytes": alg}
                    r["GBps"], r["share_of_8TBps"] = bk.rate(alg, r["kernel_ms"])
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
