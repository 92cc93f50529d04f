#!/usr/bin/env python3
"""Layer integrals, means and extremes of level batches: mifc_vlayer_hlevels / mifc_vlayer_fields with all six products,
with the sums alone and with the extremes alone, on 1, 4 and 8 device-resident fields of 1440x720x137 (the shapes of
tools/bench_vinterp.py), an open layer and the layer [300, 850] hPa -- next to the yardstick, mifc_vinterp_hlevels /
_fields with ONE target on the same inputs in the same process (it reads the same levels).  Per case: the kernel time of
each of ROUNDS calls after a warm-up call (HIP events around the launches of the call, measurement build; the calls of
the two operators alternate), its median, minimum and spread (max - min), the algorithmic bytes per call
((nfields nlev + (nlev | 1) + bounds + nfields nproducts) x 4 per cell: every field level, the coordinate or ps, the
bound fields read once, every product written once), the rate they give and its share of the 8 TB/s peak.

    python tools/bench_vlayer.py [--small]   -> one JSON line per case, then one comparison line per case
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc

NFS = (1, 4, 8)
ROUNDS = 9
ALL = ["integral", "mean", "max", "min", "coord_of_max", "coord_of_min"]
PRODUCTS = {"all six": ALL, "sums": ALL[:2], "extremes": ALL[2:]}
LAYERS = {"open": (-np.inf, np.inf), "300..850": (300.0, 850.0)}


def vlayer_bytes(nx, ny, nlev, nf, nproducts, hybrid, nbounds=0):
    return (nf * nlev + (1 if hybrid else nlev) + nbounds + nf * nproducts) * 4 * nx * ny


def vinterp_bytes(nx, ny, nlev, nf, nt, hybrid):
    return (nf * nlev + (0 if hybrid else nlev) + 1 + nf * nt) * 4 * nx * ny


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    alevel, blevel, _, ps, make_coord = bk.hybrid_atmosphere(nx, ny, nlev, dev, gen)
    all_fields = torch.randn((max(NFS), nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    coord = make_coord()
    lines = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        for nf in NFS:
            fields = all_fields[:nf]
            vi_out = torch.empty((nf, 1, ny, nx), device=dev, dtype=torch.float32)
            for kind in ("hybrid", "field"):
                hybrid = kind == "hybrid"
                calls = {}
                if hybrid:
                    calls["vinterp"] = lambda: ctx.vinterp_hlevels(fields, ps, alevel, blevel, [500.0], out=vi_out)  # noqa: B023
                else:
                    calls["vinterp"] = lambda: ctx.vinterp_fields(fields, coord, [500.0], out=vi_out)  # noqa: B023
                outs = {}
                for pname, products in PRODUCTS.items():
                    outs[pname] = torch.empty((nf, len(products), ny, nx), device=dev, dtype=torch.float32)
                    for lname, (lo, hi) in LAYERS.items():
                        if pname != "all six" and lname != "open":
                            continue
                        if hybrid:
                            call = lambda products=products, lo=lo, hi=hi, o=outs[pname]: ctx.vlayer_hlevels(  # noqa: B023, E731
                                fields, ps, alevel, blevel, products, lo, hi, out=o)  # noqa: B023
                        else:
                            call = lambda products=products, lo=lo, hi=hi, o=outs[pname]: ctx.vlayer_fields(  # noqa: B023, E731
                                fields, coord, products, lo, hi, out=o)  # noqa: B023
                        calls["vlayer %s, %s" % (pname, lname)] = call
                _, ms = bk.alternate(ctx, calls, ROUNDS)
                base = bk.stats(ms["vinterp"])
                for name, ts in ms.items():
                    if name == "vinterp":
                        alg = vinterp_bytes(nx, ny, nlev, nf, 1, hybrid)
                    else:
                        alg = vlayer_bytes(nx, ny, nlev, nf, len(PRODUCTS[name.split(",")[0][7:]]), hybrid)
                    r = {"call": name, "coordinate": kind, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, **bk.stats(ts), "algorithmic_bytes": alg}
                    r["GBps"], r["share_of_8TBps"] = bk.rate(alg, r["kernel_ms"])
                    print(json.dumps(r), flush=True)
                    if name != "vinterp":  # within_spread: median against median plus the yardstick's spread, not benchkit.not_slower (minima, two spreads)
                        lines.append({"call": name, "coordinate": kind, "nfields": nf, "kernel_ms": r["kernel_ms"], "vinterp_1_target_ms": base["kernel_ms"],
                                      "vinterp_spread_ms": base["kernel_ms_spread"], "ratio_to_vinterp": round(r["kernel_ms"] / base["kernel_ms"], 3),
                                      "within_spread": bool(r["kernel_ms"] <= base["kernel_ms"] + base["kernel_ms_spread"])})
                del outs
            del vi_out
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
