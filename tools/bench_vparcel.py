#!/usr/bin/env python3
"""Parcel ascent over level batches: mifc_vparcel_hlevels on 1440x720x137 device arrays, the source at the lowest level,
with all six outputs and with cape alone -- next to two yardsticks measured in the same process on the same arrays:

  * mifc_showalterIndex, the same seven-trip adjustment loop once per cell: its kernel time per cell and trip is the
    price of a trip (with the loop's loads and store spread over seven trips), and trips x that price is what the
    thermodynamics of the walk would cost alone;
  * mifc_vcumul_hlevels with the LOG method on one field: the same walk -- one batch and ps read, one double log per
    cell and level, a carried double sum -- without the thermodynamics (it writes a batch, like tparcel).

Per case: the kernel time of each of ROUNDS calls after a warm-up call (HIP events around the launches of the call,
measurement build; the calls alternate), its median, minimum and spread, the algorithmic bytes and the rate they give.
The adjustment trips per cell and level are counted from the result: a level is adjusted when it lies above the cell's
condensation level (p < plcl), and an adjusted level takes seven trips (the reference's `break` needs a parcel outside the
saturation table, which these soundings do not produce).

    python tools/bench_vparcel.py [--small]   -> one JSON line per call, then one summary line
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import vcumul, vparcel

ROUNDS = 9
EWT = [.000034, .000089, .000220, .000517, .001155, .002472, .005080, .01005, .01921, .03553, .06356, .1111, .1891, .3139, .5088, .8070, 1.2540,
       1.9118, 2.8627, 4.2148, 6.1078, 8.7192, 12.272, 17.044, 23.373, 31.671, 42.430, 56.236, 73.777, 95.855, 123.40, 157.46, 199.26, 250.16,
       311.69, 385.56, 473.67, 578.09, 701.13, 845.28, 1013.25]  # MetConstants.h:57-59


def qsat(t, p):
    tab = torch.tensor(EWT, device=t.device, dtype=torch.float32)
    x = ((t - 273.15) + 100.0) * 0.2
    l = x.floor().clamp(0, 39).long()
    return 0.622 * (tab[l] + (tab[l + 1] - tab[l]) * (x - l)) / p


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    # top-down, the last level is the surface; the top near 240 hPa: the levels a parcel is lifted through -- above them the
    # coldest parcels leave the saturation table (-100 C), which ends a walk by rule 3
    alevel, blevel, _ = bk.hybrid_levels(np.linspace(0.63, 1, nlev) ** 3)
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, ny, device=dev), torch.linspace(0, 12.56, nx, device=dev), indexing="ij")
    ps = (900 + 120 * torch.sin(xx) * torch.cos(yy) + torch.randn((ny, nx), generator=gen, device=dev)).clamp(700, 1040).contiguous()
    p = bk.coordinate_batch(alevel, blevel, ps, dev)
    ts = 285 + 17 * torch.cos(yy) * torch.sin(0.5 * xx)
    lapse = 0.17 + 0.04 * torch.sin(3 * xx)
    t = torch.maximum(ts[None] * (p / ps[None]) ** lapse[None], torch.full_like(p, 212.0)).contiguous()
    t += torch.randn(t.shape, generator=gen, device=dev) * 0.2
    rh = (0.65 + 0.3 * torch.sin(2 * yy + xx)).clamp(0.25, 0.98)
    q_src = (rh * qsat(t[nlev - 1], p[nlev - 1])).contiguous()
    del p
    cells = nx * ny
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        outs = {n: torch.empty((nlev, ny, nx) if n == "tparcel" else (ny, nx), device=dev) for n in vparcel.VPARCEL_OUTPUTS}
        zout = torch.empty((nlev, ny, nx), device=dev)
        # the Showalter yardstick on a 2-D field of the batch's size: eight rows of levels side by side
        rows = min(nlev, 8)
        t850 = t[nlev - rows:].reshape(rows * ny, nx).contiguous()
        t500 = (t850 - 30).contiguous()
        rh850 = torch.full_like(t850, 80.0)
        sout = torch.empty_like(t850)
        calls = {
            "vparcel all outputs": lambda: vparcel.vparcel_hlevels(ctx, t, ps, alevel, blevel, q_src, src_level=nlev - 1, from_="last",
                                                                   outputs=vparcel.VPARCEL_OUTPUTS, out=outs),
            "vparcel cape only": lambda: vparcel.vparcel_hlevels(ctx, t, ps, alevel, blevel, q_src, src_level=nlev - 1, from_="last", outputs=("cape",),
                                                                 out={"cape": outs["cape"]}),
            "vcumul log": lambda: vcumul.vcumul_hlevels(ctx, t, ps, alevel, blevel, "log", "last", out=zout),
            "showalterIndex": lambda: ctx.showalterIndex(t500, t850, rh850, 500.0, 850.0, 1, out=sout),
        }
        _, ms = bk.alternate(ctx, calls, ROUNDS)
        form = vparcel.last_vparcel_form(ctx)
        # what the walk did, from its results
        r = vparcel.vparcel_hlevels(ctx, t, ps, alevel, blevel, q_src, src_level=nlev - 1, from_="last", outputs=vparcel.VPARCEL_OUTPUTS, out=outs)
        undef = float(vparcel.UNDEF)
        pb = bk.coordinate_batch(alevel, blevel, ps, dev)
        walked = r["tparcel"] != undef
        adjusted = walked & (pb < torch.where(r["plcl"] != undef, r["plcl"], torch.zeros_like(r["plcl"]))[None])
        adjusted[nlev - 1] = False  # the source level itself is not stepped to
        share = float(adjusted.float().mean())
        trips = 7.0 * share
        cape = r["cape"]
        summary = {"cells": cells, "nlev": nlev, "form": form, "adjusted_share_of_cell_levels": round(share, 4), "trips_per_cell_and_level": round(trips, 3),
                   "walked_share": round(float(walked.float().mean()), 4), "cells_with_cape": round(float(((cape > 0) & (cape != undef)).float().mean()), 4),
                   "median_cape": round(float(cape[(cape > 0) & (cape != undef)].median()), 1) if ((cape > 0) & (cape != undef)).any() else 0.0,
                   "flags": {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r["flags"].items() if k != "tparcel"}}
    plane, batch = 4 * cells, 4 * cells * nlev
    bytes_ = {"vparcel all outputs": batch + 2 * plane + 5 * plane + batch, "vparcel cape only": batch + 2 * plane + plane, "vcumul log": 2 * batch + plane,
              "showalterIndex": 4 * 4 * t850.numel()}
    res = {}
    for name, tms in ms.items():
        s = bk.stats(tms)
        res[name] = s["kernel_ms"]
        gbps, share = bk.rate(bytes_[name], s["kernel_ms"])
        print(json.dumps({"call": name, "nx": nx, "ny": ny, "nlev": nlev, **s, "algorithmic_bytes": bytes_[name], "GBps": gbps, "share_of_8TBps": share}), flush=True)
    trip_ns = res["showalterIndex"] * 1e6 / (t850.numel() * 7.0)  # ns per cell and trip, the loop's own loads and store included
    thermo_ms = trip_ns * trips * cells * (nlev - 1) / 1e6
    summary.update({"showalter_ns_per_cell_trip": round(trip_ns, 5), "trips_times_showalter_price_ms": round(thermo_ms, 3), "vcumul_log_ms": res["vcumul log"],
                    "vparcel_all_ms": res["vparcel all outputs"], "vparcel_cape_ms": res["vparcel cape only"],
                    "vparcel_all_over_vcumul_log": round(res["vparcel all outputs"] / res["vcumul log"], 2),
                    "vparcel_all_over_trips_price": round(res["vparcel all outputs"] / thermo_ms, 2) if thermo_ms > 0 else None,
                    "vparcel_ns_per_cell_level": round(res["vparcel all outputs"] * 1e6 / (cells * (nlev - 1)), 5)})
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()
