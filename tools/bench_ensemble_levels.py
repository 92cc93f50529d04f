#!/usr/bin/env python3
"""Ensemble statistics of a level batch in one pass: mifc_ensemble_levels on 51 device-resident members of 1440x720
(nlev 1 and 10; {mean}, {mean, stddev} and the seven-product set mean, stddev, max, min and probability above three
thresholds) next to the same products through the single-field entries, one call per level and product, in the same
process on the same buffers.  Median of 9 with the min-max spread, of the synchronous call time (host clock around the
calls and a device synchronise) and of the summed kernel time (HIP events around the launches, measurement build);
algorithmic bytes (nmem + nproducts) x 4 B per cell, as a fraction of 8 TB/s over the kernel time.

    python tools/bench_ensemble_levels.py   -> two JSON lines (fused, yardstick) per (nlev, product set)
"""
import json
import statistics

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import torch

import mi_fieldcalc_amd as fc

NX, NY, NMEM = 1440, 720, 51
ROUNDS = 9
THRESHOLDS = (271.0, 273.0, 276.0)
SETS = {
    "mean": ["mean"],
    "mean+stddev": ["mean", "stddev"],
    "seven": ["mean", "stddev", "max", "min"] + [("probability", 1, [t]) for t in THRESHOLDS],
}


def report(what, name, nlev, nprod, ts, ks):
    alg = (NMEM + nprod) * 4 * nlev * NX * NY
    kms = float(statistics.median(ks))
    print(json.dumps({"call": what, "products": name, "nproducts": nprod, "nmem": NMEM, "nx": NX, "ny": NY, "nlev": nlev,
                      "ms": round(float(statistics.median(ts)), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                      "kernel_ms": round(kms, 4), "kernel_ms_min": round(min(ks), 4), "kernel_ms_max": round(max(ks), 4),
                      "algorithmic_bytes": alg, "kernel_frac_of_8TBps": bk.rate(alg, kms)[1]}), flush=True)
    return kms


def single_field(ctx, spec, fields, flags, out):
    name = spec if isinstance(spec, str) else spec[0]
    if name == "mean":
        return ctx.meanValue(fields, flags, out=out)
    if name == "stddev":
        return ctx.stddevValue(fields, flags, out=out)
    if name in ("max", "min"):
        return ctx.extremeValue(1 if name == "max" else 2, fields, out=out)
    return ctx.probability(spec[1], fields, flags, spec[2], out=out)


def main():
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    with fc.Context(0) as ctx:
        for nlev in (1, 10):
            members = torch.randn((NMEM, nlev, NY, NX), generator=gen, device=dev, dtype=torch.float32) * 3 + 273
            per_level = [[members[j, l] for j in range(NMEM)] for l in range(nlev)]
            flags = [fc.SOME_DEFINED] * NMEM
            for name, products in SETS.items():
                out = torch.empty((len(products), nlev, NY, NX), device=dev, dtype=torch.float32)
                ts, ks = bk.alternate(ctx, {"fused": (lambda: ctx.ensembleStatistics(members, products, out=out), bk.WALL_KERNEL)}, ROUNDS)  # noqa: B023
                fused = report("ensembleStatistics", name, nlev, len(products), ts["fused"], ks["fused"])

                def level(l, lv):
                    for k, spec in enumerate(products):  # noqa: B023
                        assert single_field(ctx, spec, lv, flags, out[k, l]) is not None  # noqa: B023

                def yardstick(section):
                    # at most 16 launches are timed per section: one section per level, summed
                    for l, lv in enumerate(per_level):  # noqa: B023
                        section(lambda l=l, lv=lv: level(l, lv))

                ts, ks = bk.alternate(ctx, {"yardstick": (yardstick, bk.WALL_SECTIONS)}, ROUNDS)
                ts, ks = ts["yardstick"], ks["yardstick"]
                base = report("single-field entries (yardstick, one call per level and product)", name, nlev, len(products), ts, ks)
                print(json.dumps({"products": name, "nlev": nlev, "kernel_ms_fused": round(fused, 4), "kernel_ms_yardstick": round(base, 4),
                                  "yardstick_kernel_spread_ms": round(max(ks) - min(ks), 4), "fused_over_yardstick": round(fused / base, 4)}), flush=True)
            del members, per_level


if __name__ == "__main__":
    main()
