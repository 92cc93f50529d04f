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
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIFC_LIB_PATH", os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc_measure.so"))  # mifc_timing_*: measurement build

import torch  # noqa: E402

import mi_fieldcalc_amd as fc  # noqa: E402

NX, NY, NMEM = 1440, 720, 51
PEAK = 8000.0  # GB/s
ROUNDS = 9
THRESHOLDS = (271.0, 273.0, 276.0)
SETS = {
    "mean": ["mean"],
    "mean+stddev": ["mean", "stddev"],
    "seven": ["mean", "stddev", "max", "min"] + [("probability", 1, [t]) for t in THRESHOLDS],
}


def timed(ctx, call):
    call()  # warm-up
    torch.cuda.synchronize()
    ts, ks = [], []
    for _ in range(ROUNDS):
        ctx.timing_begin()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        ks.append(ctx.timing_end_ms())
    return ts, ks


def report(what, name, nlev, nprod, ts, ks):
    alg = (NMEM + nprod) * 4 * nlev * NX * NY
    kms = float(np.median(ks))
    print(json.dumps({"call": what, "products": name, "nproducts": nprod, "nmem": NMEM, "nx": NX, "ny": NY, "nlev": nlev,
                      "ms": round(float(np.median(ts)), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4),
                      "kernel_ms": round(kms, 4), "kernel_ms_min": round(min(ks), 4), "kernel_ms_max": round(max(ks), 4),
                      "algorithmic_bytes": alg, "kernel_frac_of_8TBps": round(alg / kms / 1e6 / PEAK, 4) if kms > 0 else None}), flush=True)
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
                ts, ks = timed(ctx, lambda: ctx.ensembleStatistics(members, products, out=out))  # noqa: B023
                fused = report("ensembleStatistics", name, nlev, len(products), ts, ks)

                def yardstick():
                    # at most 16 launches are timed per section: one section per level, summed
                    k_ms = 0.0
                    for l, lv in enumerate(per_level):  # noqa: B023
                        ctx.timing_begin()
                        for k, spec in enumerate(products):  # noqa: B023
                            assert single_field(ctx, spec, lv, flags, out[k, l]) is not None  # noqa: B023
                        torch.cuda.synchronize()
                        k_ms += ctx.timing_end_ms()
                    return k_ms

                yardstick()  # warm-up
                ts, ks = [], []
                for _ in range(ROUNDS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ks.append(yardstick())
                    ts.append((time.perf_counter() - t0) * 1e3)
                base = report("single-field entries (yardstick, one call per level and product)", name, nlev, len(products), ts, ks)
                print(json.dumps({"products": name, "nlev": nlev, "kernel_ms_fused": round(fused, 4), "kernel_ms_yardstick": round(base, 4),
                                  "yardstick_kernel_spread_ms": round(max(ks) - min(ks), 4), "fused_over_yardstick": round(fused / base, 4)}), flush=True)
            del members, per_level


if __name__ == "__main__":
    main()
