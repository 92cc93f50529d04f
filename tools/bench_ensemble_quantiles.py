#!/usr/bin/env python3
"""Percentiles across ensemble members: mifc_ensembleQuantiles on 51 device-resident members of 1440x720 (nlev 1 and
10, nq 1 and 5, both methods) -- median synchronous call time (host clock around the call and a device synchronise)
and summed kernel time (HIP events around the launches, measurement build), algorithmic bytes ((nmem + nq) x 4 B per
cell: every member read once, every output written once), fraction of 8 TB/s -- next to meanValue on the same members
(one call per level) as the yardstick, in the same process on the same buffers.

    python tools/bench_ensemble_quantiles.py   -> one JSON line per (nlev, nq, method), then one per yardstick
"""
import json

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import torch

import mi_fieldcalc_amd as fc

NX, NY, NMEM = 1440, 720, 51
ROUNDS = 9
PS = {1: [50.0], 5: [10.0, 25.0, 50.0, 75.0, 90.0]}


def timed(ctx, call):
    assert call() is not None, ctx.last_error()
    ts, ks = bk.alternate(ctx, {"call": (call, bk.WALL_KERNEL)}, ROUNDS)
    return bk.stats(ts["call"], "ms")["ms"], bk.stats(ks["call"])["kernel_ms"]


def fractions(alg, ms, kms):
    return {"algorithmic_bytes": alg, "frac_of_8TBps": bk.rate(alg, ms)[1], "kernel_frac_of_8TBps": bk.rate(alg, kms)[1]}


def main():
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    with fc.Context(0) as ctx:
        for nlev in (1, 10):
            members = torch.randn((NMEM, nlev, NY, NX), generator=gen, device=dev, dtype=torch.float32) * 3 + 273
            cells = nlev * NX * NY
            for nq in (1, 5):
                out = torch.empty((nq, nlev, NY, NX), device=dev, dtype=torch.float32)
                for method in ("lower", "linear"):
                    ms, kms = timed(ctx, lambda: ctx.ensembleQuantiles(members, PS[nq], method=method, out=out))  # noqa: B023
                    print(json.dumps({"call": "ensembleQuantiles", "method": method, "nmem": NMEM, "nx": NX, "ny": NY, "nlev": nlev, "nq": nq,
                                      "ms": ms, "kernel_ms": kms, **fractions((NMEM + nq) * 4 * cells, ms, kms)}), flush=True)
            # yardstick: meanValue over the same members, one call per level (it takes 2-D fields)
            mean_out = torch.empty((NY, NX), device=dev, dtype=torch.float32)
            per_level = [[members[j, l] for j in range(NMEM)] for l in range(nlev)]
            flags = [fc.SOME_DEFINED] * NMEM

            def means():
                for lv in per_level:
                    r = ctx.meanValue(lv, flags, out=mean_out)
                return r

            ms, kms = timed(ctx, means)
            print(json.dumps({"call": "meanValue (yardstick, one call per level)", "nmem": NMEM, "nx": NX, "ny": NY, "nlev": nlev, "ms": ms,
                              "kernel_ms": kms, **fractions((NMEM + 1) * 4 * cells, ms, kms)}), flush=True)
            del members


if __name__ == "__main__":
    main()
