#!/usr/bin/env python3
"""Level batches to constant surfaces: mifc_vinterp_hlevels / mifc_vinterp_fields on 4 device-resident fields of
1440x720x137 with 8 and with 33 targets (33: the second pass reads the inputs again), both coordinate kinds, both methods
-- median kernel time over ROUNDS calls after a warm-up call (HIP events around the launches, measurement build), the
algorithmic bytes per call ((nfields nlev [+ nlev] + 1 + nfields ntargets) x 4 per cell: every input level, the
coordinate and ps read once, every output written once) and the rate they give -- next to the stream yardstick
(mifc_bench_stream2, plain two-in / two-out copy) in the same process, timed the same way, and the ratio of the two
rates.  The surface pressure is a smooth field (orography-like, 520..1040 hPa) plus small noise, the levels the 137
of a cubic eta distribution, so the targets of a wave's cells sit at neighbouring levels as they do in model output.

    python tools/bench_vinterp.py [--small]   -> one JSON line per case, then the yardstick, then the ratios
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*, mifc_bench_stream2)
import numpy as np
import torch

import mi_fieldcalc_amd as fc

NF = 4
ROUNDS = 9
BURST = 5  # calls of the stream yardstick between two events
TARGETS = {8: [1000, 925, 850, 700, 500, 300, 200, 100],
           33: list(np.linspace(1000, 40, 33))}


def algorithmic_bytes(nx, ny, nlev, nf, nt, hybrid):
    return (nf * nlev + (0 if hybrid else nlev) + 1 + nf * nt) * 4 * nx * ny


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    alevel, blevel, _, ps, make_coord = bk.hybrid_atmosphere(nx, ny, nlev, dev, gen)
    fields = torch.randn((NF, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    coord = make_coord()
    results = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        for nt, targets in TARGETS.items():
            out = torch.empty((NF, nt, ny, nx), device=dev, dtype=torch.float32)
            for kind in ("hybrid", "field"):
                for method in ("linear", "log"):
                    if kind == "hybrid":
                        call = lambda: ctx.vinterp_hlevels(fields, ps, alevel, blevel, targets, method=method, out=out)  # noqa: B023, E731
                    else:
                        call = lambda: ctx.vinterp_fields(fields, coord, targets, method=method, out=out)  # noqa: B023, E731
                    _, ms = bk.alternate(ctx, {"vinterp": call}, ROUNDS)
                    alg = algorithmic_bytes(nx, ny, nlev, NF, nt, kind == "hybrid")
                    r = {"call": "vinterp_" + ("hlevels" if kind == "hybrid" else "fields"), "method": method, "nx": nx, "ny": ny, "nlev": nlev,
                         "nfields": NF, "ntargets": nt, **bk.stats(ms["vinterp"]), "algorithmic_bytes": alg}
                    r["GBps"] = bk.rate(alg, r["kernel_ms"])[0]
                    r["defined_share"] = round(float((out != float(fc.UNDEF)).float().mean()), 3)
                    results.append(r)
                    print(json.dumps(r), flush=True)
            del out
        # the yardstick: stream two arrays in, two out, 2 x 568 MB each way at full size
        n = (nx * ny * nlev) // 4 * 4
        a, b = fields[0].reshape(-1)[:n], fields[1].reshape(-1)[:n]
        x, y = torch.empty_like(a), torch.empty_like(b)
        _, ms = bk.alternate(ctx, {"stream2": (lambda: [ctx.bench_stream2(0, 0, x, y, a, b) for _ in range(BURST)], bk.EVENTS)}, ROUNDS)
        med, best = float(np.median(ms["stream2"])) / BURST, min(ms["stream2"]) / BURST
        stream = 4 * n * 4 / med / 1e6
        print(json.dumps({"call": "mifc_bench_stream2 (yardstick: plain copy, two in, two out)", "bytes": 16 * n, "ms": round(med, 4),
                          "ms_min": round(best, 4), "GBps": round(stream, 1)}), flush=True)
        for r in results:
            print(json.dumps({"call": r["call"], "method": r["method"], "ntargets": r["ntargets"], "GBps": r["GBps"],
                              "ratio_to_stream2": round(r["GBps"] / stream, 3)}), flush=True)


if __name__ == "__main__":
    main()
