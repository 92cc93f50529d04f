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
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIFC_LIB_PATH", os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc_measure.so"))  # mifc_timing_*, mifc_bench_stream2

import torch  # noqa: E402

import mi_fieldcalc_amd as fc  # noqa: E402

NX, NY, NLEV, NF = 1440, 720, 137, 4
ROUNDS = 9
TARGETS = {8: [1000, 925, 850, 700, 500, 300, 200, 100],
           33: list(np.linspace(1000, 40, 33))}


def algorithmic_bytes(nx, ny, nlev, nf, nt, hybrid):
    return (nf * nlev + (0 if hybrid else nlev) + 1 + nf * nt) * 4 * nx * ny


def kernel_ms(ctx, call):
    call()  # warm-up: code object, scratch
    torch.cuda.synchronize()
    ks = []
    for _ in range(ROUNDS):
        ctx.timing_begin()
        call()
        torch.cuda.synchronize()
        ks.append(ctx.timing_end_ms())
    return float(np.median(ks)), float(min(ks))


def event_ms(call, inner=5):
    call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ROUNDS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(inner):
            call()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / inner)
    return float(np.median(ts)), float(min(ts))


def main():
    nx, ny, nlev = (360, 180, 24) if "--small" in sys.argv else (NX, NY, NLEV)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    eta = np.linspace(0.01, 1, nlev) ** 3
    alevel, blevel = (1000 * (eta - eta ** 2)).astype(np.float32), (eta ** 2).astype(np.float32)
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, ny, device=dev), torch.linspace(0, 12.56, nx, device=dev), indexing="ij")
    ps = (780 + 260 * torch.sin(xx) * torch.cos(yy) + torch.randn((ny, nx), generator=gen, device=dev)).clamp(520, 1040).contiguous()
    fields = torch.randn((NF, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    coord = (torch.from_numpy(alevel).to(dev)[:, None, None] + torch.from_numpy(blevel).to(dev)[:, None, None] * ps[None]).contiguous()
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
                    med, best = kernel_ms(ctx, call)
                    alg = algorithmic_bytes(nx, ny, nlev, NF, nt, kind == "hybrid")
                    _, fd = call()
                    r = {"call": "vinterp_" + ("hlevels" if kind == "hybrid" else "fields"), "method": method, "nx": nx, "ny": ny, "nlev": nlev,
                         "nfields": NF, "ntargets": nt, "kernel_ms": round(med, 4), "kernel_ms_min": round(best, 4), "algorithmic_bytes": alg,
                         "GBps": round(alg / med / 1e6, 1), "defined_share": round(float((out != float(fc.UNDEF)).float().mean()), 3)}
                    results.append(r)
                    print(json.dumps(r), flush=True)
            del out
        # the yardstick: stream two arrays in, two out, 2 x 568 MB each way at full size
        n = (nx * ny * nlev) // 4 * 4
        a, b = fields[0].reshape(-1)[:n], fields[1].reshape(-1)[:n]
        x, y = torch.empty_like(a), torch.empty_like(b)
        med, best = event_ms(lambda: ctx.bench_stream2(0, 0, x, y, a, b))
        stream = 4 * n * 4 / med / 1e6
        print(json.dumps({"call": "mifc_bench_stream2 (yardstick: plain copy, two in, two out)", "bytes": 16 * n, "ms": round(med, 4),
                          "ms_min": round(best, 4), "GBps": round(stream, 1)}), flush=True)
        for r in results:
            print(json.dumps({"call": r["call"], "method": r["method"], "ntargets": r["ntargets"], "GBps": r["GBps"],
                              "ratio_to_stream2": round(r["GBps"] / stream, 3)}), flush=True)


if __name__ == "__main__":
    main()
