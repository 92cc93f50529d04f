#!/usr/bin/env python3
"""Iterative vessel-icing models on the GPU: vesselIcingModStall and vesselIcingMincog (alt 1) on one device-resident
1440x720 field, and a 51-member batch through mifc_vesselIcing_levels with the depth shared.  HIP events around the
synchronous call after warm-up -> Mcells/s and the ratio to the compiled reference on one host core (6.7 s and 14.8 s
per field, measured with the same input ranges).  Also, on the same field: the fraction of defined cells that are
bit-identical to the reference (oracle/_ref through tests/icing_ref_shim.cc, in row bands on 16 threads), and the
trip-count distribution of the data-dependent loops from the host build of the cell header (a row sample).

    python tools/bench_vessel_icing.py [--no-ref]   -> one JSON line per measurement
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import icing_cases as ic  # noqa: E402
import mi_fieldcalc_amd as fc  # noqa: E402

NX, NY, NLEV = 1440, 720, 51
REF_ONE_CORE_S = {"modstall": 6.7, "mincog": 14.8}  # one 1440x720 field, g++ -O3 -mavx2, one core
ROUNDS = 5
NO_REF = "--no-ref" in sys.argv


def timed(fn, rounds=ROUNDS):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def histogram(h, edges):
    out = {}
    for lo, hi in zip(edges[:-1], edges[1:]):
        c = int(h[lo:hi].sum())
        if c:
            out["%d-%d" % (lo, hi - 1) if hi - lo > 1 else str(lo)] = c
    return out


def main():
    ctx = fc.Context(0)
    host = ic.make_inputs(NX, NY, seed=2024)
    dev = [torch.from_numpy(f).cuda() for f in host]
    out = torch.empty((NY, NX), dtype=torch.float32, device="cuda")
    s = ic.SCALARS
    tmp = tempfile.mkdtemp()
    ref = ic.RefShim(tmp) if (ic.ref_available() and not NO_REF) else None
    cell = ic.CellShim(tmp)
    for name, model, alt in (("modstall", ic.MODSTALL, 1), ("mincog", ic.MINCOG, 1)):
        if model == ic.MODSTALL:
            call = lambda: ctx.vesselIcingModStall(*dev, s["vs"], s["alpha"], s["zmin"], s["zmax"], undef=ic.UNDEF, out=out)  # noqa: E731
        else:
            call = lambda: ctx.vesselIcingMincog(*dev, s["vs"], s["alpha"], s["zmin"], s["zmax"], alt, undef=ic.UNDEF, out=out)  # noqa: E731
        med, lo, hi = timed(call)
        rec = {"model": name, "alt": alt, "grid": [NX, NY], "levels": 21, "ms_median": round(med, 3), "ms_min": round(lo, 3),
               "ms_max": round(hi, 3), "mcells_per_s": round(NX * NY / med / 1e3, 1),
               "speedup_vs_one_core_ref": round(REF_ONE_CORE_S[name] * 1e3 / med, 0)}
        got = out.cpu().numpy()
        if ref is not None:
            _, rflag, theirs = ref.run_rows(model, host, alt=alt, fdefined=ic.SOME_DEFINED, **s)
            placed, frac, excess, ndef = ic.contract(got, theirs)
            rec.update({"undef_placement_equal": placed, "bit_identical_fraction": round(frac, 6), "defined_cells": ndef,
                        "worst_excess_over_bound": excess})
        # trip counts on every 16th row (the host build of mifc_icing_cell.h counts them)
        sample = [f[::16] for f in host]
        _, _, _, (dh, lh) = cell.run(model, sample, alt=alt, trips=True, **s)
        rec["sampled_cells"] = int(sample[0].size)
        rec["shallow_water_trips"] = histogram(dh, [1, 2, 3, 4, 5, 6, 8, 11, 16, 21, 51, 101, 1001, 10001, 10002])
        rec["per_level_trips"] = histogram(lh, [0, 1, 2, 3, 4, 5, 6, 8, 11, 16, 17, 18, 21, 51, 101, 1001, 1002])
        print(json.dumps(rec), flush=True)

    # 51 members, depth shared by all
    batch = ic.make_inputs(NX, NY, seed=51, nlev=NLEV)
    batch[10] = batch[10][0].copy()
    bdev = [torch.from_numpy(f).cuda() for f in batch]
    del batch
    bout = torch.empty((NLEV, NY, NX), dtype=torch.float32, device="cuda")
    for name, alt in (("modstall", 1), ("mincog", 1)):
        call = lambda: ctx.vesselIcing_levels(name, bdev, alt=alt, undef=ic.UNDEF, out=bout, **s)  # noqa: E731
        med, lo, hi = timed(call, rounds=3)
        print(json.dumps({"model": name, "alt": alt, "batch": NLEV, "grid": [NX, NY], "shared": ["depth"], "ms_median": round(med, 2),
                          "ms_min": round(lo, 2), "ms_max": round(hi, 2), "mcells_per_s": round(NLEV * NX * NY / med / 1e3, 1),
                          "speedup_vs_one_core_ref": round(NLEV * REF_ONE_CORE_S[name] * 1e3 / med, 0)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
