#!/usr/bin/env python3
"""Neighbourhood statistics table: neighbourProbFunctions / neighbourFunctions on a device-resident 1440x720xNLEV
batch through mifc_neighbour_levels -- GPU time of the synchronous call and the summed kernel time (HIP events around
the launches, measurement build), algorithmic bytes (8 B per cell: the field read once, the result written once),
fraction of the 8 TB/s roofline -- next to the compiled reference on one core for one level (oracle/_ref through
tests/neighbour_ref_shim.cc), scaled to the batch.

    python tools/bench_neighbour.py [NLEV] [--no-cpu]   -> one JSON line per (function, compute, r, step)
"""
import json
import sys
import tempfile
import time

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc

bk.tests_on_path()
import neighbour_cases as nc  # noqa: E402  (CPU baseline and the seeded field only)

NX, NY = 1440, 720
ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
NLEV = int(ARGS[0]) if ARGS else 51
NO_CPU = "--no-cpu" in sys.argv
ROUNDS = 7

# (which, compute, constants, r, step)
CASES = [
    ("prob", 5, [1, 1], 1, 1), ("prob", 5, [1, 3], 3, 1), ("prob", 5, [1, 10], 10, 1), ("prob", 6, [1, 40], 40, 1),
    ("functions", 5, [1, 3, 1], 3, 1), ("functions", 5, [1, 3, 3], 3, 3),
    ("functions", 1, [1, 1], 1, 1), ("functions", 1, [3, 1], 3, 1), ("functions", 2, [3, 1], 3, 1), ("functions", 3, [3, 3], 3, 3),
    ("functions", 1, [10, 1], 10, 1), ("functions", 1, [10, 3], 10, 3),
    ("functions", 4, [50, 1, 1], 1, 1), ("functions", 4, [90, 3, 1], 3, 1), ("functions", 4, [50, 3, 3], 3, 3), ("functions", 4, [50, 10, 3], 10, 3),
]


def main():
    dev = torch.device("cuda", 0)
    field = torch.from_numpy(nc.make_field(NX, NY, 2024, nlev=NLEV)).to(dev)
    out = torch.empty_like(field)
    shim = None
    if not NO_CPU and nc.ref_available():
        shim = nc.RefShim(tempfile.mkdtemp(prefix="nbbench"))
    level0 = field[0].cpu().numpy()
    cells = NX * NY * NLEV
    with fc.Context(0) as ctx:
        for which, compute, consts, r, step in CASES:
            call = lambda: ctx.neighbour_levels(which, compute, field, consts, out=out)  # noqa: E731
            assert call() is not None, ctx.last_error()
            ts, ks = bk.alternate(ctx, {"call": (call, bk.WALL_KERNEL)}, ROUNDS)
            ms, kms = bk.stats(ts["call"], "ms")["ms"], bk.stats(ks["call"])["kernel_ms"]
            alg = 8 * cells
            rec = {"function": "neighbourProbFunctions" if which == "prob" else "neighbourFunctions", "compute": compute, "r": r, "step": step,
                   "nx": NX, "ny": NY, "nlev": NLEV, "ms": ms, "kernel_ms": kms, "algorithmic_bytes": alg,
                   "frac_of_8TBps": bk.rate(alg, ms)[1], "kernel_frac_of_8TBps": bk.rate(alg, kms)[1]}
            if shim is not None:
                res = np.empty((NY, NX), np.float32)
                t0 = time.perf_counter()
                ok, _ = shim.run(which, NX, NY, level0, consts, compute, res, fc.ALL_DEFINED)
                one = (time.perf_counter() - t0) * 1e3
                assert ok
                same = np.array_equal(np.nan_to_num(res), np.nan_to_num(out[0].cpu().numpy())) if compute != 4 else None
                rec.update({"ref_ms_per_level_1core": round(one, 2), "ref_ms_batch_1core": round(one * NLEV, 1),
                            "speedup_vs_ref_1core": round(one * NLEV / ms, 1), "level0_equal_ref": same})
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
