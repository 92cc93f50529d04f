#!/usr/bin/env python3
"""Level batches to per-cell target surfaces: mifc_vregrid_hlevels on 4 device-resident fields of 1440x720x137, LOG and
OUTSIDE_CLAMP, (a) to the 137 hybrid levels of a second surface pressure (model levels to model levels) and (b) to 3 of
those planes -- next to what a caller had before, mifc_vinterp_hlevels with 3 constant targets on the same batch, in the
same process on the same arrays, the calls alternating.

Per case: the kernel time (HIP events around the launches of the call, measurement build; absent where a call has more
launches than a timing section holds) and the call time on the host clock over ROUNDS calls after a warm-up call, median,
minimum and spread; the algorithmic bytes (every input level, ps, every target plane read once, every output written
once), the modelled bytes of the traffic model of DESIGN.md 4.27 (a pass reads NF nlev + 1 planes and its tb target
planes and writes NF tb planes; ceil(ntargets / tb) passes) and the rates both give.  The yardstick of (b) is the vinterp
time scaled by the ratio of the modelled bytes (vregrid also reads the target planes).  Then the same two cases for every
pass size MIFC_VREGRID_TB allows, in the vector form and in the scalar form (MIFC_VREGRID_V): the table TB and V are
chosen from.

    python tools/bench_vregrid.py [--small] [--out PATH]   -> one JSON line per case, also written to PATH
                                                               (default profiles/vregrid.txt)
"""
import json
import os
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import vregrid

NF = 4
ROUNDS = 9
PLANES_B = (40, 90, 130)  # the target levels of case (b)
SWEEP = {4: (8, 15), 1: (8, 16, 20, 24, 28, 32)}  # cells per lane -> pass sizes
MAX_TIMED = 16  # launches a timing section holds (mifc_ctx.h)


def planes(nlev, nf, nt, tb):
    """(algorithmic, modelled) planes of a hybrid call."""
    passes = -(-nt // tb)
    return nf * nlev + 1 + nt + nf * nt, passes * (nf * nlev + 1) + nt + nf * nt


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(bk.ROOT, "profiles", "vregrid.txt")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2024)
    alevel, blevel, _, ps, _ = bk.hybrid_atmosphere(nx, ny, nlev, dev, gen)
    # the second model: its own orography (ps +- 40 hPa, smooth), the same number of levels on another eta distribution
    yy, xx = torch.meshgrid(torch.linspace(0, 9.42, ny, device=dev), torch.linspace(0, 18.84, nx, device=dev), indexing="ij")
    ps_dst = (ps + 40 * torch.cos(xx) * torch.sin(yy)).contiguous()
    a_dst, b_dst, _ = bk.hybrid_levels(np.linspace(0.012, 1, nlev) ** 2.7)
    tcoord = bk.coordinate_batch(a_dst, b_dst, ps_dst, dev)
    few = tcoord[list(PLANES_B)].contiguous() if nlev > max(PLANES_B) else tcoord[:3].contiguous()
    few_const = [float(few[t].mean()) for t in range(3)]
    cells = nx * ny
    aligned = torch.randn((NF, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 3 + 250
    out_all = torch.empty((NF, nlev, ny, nx), device=dev, dtype=torch.float32)
    out_few = torch.empty((NF, 3, ny, nx), device=dev, dtype=torch.float32)
    lines = []

    def emit(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)

    with fc.Context(0) as ctx:
        ctx.use_torch_stream()

        def measure(fields, tag):
            calls = {
                "vregrid (a) %d -> %d" % (nlev, nlev): lambda: vregrid.vregrid_hlevels(ctx, fields, ps, alevel, blevel, tcoord, "log", "first", "clamp", out=out_all),
                "vregrid (b) %d -> 3" % nlev: lambda: vregrid.vregrid_hlevels(ctx, fields, ps, alevel, blevel, few, "log", "first", "clamp", out=out_few),
                "vinterp 3 constant targets": lambda: ctx.vinterp_hlevels(fields, ps, alevel, blevel, few_const, method="log", out=out_few),
            }
            forms = {}
            for name, call in calls.items():  # the form of each call (vinterp: its own, four cells per lane on these arrays, one pass)
                call()
                forms[name] = vregrid.last_vregrid_form(ctx) if name.startswith("vregrid") else {"v": 4, "tb": 32, "passes": 1}
            timed = max(f["passes"] for f in forms.values()) <= MAX_TIMED
            how = {name: (call, bk.WALL_KERNEL if (timed or "(a)" not in name) else bk.WALL) for name, call in calls.items()}
            wall, kernel = bk.alternate(ctx, how, ROUNDS)
            rows = {}
            for name in calls:
                nt, form = (nlev if "(a)" in name else 3), forms[name]
                alg, model = planes(nlev, NF, nt, form["tb"])
                if not name.startswith("vregrid"):
                    alg, model = alg - nt, model - nt  # constant targets: no planes to read
                r = {"call": name, "case": tag, "nx": nx, "ny": ny, "nlev": nlev, "nfields": NF, "ntargets": nt, "v": form["v"], "tb": form["tb"],
                     "passes": form["passes"]}
                if kernel[name]:
                    r.update(bk.stats(kernel[name]))
                r.update(bk.stats(wall[name], "wall_ms"))
                r["algorithmic_bytes"], r["modelled_bytes"] = alg * 4 * cells, model * 4 * cells
                key = "kernel_ms" if kernel[name] else "wall_ms"
                r["GBps_algorithmic"], _ = bk.rate(r["algorithmic_bytes"], r[key])
                r["GBps_modelled"], r["share_of_8TBps_modelled"] = bk.rate(r["modelled_bytes"], r[key])
                rows[name] = r
                emit(r)
            b, vi_ = rows["vregrid (b) %d -> 3" % nlev], rows["vinterp 3 constant targets"]
            yard = vi_["kernel_ms"] * b["modelled_bytes"] / vi_["modelled_bytes"]
            emit({"case": tag, "v": b["v"], "tb": b["tb"], "yardstick_b_ms": round(yard, 4), "vregrid_b_kernel_ms": b["kernel_ms"],
                  "ratio_to_yardstick": round(b["kernel_ms"] / yard, 3), "defined_share_a": round(float((out_all != float(fc.UNDEF)).float().mean()), 3)})

        saved = {k: os.environ.get(k) for k in ("MIFC_VREGRID_TB", "MIFC_VREGRID_V")}
        measure(aligned, "default")
        try:
            for v, sizes in SWEEP.items():
                os.environ["MIFC_VREGRID_V"] = str(v)
                for tb in sizes:
                    os.environ["MIFC_VREGRID_TB"] = str(tb)
                    ctx.reload_env()
                    measure(aligned, "sweep")
        finally:
            for k, value in saved.items():
                if value is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = value
            ctx.reload_env()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
