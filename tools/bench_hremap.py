#!/usr/bin/env python3
"""Level batches regridded by a weight table: mifc_hremap_levels on device-resident fields (every level ALL_DEFINED, and once
more with every value tested), next to two yardsticks in the same process on the same data: torch.sparse.mm of the same
table as a CSR tensor with the batch laid out (nsrc, nlev) -- if this torch build runs it on the device --, and
hinterp_levels bilinear to the centres of the same destination grid, which is what a caller can do today and is not
conservative.  The yardsticks are a comparison of speed, never of results.  Cases:
  a  one 1440x720x137 field to 720x360 by conservative 2x2;
  b  the same to 480x240 (3x3) and to 1000x500 (non-aligned, 4 to 9 entries per row);
  c  200 destinations x 137 levels x 8 fields, rows of 50 to 400 entries: the small-ndst case the level chunks exist for.
Per call: the device-synchronised call time (host clock around the call and a synchronisation) of each of ROUNDS calls
after a warm-up call, the calls alternating, its median, minimum and spread; for the mifc calls the kernel time too (HIP
events around the launches of the call, measurement build); and for hremap the algorithmic bytes -- every touched source
value once, the output, and the tables (8 bytes per padded entry, len and Wall per destination, offset and width per
slice) once per level chunk and launch -- with the rate they give over the kernel time.

    python tools/bench_hremap.py [--small]      -> one JSON line per call, then one comparison line per hremap call
    python tools/bench_hremap.py --profile      -> the hremap calls alone, three times each (for a kernel trace)
    python tools/bench_hremap.py --only=ac      -> the cases whose letter is named (MIFC_HREMAP_LEVEL_CHUNK=n for an A/B of the level chunks)
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import hremap

ROUNDS = 9
MIFC, FOREIGN = bk.WALL_KERNEL, bk.WALL  # how a library call and a torch call are timed


def table_bytes(rowptr):
    """The bytes of the plan's device tables: the padded entries, len and Wall per padded destination, offset and width per slice."""
    n = np.diff(rowptr)
    nslices = -(-n.size // 64)
    padded = np.zeros(nslices * 64, np.int64)
    padded[:n.size] = n
    widths = padded.reshape(nslices, 64).max(axis=1)
    return int(8 * 64 * widths.sum() + 12 * 64 * nslices + 12 * nslices)


def random_rows(ndst, nsrc, lo, hi, seed):
    """ndst rows of lo..hi entries over nsrc cells: regions of scattered cells, weights that sum to 1."""
    rng = np.random.default_rng(seed)
    n = rng.integers(lo, hi + 1, ndst)
    rowptr = np.zeros(ndst + 1, np.int64)
    np.cumsum(n, out=rowptr[1:])
    col = np.concatenate([np.sort(rng.choice(nsrc, k, replace=False)) for k in n])
    w = np.concatenate([np.full(k, 1.0 / k) for k in n])
    return rowptr.astype(np.int32), col.astype(np.int32), w.astype(np.float32)


def run_case(ctx, case, fields, table, dst_shape, lines, profile):
    nf, nlev, ny, nx = fields.shape
    rowptr, col, w = table
    ndst = rowptr.size - 1
    dev = fields.device
    every = np.zeros((nf, nlev), np.int32)  # ALL_DEFINED
    out = torch.empty((nf, nlev, ndst), device=dev, dtype=torch.float32)
    with hremap.Plan(ctx, rowptr, col, w, nsrc=ny * nx) as plan:
        calls = {"hremap strict, ALL_DEFINED": (lambda: hremap.hremap_levels(ctx, plan, fields, "strict", fdefined_in=every, out=out), MIFC),
                 "hremap strict, tested": (lambda: hremap.hremap_levels(ctx, plan, fields, "strict", out=out), MIFC),
                 "hremap renorm, tested": (lambda: hremap.hremap_levels(ctx, plan, fields, "renorm", 0.5, out=out), MIFC)}
        if profile:
            for call, _ in calls.values():
                for _ in range(3):
                    call()
            torch.cuda.synchronize()
            return
        notes = {}
        if dst_shape is not None:  # what a caller can do today: sample the centres of the destination cells
            gy, gx = dst_shape
            xs = ((torch.arange(gx, device=dev, dtype=torch.float32) + 0.5) * (nx / gx) - 0.5).clamp(0, nx - 1)
            ys = ((torch.arange(gy, device=dev, dtype=torch.float32) + 0.5) * (ny / gy) - 0.5).clamp(0, ny - 1)
            yy, xx = torch.meshgrid(ys, xs, indexing="ij")
            xx, yy = xx.contiguous(), yy.contiguous()
            hout = torch.empty((nf, nlev, gy, gx), device=dev, dtype=torch.float32)
            calls["hinterp bilinear, ALL_DEFINED"] = (lambda: ctx.hinterp_levels(fields, xx, yy, "bilinear", fdefined_in=every, out=hout), MIFC)
        try:  # the same table as a CSR tensor, the batch laid out (nsrc, nf * nlev) beforehand
            csr = torch.sparse_csr_tensor(torch.from_numpy(rowptr.astype(np.int64)).to(dev), torch.from_numpy(col.astype(np.int64)).to(dev),
                                          torch.from_numpy(w).to(dev), size=(ndst, ny * nx))
            dense = fields.reshape(nf * nlev, ny * nx).t().contiguous()
            torch.sparse.mm(csr, dense)
            torch.cuda.synchronize()
            calls["torch.sparse.mm"] = (lambda: torch.sparse.mm(csr, dense), FOREIGN)
        except Exception as e:  # noqa: BLE001
            notes["torch.sparse.mm"] = "not run on the device by this torch build: %s" % (str(e).splitlines()[0][:160],)
        call_ms, kernel_ms = bk.alternate(ctx, calls, ROUNDS)
        hremap.hremap_levels(ctx, plan, fields, "strict", fdefined_in=every, out=out)
        launch = hremap.last_hremap_form(ctx)
        hremap.hremap_levels(ctx, plan, fields, "strict", out=out)
        launch_tested = hremap.last_hremap_form(ctx)
        hremap.hremap_levels(ctx, plan, fields, "renorm", 0.5, out=out)
        launch_renorm = hremap.last_hremap_form(ctx)
    tables = table_bytes(rowptr)
    touched = int(np.unique(col).size)
    results = {}
    for name in calls:
        r = {"case": case, "call": name, "nx": nx, "ny": ny, "nlev": nlev, "nfields": nf, "ndst": ndst, "nnz": int(rowptr[-1]), **bk.stats(call_ms[name], "call_ms")}
        if kernel_ms[name]:
            r.update(bk.stats(kernel_ms[name], "kernel_ms"))
        if name.startswith("hremap"):
            form = launch if "ALL_DEFINED" in name else (launch_renorm if "renorm" in name else launch_tested)
            r["algorithmic_bytes"] = 4 * nf * nlev * (touched + ndst) + tables * form["level_chunks"] * form["launches"]
            r["table_bytes_once"] = tables
            r["GBps_over_kernel_time"] = bk.rate(r["algorithmic_bytes"], r["kernel_ms"])[0]
            r["launch"] = form
        results[name] = r
        print(json.dumps(r), flush=True)
    for name, note in notes.items():
        print(json.dumps({"case": case, "call": name, "note": note}), flush=True)
    for name, r in results.items():
        if name.startswith("hremap"):
            line = {"case": case, "call": name, "call_ms": r["call_ms"], "kernel_ms": r["kernel_ms"]}
            for yard in ("hinterp bilinear, ALL_DEFINED", "torch.sparse.mm"):
                if yard in results:
                    line[yard + " call_ms"] = results[yard]["call_ms"]
                    line[yard + " over hremap"] = round(results[yard]["call_ms"] / r["call_ms"], 3)
            lines.append(line)


def main():
    small, profile = "--small" in sys.argv, "--profile" in sys.argv
    only = "".join(a.split("=", 1)[1] for a in sys.argv if a.startswith("--only=")) or "abc"
    nx, ny, nlev = bk.shape(sys.argv)
    nf_c = 4 if small else 8
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2025)
    xe, ye = np.arange(nx + 1, dtype=np.float64), np.arange(ny + 1, dtype=np.float64)
    grids = {"a 2x2": (ny // 2, nx // 2), "b 3x3": (ny // 3, nx // 3), "b non-aligned": ((ny * 25) // 36, (nx * 25) // 36)}
    lines = []
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        fields = torch.randn((nf_c, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 10 + 280
        for case, (gy, gx) in grids.items():
            if case[0] not in only:
                continue
            table = hremap.conservative_weights_regular(xe, ye, np.linspace(0, nx, gx + 1), np.linspace(0, ny, gy + 1))
            run_case(ctx, case, fields[:1], table, (gy, gx), lines, profile)
        if "c" in only:
            run_case(ctx, "c 200 regions", fields, random_rows(200, nx * ny, 50, 400, 7), None, lines, profile)
    for line in lines:
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
