#!/usr/bin/env python3
"""Which kernel every wind-family launch takes (relvort, divergence, the fused pair, absvort, the Jacobian, the pair with
the wind speed), over a fixed list of cases: one launch per case on device-resident arrays.

    run      walks the list on the GPU and writes, per case, the request and mifc_last_stencil_form().  Run it under
             `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/record_wind_plans.py run --out cases.json`
    records  joins cases.json with the trace's vortdiv_* dispatches (in order): kernel name, template arguments, grid,
             workgroup size and LDS bytes per case.  Two libraries dispatch the same iff their records files are equal;
             the records of the parent library are tests/golden/wind_plans.json (tests/test_vortdiv_plan_cpu.py).
    compare  two records files, case by case.
    coverage the instantiations of a code object (the .amdhsa_kernel lines of its assembly listing, `hipcc --cuda-device-only -S`)
             that the records never dispatch.

MIFC_LIB_PATH selects the library (see mi-fieldcalc_amd/_capi.py)."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ("vortdiv", "relvort", "divergence", "absvort", "jacobian", "vortdiv_ff")
# tests/test_gpu_parity.py::test_vortdiv_levels_matches_per_level_reference_calls
LEVEL_SHAPES = [(64, 48, 9), (516, 70, 6), (260, 11, 5), (17, 9, 7), (1440, 75, 5)]
# tests/test_gpu_parity.py::test_wind_operators_on_ragged_widths
RAGGED_SHAPES = [(949, 23, 4), (1001, 13, 3), (258, 9, 2), (6, 300, 2), (4, 3, 1), (5, 4, 3), (1443, 7, 2)]
# nx % 256 == 1, a deep ragged batch, the headline field at four depths, one big level
OTHER_SHAPES = [(257, 40, 8), (1443, 720, 16), (1440, 720, 1), (1440, 720, 2), (1440, 720, 8), (1440, 720, 137), (4000, 4000, 1)]
# every MIFC_VORTDIV_TUNE string under tests/
TUNES = ["R=7,D=0", "R=5,D=1,NT=1", "R=64,D=1,WPB=8", "K=1", "K=1,XCD=0,NT=0", "K=2", "K=2,XCD=0", "R=1", "R=2,WPB=2", "R=2,WPB=1", "R=8", "K=2,LG=8",
         "K=2,LG=4,XCD=0", "K=1,LG=3", "K=2,RB=14", "K=2,RB=14,LG=16", "K=3", "K=3,RB=8,LG=2", "K=3,RB=16,LG=4,XCD=0", "K=3,RB=12,LG=1",
         "K=3,RB=16,LG=3,D=0", "K=3,RB=8,D=0,LG=4", "K=3,RB=16,LG=2,D=0,ZZ=1", "K=3,RB=12,D=1,ZZ=1", "K=3,RB=8,LG=5,D=0,ZZ=1,XCD=0", "K=4", "K=4,D=0,LG=1",
         "K=4,D=1,LG=3", "K=4,D=2,LG=2,XCD=0", "K=4,RB=6,D=2,LG=4", "K=4,RB=8,D=1,LG=5", "K=4,RB=12,D=1,LG=2", "K=4,RB=6,D=0", "K=4,D=1", "K=4,RB=6,D=2"]
# shapes that only a tuning string reaches (tools/ use them): they complete the coverage of the code object
EXTRA_TUNES = ["V=1", "V=3", "V=3,D=0", "NT=0", "NT=0,V=1", "NT=0,V=3", "D=0,V=1", "K=3,RB=12,D=0", "K=3,RB=12,D=1", "K=3,RB=16,D=1", "K=3,RB=8,D=1",
               "K=3,RB=8,D=1,ZZ=1", "K=3,RB=16,D=1,ZZ=1", "K=4,RB=6,D=1", "K=4,RB=8,D=0", "K=4,RB=8,D=2", "K=4,RB=12,D=0", "K=4,RB=12,D=2", "K=4,RB=12,WPB=4,D=1",
               "K=4,RB=12,WPB=4,D=0", "K=4,RB=14,D=1", "K=4,RB=14,D=0", "K=4,RB=10,WPB=2,D=1", "K=4,RB=10,WPB=2,D=0", "K=4,RB=10,D=2", "K=4,RB=10,D=0",
               "K=4,RB=12,D=0,WPB=2,LG=6", "K=3,RB=16,ZZ=0", "K=3,RB=16,ZZ=0,D=0", "K=3,RB=12,ZZ=0", "K=3,RB=12,ZZ=0,D=0", "K=3,RB=8,ZZ=0", "K=3,RB=8,ZZ=0,D=0"]
# ... of which the single outputs have instantiations of their own
SINGLE_OUTPUT_TUNES = ["R=8", "V=1", "V=3", "NT=0", "NT=0,V=1", "NT=0,V=3", "K=1,XCD=0,NT=0", "K=2", "K=3", "K=4,RB=12,D=0", "K=4,RB=12,D=1"]
SWITCHES = ["MIFC_VORTDIV_SPLIT=0", "MIFC_VORTDIV_LEVELWALK=0", "MIFC_RAGGED_SPLIT=0", "MIFC_LEVELWALK_MIN_UNITS=1", "MIFC_FORCE_CELL_KERNEL=1"]
ENV_KEYS = ["MIFC_VORTDIV_TUNE"] + [s.split("=")[0] for s in SWITCHES]


def case(op, shape, flags, nan=False, tune="", switch="", slab=None):
    nx, ny, nlev = shape
    c = {"op": op, "nx": nx, "ny_global": ny, "j0": 0, "ny_local": ny, "nlev": nlev, "row_begin": 0, "row_end": 0, "flags": flags, "nan_undef": int(nan),
         "tune": tune, "switch": switch}
    if slab:
        c.update(j0=slab[0], ny_local=slab[1], row_begin=slab[2], row_end=slab[3])
    return c


def case_list():
    out = []
    # the tests' shapes: every operator, flags alternating; the other shapes: every operator with both
    for i, shape in enumerate(LEVEL_SHAPES + RAGGED_SHAPES):
        for j, op in enumerate(OPS):
            out.append(case(op, shape, "mixed" if (i + j) % 2 == 0 else "all"))
    for shape in OTHER_SHAPES:
        for op in OPS:
            for flags in ("all", "mixed"):
                out.append(case(op, shape, flags))
    for shape in [(516, 70, 6), (1440, 720, 1), (1440, 720, 137), (4000, 4000, 1)]:
        for op in OPS:
            out.append(case(op, shape, "mixed", nan=True))
    # tunings: the fused pair tested, one single output in turn, and the fused pair untested
    for i, tune in enumerate(TUNES + EXTRA_TUNES):
        out.append(case("vortdiv", (516, 70, 6), "mixed", tune=tune))
        out.append(case(OPS[1 + i % 4], (516, 70, 6), "all", tune=tune))
        out.append(case("vortdiv", (1440, 75, 5), "all", tune=tune))
    for tune in SINGLE_OUTPUT_TUNES:
        for op in OPS[1:5]:
            for flags in ("all", "mixed"):
                out.append(case(op, (516, 70, 6), flags, tune=tune))
    for tune in ("K=4", "K=3", "R=8"):  # forced tunings against a NaN undef, a ragged width, the third output
        for op in ("vortdiv", "absvort", "jacobian"):
            out.append(case(op, (516, 70, 6), "mixed", nan=True, tune=tune))
        out.append(case("vortdiv", (949, 23, 4), "mixed", tune=tune))
        out.append(case("vortdiv_ff", (516, 70, 6), "mixed", tune=tune))
    for sw in SWITCHES:
        for shape in [(516, 70, 6), (1443, 720, 16), (1440, 720, 137)]:
            for op in ("vortdiv", "divergence", "absvort", "vortdiv_ff"):
                out.append(case(op, shape, "mixed" if shape[2] != 137 else "all", switch=sw))
    # row slabs of one level: (j0, ny_local, row_begin, row_end) of a (nx, ny_global) field
    for nx, nyg in [(1440, 720), (4000, 4000)]:
        q = nyg // 4
        for i, slab in enumerate([(0, q, 0, 0), (q, q, 0, 0), (nyg - q, q, 0, 0), (q, q, 1, q - 1), (q, q, 0, 1), (0, q, 2, q - 1), (nyg - q, q, 0, q - 2)]):
            out.append(case("vortdiv", (nx, nyg, 1), "mixed", slab=slab))
            out.append(case(("relvort", "divergence")[i % 2], (nx, nyg, 1), "all", slab=slab))
    for tune in ("K=2", "R=8", "K=4,D=1", "K=4,RB=6,D=2"):  # tests/test_gpu_parity.py::test_vortdiv_row_slabs_equal_whole_field
        out.append(case("vortdiv", (256, 96, 1), "mixed", tune=tune, slab=(24, 24, 0, 0)))
    return out


def request_of(c):
    """What the launcher is asked, as tests/test_vortdiv_plan_cpu.py hands it to plan_wind (see csrc/mifc_vortdiv_plan.h)."""
    nx, nlev = c["nx"], c["nlev"]
    op = c["op"]
    slab = c["ny_local"] != c["ny_global"] or c["row_end"] > c["row_begin"]
    every_all = c["flags"] == "all"
    rq = {k: c[k] for k in ("nx", "ny_global", "j0", "ny_local", "nlev", "row_begin", "row_end", "nan_undef", "tune", "switch")}
    rq["op"] = "vortdiv" if op == "vortdiv_ff" else op
    rq["rv"] = int(op != "divergence")
    rq["dv"] = int(op in ("vortdiv", "vortdiv_ff", "divergence"))
    rq["ff"] = int(op == "vortdiv_ff")
    rq["fc"] = int(op == "absvort")
    # arrays of their own, 256-byte aligned, levels nx * ny floats apart: only the width makes rows start off 16-byte boundaries
    rq["ragged"] = int(nx % 4 != 0 or (nlev > 1 and (nx * c["ny_global"]) % 4 != 0))
    rq["all_defined"] = int(every_all)
    # the context's buffer for per-workgroup counts (stencil_partials in csrc/mifc_capi_stencil.hip); the slab and the three-output entries pass none
    per_level = (c["ny_local"] // 4 + 2) * (nx // 256 + 1)
    units = per_level * nlev
    has = (not every_all) and not slab and op != "vortdiv_ff" and per_level >= 2048 and units <= (1 << 24)
    rq["partials_cap"] = units * 1024 if has else 0
    return rq


def run(args):
    import numpy as np
    import torch

    import mi_fieldcalc_amd as fc

    dev = torch.device("cuda", 0)
    ctx = fc.Context(0)
    ctx.use_torch_stream()
    cache = {}

    def arrays(shape):
        if cache.get("shape") != shape:
            cache.clear()
            torch.cuda.empty_cache()
            nlev, ny, nx = shape
            cache["shape"] = shape
            cache["in"] = [torch.ones(shape, dtype=torch.float32, device=dev) for _ in range(2)]
            cache["out"] = [torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3)]
            cache["map"] = [torch.ones((ny, nx), dtype=torch.float32, device=dev) for _ in range(3)]
            cache["cnt"] = [torch.zeros(nlev, dtype=torch.int64, device=dev) for _ in range(2)]
        return cache

    done = []
    for c in case_list():
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        if c["tune"]:
            os.environ["MIFC_VORTDIV_TUNE"] = c["tune"]
        if c["switch"]:
            k, v = c["switch"].split("=")
            os.environ[k] = v
        ctx.reload_env()
        nx, nlev = c["nx"], c["nlev"]
        undef = float("nan") if c["nan_undef"] else float(fc.UNDEF)
        flags = np.full(nlev, fc.ALL_DEFINED if c["flags"] == "all" else fc.SOME_DEFINED, np.int32)
        if c["flags"] == "mixed" and nlev > 1:
            flags[::2] = fc.ALL_DEFINED
        slab = c["ny_local"] != c["ny_global"] or c["row_end"] > c["row_begin"]
        op = c["op"]
        if slab:
            a = arrays((1, c["ny_local"] + 2, nx))
            own = slice(0, c["ny_local"])
            rv, dv = a["out"][0][0][own], a["out"][1][0][own]
            ok = ctx.vortdiv_slab_enqueue(nx, c["ny_global"], c["j0"], c["ny_local"], a["in"][0][0], a["in"][1][0], a["map"][0][own], a["map"][1][own],
                                          rv if op != "divergence" else None, dv if op != "relvort" else None, fdefined_in=int(flags[0]), undef=undef,
                                          n_undefined=a["cnt"][0], rows=(c["row_begin"], c["row_end"]) if c["row_end"] > c["row_begin"] else None)
        else:
            a = arrays((nlev, c["ny_global"], nx))
            (u, v), (o0, o1, o2), (xm, ym, fcor), (n0, n1) = a["in"], a["out"], a["map"], a["cnt"]
            if op == "vortdiv_ff":
                ok = ctx.vortdiv_ff_levels_enqueue(u, v, xm, ym, o0, o1, o2, fdefined=flags, undef=undef, n_undefined=n0, n_undefined_ff=n1)
            else:
                ok = ctx.stencil_levels_enqueue(op, u, v, xm, ym, fcor if op == "absvort" else None, o0, o1 if op == "vortdiv" else None, fdefined=flags,
                                                undef=undef, n_undefined=n0)
        if not ok:
            raise RuntimeError("%r: %s" % (c, ctx.last_error()))
        rq = request_of(c)
        rq["form"] = ctx.last_stencil_form()
        done.append(rq)
        print(json.dumps(rq), flush=True)
        torch.cuda.synchronize()
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    ctx.reload_env()
    with open(args.out, "w") as f:
        json.dump(done, f)


def trace_rows(path):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    rows = []
    for fn in files:
        with open(fn, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [r for r in rows if "vortdiv_" in r["Kernel_Name"]]


def parse_kernel(name):
    m = re.search(r"(vortdiv_\w+?)_kernel<(.*?)>\(", name)
    targs = [{"true": 1, "false": 0}.get(t.strip(), t.strip()) for t in m.group(2).split(",")]
    return m.group(1), [int(t) for t in targs]


FIELDS = ("op", "nx", "ny_global", "j0", "ny_local", "nlev", "row_begin", "row_end", "rv", "dv", "ff", "fc", "ragged", "all_defined", "nan_undef", "partials_cap",
          "tune", "switch", "form", "kernel", "targs", "grid", "block", "lds")


def save_records(path, recs):
    """One row per record, the field names once (a record without a wind kernel has null in the last five)."""
    with open(path, "w") as f:
        f.write('{"fields":' + json.dumps(FIELDS, separators=(",", ":")) + ',\n"records":[\n')
        f.write(",\n".join(json.dumps([c.get(k) for k in FIELDS], separators=(",", ":")) for c in recs) + "\n]}\n")


def load_records(path):
    with open(path) as f:
        d = json.load(f)
    return [{k: v for k, v in zip(d["fields"], row) if v is not None} for row in d["records"]]


def records(args):
    with open(args.cases) as f:
        cases = json.load(f)
    rows = trace_rows(args.trace)
    it = iter(rows)
    out = []
    for c in cases:
        c = dict(c)
        if c["ff"] and c["form"] != "wind_split_ff":
            # declined; the entry then launches the pair without the third output: that request is the record that follows
            out.append(dict(c, form=""))
            c["ff"] = 0
        if c["form"].startswith("wind_"):
            r = next(it)
            c["kernel"], c["targs"] = parse_kernel(r["Kernel_Name"])
            c["block"] = int(r["Workgroup_Size_X"])
            c["grid"] = int(r["Grid_Size_X"]) // c["block"]
            c["lds"] = int(r["LDS_Block_Size"])
            if int(r["Workgroup_Size_Y"]) != 1 or int(r["Grid_Size_Y"]) != 1:
                raise SystemExit("a wind kernel with a 2-d grid: %r" % r)
        out.append(c)
    if next(it, None) is not None:
        raise SystemExit("more vortdiv_* dispatches in the trace than cases with a wind form")
    save_records(args.out, out)
    print("%d records, %d dispatches, %d distinct kernels" % (len(out), len(rows), len({(c["kernel"], tuple(c["targs"])) for c in out if "kernel" in c})))


def compare(args):
    a, b = (load_records(p) for p in (args.a, args.b))
    bad = [(x, y) for x, y in zip(a, b) if x != y]
    for x, y in bad[:20]:
        print("-", json.dumps(x))
        print("+", json.dumps(y))
    print("%d / %d records, %d differ" % (len(a), len(b), len(bad)))
    sys.exit(1 if bad or len(a) != len(b) else 0)


def coverage(args):
    """args.symbols: text that names the code object's kernels mangled (an assembly listing's .amdhsa_kernel lines)."""
    mangled = sorted(set(re.findall(r"\.amdhsa_kernel\s+(\S+)", open(args.symbols).read())))
    names = subprocess.run([args.cxxfilt], input="\n".join(mangled), capture_output=True, text=True, check=True).stdout.split("\n")
    have = {(k, tuple(t)) for k, t in (parse_kernel(n) for n in names if "vortdiv_" in n)}
    seen = {(c["kernel"], tuple(c["targs"])) for c in load_records(args.records) if "kernel" in c}
    print("%d instantiations in the code object, %d dispatched" % (len(have), len(seen & have)))
    for k, t in sorted(have - seen):
        print("never dispatched: vortdiv_%s_kernel<%s>" % (k[8:], ", ".join(str(x) for x in t)))
    if seen - have:
        print("dispatched but not in the listing:", sorted(seen - have))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("run")
    p.add_argument("--out", required=True)
    p = sub.add_parser("records")
    p.add_argument("--cases", required=True)
    p.add_argument("--trace", required=True, help="the kernel-trace csv, or the directory it was written under")
    p.add_argument("--out", required=True)
    p = sub.add_parser("compare")
    p.add_argument("a")
    p.add_argument("b")
    p = sub.add_parser("coverage")
    p.add_argument("--symbols", required=True)
    p.add_argument("--records", required=True)
    p.add_argument("--cxxfilt", default="c++filt")
    args = ap.parse_args()
    {"run": run, "records": records, "compare": compare, "coverage": coverage}[args.cmd](args)


if __name__ == "__main__":
    main()
