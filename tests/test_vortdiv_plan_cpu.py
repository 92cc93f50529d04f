"""plan_wind() (csrc/mifc_vortdiv_plan.h) against the dispatches recorded on the GPU, without a GPU.

tests/golden/wind_plans.json holds, per case of tools/record_wind_plans.py, the request and what the library at the parent of
the commit that introduced the planner launched for it: mifc_last_stencil_form(), and from the kernel trace the kernel, its
template arguments, grid, workgroup size and LDS bytes.  The planner, compiled here with the host compiler, has to plan
exactly that launch for every case."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"relvort": 0, "divergence": 1, "vortdiv": 2, "absvort": 3, "jacobian": 4}
FORMS = {None: 0, "vortdiv_rows": 1, "vortdiv_oneshot": 2, "vortdiv_tile": 3, "vortdiv_levelwalk": 4, "vortdiv_split": 5}
OUT = ("form", "grid", "block", "lds", "R", "V", "D", "NT", "WPB", "tiles.tile_rows", "levelwalk.waves", "levelwalk.halo_waves", "levelwalk.prefetch",
       "split.tile_rows", "split.loaders", "split.prefetch", "lgroup", "uB", "uW", "n_logical", "counts_by_partials")
# the kernels' template parameters that the plan names (position in the argument list)
SHAPE = {"vortdiv_rows": {"D": 4, "NT": 5, "V": 6}, "vortdiv_oneshot": {"NT": 3}, "vortdiv_tile": {"tiles.tile_rows": 4},
         "vortdiv_levelwalk": {"levelwalk.waves": 4, "levelwalk.prefetch": 5, "levelwalk.halo_waves": 6},
         "vortdiv_split": {"split.tile_rows": 2, "split.loaders": 3, "split.prefetch": 4}}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    so = str(tmp_path_factory.mktemp("plan") / "libplan_shim.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mi-fieldcalc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "vortdiv_plan_shim.cc"), "-o", so], check=True)
    fn = ctypes.CDLL(so).mifc_test_plan_wind
    fn.restype = None

    def call(c):
        rq = (ctypes.c_int * 15)(OPS[c["op"]], c["nx"], c["ny_global"], c["j0"], c["ny_local"], c["nlev"], c["row_begin"], c["row_end"], c["rv"], c["dv"],
                                 c["ff"], c["fc"], c["ragged"], c["all_defined"], c["nan_undef"])
        sw = {"MIFC_VORTDIV_SPLIT": 1, "MIFC_VORTDIV_LEVELWALK": 1, "MIFC_RAGGED_SPLIT": 1, "MIFC_LEVELWALK_MIN_UNITS": 0, "MIFC_FORCE_CELL_KERNEL": 0}
        if c["switch"]:
            k, v = c["switch"].split("=")
            sw[k] = int(v)
        out = (ctypes.c_long * len(OUT))()
        note = ctypes.create_string_buffer(64)
        fn(rq, c["tune"].encode(), (ctypes.c_int * 5)(*sw.values()), ctypes.c_long(c["partials_cap"]), out, note, 64)
        return dict(zip(OUT, out)), note.value.decode()

    return call


def _cases():
    with open(os.path.join(ROOT, "tests", "golden", "wind_plans.json")) as f:
        d = json.load(f)
    return [{k: v for k, v in zip(d["fields"], row) if v is not None} for row in d["records"]]


def test_golden_file_covers_the_forms():
    cases = _cases()
    assert len(cases) >= 300
    assert {c.get("kernel") for c in cases} == set(FORMS)


def test_plan_wind_plans_the_recorded_launches(plan):
    bad = []
    for c in _cases():
        got, note = plan(c)
        kernel = c.get("kernel")
        want = {"form": FORMS[kernel]}
        if kernel:
            # the recorded launch: grid and workgroup size as traced.  The trace's LDS bytes are the kernel's static ones; only
            # the row-walking kernel (no static LDS) asks for dynamic LDS: R rows of 256 * V map-factor float4 columns, two
            # arrays (three with the Coriolis parameter), plus whole KiB of the LDSX experiment
            want.update(grid=c["grid"], block=c["block"])
            if kernel == "vortdiv_rows":
                assert c["lds"] == 0
                per_row = 1024 * c["targs"][6] * (3 if c["targs"][3] else 2)
                tile = got["R"] * per_row
                assert 1 <= got["R"] <= 32 // c["targs"][6] and got["lds"] >= tile and (got["lds"] - tile) % 1024 == 0, (c, got)
                if "LDSX" not in c["tune"]:
                    want["lds"] = tile
            else:
                want["lds"] = 0
            want.update({name: c["targs"][i] for name, i in SHAPE[kernel].items()})
            if kernel == "vortdiv_rows":
                want["WPB"] = c["block"] // 64
            if kernel == "vortdiv_split":
                assert c["block"] == 64 * (c["targs"][2] + c["targs"][3])
        mism = {k: (got[k], v) for k, v in want.items() if got[k] != v}
        if kernel and note != c["form"]:
            mism["note"] = (note, c["form"])
        if mism:
            bad.append((c, mism))
    assert not bad, "%d of the recorded launches are planned differently (planned, recorded); the first: %r" % (len(bad), bad[:3])
