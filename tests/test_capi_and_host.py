"""CPU-side checks of the boundary and the host logic (no GPU, no compute calls):
the C-ABI library loads and exports every symbol include/mifc.h declares, the
source-compatible C++ header compiles and links, the operators fail loudly
without a device, and the sharding helpers partition correctly."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc.so")
CXXLIB = os.path.join(ROOT, "mi-fieldcalc_amd", "libmi-fieldcalc.so")


@pytest.fixture(scope="module")
def built():
    if not (os.path.exists(LIB) and os.path.exists(CXXLIB)):
        import __graft_entry__ as g

        g.build()
    return LIB


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "mifc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mifc_[A-Za-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(built):
    declared = _declared_symbols()
    assert len(declared) >= 30
    lib = ctypes.CDLL(built)
    missing = [s for s in declared if not hasattr(lib, s)]
    assert not missing, missing
    import mi_fieldcalc_amd._capi as capi

    assert sorted(capi.SIGNATURES) == declared  # the ctypes table mirrors the header one to one
    assert capi.lib().mifc_abi_version() == 1


def test_classify_is_checkdefined(built):
    import mi_fieldcalc_amd as fc

    assert fc.classify(0, 10) == fc.ALL_DEFINED
    assert fc.classify(10, 10) == fc.NONE_DEFINED
    assert fc.classify(3, 10) == fc.SOME_DEFINED
    assert fc.classify(0, 0) == fc.ALL_DEFINED  # FieldDefined.cc:64 tests n_undefined == 0 first


def test_no_silent_cpu_fallback(built):
    """On a box without a GPU the product path must refuse to run, not compute on the CPU."""
    import mi_fieldcalc_amd as fc
    import mi_fieldcalc_amd._capi as capi

    if capi.lib().mifc_device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        fc.Context(0)


def test_product_never_touches_the_oracle():
    """The oracle is test infrastructure: nothing under mi-fieldcalc_amd/ may reference it."""
    pkg = os.path.join(ROOT, "mi-fieldcalc_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cc", ".cpp", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "mifc_oracle" not in text and "cpulib" not in text and "libmifc_ref" not in text, os.path.join(dirpath, f)
    out = subprocess.run(["ldd", LIB], capture_output=True, text=True).stdout
    assert "oracle" not in out and "mifc_ref" not in out


CXX_CALLER = r"""
// An existing caller of the reference API, unchanged: includes the installed
// header, uses the namespaces, enum, constants and operator signatures.
#include <mi_fieldcalc/FieldCalculations.h>
#include <mi_fieldcalc/MetConstants.h>
#include <mi_fieldcalc/math_util.h>
#include <mi_fieldcalc/mi_fieldcalc_version.h>
#include <cstdio>
#include <string>
#include <vector>
int main()
{
  using namespace miutil;
  const int nx = 8, ny = 5;
  std::vector<float> u(nx * ny, 3.f), v(nx * ny, 4.f), xm(nx * ny, 1e-5f), ym(nx * ny, 1e-5f), out(nx * ny, -1.f);
  ValuesDefined fDefined = ALL_DEFINED;
  const bool ok1 = fieldcalc::vectorabs(nx, ny, u.data(), v.data(), out.data(), fDefined, UNDEF);
  ValuesDefined f2 = SOME_DEFINED;
  const bool ok2 = fieldcalc::relvort(nx, ny, u.data(), v.data(), xm.data(), ym.data(), out.data(), f2, fieldUndef);
  const bool ok3 = fieldcalc::relvort(2, 2, u.data(), v.data(), xm.data(), ym.data(), out.data(), f2, fieldUndef); // too small -> false
  const bool d = fieldcalc::is_defined(false, 1.f, 2.f, UNDEF) && !fieldcalc::is_defined(false, 1.f, UNDEF, UNDEF) &&
                 fieldcalc::is_defined(true, UNDEF, UNDEF) && fieldcalc::is_defined(1.f, UNDEF);
  std::printf("%d %d %d %d %g %g v%d %d\n", ok1, ok2, ok3, d, (double)absval(3.f, 4.f), (double)constants::t0,
              MI_FIELDCALC_VERSION_CURRENT_INT, (int)checkDefined((size_t)0, (size_t)5));
  // the rest of the catalogue and the ensemble reductions: std::vector signatures included
  ValuesDefined f3 = ALL_DEFINED;
  const bool ok4 = fieldcalc::fieldOPERfield(1, nx, ny, u.data(), v.data(), out.data(), f3, UNDEF);
  const float sum1 = out[7];
  std::vector<float*> members;
  members.push_back(u.data());
  members.push_back(v.data());
  members.push_back(u.data());
  ValuesDefined f4 = SOME_DEFINED;
  const bool ok5 = fieldcalc::sumFields(nx, ny, members, out.data(), f4, UNDEF);
  const float sum2 = out[7];
  std::vector<ValuesDefined> fin(3, ALL_DEFINED);
  ValuesDefined f5 = SOME_DEFINED;
  const bool ok6 = fieldcalc::meanValue(nx, ny, members, fin, out.data(), f5, UNDEF);
  const float mean = out[7];
  std::vector<float> limits;
  limits.push_back(0.f);
  limits.push_back(3.5f);
  limits.push_back(7.f);
  limits.push_back(10.f);
  ValuesDefined f6 = ALL_DEFINED;
  const bool ok7 = fieldcalc::values2classes(nx, ny, v.data(), out.data(), limits, f6, UNDEF);
  const float cls = out[7];
  ValuesDefined f7 = ALL_DEFINED;
  fieldcalc::maxvalueFieldConst(nx, ny, u.data(), 3.5f, out.data(), f7, UNDEF); // a void function of the reference
  std::printf("%d %g %d %g %d %g %d %g %g\n", ok4, (double)sum1, ok5, (double)sum2, ok6, (double)mean, ok7, (double)cls, (double)out[7]);
  // a reference function that is outside the hot-path scope: false, and last_error() says so
  // (an argument-validation failure -- the too-small relvort above -- leaves it empty)
  ValuesDefined f8 = ALL_DEFINED;
  const bool ok8 = fieldcalc::neighbourFunctions(nx, ny, u.data(), limits, 1, out.data(), f8, UNDEF);
  const std::string why = fieldcalc::last_error();
  ValuesDefined f9 = SOME_DEFINED;
  fieldcalc::relvort(2, 2, u.data(), v.data(), xm.data(), ym.data(), out.data(), f9, fieldUndef);
  const std::string why2 = fieldcalc::last_error();
  std::printf("%d|%s|%s\n", ok8, why.c_str(), why2.c_str());
  return 0;
}
"""


def test_cxx_header_is_source_compatible(built, tmp_path):
    src = tmp_path / "caller.cc"
    src.write_text(CXX_CALLER)
    exe = tmp_path / "caller"
    inc = os.path.join(ROOT, "mi-fieldcalc_amd", "include")
    libdir = os.path.join(ROOT, "mi-fieldcalc_amd")
    subprocess.run(
        ["g++", "-std=c++11", "-Wall", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lmi-fieldcalc", "-lmifc",
         "-Wl,-rpath," + libdir],
        check=True,
    )
    res = subprocess.run([str(exe)], capture_output=True, text=True, check=True)
    fields = res.stdout.split()
    import mi_fieldcalc_amd._capi as capi

    have_gpu = capi.lib().mifc_device_count() > 0
    # without a GPU every operator returns false (no CPU fallback); the pure host helpers still work
    assert fields[0] == ("1" if have_gpu else "0") and fields[1] == fields[0]
    assert fields[2] == "0" and fields[3] == "1" and fields[4] == "5" and fields[5].startswith("273.1")
    assert fields[6] == "v1009" and fields[7] == "0"
    more = res.stdout.splitlines()[1].split()
    if have_gpu:  # u = 3, v = 4 everywhere
        assert more == ["1", "7", "1", "10", "1", "3.33333", "1", "1", "3.5"], more
    else:
        assert more[0] == more[2] == more[4] == more[6] == "0"
    ok8, why, why2 = res.stdout.splitlines()[2].split("|")
    assert ok8 == "0"
    if have_gpu:
        assert "neighbourFunctions: not built on the GPU" in why and why2 == ""


REF_PYBIND_SRC = "/root/reference/python/py_mi_fieldcalc.cc"


@pytest.mark.skipif(not os.path.exists(REF_PYBIND_SRC), reason="reference sources not present (GPU box)")
def test_reference_pybind_module_builds_unchanged_against_this_library(built, tmp_path):
    """Source compatibility, proven with the reference's OWN caller: its pybind11 module
    (python/py_mi_fieldcalc.cc, compiled where it lies, nothing copied) builds against this
    repo's headers, links against this repo's library and imports.  The build product is a
    throw-away under tmp_path; the shipped Python surface is mi_fieldcalc.py."""
    try:
        import pybind11
    except ImportError:
        pytest.skip("pybind11 not importable")
    import sysconfig

    inc = os.path.join(ROOT, "mi-fieldcalc_amd", "include")
    libdir = os.path.join(ROOT, "mi-fieldcalc_amd")
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    mod = tmp_path / ("mi_fieldcalc" + ext)
    cmd = ["g++", "-std=c++11", "-O1", "-shared", "-fPIC", "-I", inc, "-I", pybind11.get_include(), "-I", sysconfig.get_paths()["include"],
           REF_PYBIND_SRC, "-o", str(mod), "-L", libdir, "-lmi-fieldcalc", "-lmifc", "-Wl,-rpath," + libdir]
    subprocess.run(cmd, check=True)
    probe = ("import sys; sys.path.insert(0, %r); import mi_fieldcalc as m, numpy as np; "
             "print(sorted(n for n in dir(m) if not n.startswith('_'))); "
             "r = m.abshum(np.array([[293.16]], dtype=np.float32), np.array([[0.8]], dtype=np.float32), -1.0); "
             "print('abshum', None if r is None else float(r[0, 0]))") % str(tmp_path)
    res = subprocess.run([sys.executable, "-c", probe], capture_output=True, text=True, check=True, cwd=str(tmp_path))
    names, result = res.stdout.strip().splitlines()[-2:]
    for fn in ("kIndex", "ductingIndex", "showalterIndex", "boydenIndex", "sweatIndex", "seaSoundSpeed", "cvtemp", "cvhum", "abshum", "windCooling",
               "underCooledRain", "vesselIcingOverland", "vesselIcingMertins", "vesselIcingModStall", "vesselIcingMincog", "ValuesDefined"):
        assert fn in names
    import mi_fieldcalc_amd._capi as capi

    if capi.lib().mifc_device_count() > 0:
        assert abs(float(result.split()[1]) - 13.83) <= 0.02  # python/test_mi_fieldcalc.py:36-41
    else:
        assert result == "abshum None"  # no GPU: the operator returns false, the module None -- no CPU fallback


_ICAO = {
    "alt": "_ZN6miutil9constants31ICAO_geo_altitude_from_pressureEd",
    "prs": "_ZN6miutil9constants31ICAO_pressure_from_geo_altitudeEd",
    "fl": "_ZN6miutil9constants20FL_from_geo_altitudeEd",
    "alt_fl": "_ZN6miutil9constants20geo_altitude_from_FLEd",
}
# ICAO doc 7488, as in the reference's test/MetConstantsTest.cc:39-58 (pressure hPa, altitude m)
_DOC7488 = [(8.7, 31985), (10.0, 31055), (11.1, 30360), (19.4, 26680), (97.3, 16353), (139.5, 14069), (244.1, 10517), (354.2, 8035), (459.7, 6189),
            (590.8, 4324), (739.7, 2576), (840.7, 1547), (936.8, 657), (1010.0, 27), (1020.0, -56), (1050.0, -302), (1130.0, -929)]


def _icao(libpath):
    lib = ctypes.CDLL(libpath)
    fns = {}
    for k, sym in _ICAO.items():
        f = getattr(lib, sym)
        f.argtypes = [ctypes.c_double]
        f.restype = ctypes.c_int if k == "fl" else ctypes.c_double
        fns[k] = f
    return fns


def test_icao_standard_atmosphere_helpers(built):
    """The host-side helpers of MetConstants.h (not operators, no GPU): the reference's own
    known answers (test/MetConstantsTest.cc:61-120) and, where the compiled reference is
    available, agreement with it over the whole range."""
    mine = _icao(CXXLIB)
    for p, h in _DOC7488:
        assert abs(mine["alt"](p) - h) <= 1.55  # :66
        assert abs(mine["prs"](h) - p) <= 0.01 * p  # :101
    for p, fl in ((600, 140), (500, 185), (400, 235), (300, 300), (250, 340), (200, 385), (150, 445)):  # :49-58, :72-80
        assert mine["fl"](mine["alt"](p)) == fl
    ptab = [1000, 925, 850, 800, 700, 500, 400, 300, 250, 200, 150, 100, 70, 50, 30, 10]
    ftab = [5, 25, 50, 65, 100, 185, 235, 300, 340, 385, 445, 530, 605, 675, 780, 1020]
    for p, fl in zip(ptab, ftab):  # :82-90
        assert mine["fl"](mine["alt"](p)) == fl
    assert abs(mine["alt_fl"](100) - 10000 / 3.2808399) < 1e-9
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libmifc_ref.so")
    if os.path.exists(ref_path):
        ref = _icao(ref_path)
        for p in np.geomspace(0.002, 1200.0, 400):
            a, b = mine["alt"](float(p)), ref["alt"](float(p))
            assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), p
        for h in np.linspace(-1500.0, 90000.0, 400):
            a, b = mine["prs"](float(h)), ref["prs"](float(h))
            assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), h
            assert mine["fl"](float(h)) == ref["fl"](float(h))


def test_shard_range_partitions_exactly():
    from mi_fieldcalc_amd.sharding import shard_range, slab_rows

    for n, w in ((137, 8), (6987, 8), (137, 1), (5, 8), (4000, 8), (137, 3)):
        covered = []
        sizes = []
        for r in range(w):
            a, b = shard_range(n, w, r)
            covered.extend(range(a, b))
            sizes.append(b - a)
        assert covered == list(range(n))
        assert max(sizes) - min(sizes) <= 1
    assert slab_rows(4000, 8, 3) == (1500, 500)


def test_synth_is_deterministic():
    import mi_fieldcalc_amd.synth as synth

    u1, v1 = synth.wind(64, 32, 123, nlev=3)
    u2, v2 = synth.wind(64, 32, 123, nlev=3)
    assert np.array_equal(u1, u2) and np.array_equal(v1, v2)
    assert float(np.abs(u1).max()) < 21.0
    xm, ym, fc = synth.grid_maps(1440, 720)
    assert xm.dtype == np.float32 and np.all(np.abs(fc) >= 1e-5) and np.all(xm >= ym - 1e-12)
    a, b = synth.hybrid_levels(137)
    assert np.all(a >= 0) and np.all(b >= 0) and np.all(b <= 1) and not np.any((a == 0) & (b == 0))


def test_cxx_library_exports_the_reference_symbols(built):
    """Binary drop-in: every miutil::fieldcalc / miutil::constants function the compiled
    reference exports (recorded in tests/golden/reference_symbols.txt; where oracle/_ref/
    holds the compiled reference, the recording must equal what it exports) is exported by
    libmi-fieldcalc.so under the same mangled name."""
    import golden_util

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}

    ref = set(golden_util.reference_symbols())
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libmifc_ref.so")
    if os.path.exists(ref_path):
        assert {s for s in exported(ref_path) if s.startswith("_ZN6miutil")} == ref, "stale tests/golden/reference_symbols.txt"
    mine = exported(CXXLIB)
    # internal helpers the reference happens to export: its OpenMP thread heuristic and a file-local predicate
    internal = {s for s in ref if "compute_num_threads" in s or "bad_hlevel" in s}
    assert len(ref) > 70
    assert not (ref - internal - mine), sorted(ref - internal - mine)


def _header_prototypes():
    """name -> number of parameters, for every function declared in include/mifc.h."""
    text = open(os.path.join(ROOT, "include", "mifc.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(mifc_[a-zA-Z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def test_python_binding_mirrors_the_header():
    """The ctypes table (mi-fieldcalc_amd/_capi.py) is hand-written: every prototype of include/mifc.h must be in
    it with the same number of parameters -- a drifted signature would pass garbage across the C ABI."""
    import mi_fieldcalc_amd._capi as capi

    protos = _header_prototypes()
    assert len(protos) > 90
    missing = sorted(set(protos) - set(capi.SIGNATURES))
    assert not missing, missing
    for name, (res, args) in capi.SIGNATURES.items():
        assert name in protos, name + " is bound but not declared in include/mifc.h"
        assert len(args) == protos[name], (name, len(args), protos[name])


def test_measurement_knobs_exist_in_the_measurement_build_only(built):
    """knobs that give wrong results by design (loads / stores / halo rows switched off) must not be
    reachable in the library callers link.  They are compiled into libmifc_measure.so (tools/ only)."""
    product = open(LIB, "rb").read()
    measure_path = os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc_measure.so")
    assert os.path.exists(measure_path)
    measure = open(measure_path, "rb").read()
    for key in (b"PADROWS", b"MIFC_MEASUREMENT_KNOBS"):
        assert key not in product, key
    assert b"PADROWS" in measure
    # round 3: the yardsticks, the division self-check and the per-launch event timing too (include/mifc_measure.h)
    out = {which: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout for which, path in
           (("product", LIB), ("measure", measure_path))}
    for sym in ("mifc_timing_begin", "mifc_timing_end_ms", "mifc_bench_stream2", "mifc_diag_division"):
        assert (" T " + sym) not in out["product"] and (" T " + sym) in out["measure"], sym
    assert "stream2_kernel" not in out["product"] and b"stream2_kernel" not in product
    pkg = os.path.join(ROOT, "mi-fieldcalc_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            assert "libmifc_measure" not in open(os.path.join(pkg, f)).read(), f


def test_environment_is_read_in_one_place_only():
    """No launch path calls getenv: the MIFC_* variables are read into a snapshot by mifc_create / mifc_reload_env
    (csrc/mifc_env.hip); MIFC_DEVICE belongs to the C++ API's per-thread context (src/FieldCalculations.cc)."""
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")) and f != "mifc_env.hip":
            code = re.sub(r"//.*", "", open(os.path.join(csrc, f)).read())
            assert "getenv" not in code, f


def test_scratch_slots_are_touched_by_the_staging_object_only():
    """The context's scratch slots are handed out per call by mifc_host::Staging (csrc/mifc_ctx.h, mifc_ctx.hip): no
    other file indexes them or names the helpers that took a slot number, and CTX_OR_FAIL is defined once."""
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    defines = 0
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(csrc, f)).read()
        defines += text.count("#define CTX_OR_FAIL")
        if f not in ("mifc_ctx.h", "mifc_ctx.hip"):
            for word in ("->slot[", "slot_bytes", "NSLOT", "stage_in(", "stage_out(", "fetch_out(", "ensure_slot("):
                assert word not in text, (f, word)
    assert defines == 1


def test_choose_placement_keeps_the_fastest_candidate():
    """placement.choose_placement: every candidate is allocated and probed once, the fastest is returned,
    the report names it; the losers are released."""
    import gc
    import weakref

    from mi_fieldcalc_amd.placement import choose_placement

    class Cand:
        def __init__(self, k):
            self.k = k

    made, refs = [], []
    times = [3.0, 1.5, 2.0, 1.7]

    def allocate():
        c = Cand(len(made))
        made.append(c.k)
        refs.append(weakref.ref(c))
        return c

    best, report = choose_placement(allocate, lambda c: times[c.k], tries=4, device="cpu")
    assert made == [0, 1, 2, 3] and best.k == 1
    assert report == {"tries": 4, "probe_ms": times, "chosen": 1}
    gc.collect()
    assert [r() is not None for r in refs] == [False, True, False, False]
    with pytest.raises(ValueError):
        choose_placement(allocate, lambda c: 0.0, tries=0)


def test_choose_search_finds_the_fast_combination():
    """placement.choose_search: the time is a property of the COMBINATION (here: fast only when the two outputs are
    a particular pair and the inputs avoid one array); structured + random sets, then coordinate descent, stay within
    the probe budget and end on a fast set; the report names it."""
    from mi_fieldcalc_amd.placement import choose_search

    made = []

    def allocate():
        made.append(len(made))
        return made[-1]

    calls = [0]

    def probe(arrays):
        calls[0] += 1
        u, v, r, d = arrays
        t = 0.435
        if (r + d) % 5 == 0:
            t -= 0.02
        if u % 3 != 0 and v % 3 != 0:
            t -= 0.015
        return t

    chosen, report = choose_search(allocate, 4, probe, pool_size=16, random_sets=8, max_probes=80)
    assert len(made) == 16 and len(set(chosen)) == 4
    assert report["probes"] <= 80 and calls[0] == report["probes"] + 1  # + the confirming probe
    assert abs(report["chosen_ms"] - 0.40) < 1e-9 and report["chosen"] == list(chosen)
    assert report["allocated_in_one_go_ms"] == round(probe((0, 1, 2, 3)), 4)
    with pytest.raises(ValueError):
        choose_search(allocate, 4, probe, pool_size=3)


def test_choose_search_rounds_takes_the_best_pool():
    """placement.choose_search_rounds: a pool can hold no fast set at all; the next pool comes from OTHER memory (the freed part
    of the previous one is re-occupied by ballast while it is searched) and the best set over all pools is returned."""
    from mi_fieldcalc_amd.placement import choose_search_rounds

    made = []

    def allocate():  # "addresses": consecutive numbers; nothing is ever handed out twice while it is held
        made.append(len(made))
        return made[-1]

    def probe(arrays):  # only arrays of the SECOND pool's range can form the fast set
        fast = all(32 <= a < 48 for a in arrays) and sum(arrays) % 2 == 0
        return 0.38 if fast else 0.41

    chosen, report = choose_search_rounds(allocate, 4, probe, rounds=3, pool_size=16, random_sets=8, max_probes=60)
    # 16 (pool 1) + 12 (ballast) + 16 (pool 2) + 12 (ballast) + 16 (pool 3)
    assert len(made) == 72
    assert report["rounds_chosen_ms"] == [0.41, 0.38, 0.41] and report["chosen_ms"] == 0.38
    assert all(32 <= a < 48 for a in chosen) and "best of 3 pools" in report["method"]


def test_saturation_table_image_is_current():
    """csrc/mifc_ewt_image.h (the LDS image the kernels copy per workgroup) is what tools/gen_ewt_image.py generates
    from the reference's table (MetConstants.h:57-59), and its reciprocals are those of the FLOAT bin widths."""
    import struct
    import subprocess

    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ewt_image.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_ewt_image as g

    words, first = g.image()
    tab = np.array(words[:41], dtype=np.uint32).view(np.float32)
    assert tab[0] == np.float32(.000034) and tab[40] == np.float32(1013.25)
    assert all(w == 0x7f800000 for w in words[41:41 + g.N_PAD])  # +inf behind the table: the inverse lookup reads past it unchecked
    assert words[41 + g.N_PAD:41 + g.N_PAD + g.N_FIRST] == first
    rcp = np.array(words[41 + g.N_PAD + g.N_FIRST + 1:], dtype=np.uint32).view(np.float64)
    assert len(rcp) == 41 and rcp[40] == 0.0
    assert all(rcp[k] == 1.0 / np.float64(tab[k + 1] - tab[k]) for k in range(40))
    # first[b]: the walk of MetConstants.cc:37-45 from the top of the table stops there for et = 2^(b-15)
    for b, k in enumerate(first):
        et = np.float32(2.0) ** np.float32(b - 15)
        ll = 40
        while ll > 0 and tab[ll] > et:
            ll -= 1
        assert ll == k
