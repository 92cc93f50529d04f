"""CPU checks of mifc_hdist_*: the two numpy restatements (tests/hdist_restate.py, the oracle of the GPU tests) against
each other and on hand-computed rows, each named mistake shown to change the cases aimed at it, the rules header
(mi-fieldcalc_amd/csrc/mifc_hdist_rules.h) compiled with the host compiler -- through a shim and, under the address and
undefined-behaviour sanitizers, as a stand-alone program -- and held to the restatement, that the entries are declared,
bound and configured where the others are, and the front's marshalling and refusals against a recording stub library."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hdist_restate as hd
import test_python_front_cpu as front
from mi_fieldcalc_amd import hdist as hdist_module  # (without the feature the file fails here)
from test_python_front_cpu import _data, _stub_context

U = hd.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
A, S_, N = hd.ALL_DEFINED, hd.SOME_DEFINED, hd.NONE_DEFINED
TINY = np.float32(1.0e-45)
# the host tables of the two entries for the recording stub: positions after the context
front.SPEC.setdefault("mifc_hdist_histogram_levels", [(3, "ptr", front._at(5))])
front.SPEC.setdefault("mifc_hdist_quantile_levels", [(3, "ptr", front._at(5))])


def level(values, nx=None):
    v = np.asarray(values, np.float32)
    return v.reshape(1, 1, 1, -1) if nx is None else v.reshape(1, 1, -1, nx)


def special_values():
    return np.array([-np.inf, -3.4028235e38, -1.0, -1.0e-40, -TINY, -0.0, 0.0, TINY, 1.0e-40, 1.0, 3.4028235e38, np.inf], np.float32)


def random_case(seed=0, nf=2, nlev=2, ny=4, nx=9):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 2, (nf, nlev, ny, nx)).astype(np.float32)
    pick = rng.random(x.shape) < 0.2
    x[pick] = rng.choice(special_values(), size=int(pick.sum()))
    x = hd.sprinkle(x, rng, 0.1, U)
    x[0, 0, 0, 0] = np.nan
    mask = hd.sprinkle(np.ones((ny, nx), np.float32), rng, 0.25, U)
    flags = rng.choice([A, S_, N], size=(nf, nlev))
    flags[0, 0] = A
    return x, mask, flags


# ------------------------------------------------------------------------------------- the two restatements agree
@pytest.mark.parametrize("seed", range(4))
def test_the_two_restatements_agree(seed):
    x, mask, flags = random_case(seed)
    edges = np.array([[-np.inf, -1.0, -TINY, 0.0, 1.0e-40, 1.5], [-2.0, -0.0, TINY, 1.0, 3.0, np.inf]], np.float32)
    for box in (None, (1, 8, 1, 4), (3, 4, 2, 3)):
        for m, fm in ((None, S_), (mask, S_), (mask, A)):
            for mode in (hd.AREA, hd.ROWS):
                a = hd.histogram(x, edges, m, fm, box, mode, flags)
                b = hd.histogram_literal(x, edges, m, fm, box, mode, flags)
                assert a.dtype == np.int32 and (a == b).all()
            rows, area = hd.histogram(x, edges, m, fm, box, hd.ROWS, flags), hd.histogram(x, edges, m, fm, box, hd.AREA, flags)
            assert (rows.sum(axis=2, keepdims=True) == area).all()
            for method in (hd.LOWER, hd.LINEAR):
                ps = [0, 2, 25, 50, 50, 77.7, 98, 100]
                with np.errstate(all="ignore"):
                    q, fd = hd.quantiles(x, ps, method, m, fm, box, flags)
                    lq, lfd = hd.quantiles_literal(x, ps, method, m, fm, box, flags)
                assert hd.same(q, lq) and np.array_equal(fd, lfd)


# -------------------------------------------------------------------------------- hand-computed rows: the header's text
def test_hand_computed_histograms():
    edges = [0.0, 1.0, 2.5]
    h = hd.histogram(level([-1, -0.0, 0.0, 0.5, 1.0, 2.4999998, 2.5, 7, U, np.nan]), edges)
    assert h.tolist() == [[[[1, 3, 2, 2, 0]]]]  # undef and the NaN are tested away
    h = hd.histogram(level([-1, -0.0, 0.0, 0.5, 1.0, 2.4999998, 2.5, 7, U, np.nan]), edges, flags=[[A]])
    assert h.tolist() == [[[[1, 3, 2, 3, 1]]]]  # ALL_DEFINED: the stored undef is a value of the last bin, the NaN has its slot
    assert hd.histogram(level([-0.0, 0.0]), [-0.0]).tolist() == hd.histogram(level([-0.0, 0.0]), [0.0]).tolist() == [[[[0, 2, 0]]]]
    assert hd.histogram(level([-np.inf, np.inf, 3]), [-np.inf, np.inf]).tolist() == [[[[0, 2, 1, 0]]]]
    x = level([1, 2, 3, 4, 5, 6], nx=3)
    mask = np.array([[1, U, 1], [1, 1, U]], np.float32)
    assert hd.histogram(x, [3.5], mask=mask, mode="rows").tolist() == [[[[2, 0, 0], [0, 2, 0]]]]
    assert hd.histogram(x, [3.5], mask=mask, fdef_mask=A, mode="rows").tolist() == [[[[3, 0, 0], [0, 3, 0]]]]
    assert hd.histogram(x, [3.5], box=(1, 3, 0, 2)).tolist() == [[[[2, 2, 0]]]]
    assert hd.check_edges([1, 2, 2]) == 2 and hd.check_edges([1, np.nan]) == 1 and hd.check_edges([-0.0, 0.0]) == 1 and hd.check_edges([-np.inf, 0, np.inf]) == -1


def test_hand_computed_percentiles():
    x = level([4, 1, 3, 2, U])
    q, fd = hd.quantiles(x, [0, 50, 100, 40], hd.LOWER)
    assert q.tolist() == [[[1, 3, 4, 2]]] and fd.tolist() == [[A]]  # (int)(4 * 50 / 100) = 2; p = 100 clamps to n - 1; (int)1.6 = 1
    q, _ = hd.quantiles(x, [0, 50, 100, 40], hd.LINEAR)
    assert q.tolist() == [[[1, 2.5, 4, float(np.float32(2.2))]]]  # h = (3 * 40) / 100 = 1.2: x[1] + 0.2 * (x[2] - x[1])
    q, fd = hd.quantiles(level([U, np.nan]), [50])
    assert q.tolist() == [[[float(U)]]] and fd.tolist() == [[N]]  # n == 0
    q, fd = hd.quantiles(level([U, 2]), [50], flags=[[A]])
    assert q[0, 0, 0] == np.float32((2.0 + float(U)) / 2) and fd.tolist() == [[A]]  # a stored undef under ALL_DEFINED is a value
    q, _ = hd.quantiles(level([0.0, -0.0, 0.0, -0.0]), [0, 34, 50, 100], hd.LOWER)
    assert np.signbit(q[0, 0]).tolist() == [True, True, False, False]  # -0 < +0
    q, _ = hd.quantiles(level([np.nan, np.inf, 1]), [0, 50, 100], hd.LOWER, flags=[[A]])
    assert q[0, 0, 0] == 1 and q[0, 0, 1] == np.inf and np.isnan(q[0, 0, 2])  # every NaN above +inf
    # the float rule of LOWER: n = 125, p = (float)5.6 gives 6.9999998... in double and 7 in float
    p = np.float32(5.6)
    assert int((np.float32(125) * p) / np.float32(100)) == 7 and int(125 * float(p) / 100.0) == 6
    assert hd.quantiles(level(np.arange(125)), [p], hd.LOWER)[0].tolist() == [[[7.0]]]


# ------------------------------------------------------------------------------------------- each mistake is visible
def test_each_mistake_changes_the_cases_aimed_at_it():
    zeros = level([-0.0, 0.0, -TINY, TINY])
    on_edge = level([1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0])
    with_nan = level([np.nan, 1.0, 5.0])
    many = np.full((1, 1, 300, 300), 2.0, np.float32)
    hist_cases = {
        "binned on the total-order key": (zeros, [0.0], {}),
        "less at an edge": (on_edge, [1.0, 2.0], {}),
        "nan in the last bin": (with_nan, [2.0], dict(flags=[[A]])),
        "counters wrap at 2^16": (many, [1.0], {}),
    }
    for name, (x, edges, kw) in hist_cases.items():
        right, wrong = hd.histogram(x, edges, **kw), hd.histogram(x, edges, mistakes=(name,), **kw)
        assert (right == hd.histogram_literal(x, edges, **kw)).all() and (right != wrong).any(), name
    p = np.float32(5.6)
    ramp = level(np.arange(125))
    signed = level([0.0, -0.0, 0.0, -0.0, 0.0])
    quant_cases = {
        "lower rank in double": (ramp, [p], hd.LOWER),
        "no clamp at 100": (ramp, [100.0], hd.LOWER),
        "sort without signed zeros": (signed, [0.0, 30.0], hd.LOWER),
        "linear with a float difference": (level([-3.0e38, 3.0e38]), [50.0], hd.LINEAR),
    }
    for name, (x, ps, method) in quant_cases.items():
        with np.errstate(all="ignore"):
            right, wrong = hd.quantiles(x, ps, method)[0], hd.quantiles(x, ps, method, mistakes=(name,))[0]
            assert hd.same(right, hd.quantiles_literal(x, ps, method)[0]) and not hd.same(right, wrong), name
    assert set(hist_cases) | set(quant_cases) == set(hd.MISTAKES)


# ------------------------------------------------------------------------ the rules header through the host compiler
def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    return cxx


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hdist") / "libhdist_rules_shim.so")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "hdist_rules_shim.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.mifc_test_hdist_check_edges.restype = ctypes.c_int
    lib.mifc_test_hdist_interpolate.restype = ctypes.c_float
    lib.mifc_test_hdist_interpolate.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_double]
    lib.mifc_test_hdist_select.restype = ctypes.c_uint
    lib.mifc_test_hdist_rank.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.mifc_test_hdist_plan.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p]
    lib.mifc_test_hdist_scan_step.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    lib.mifc_test_hdist_select.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p]
    for fn in (lib.mifc_test_hdist_keys, lib.mifc_test_hdist_slots):
        fn.restype = None
    lib.mifc_test_hdist_keys.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3
    lib.mifc_test_hdist_slots.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    lib.mifc_test_hdist_check_edges.argtypes = [ctypes.c_void_p, ctypes.c_int]
    return lib


def _values(seed=0, n=400):
    rng = np.random.default_rng(seed)
    v = np.concatenate([special_values(), np.array([np.nan, -np.nan], np.float32), rng.normal(0, 3, n).astype(np.float32),
                        rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    return np.ascontiguousarray(v, np.float32)


def test_header_keys_against_the_restatement(shim):
    x = _values()
    order, bins, back = np.zeros(x.size, np.uint32), np.zeros(x.size, np.uint32), np.zeros(x.size, np.float32)
    shim.mifc_test_hdist_keys(x.ctypes.data, x.size, order.ctypes.data, bins.ctypes.data, back.ctypes.data)
    assert (order == hd.order_key(x)).all() and (bins[~np.isnan(x)] == hd.bin_key(x)[~np.isnan(x)]).all()
    assert hd.same(back, hd.key_value(hd.order_key(x))) and hd.same(back, x)
    assert (order[np.isnan(x)] == 0xFFFFFFFF).all() and order[~np.isnan(x)].max() == 0xFF800000


def test_header_edge_check_and_bin_search_against_the_restatement(shim):
    x = _values(1)
    rng = np.random.default_rng(1)
    sets = [np.array([0.0], np.float32), np.array([-0.0], np.float32), np.array([-np.inf, np.inf], np.float32), np.array([-TINY, 0.0, TINY, 1.0e-40], np.float32),
            np.sort(rng.normal(0, 3, 63).astype(np.float32)), np.sort(rng.normal(0, 3, 64).astype(np.float32)), np.linspace(-9, 9, 65).astype(np.float32),
            np.linspace(-9, 9, 1024).astype(np.float32), np.unique(x[~np.isnan(x) & (x != 0)])[:1024]]
    for e in sets:
        e = np.ascontiguousarray(e, np.float32)
        assert shim.mifc_test_hdist_check_edges(e.ctypes.data, e.size) == hd.check_edges(e) == -1
        probe = np.ascontiguousarray(np.concatenate([x, e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf))]), np.float32)
        slot = np.zeros(probe.size, np.int32)
        shim.mifc_test_hdist_slots(e.ctypes.data, e.size, probe.ctypes.data, probe.size, slot.ctypes.data)
        assert (slot == hd.slots(probe, e)).all()
        with np.errstate(invalid="ignore"):
            literal = np.where(np.isnan(probe), e.size + 1, (e[None, :] <= probe[:, None]).sum(axis=1))
        assert (slot == literal).all()
    for bad in ([1, 2, 2], [1, np.nan, 3], [np.nan], [-0.0, 0.0], [0.0, -0.0], [3, 2], [-np.inf, -np.inf], [1, 2, 3, 4, 3.5]):
        e = np.array(bad, np.float32)
        got = shim.mifc_test_hdist_check_edges(e.ctypes.data, e.size)
        assert got == hd.check_edges(e) and got >= 0, bad


def test_header_rank_rules_against_the_restatement(shim):
    k, k1, t = ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
    ps = [0.0, 1.0e-6, 2.0, 5.6, 25.0, 33.3, 50.0, 75.0, 98.0, 99.99999, 100.0]
    for n in [1, 2, 3, 4, 7, 125, 100, 1000, 65537, 16777217, 2**31 - 1]:
        for p in ps:
            for method in (hd.LOWER, hd.LINEAR):
                shim.mifc_test_hdist_rank(method, n, p, ctypes.addressof(k), ctypes.addressof(k1), ctypes.addressof(t))
                assert (k.value, k1.value, t.value) == hd.rank(method, n, p), (n, p, method)
    for a, b, tt in [(1.0, 2.0, 0.25), (-3.0e38, 3.0e38, 0.5), (1.0, np.inf, 0.5), (-np.inf, np.inf, 0.5), (16777216.0, 16777218.0, 0.25), (1.0e-45, 3.0e-45, 0.5),
                     (5.0, 7.0, 0.0)]:
        with np.errstate(all="ignore"):
            assert hd.same(np.float32(shim.mifc_test_hdist_interpolate(a, b, tt)), hd.interpolate(a, b, tt)), (a, b, tt)


def test_header_digit_plan_for_every_first_differing_bit(shim):
    out = (ctypes.c_int * 8)()
    rng = np.random.default_rng(2)
    for bit in list(range(32)) + [None]:
        for _ in range(8):
            a = int(rng.integers(0, 2**32))
            if bit is None:
                b = a
            else:
                b = (a ^ (1 << bit)) ^ (int(rng.integers(0, 2**32)) & ((1 << bit) - 1))  # equal above `bit`, different at it, anything below
            kmin, kmax = min(a, b), max(a, b)
            shim.mifc_test_hdist_plan(kmin, kmax, out)
            prefix, passes, plan = hd.digit_plan(kmin, kmax)
            assert (out[0], out[1]) == (prefix, passes) == ((32, 0) if bit is None else (31 - bit, -(-(bit + 1) // 11)))
            assert [(out[2 + 2 * j], out[3 + 2 * j]) for j in range(passes)] == plan
            assert all(out[3 + 2 * j] == 0 for j in range(passes, 3)) and passes <= 3
            assert sum(w for _, w in plan) == 32 - prefix and all(1 <= w <= 11 for _, w in plan)


def test_header_scan_step_and_selection_against_the_sort(shim):
    rng = np.random.default_rng(3)
    digit, left = ctypes.c_int(), ctypes.c_uint()
    for nbins in (1, 2, 32, 64, 2048):
        hist = np.ascontiguousarray(rng.integers(0, 5, nbins) * (rng.random(nbins) < 0.6), np.uint32)
        hist[rng.integers(0, nbins)] += 1
        for r in sorted({0, min(1, int(hist.sum()) - 1), int(hist.sum()) // 2, int(hist.sum()) - 1}):
            shim.mifc_test_hdist_scan_step(hist.ctypes.data, nbins, r, ctypes.addressof(digit), ctypes.addressof(left))
            assert (digit.value, left.value) == hd.scan_step(hist, r), (nbins, r)
    passes = ctypes.c_int()
    for bit in range(32):
        v, lo, hi = hd.two_valued(bit, n=9)
        keys = np.ascontiguousarray(hd.order_key(v))
        for r in range(9):
            got = shim.mifc_test_hdist_select(keys.ctypes.data, 9, r, ctypes.addressof(passes))
            assert got == np.sort(keys)[r] and passes.value == -(-(bit + 1) // 11)
    x = _values(4)
    keys = np.ascontiguousarray(hd.order_key(x))
    for r in (0, 1, x.size // 3, x.size // 2, x.size - 2, x.size - 1):
        assert shim.mifc_test_hdist_select(keys.ctypes.data, x.size, r, ctypes.addressof(passes)) == np.sort(keys)[r] and passes.value == 3


def test_rules_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "hdist_rules_asan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "host", "hdist_rules_main.cc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)  # (the environment as it is: the runtimes are linked in)
    assert run.returncode == 0 and " checks, 0 failures" in run.stdout, run.stdout + run.stderr


# ------------------------------------------------------------------------------- declared, bound and configured
def test_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    names = ("mifc_hdist_histogram_levels", "mifc_hdist_quantile_levels", "mifc_last_hdist_form")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert [len(capi.SIGNATURES[n][1]) for n in names] == [16, 17, 0]
    assert capi.SIGNATURES["mifc_hdist_histogram_levels"][1][-2:] == ["f", "i"] and capi.SIGNATURES["mifc_last_hdist_form"][0] == "s"
    assert hdist_module.QUANTILE_METHODS == {"lower": 0, "linear": 1} and re.search(r"MIFC_QUANTILE_LOWER = 0, MIFC_QUANTILE_LINEAR = 1", header)
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if '"MIFC_HDIST_CHUNK_MIB"' in open(p, errors="replace").read()]
    assert readers == ["mifc_env.hip"], readers
    host = open(os.path.join(CSRC, "mifc_capi_hdist.hip")).read()
    assert "getenv" not in host and re.search(r"hdist_chunk_mib > 0 \? mifc::env\(\)\.hdist_chunk_mib : 256", host)
    for shared in ("LevelBatchCall", "check_grid", "check_levels", "check_overlaps", "LevelTable", "Staging", "BandPlan", "hdist_check_edges"):
        assert shared in host, shared
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_hdist.hip") == 1 and makefile.count("mifc_capi_hdist.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    assert makefile.count("mifc_hdist_rules.h") == 1  # HDRS
    rules = open(os.path.join(CSRC, "mifc_hdist_rules.h")).read()
    assert "hip" not in re.sub(r"//.*", "", rules).lower()  # HIP-free: the host compiler builds it
    kernel = open(os.path.join(CSRC, "mifc_hdist.hip")).read()
    assert '#include "mifc_hdist_rules.h"' in kernel and '#include "mifc_hdist_rules.h"' in host
    for rule in ("hdist_order_key", "hdist_slot", "hdist_rank", "hdist_digit_plan", "hdist_scan_step", "hdist_interpolate"):
        assert rule in kernel, rule
    whole = open(os.path.join(ROOT, "include", "mifc.h")).read()
    assert "histograms and percentiles over an area;" not in whole and "mifc_hdist_* entries below" in whole
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "histograms and percentiles\nover an area" not in design and "histograms and percentiles over an area" not in design and "### 4.25" in design


# ------------------------------------------------------------------------------- the front against a recording stub
def _front(rc=1):
    d = _data()
    ctx, lib = _stub_context(d, rc)
    return d, ctx, lib


def test_front_marshals_the_entries_in_header_order():
    d, ctx, lib = _front()
    h = hdist_module.histogram_levels(ctx, d["F2"], [1.0, 5.0, 9.0], mask=d["W"], box=(1, 4, 0, 3), mode="rows", fdefined_in=[A, S_], undef=-5.0)
    name, a = lib.calls[-1]
    assert name == "mifc_hdist_histogram_levels" and a[:3] == [5, 4, 3] and a[3] == [["F2", 0], ["F2", 4 * 60]]
    assert a[4]["values"] == [A, A, A, S_, S_, S_] and a[5] == 2 and a[6]["values"] == [1.0, 5.0, 9.0] * 2 and a[6]["numpy"] == "float32" and a[7] == 3
    assert a[8] == ["W", 0] and a[9] == S_ and a[10]["values"] == [1, 4, 0, 3] and a[11] == 1 and a[13] == -5.0 and a[14] == 0 and len(a) == 15
    assert h.shape == (2, 3, 3, 5) and h.dtype == np.int32 and (h == -1).all()  # (the stub writes nothing: the pre-fill)
    h = hdist_module.histogram_levels(ctx, d["B"], [[2.0, 4.0]])
    name, a = lib.calls[-1]
    assert a[3] == [["B", 0]] and a[4] is None and a[5] == 1 and a[6]["values"] == [2.0, 4.0] and a[7] == 2 and a[8] is None and a[10] is None and a[11] == 0
    assert h.shape == (3, 1, 4)
    hdist_module.histogram_levels(ctx, [d["B"], d["V"]], [[2.0, 4.0], [1.0, 3.0]])
    assert lib.calls[-1][1][6]["values"] == [2.0, 4.0, 1.0, 3.0]
    q, fd = hdist_module.quantile_levels(ctx, d["F2"], [2, 98], "lower", mask=d["W"], fdef_mask=A, box=[0, 5, 1, 2], out=d["OUT"][:12].reshape(2, 3, 2))
    name, a = lib.calls[-1]
    assert name == "mifc_hdist_quantile_levels" and a[:3] == [5, 4, 3] and a[3] == [["F2", 0], ["F2", 4 * 60]] and a[4] is None and a[5] == 2
    assert a[6]["values"] == [2.0, 98.0] and a[7] == 2 and a[8] == 0 and a[9] == ["W", 0] and a[10] == A and a[11]["values"] == [0, 5, 1, 2]
    assert a[12] == ["OUT", 0] and a[13]["numpy"] == "int32" and a[13]["shape"] == [2, 3] and a[14] == float(U) and a[15] == 0 and len(a) == 16
    assert q.shape == (2, 3, 2) and fd.shape == (2, 3)
    q, fd = hdist_module.quantile_levels(ctx, d["B"], 50)
    assert lib.calls[-1][1][8] == 1 and q.shape == (3, 1) and fd.shape == (3,)


def test_front_refusals_that_need_no_library():
    d, ctx, lib = _front()
    n = len(lib.calls)
    with pytest.raises(ValueError, match="edges must"):
        hdist_module.histogram_levels(ctx, d["F2"], [[1.0, 2.0]] * 3)
    with pytest.raises(ValueError, match="1..1024"):
        hdist_module.histogram_levels(ctx, d["B"], np.arange(1025))
    with pytest.raises(ValueError, match="1..1024"):
        hdist_module.histogram_levels(ctx, d["B"], [])
    with pytest.raises(ValueError, match="mask must have the shape"):
        hdist_module.histogram_levels(ctx, d["B"], [1.0], mask=d["B"])
    with pytest.raises(ValueError, match="box is"):
        hdist_module.histogram_levels(ctx, d["B"], [1.0], box=(0, 1, 2))
    with pytest.raises(ValueError, match="1..16"):
        hdist_module.quantile_levels(ctx, d["B"], np.arange(17))
    with pytest.raises(ValueError, match="1..16"):
        hdist_module.quantile_levels(ctx, d["B"], [])
    with pytest.raises(ValueError, match="out must have shape"):
        hdist_module.quantile_levels(ctx, d["B"], [50], out=d["OUT"][:6].reshape(3, 2))
    with pytest.raises(ValueError, match="fields must be"):
        hdist_module.quantile_levels(ctx, d["W"], [50])
    assert len(lib.calls) == n  # nothing reached the library
    d, ctx, lib = _front(rc=0)  # a refusal of the library comes back as Refused, a ValueError and a RuntimeError
    with pytest.raises(hdist_module.Refused) as e:
        hdist_module.histogram_levels(ctx, d["B"], [1.0], mode="columns")
    assert isinstance(e.value, ValueError) and isinstance(e.value, RuntimeError) and lib.calls[-1][1][11] == -1
    with pytest.raises(hdist_module.Refused):
        hdist_module.quantile_levels(ctx, d["B"], [50], method="nearest")
    assert lib.calls[-1][1][8] == -1
