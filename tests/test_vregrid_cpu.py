"""mifc_vregrid_* without a GPU: hand-computed columns pin the restatement (tests/vregrid_restate.py) to the text of
include/mifc.h, with constant target planes it is vinterp_restate bit for bit, every named mistake changes the cases
aimed at it, the rules the kernel is built from (mi-fieldcalc_amd/csrc/mifc_vregrid_rules.h) compiled with the host
compiler -- through a shim and, under the address and undefined-behaviour sanitizers, as a stand-alone program -- are
held to the restatement cell by cell, the allowance of MIFC_VINTERP_LOG is guarded, and the entries are declared, bound
and configured."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vinterp_restate as vi
import vregrid_cases as vc
import vregrid_restate as vg
from cases import same_bits
from mi_fieldcalc_amd import vregrid as vregrid_module  # (without the feature the file fails here)

U = vg.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
A, S, N = vg.ALL_DEFINED, vg.SOME_DEFINED, vg.NONE_DEFINED
NAN, INF = np.float32(np.nan), np.float32(np.inf)
EVERY = [(m, f, o) for m in ("linear", "log") for f in ("first", "last") for o in ("undef", "clamp")]


def column(c, x, targets, method=vg.LINEAR, from_=vg.FROM_FIRST, outside=vg.OUTSIDE_UNDEF, with_flags=False, **kw):
    """One column (ny = nx = 1) of one field on a coordinate batch: the results per target as a list (and the flags)."""
    c, x, t = (np.asarray(a, np.float32).reshape(-1, 1, 1) for a in (c, x, targets))
    out, fd = vg.coord_fields(x[None], c, t, method, from_, outside, **kw)
    return (out.ravel().tolist(), fd.ravel().tolist()) if with_flags else out.ravel().tolist()


# ------------------------------------------------------------------------------ hand-computed columns: the header's text
def test_monotone_columns_by_hand():
    down, up, x, xr = [100, 200, 400, 800], [800, 400, 200, 100], [1, 2, 4, 8], [8, 4, 2, 1]
    for fr in (vg.FROM_FIRST, vg.FROM_LAST):
        assert column(down, x, [150, 200, 600, 50, 900], from_=fr) == [1.5, 2.0, 6.0, U, U]  # 200: weight 1 of pair 0 or weight 0 of pair 1
        assert column(up, xr, [150, 200, 600, 50, 900], from_=fr, outside=vg.OUTSIDE_CLAMP) == [1.5, 2.0, 6.0, 1.0, 8.0]  # kmin = 3, kmax = 0


def test_first_and_last_bracket_of_a_non_monotone_column():
    wavy = [100, 500, 200, 400]  # 300 lies in (0, 1), (1, 2) and (2, 3)
    assert column(wavy, [10, 50, 20, 40], [300]) == [30.0] and column(wavy, [10, 50, 0, 999], [300]) == [30.0]
    assert column(wavy, [10, 50, 20, 60], [300], from_=vg.FROM_LAST) == [40.0] and column(wavy, [0, 999, 20, 60], [300], from_=vg.FROM_LAST) == [40.0]
    # the pair is (k, k + 1) also when it is found from the end: 1/3 of the way from level 2 to level 3
    w = (np.float64(np.float32(266)) - 200.0) / (400.0 - 200.0)
    assert column(wavy, [0, 0, 0.1, 0.7], [266], from_=vg.FROM_LAST) == [float(np.float32(np.float64(np.float32(0.1)) + w * (np.float64(np.float32(0.7)) - np.float64(np.float32(0.1)))))]


def test_a_target_on_a_level_and_equal_levels():
    assert column([100, 300, 300, 500], [1, 2, 3, 4], [300]) == [2.0]  # the pair (0, 1), weight 1
    assert column([100, 300, 300, 500], [1, 2, 3, 4], [300], from_=vg.FROM_LAST) == [3.0]  # the pair (2, 3), weight 0
    assert column([300, 300], [7, 9], [300], from_=vg.FROM_LAST) == [7.0] and column([300, 300], [7, 9], [300]) == [7.0]  # x_k, nothing is divided
    assert column([100, 300, 300, 500], [1, U, 3, 4], [300]) == [U]  # the first bracket decides, its value is missing


def test_holes_and_targets_beyond_the_ends():
    x = [1, 2, 4, 8]
    for fr in (vg.FROM_FIRST, vg.FROM_LAST):
        kw = dict(from_=fr, outside=vg.OUTSIDE_CLAMP)
        assert column([100, U, 400, 800], x, [150, 50, 900, 400], **kw) == [U, 1.0, 8.0, 4.0]  # 150: inside the range, the hole took its bracket
        assert column([U, U], [1, 2], [5], **kw) == [U] and column([NAN, U, NAN], [1, 2, 3], [5], **kw) == [U]  # no usable level
        assert column([100, 200, 400, 800], [U, 2, 4, 8], [50], **kw) == [U]  # the clamped value is undefined
        assert column([100, 200, 400, 800], [U, 2, 4, 8], [50], flags=[[A, S, S, S]], **kw) == [float(U)]  # ... or counts as a value
    out, fd = column([100, 200, 400, 800], [U, 2, 4, 8], [50, 150], outside=vg.OUTSIDE_CLAMP, with_flags=True)
    assert out == [U, U] and fd == [N, N]


def test_ties_and_signed_zeros():
    for fr in (vg.FROM_FIRST, vg.FROM_LAST):
        kw = dict(from_=fr, outside=vg.OUTSIDE_CLAMP)
        assert column([100, 100, 400, 400], [1, 2, 4, 8], [50, 900], **kw) == [1.0, 4.0]  # the lowest index that attains the extreme
        assert column([0.0, -0.0, 5], [1, 2, 3], [-1], **kw) == [1.0] and column([-0.0, 0.0, -5], [1, 2, 3], [1], **kw) == [1.0]  # -0 == +0 is a tie
    assert column([-0.0, 10], [1, 2], [0.0]) == [1.0] and column([0.0, 10], [1, 2], [-0.0]) == [1.0]  # and a bracket


def test_targets_that_are_not_usable():
    out, fd = column([100, 200, 400, 800], [1, 2, 4, 8], [U, NAN, 150], outside=vg.OUTSIDE_CLAMP, with_flags=True)
    assert out == [U, U, 1.5] and fd == [N, N, A]
    out, fd = column([100, 200, 400, 800], [1, 2, 4, 8], [U, NAN, 150], outside=vg.OUTSIDE_CLAMP, with_flags=True, fdef_tcoord=[A, A, A])
    assert out == [8.0, U, 1.5] and fd == [A, N, A]  # ALL_DEFINED: 1e35 is a number, far above the column
    out = column([100, 200], [1, 2], [NAN, 150], undef=NAN)
    assert np.isnan(out[0]) and out[1] == 1.5


def test_log_by_hand():
    out = column([100, 400], [1, 3], [200, 0, -5, 50], method=vg.LOG, outside=vg.OUTSIDE_CLAMP)
    w = (np.log(np.float64(200)) - np.log(np.float64(100))) / (np.log(np.float64(400)) - np.log(np.float64(100)))
    assert out == [float(np.float32(1.0 + w * 2.0)), U, U, 1.0] and abs(out[0] - 2.0) < 1e-6
    assert column([-100, 400], [1, 3], [200], method=vg.LOG) == [U] and column([0, 400], [1, 3], [200], method=vg.LOG) == [U]  # a coordinate <= 0 at the bracket
    assert column([0, 400], [1, 3], [500], method=vg.LOG, outside=vg.OUTSIDE_CLAMP) == [3.0]  # the clamp copies, whatever the coordinates
    assert column([-5, 400], [1, 3], [-7], method=vg.LOG, outside=vg.OUTSIDE_CLAMP) == [U]  # but the target must be usable


# --------------------------------------------------------------------------- constant planes: vinterp's restatement
@pytest.mark.parametrize("method", ["linear", "log"])
@pytest.mark.parametrize("kind", ["hybrid", "field"])
def test_constant_target_planes_are_vinterp(kind, method):
    for case in (vc.main(kind), vc.main(kind, bottom_up=True)) + ((vc.wavy(),) if kind == "field" else ()):
        targets = vi.MAIN_TARGETS
        tc = np.broadcast_to(targets[:, None, None], (targets.size,) + case["fields"].shape[2:])
        m = vc.METHODS[method]
        if kind == "hybrid":
            exp, efd = vi.hlevels(case["fields"], case["coord"], case["ab"][0], case["ab"][1], targets, m)
            got, gfd = vg.hlevels(case["fields"], case["coord"], case["ab"][0], case["ab"][1], tc, m)
        else:
            exp, efd = vi.coord_fields(case["fields"], case["coord"], targets, m)
            got, gfd = vg.coord_fields(case["fields"], case["coord"], tc, m)
        assert same_bits(got, exp, nan_payload=False) and np.array_equal(gfd, efd)
        assert (exp != U).mean() > 0.3


# ------------------------------------------------------------------------------------------------- the named mistakes
def changed(case, method, from_, outside, mistake):
    exp, efd = vc.expected(case, method, from_, outside)
    got, gfd = vc.expected(case, method, from_, outside, mistakes=(mistake,))
    return int(((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp))).sum())


def test_each_mistake_changes_the_cases_aimed_at_it():
    aimed = {
        "last bracket under from first": (vc.wavy(), "linear", "first", "undef"),
        "pair oriented by the walk": (vc.heights(), "linear", "last", "undef"),  # (equal neighbours: x_k, not x_k+1; elsewhere both orders round alike)
        "clamp to the end levels": (vc.heights(), "linear", "first", "clamp"),
        "clamp inside a gap": (vc.heights(), "linear", "last", "clamp"),
        "highest index on a tie": (vc.heights(), "linear", "first", "clamp"),
        "weight from a float log": (vc.main("field"), "log", "first", "undef"),
        "open bracket end": (vc.heights(), "linear", "first", "undef"),
        "undefined target as a number": (vc.main("hybrid"), "log", "first", "clamp"),
    }
    assert set(aimed) == set(vg.MISTAKES)
    for mistake, (case, method, from_, outside) in aimed.items():
        assert changed(case, method, from_, outside, mistake) > 0, mistake
    # ... and the orientation shows where c_k == c_k+1 gives x_k
    assert column([300, 300], [7, 9], [300], from_=vg.FROM_LAST, mistakes=("pair oriented by the walk",)) == [9.0]


def test_seeded_cases_reach_what_they_are_for():
    first, _ = vc.expected(vc.wavy(), "linear", "first")
    last, _ = vc.expected(vc.wavy(), "linear", "last")
    assert ((first != last) & (first != U)).mean() > 0.1  # first and last bracket differ
    for kind in ("hybrid", "field", "levels"):
        plain, _ = vc.expected(vc.main(kind), "linear", "first", "undef")
        clamped, fd = vc.expected(vc.main(kind), "linear", "first", "clamp")
        assert 0.02 < ((plain == U) & (clamped != U)).mean() < 0.5 and 0.3 < (plain != U).mean()  # some targets beyond the ends, most inside
        assert (fd == S).all()
    h = vc.heights()
    plain, _ = vc.expected(h, "linear", "first", "undef")
    clamped, _ = vc.expected(h, "linear", "first", "clamp")
    assert ((plain == U) & (clamped == U)).mean() > 0.05 and ((plain == U) & (clamped != U)).mean() > 0.05 and (plain != U).mean() > 0.3


# ------------------------------------------------------------------------------------------- the allowance of LOG
@pytest.mark.parametrize("kind", ["hybrid", "field", "levels"])
def test_log_results_move_by_one_float_step_at_most_when_log_is_an_ulp_off(kind):
    """A device's double log() may differ from numpy's by an ulp or so: with every log() result moved by one ulp of double
    -- all up, all down, each its own way -- at most 1 % of the compared results change, none by more than one float
    step.  These are the LOG cases tests/test_gpu_vregrid.py compares with that allowance."""
    rng = np.random.default_rng(17)
    moves = {"up": lambda v: np.nextafter(np.log(v), np.inf), "down": lambda v: np.nextafter(np.log(v), -np.inf),
             "mixed": lambda v: np.nextafter(np.log(v), np.where(rng.random(np.shape(v)) < 0.5, np.inf, -np.inf))}
    for case in (vc.main(kind), vc.main(kind, bottom_up=True), vc.main(kind, 1, 4, 3, 1100, 3, 7)):
        for from_, outside in (("first", "undef"), ("last", "clamp")):
            exp, efd = vc.expected(case, "log", from_, outside)
            for name, moved in moves.items():
                got, gfd = vc.expected(case, "log", from_, outside, log=moved)
                assert np.array_equal(gfd, efd) and np.array_equal(got == U, exp == U)
                d = exp != U
                steps = np.abs(got.view(np.int32)[d].astype(np.int64) - exp.view(np.int32)[d].astype(np.int64))
                assert steps.max() <= 1 and (steps != 0).mean() <= 0.01, (kind, name, int(steps.max()), float((steps != 0).mean()))


# ----------------------------------------------------------------------------------- the rules header, host compiler
def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    return cxx


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vregrid") / "libvregrid_rules_shim.so")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                    os.path.join(ROOT, "tests", "vregrid_rules_shim.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.mifc_test_vregrid_run.restype = None
    lib.mifc_test_vregrid_run.argtypes = [i, i, i, i, i, i, p, p, p, i, p, p, p, p, p, i, i, i, f, p, p]
    lib.mifc_test_vregrid_extremes.restype = None
    lib.mifc_test_vregrid_extremes.argtypes = [p, i, i, p]
    lib.mifc_test_vregrid_brackets.argtypes = [f, f, f]
    return lib


def header_run(shim, case, method, from_, outside):
    kind = {"hybrid": 0, "field": 1, "levels": 2}[case["kind"]]
    fields, tcoord = np.ascontiguousarray(case["fields"], np.float32), np.ascontiguousarray(case["tcoord"], np.float32)
    nf, nlev, ny, nx = fields.shape
    nt = tcoord.shape[0]
    coord = np.ascontiguousarray(case["coord"], np.float32)
    ints = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)  # noqa: E731
    flags = case.get("flags")
    if flags is not None and np.ndim(flags) == 1:
        flags = np.repeat(np.asarray(flags).reshape(-1, 1), nlev, axis=1)
    fin, fco, ftc = ints(flags), ints(case.get("fdef_c") if kind == 1 else None), ints(case.get("fdef_t"))
    fdef_ps = int(case["fdef_c"]) if kind == 0 and case.get("fdef_c") is not None else S
    a, b = (np.ascontiguousarray(v, np.float32) for v in case["ab"]) if kind == 0 else (None, None)
    ptr = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    out, fd = np.full((nf, nt, ny, nx), -7.0, np.float32), np.full((nf, nt), -1, np.int32)
    shim.mifc_test_vregrid_run(kind, nx, ny, nlev, nf, nt, ptr(fields), ptr(fin), ptr(coord), fdef_ps, ptr(fco), ptr(a), ptr(b), ptr(tcoord), ptr(ftc),
                               vc.METHODS[method], vc.FROM[from_], vc.OUTSIDE[outside], float(np.float32(case.get("undef", U))), ptr(out), ptr(fd))
    return out, fd


SEEDED = {"hybrid": lambda: vc.main("hybrid"), "field": lambda: vc.main("field"), "levels": lambda: vc.main("levels"),
          "bottom-up": lambda: vc.main("hybrid", bottom_up=True), "wavy": vc.wavy, "heights": vc.heights, "flagged": vc.flagged,
          "undef = NaN": lambda: vc.with_nan_undef(vc.main("field")), "NaN heights": lambda: vc.with_nan_undef(vc.heights())}


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_header_against_the_restatement_on_the_seeded_cases(shim, name):
    case = SEEDED[name]()
    for method, from_, outside in EVERY:
        exp, efd = vc.expected(case, method, from_, outside)
        got, gfd = header_run(shim, case, method, from_, outside)
        label = (name, method, from_, outside)
        assert np.array_equal(gfd, efd), label
        if method == "linear":
            assert same_bits(got, exp, nan_payload=False), label
        else:  # the host's libm log() against numpy's: the allowance of the header
            isun = np.isnan if np.isnan(case.get("undef", U)) else (lambda v: v == U)
            assert np.array_equal(isun(got), isun(exp)), label
            d = ~isun(exp) & ~(np.isnan(got) & np.isnan(exp))
            steps = np.abs(got.view(np.int32)[d].astype(np.int64) - exp.view(np.int32)[d].astype(np.int64))
            assert steps.size == 0 or (steps.max() <= 1 and (steps != 0).mean() <= 0.01), label


def test_header_extremes_and_brackets(shim):
    out = np.zeros(2, np.int32)
    for col, want in (([3, 1, 1, 3], (1, 0)), ([NAN, 2, NAN, 2], (1, 1)), ([NAN] * 4, (-1, -1)), ([INF, INF, -INF, -INF], (2, 0)), ([0.0, -0.0, 0.0], (0, 0))):
        c = np.asarray(col, np.float32)
        for descending in (0, 1):
            shim.mifc_test_vregrid_extremes(c.ctypes.data, c.size, descending, out.ctypes.data)
            assert tuple(out) == want, (col, descending)
    br = shim.mifc_test_vregrid_brackets
    assert br(1, 2, 1) and br(1, 2, 2) and br(2, 1, 1.5) and br(-0.0, 1, 0.0) and br(0.0, 1, -0.0) and br(5, 5, 5) and br(INF, 0, 7)
    assert not br(1, 2, 2.5) and not br(NAN, 2, 1) and not br(1, NAN, 1) and not br(1, 2, NAN)


def test_rules_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "vregrid_rules_asan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "host", "vregrid_rules_main.cc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)  # (the environment as it is: the runtimes are linked in)
    assert run.returncode == 0 and " checks, 0 failures" in run.stdout, run.stdout + run.stderr


# ------------------------------------------------------------------------------- declared, bound and configured
def test_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    whole = open(os.path.join(ROOT, "include", "mifc.h")).read()
    header = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    for name, nargs in (("mifc_vregrid_hlevels", 21), ("mifc_vregrid_fields", 19), ("mifc_vregrid_levels", 18)):
        declared = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        sig = capi.SIGNATURES[name]
        assert len(declared.split(",")) == nargs == len(sig[1]) and sig[0] == "i" and sig[1][-2:] == ["f", "i"], name
    assert capi.SIGNATURES["mifc_last_vregrid_form"] == ("s", []) and re.search(r"\bmifc_last_vregrid_form\s*\(", header)
    for rule in ("1. Source coordinate.", "2. Target.", "3. Bracket.", "4. Values, weight, result.", "5. No bracket.", "6. Flags."):
        assert rule in whole, rule
    for var in ("MIFC_VREGRID_CHUNK_MIB", "MIFC_VREGRID_TB", "MIFC_VREGRID_V"):
        readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if '"%s"' % var in open(p, errors="replace").read()]
        assert readers == ["mifc_env.hip"], (var, readers)
    host = open(os.path.join(CSRC, "mifc_capi_vregrid.hip")).read()
    assert "getenv" not in host and re.search(r"vregrid_chunk_mib > 0 \? mifc::env\(\)\.vregrid_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_vregrid.hip") == 1 and makefile.count("mifc_capi_vregrid.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    assert makefile.count("mifc_vregrid_rules.h") == 1  # HDRS
    rules = open(os.path.join(CSRC, "mifc_vregrid_rules.h")).read()
    assert "hip" not in re.sub(r"//.*", "", rules).lower()  # HIP-free: the host compiler builds it
    kernel = open(os.path.join(CSRC, "mifc_vregrid.hip")).read()
    assert '#include "mifc_vregrid_rules.h"' in kernel
    for rule in ("vregrid_target", "vregrid_weight", "vregrid_value", "vregrid_extremes_level", "vregrid_clamp_level"):
        assert rule in kernel, rule
    # no more kernel instances than mifc_vinterp.hip has: coordinate kind x method x fields x cells per lane
    assert len(re.findall(r"launch_v<HYBRID, LOG, \d>", kernel)) == 8 and "template <bool HYBRID, bool LOG, int NF, int V>" in kernel
    assert "### 4.27" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert vregrid_module.VREGRID_FROM == {"first": 0, "last": 1} and vregrid_module.VREGRID_OUTSIDE == {"undef": 0, "clamp": 1}
