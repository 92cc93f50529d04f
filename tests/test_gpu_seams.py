"""The seam cases of tests/seam_cases.py on the GPU, with host pointers and with device-resident fields.

Three bars, by what an operator computes:

  * everything outside gpu_util.uses_device_powf: bit for bit against the CPU restatement, output flag included;
  * the libm class (logField, log10Field, expField, pow10Field, powerField): every finite cell within 1 ulp of the float64
    result rounded to float32 -- the claim of mifc_device.h, and a bound the restatement itself meets on these inputs
    (tests/test_seam_cases_cpu.py) -- with zeros, infinities, NaNs and undefined cells where the restatement has them and
    equal flags; no relative tolerance, no floor.  pow_kappa is held to the same bound through aleveltemp with theta == 1;
  * the composites that chain such a result through the saturation-pressure table or a polynomial (from potential
    temperature: *leveltemp, *levelhum, *levelthe, *levelducting; windCooling, abshum, snow_in_cm): the 1e-5 bound of
    gpu_util.compare with its conditioning slack, identical undef / NaN placement and equal flags, except for the cells
    listed in ALLOWED_FLIPS.
"""
import numpy as np
import pytest

import cases
import gpu_util
import seam_cases as sc
from test_seam_cases_cpu import check_against_float64, ordered

pytestmark = pytest.mark.gpu

F = np.float32
UNDEF = cases.UNDEF

# Composite cells that may be defined on one side and undefined on the other: the device's power and glibc's differ by one
# ulp in a fraction of the arguments, and a temperature one float across a validity end of the table (x == -1, x == 40)
# changes ok().  label -> cell indices; at most 4 per case, each within two float spacings of an end in float64 (checked
# below).  Empty: on the committed seam inputs no cell flips.
ALLOWED_FLIPS = {}
TABLE_ENDS_KELVIN = tuple(float(np.float64(sc.T0) + tc) for tc in (-105.0, 100.0))  # x == -1 and x == 40


def _expected(oracle, case):
    with np.errstate(all="ignore"):
        return cases.run_cpu(oracle, case)


def _check_exact(case, got, flag, out_e, flag_e):
    gpu_util.compare(case, np.asarray(got), np.asarray(out_e), True)
    assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)


def _check_libm(case, got, flag, out_e, flag_e):
    got, out_e = np.asarray(got, F), np.asarray(out_e, F)
    check_against_float64(case, got, out_e, "device")
    # ... and special values where the restatement has them (it agrees with float64 on these, see the CPU test)
    for name, gm, em in (("undef", got == UNDEF, out_e == UNDEF), ("NaN", np.isnan(got), np.isnan(out_e)), ("inf", np.isinf(got), np.isinf(out_e)),
                         ("zero", got == 0, out_e == 0)):
        assert np.array_equal(gm, em), "%s: %s placement differs from the restatement" % (case["label"], name)
    s = np.isinf(out_e) | (out_e == 0)
    assert np.array_equal(got[s].view(np.uint32), out_e[s].view(np.uint32)), "%s: sign of a zero or an infinity" % case["label"]
    assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)


def _check_bare_power(case, got, flag, out_e, flag_e):
    """aleveltemp, theta == 1.0f, kelvin out: the output is pow_kappa(p * p0inv) itself.  Within 1 ulp of
    float32(float64(float32(p * p0inv)) ** kappa), kappa the project's float constant widened to double; special values as
    pow_kappa_rare documents them (finite x < 0 and NaN -> NaN, 0 -> 0, +-inf -> +inf), which is what powf and float64 give."""
    got, out_e = np.asarray(got, F).ravel(), np.asarray(out_e, F).ravel()
    p = np.asarray(case["args"][1], F).ravel()
    und = out_e == UNDEF
    assert np.array_equal(got == UNDEF, und), "%s: undef placement" % case["label"]
    with np.errstate(all="ignore"):
        x = (p * sc.P0INV).astype(F)
        want = np.power(x.astype(np.float64), np.float64(sc.KAPPA)).astype(F)
    g, w, e, xs = got[~und], want[~und], out_e[~und], x[~und]
    for name, fn in (("NaN", np.isnan), ("inf", np.isinf), ("zero", lambda a: a == 0)):
        assert np.array_equal(fn(g), fn(w)), "%s: %s placement differs from float64 at x = %r" % (case["label"], name, xs[np.nonzero(fn(g) != fn(w))[0][:4]])
        assert np.array_equal(fn(g), fn(e)), "%s: %s placement differs from the restatement" % (case["label"], name)
    assert np.all(np.isnan(g[((xs < 0) & np.isfinite(xs)) | np.isnan(xs)])) and np.all(g[xs == 0] == 0) and not np.any(np.signbit(g[xs == 0]))
    assert np.all(g[np.isinf(xs)] == np.inf)
    fin = np.isfinite(w) & (w != 0)
    d = np.abs(ordered(g[fin]) - ordered(w[fin]))
    if d.size and d.max() > 1:
        k = int(np.argmax(d))
        raise AssertionError("%s: pow_kappa %d ulp from float64 at x = %r: got %r, float64 gives %r (%d cells beyond 1 ulp)" % (
            case["label"], d[k], xs[fin][k], g[fin][k], w[fin][k], np.count_nonzero(d > 1)))
    assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)


def _check_composite(case, got, flag, out_e, flag_e):
    got, out_e = np.asarray(got, F), np.asarray(out_e, F)
    flips = np.nonzero(((got == UNDEF) != (out_e == UNDEF)).ravel())[0]
    listed = tuple(ALLOWED_FLIPS.get(case["label"], ()))
    assert set(flips.tolist()) <= set(listed), "%s: cells %s are undefined on one side only" % (case["label"], sorted(set(flips.tolist()) - set(listed)))
    if flips.size:
        got = got.copy()
        got.reshape(-1)[flips] = out_e.reshape(-1)[flips]
    gpu_util.compare(case, got, out_e, False)  # identical undef / NaN / inf placement, 1e-5 with the conditioning slack
    assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)


def _check(ctx, oracle, case, device):
    ok_e, out_e, flag_e = _expected(oracle, case)
    ok, got, flag = gpu_util.run_gpu(ctx, case, device=device)
    assert ok == ok_e, case["label"]
    if not ok_e:
        return
    if case["op"] in sc.LIBM_OPS:
        _check_libm(case, got, flag, out_e, flag_e)
    elif "bare-power" in case["label"]:
        _check_bare_power(case, got, flag, out_e, flag_e)
    elif gpu_util.uses_device_powf(case):
        _check_composite(case, got, flag, out_e, flag_e)
    else:
        _check_exact(case, got, flag, out_e, flag_e)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_seam_family(gpu_ctx, oracle, name, device):
    for case in sc.family(name):
        _check(gpu_ctx, oracle, case, device)


def test_the_three_bars_are_applied_to_the_operators_they_are_meant_for():
    """No GPU work: which check each seam case gets."""
    exact_ops, composite_ops = set(), set()
    for case in sc.all_cases():
        if case["op"] in sc.LIBM_OPS or "bare-power" in case["label"]:
            continue
        (composite_ops if gpu_util.uses_device_powf(case) else exact_ops).add(case["op"])
    assert {"windCooling", "abshum", "snow_in_cm", "alevelhum", "hlevelthe", "alevelducting", "hleveltemp"} <= composite_ops
    assert {"plevelhum", "cvhum", "kIndex", "ductingIndex", "showalterIndex", "pressure2FlightLevel", "values2classes", "underCooledRain",
            "vesselIcingMertins", "vesselIcingOverland", "seaSoundSpeed", "fieldOPERfield", "minvalueFields", "replaceDefined"} <= exact_ops
    assert not (composite_ops & set(sc.LIBM_OPS))


def test_allowed_flips_are_few_and_sit_on_a_validity_end():
    by_label = {c["label"]: c for c in sc.family("composite")}
    for label, cells in ALLOWED_FLIPS.items():
        assert label in by_label and 0 < len(cells) <= 4, label
        tk = sc.composite_kelvin64(by_label[label]).ravel()
        for i in cells:
            assert min(abs(tk[i] - end) / np.spacing(F(end)) for end in TABLE_ENDS_KELVIN) <= 2.0, (label, i, tk[i])
