"""The seam cases of tests/seam_cases.py on the CPU: pinned to the compiled reference before any GPU is involved, the
float64 judge of the libm class checked on the restatement itself, and the coverage the cases claim asserted from results.

  * every case: restatement == compiled reference, results and flags, bit for bit (skipped where the reference is not built)
  * logField, log10Field, expField, pow10Field, powerField: the restatement (glibc's float functions) is within 1 ulp of
    float32(f(float64(x))) in every finite cell, zeros, infinities and NaNs in the same cells -- the bound
    tests/test_gpu_seams.py holds the device code to
  * coverage: every knot of the saturation-pressure table hit exactly, both validity ends with a defined and an undefined
    neighbour, every class of values2classes and of the Mertins ladder, both outcomes of each underCooledRain threshold,
    the flight-level table value at each of its pressures
"""
import numpy as np
import pytest

import cases
import seam_cases as sc

F = np.float32
UNDEF = cases.UNDEF


def ordered(a):
    """float32 -> integers in which neighbouring floats differ by 1 (both zeros map to 0)."""
    i = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def float64_result(case):
    """The libm-class operators restated in float64 and rounded to float32 once."""
    op, x = case["op"], np.asarray(case["args"][0], F).astype(np.float64)
    with np.errstate(all="ignore"):
        if op == "logField":
            r = np.log(x)
        elif op == "log10Field":
            r = np.log10(x)
        elif op == "expField":
            r = np.exp(x)
        elif op == "pow10Field":
            r = np.power(10.0, x)
        else:
            r = np.power(x, np.float64(F(case["args"][1])))
        return r.astype(F)


def check_against_float64(case, got, expected_flags_from, what):
    """got: a result of the operator; expected_flags_from: the oracle's result (for the undefined cells).  Every finite cell
    within 1 ulp of the float64 result, special values in the same cells.  Returns the number of cells that differ at all."""
    want = float64_result(case)
    got = np.asarray(got, F)
    und = np.asarray(expected_flags_from, F) == UNDEF
    if case["fdefined"] == cases.ALL_DEFINED:
        und = np.zeros_like(und)
    assert np.array_equal(got == UNDEF, und), "%s %s: undef placement" % (what, case["label"])
    g, w, x = got[~und], want[~und], np.asarray(case["args"][0], F)[~und]
    for name, gm, wm in (("NaN", np.isnan(g), np.isnan(w)), ("inf", np.isinf(g), np.isinf(w)), ("zero", g == 0, w == 0)):
        if not np.array_equal(gm, wm):
            k = np.nonzero(gm != wm)[0][0]
            raise AssertionError("%s %s: %s placement differs at x = %r: got %r, float64 gives %r" % (what, case["label"], name, x[k], g[k], w[k]))
    special = np.isnan(w) | np.isinf(w) | (w == 0)
    assert np.array_equal(g[special].view(np.uint32)[~np.isnan(w[special])], w[special].view(np.uint32)[~np.isnan(w[special])]), \
        "%s %s: sign of a zero or an infinity" % (what, case["label"])
    d = np.abs(ordered(g[~special]) - ordered(w[~special]))
    if d.size and d.max() > 1:
        k = int(np.argmax(d))
        raise AssertionError("%s %s: %d ulp from the float64 result at x = %r: got %r, float64 gives %r (%d cells beyond 1 ulp)" % (
            what, case["label"], d[k], x[~special][k], g[~special][k], w[~special][k], np.count_nonzero(d > 1)))
    return int(np.count_nonzero(d))


def _run(lib, case):
    with np.errstate(all="ignore"):
        return cases.run_cpu(lib, case)


@pytest.mark.parametrize("name", sorted(sc.FAMILIES))
def test_restatement_equals_compiled_reference_on_the_seams(oracle, ref, name):
    cs = sc.family(name)
    assert len(cs) >= 4
    for case in cs:
        assert case["ny"] == 1 and case["nx"] <= 4000
        ok_o, out_o, flag_o = _run(oracle, case)
        ok_r, out_r, flag_r = _run(ref, case)
        assert ok_o == ok_r, case["label"]
        if not ok_r:
            continue
        assert flag_o == flag_r, case["label"]
        if not cases.same_bits(out_o, out_r, nan_payload=False):
            bad = np.nonzero((out_o.view(np.uint32) != out_r.view(np.uint32)) & ~(np.isnan(out_o) & np.isnan(out_r)))
            raise AssertionError("%s: %d cells differ, first at %s: oracle %r ref %r" % (case["label"], len(bad[0]), bad[1][0], out_o[bad][0], out_r[bad][0]))


def test_every_case_comes_in_both_lengths_and_both_flag_modes():
    seen = {}
    for case in sc.all_cases():
        key = case["label"].rsplit("-", 2)[0]
        seen.setdefault(key, set()).add((case["nx"] % 4 == 0, case["fdefined"]))
        if case["fdefined"] == cases.SOME_DEFINED and case["op"] not in ("replaceUndefined", "replaceDefined"):
            assert any(np.any(np.asarray(a) == UNDEF) for a in case["args"] if isinstance(a, np.ndarray)), case["label"]
    for key, combos in seen.items():
        assert {c[0] for c in combos} == {True, False}, key
        if "-flag" not in key:
            assert {c[1] for c in combos} == {cases.ALL_DEFINED, cases.SOME_DEFINED}, key


def test_libm_class_restatement_is_within_one_ulp_of_float64(oracle):
    n_cases = 0
    for case in sc.family("libm"):
        assert case["op"] in sc.LIBM_OPS
        ok, out, _ = _run(oracle, case)
        assert ok
        check_against_float64(case, out, out, "restatement")
        n_cases += 1
    assert n_cases >= 60


def _first(family, label):
    found = [c for c in sc.family(family) if c["label"] == label]
    assert len(found) == 1, label
    return found[0]


def test_every_table_knot_and_both_validity_ends_are_hit(oracle):
    case = _first("table", "seam-plevelhum1-body-all")
    tk = np.asarray(case["args"][0], F).ravel()
    x = (((tk - F(273.15)).astype(np.float64) + 100.0) * 0.2).astype(F)  # MetConstants.h:65, restated here
    ok, out, flag = _run(oracle, case)
    out = out.ravel()
    assert ok and flag == cases.SOME_DEFINED
    for k in range(0, 41):
        hit = np.nonzero(x == F(k))[0]
        assert hit.size, "knot %d is not hit exactly" % k
        assert np.all((out[hit] != UNDEF) == (k < 40)), k
    for end, inside in ((-1, +1), (40, -1)):
        i = np.nonzero(x == F(end))[0]
        assert i.size and np.all(out[i] == UNDEF), end
        nb = np.nonzero(x == np.nextafter(F(end), F(end + inside)))[0]
        if not nb.size:  # the neighbouring Kelvin input moves x by more than one float
            nb = np.nonzero((x - F(end)) * inside > 0)[0]
            nb = nb[np.argsort(np.abs(x[nb] - F(end)))[:1]]
        assert nb.size and np.all(out[nb] != UNDEF), end
        outside = np.nonzero(((x - F(end)) * inside < 0) & (np.abs(x - F(end)) < 1e-4))[0]
        assert outside.size and np.all(out[outside] == UNDEF), end
    for v in (np.nan, np.inf, -np.inf):
        i = np.nonzero(np.isnan(tk) if np.isnan(v) else tk == v)[0]
        assert i.size and np.all(out[i] == UNDEF), v


def test_inverse_lookup_is_asked_for_every_table_entry_exactly(oracle):
    """Dew point from a humidity that makes e equal a table entry: the result is that entry's temperature, exactly."""
    case = _first("inverse", "seam-cvhum3-inverse-body-all")
    tc, rh = (np.asarray(a, F).ravel() for a in case["args"][:2])
    ok, out, _ = _run(oracle, case)
    out = out.ravel()
    x = ((tc.astype(np.float64) + 100.0) * 0.2).astype(F)
    inside = (x > -1) & (x < 40) & ~np.isnan(rh)
    r = np.clip((0.01 * rh.astype(np.float64)).astype(F), F(0.02), F(1.0))
    l = np.clip(x.astype(np.int64), 0, 39)
    et = (sc.EWT[l] + (sc.EWT[l + 1] - sc.EWT[l]) * (x - l.astype(F))).astype(F)
    etd = (r * et).astype(F)
    for m in range(0, 40):
        hit = np.nonzero(inside & (etd == sc.EWT[m]))[0]
        assert hit.size, "no cell has e == ewt[%d]" % m
        assert np.all(out[hit] == F(-100.0 + 5.0 * m)), m
        if m < 39:
            assert np.any(inside & (etd == np.nextafter(sc.EWT[m], F(0)))) and np.any(inside & (etd == np.nextafter(sc.EWT[m], F(np.inf)))), m
    for b in range(-14, 10):
        p = F(2.0) ** F(b)
        assert np.any(inside & (etd == p)) and np.any(inside & (etd == np.nextafter(p, F(0)))) and np.any(inside & (etd == np.nextafter(p, F(np.inf)))), b
    for v in (2.0, 100.0):
        assert np.any(rh == F(v)) and np.any(rh == np.nextafter(F(v), F(0))) and np.any(rh == np.nextafter(F(v), F(1000)))


def test_flight_level_at_each_table_pressure(oracle):
    case = _first("flightlevel", "seam-pressure2FlightLevel-body-all")
    p = np.asarray(case["args"][0], F).ravel()
    ok, out, flag = _run(oracle, case)
    out = out.ravel()
    assert ok
    for pk, fk in zip(sc.PLEVELTABLE, sc.FLEVELTABLE):
        i = np.nonzero(p == pk)[0]
        assert i.size and np.all(out[i] == fk), pk
        assert np.any(p == np.nextafter(pk, F(0))) and np.any(p == np.nextafter(pk, F(1e9)))
    assert np.all(out[p > 1000] == F(5)) and np.all(out[(p < 10) & ~np.isnan(p)] == F(1020))


def test_every_class_and_both_range_ends_of_values2classes(oracle):
    for tag, limits in zip(("six", "two"), sc.CLASS_LIMITS):
        case = _first("classes", "seam-values2classes-%s-body-all" % tag)
        f = np.asarray(case["args"][0], F).ravel()
        ok, out, _ = _run(oracle, case)
        out = out.ravel()
        assert ok
        defined = out != UNDEF
        assert set(out[defined].tolist()) == set(float(k) for k in range(max(1, len(limits) - 2))), tag
        for v in limits:
            assert np.any(f == F(v)) and np.any(f == np.nextafter(F(v), F(-1e9))) and np.any(f == np.nextafter(F(v), F(1e9)))
        assert np.all(defined[f == F(limits[0])]) and not np.any(defined[f == F(limits[-1])])  # [fmin, fmax)
        assert not np.any(defined[f == np.nextafter(F(limits[0]), F(-1e9))]) and np.all(defined[f == np.nextafter(F(limits[-1]), F(-1e9))])


def test_every_mertins_class_and_both_sides_of_the_icing_gates(oracle):
    cs = sc.icing_cases(oracle)  # the generator's own assertion
    case = [c for c in cs if c["label"] == "seam-vesselIcingMertins-body-all"][0]
    ok, out, _ = _run(oracle, case)
    out = out.ravel()
    for v in sc.MERTINS_CLASSES:
        assert np.any(out == F(v)), v
    ice = np.asarray(case["args"][5], F).ravel()
    assert np.all(out[ice == F(0.4)] == UNDEF)  # 0.4f > 0.4: the compare is in double
    assert np.all(out[ice == np.nextafter(F(0.4), F(0))] != UNDEF)


def test_both_outcomes_of_each_undercooled_rain_threshold(oracle):
    case = _first("undercooled", "seam-underCooledRain-body-all")
    precip, snow, tk = (np.asarray(a, F).ravel() for a in case["args"][:3])
    ok, out, _ = _run(oracle, case)
    out = out.ravel()
    a = precip >= F(sc.UCR["precipMin"])
    b = tk <= F(F(sc.UCR["tcMax"]) + F(273.15))
    c = snow <= (precip * F(sc.UCR["snowRateMax"])).astype(F)
    assert np.array_equal(out == 1, a & b & c) and np.array_equal(out == 0, ~(a & b & c))
    for only_this_fails in (~a & b & c, a & ~b & c, a & b & ~c):
        assert np.any(only_this_fails)
    assert np.any(a & b & c & (precip == F(sc.UCR["precipMin"])) & (tk == F(F(sc.UCR["tcMax"]) + F(273.15))) & (snow == (precip * F(sc.UCR["snowRateMax"])).astype(F)))
