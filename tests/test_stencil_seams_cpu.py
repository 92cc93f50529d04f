"""tests/stencil_seam_cases.py on the CPU: the cases reach what they are built to reach (a condition of the generator, not a
measurement -- a case that degrades into comparing NaN with NaN fails here), and on every case the oracle equals the compiled
reference bit for bit, flags and return values included, where oracle/_ref is built.  That ties the yardstick of
tests/test_gpu_stencil_seams.py to the reference at these inputs.  -s prints the table of result classes per operator."""
import numpy as np
import pytest

import cases
import stencil_seam_cases as sc

MIN_CELLS = 8
MIN_GOOD = 0.30


def _results(oracle, op, nx):
    out = []
    for case in sc.cases_for(op, nx):
        outs, flags, ok = sc.expect(oracle, case)
        assert ok, case["label"]
        out.append((case, outs, flags))
    return out


@pytest.mark.parametrize("nx", sc.NX_FORMS)
@pytest.mark.parametrize("op", sorted(sc.OPS))
def test_cases_reach_the_ends_of_the_range(oracle, op, nx):
    """Per case at least 30 % of the oracle's interior results are finite, non-zero and not undef; over an operator's cases
    +inf, -inf, NaN, +0, -0, a finite value above 1e30 and a denormal each occur in at least 8 interior cells (but for what the
    operator's arithmetic cannot produce, sc.EXEMPT)."""
    total = dict.fromkeys(sc.CLASSES, 0)
    rows = []
    for case, outs, flags in _results(oracle, op, nx):
        good = cells = 0
        per_case = dict.fromkeys(sc.CLASSES, 0)
        for l in range(case["nlev"]):
            if case["flags"][l] == sc.ALL_DEFINED and case["undef"] == case["undef"]:
                assert not any(np.any(f[l] == case["undef"]) for f in case["fields"]), case["label"]
            for o in outs[l]:
                counts, g, n = sc.classify_results(o, case["undef"])
                good += g
                cells += n
                for k, v in counts.items():
                    per_case[k] += v
                    total[k] += v
        rows.append("%-62s %5.1f %%   %s" % (case["label"], 100.0 * good / cells, "  ".join("%s %d" % kv for kv in per_case.items())))
        assert good >= MIN_GOOD * cells, (case["label"], good, cells)
    print("\n".join(rows))
    print("%-62s           %s" % (op + " over its cases", "  ".join("%s %d" % kv for kv in total.items())))
    for k, v in total.items():
        if k not in sc.EXEMPT.get(op, ()):
            assert v >= MIN_CELLS, (op, nx, k, v)


@pytest.mark.parametrize("nx", sc.NX_FORMS)
@pytest.mark.parametrize("op", sc.GEOSTROPHIC)
def test_geostrophic_cases_divide_by_every_kind_of_coriolis_parameter(op, nx):
    """Interior cells with fcoriolis == 0 under a non-zero and under a zero numerator, with a denormal and with an infinite
    fcoriolis: at least 8 each over the operator's cases (cells whose stencil holds an undefined value on a tested level do
    not count: the division is not done there)."""
    seen = dict.fromkeys(("zero, numerator not", "zero, numerator too", "denormal", "infinite"), 0)
    for case in sc.cases_for(op, nx):
        z, fc = case["fields"][0], sc.interior(case["fc"])
        for l in range(case["nlev"]):
            f = z[l]
            with np.errstate(all="ignore"):
                dx, dy = f[1:-1, 2:] - f[1:-1, :-2], f[2:, 1:-1] - f[:-2, 1:-1]
                lap = (f[1:-1, 2:] - 2.0 * f[1:-1, 1:-1].astype(np.float64) + f[1:-1, :-2]) + (f[2:, 1:-1] - 2.0 * f[1:-1, 1:-1].astype(np.float64) + f[:-2, 1:-1])
            bad = np.isnan(f) | (f == case["undef"])
            used = ~(bad[1:-1, 2:] | bad[1:-1, :-2] | bad[2:, 1:-1] | bad[:-2, 1:-1] | bad[1:-1, 1:-1]) if case["flags"][l] != sc.ALL_DEFINED else np.ones_like(dx, bool)
            num = {"plevelgwind_xcomp": dy, "plevelgwind_ycomp": dx, "plevelgvort": lap}.get(op)
            nonzero = (num != 0) if num is not None else ((dx != 0) | (dy != 0))
            zero = (num == 0) if num is not None else ((dx == 0) & (dy == 0))
            seen["zero, numerator not"] += int(np.count_nonzero(used & (fc == 0) & nonzero))
            seen["zero, numerator too"] += int(np.count_nonzero(used & (fc == 0) & zero))
            seen["denormal"] += int(np.count_nonzero(used & (fc != 0) & (np.abs(fc) < sc.FLT_MIN)))
            seen["infinite"] += int(np.count_nonzero(used & np.isinf(fc)))
    for k, v in seen.items():
        assert v >= MIN_CELLS, (op, nx, k, v)


@pytest.mark.parametrize("nx", sc.NX_FORMS)
def test_thermal_front_parameter_divides_by_zero_and_infinite_gradients(oracle, nx):
    """|grad t|, the divisor of thermalFrontParameter's second pass, is zero (the plateau: rejected whatever the flag says) and
    infinite in at least 8 interior cells each over the operator's cases."""
    zero = infinite = 0
    for case in sc.cases_for("thermalFrontParameter", nx):
        for l in range(case["nlev"]):
            ok, g, _ = oracle.call("gradient", nx, case["ny"], case["fields"][0][l], case["xm"], case["ym"], 3, fdefined=int(case["flags"][l]),
                                   undef=case["undef"])
            assert ok
            zero += int(np.count_nonzero(sc.interior(g) == 0))
            infinite += int(np.count_nonzero(np.isinf(sc.interior(g))))
    assert zero >= MIN_CELLS and infinite >= MIN_CELLS, (nx, zero, infinite)


def test_cases_are_deterministic_and_labelled():
    a = sc.make_case("jacobian", "huge", 68)
    b = sc.make_case("jacobian", "huge", 68)
    assert all(cases.same_bits(x, y) for x, y in zip(a["fields"] + [a["xm"], a["ym"], a["fc"]], b["fields"] + [b["xm"], b["ym"], b["fc"]]))
    labels = [c["label"] for op in sc.OPS for nx in sc.NX_FORMS for c in sc.cases_for(op, nx)]
    assert len(set(labels)) == len(labels)
    for op in sc.OPS:
        cs = sc.cases_for(op, 68)
        assert {c["maps"] for c in cs} == {"some", "all", "none"}, op
        assert sum(1 for c in cs if c["undef"] != c["undef"]) == 1, op
        assert all(list(c["flags"]) == [sc.ALL_DEFINED, sc.SOME_DEFINED, sc.SOME_DEFINED] for c in cs)
        # the equator: a whole row of +0
        assert all(np.all(c["fc"][c["ny"] // 2] == 0) and not np.any(np.signbit(c["fc"][c["ny"] // 2])) for c in cs)


@pytest.mark.parametrize("nx", sc.NX_FORMS)
@pytest.mark.parametrize("op", sorted(sc.OPS))
def test_oracle_equals_the_reference_on_every_seam_case(oracle, ref, op, nx):
    """Outputs bit for bit (NaN for NaN), flags and return values."""
    for case in sc.cases_for(op, nx):
        o_out, o_flags, o_ok = sc.expect(oracle, case)
        r_out, r_flags, r_ok = sc.expect(ref, case)
        assert o_ok == r_ok, case["label"]
        assert o_flags == r_flags, (case["label"], o_flags, r_flags)
        for l in range(case["nlev"]):
            for k, (a, b) in enumerate(zip(o_out[l], r_out[l])):
                assert cases.same_bits(a, b, nan_payload=False), (case["label"], l, k)
