"""The scaled and special cases of mifc_vparcel_* (tests/vparcel_range_cases.py) on the CPU, from the restatement alone:
every scale puts the levels of one column on both sides of the seam it is named for; the conditions on the inputs hold (at
most 2 % of a case's cells unstable, no output wholly undef except where the physics says so); and for every seam, which of
the named mistakes of tests/vparcel_restate.py the cases can see -- a stable value moved beyond the bound that
tests/test_gpu_vparcel_range.py holds the kernel to, or an undef cell that changes -- and which they cannot.  A seam that no
mistake makes visible is reached, not covered: DESIGN.md lists it so."""
import numpy as np
import pytest

import vparcel_cases as vc
import vparcel_range_cases as vr
import vparcel_restate as vp

F = np.float32
U = vp.UNDEF
QSAT_RCP, A1_RCP, POW_2ULP, QSAT_FLUSH = vp.MISTAKES

# scale -> mistake -> outputs in which it shows (an empty tuple: reached, not observable), as the restatement gives it.
# The low side (the parcel has latent heat) sees a wrong quotient by p in CAPE.  The high side has no LFC: a wrong quotient
# by p moves nothing there (p_b = 2^40 is reached, not observable), a flushed qsat moves the LCL.  The power two ulp off shows
# where the end of the fast domain lies INSIDE the walk (s = -32, 32: one point of a step is moved, the other is not, and the
# ratio pi_k / pi_k-1 changes); where every point lies beyond it the shift cancels in the ratio up to rounding (s = -49 and
# 78 catch such a rounding, s = +-96 do not: the second rescaling is reached, not observable).  a1 enters only through
# 1 + a1 * a2 in double: a last-bit error of it is never seen (cplr * qcl = 2^+-64: reached, not observable).
OBSERVABLE = {
    "s-96": {QSAT_RCP: ("cape",), A1_RCP: (), POW_2ULP: (), QSAT_FLUSH: ()},
    "s-49": {QSAT_RCP: ("cape",), A1_RCP: (), POW_2ULP: ("cape",), QSAT_FLUSH: ()},
    "s-32": {QSAT_RCP: ("cape",), A1_RCP: (), POW_2ULP: ("plcl",), QSAT_FLUSH: ()},
    "s31": {QSAT_RCP: (), A1_RCP: (), POW_2ULP: (), QSAT_FLUSH: ()},
    "s32": {QSAT_RCP: (), A1_RCP: (), POW_2ULP: ("plcl",), QSAT_FLUSH: ()},
    "s78": {QSAT_RCP: (), A1_RCP: (), POW_2ULP: ("plcl",), QSAT_FLUSH: ()},
    "s96": {QSAT_RCP: (), A1_RCP: (), POW_2ULP: (), QSAT_FLUSH: ()},
    "s116": {QSAT_RCP: (), A1_RCP: (), POW_2ULP: (), QSAT_FLUSH: ("plcl",)},
    "pa": {QSAT_RCP: (), A1_RCP: (), POW_2ULP: (), QSAT_FLUSH: ()},
}


def clean(scale=None):
    return [c for c in vr.cases() if not c["name"].endswith("_special") and (scale is None or c["scale"] == scale)]


def test_shapes_directions_and_sources():
    mine = clean()
    assert {(c["nlev"], c["ny"], c["nx"]) for c in mine} == {(7, 9, 16), (12, 9, 13), (7, 10, 206)}
    assert {c["from"] for c in mine} == {"first", "last"} and {c["source"] for c in mine} == set(vc.SOURCES)
    assert {c["scale"] for c in mine} == set(vr.SCALES) == set(OBSERVABLE)
    for scale in vr.SCALES:
        assert len(clean(scale)) >= 2, scale
    special = [c for c in vr.cases() if c["name"].endswith("_special")]
    assert len(special) == len(vr.SPECIAL_SCALES) and len(vr.cases()) == len(mine) + len(special)


def test_the_unscaled_generator_is_unchanged():
    """factor = 1 is the default: a case of tests/vparcel_cases.py made with it explicitly has the same bits."""
    a, b = vc.make(7, 9, 16, "first", "planes"), vc.make(7, 9, 16, "first", "planes", factor=1.0)
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v.view(np.uint32) if v.dtype == np.float32 else v, b[k].view(np.uint32) if v.dtype == np.float32 else b[k]), k


@pytest.mark.parametrize("scale", [s for s in vr.SCALES if s != "pa"])
def test_the_levels_of_one_column_straddle_the_seam(scale):
    s = int(scale[1:])
    for c in clean(scale):
        p = vp.hybrid_pressure(c["ps"], c["al"], c["bl"])
        p = np.where(np.isnan(p).any(axis=0)[None], F(1.0), p)  # (a column without pressure straddles nothing)
        x = (p * vp.P0INV).astype(F)
        lo, hi, xlo, xhi = p.min(axis=0), p.max(axis=0), x.min(axis=0), x.max(axis=0)
        across = lambda a, b, seam: bool(((a < F(seam)) & (b >= F(seam))).any())  # noqa: E731  (in some column)
        if s in (-96, -32, 32, 96):  # the domains of pow_kappa and of its second rescaling
            assert across(xlo, xhi, 2.0 ** s), c["name"]
        if s == -49:  # p_b = 2^-40; cplr * qcl = 2^64
            q = c["q_src"][(c["q_src"] != U) & ~np.isnan(c["q_src"])]
            assert across(lo, hi, 2.0 ** -40) and ((vp.CPLR * q).astype(F) < F(2.0 ** 64)).any() and ((vp.CPLR * q).astype(F) >= F(2.0 ** 64)).any(), c["name"]
        if s == 31:
            assert across(lo, hi, 2.0 ** 40), c["name"]
        if s == 78:
            q = c["q_src"][(c["q_src"] != U) & ~np.isnan(c["q_src"])]
            assert ((vp.CPLR * q).astype(F) < F(2.0 ** -64)).any() and ((vp.CPLR * q).astype(F) >= F(2.0 ** -64)).any(), c["name"]
        if s == 116:  # qsat on both sides of FLT_MIN
            ok, qsat = vp.sat_test((vp.CP * c["t"]).astype(F), p)
            qsat = qsat[ok & (qsat > 0)]
            assert (qsat < np.finfo(F).tiny).any() and (qsat >= np.finfo(F).tiny).any(), c["name"]


@pytest.mark.parametrize("name", vr.case_names())
def test_conditions_on_the_inputs(name):
    """At most 2 % of the cells unstable (the condition of tests/test_vparcel_cpu.py); no output wholly undef, except cin,
    plfc and pel on the high side, where a parcel without latent heat has no LFC; the clean cases make no NaN and no
    infinity; the low side keeps the shares of the ordinary cases (most cells have CAPE, an LCL, an LFC)."""
    c = vr.by_name(name)
    special = name.endswith("_special")
    for form in vc.FORMS:
        ref = vr.reference(name, form)
        assert (~ref.stable).mean() <= 0.02, (name, form, float((~ref.stable).mean()))
        r0 = ref.r0
        shares = {n: float((r0[n] != U).mean()) for n in vp.OUTPUTS}
        print("%-36s %s unstable %.3f adjusted %.2f defined %s" % (name, form, (~ref.stable).mean(), ref.diag["adjusted"].mean(), {n: round(v, 2) for n, v in shares.items()}))
        low = c["scale"] in vr.LOW_SIDE or c["scale"] is None
        for n in vp.OUTPUTS:
            if low and n != "pel" or n in ("cape", "plcl", "tparcel"):
                assert shares[n] > 0.1, (name, form, n, shares)
        if low and not special:
            assert shares["cape"] > 0.85 and shares["plcl"] > 0.7 and shares["plfc"] > 0.55 and ref.diag["adjusted"].mean() > 0.25, (name, form, shares)
        if not special:
            assert all(np.isfinite(r0[n]).all() for n in vp.OUTPUTS), (name, form)


def test_the_special_cases_hold_the_specials():
    edges = vr.table_edge_temperatures()
    ok = vp.sat_test((vp.CP * edges).astype(F), np.full(4, 1000.0, F))[0]
    assert list(ok) == [False, True, True, False] and np.nextafter(edges[0], edges[1]) == edges[1] and np.nextafter(edges[2], edges[3]) == edges[3]
    for c in vr.cases():
        if not c["name"].endswith("_special"):
            continue
        t = c["t"]
        for v in list(edges) + [0.0, vr.DENORM_MIN, -vr.DENORM_MIN, vr.FLT_MAX, -vr.FLT_MAX, np.inf, -np.inf, vr.UNDEF_BELOW, vr.UNDEF_ABOVE]:
            assert (t == F(v)).any(), (c["name"], v)
        on_all = np.broadcast_to((c["fdefined_in"] == vp.ALL_DEFINED)[:, None, None], t.shape)
        assert (t[on_all] == U).any() and np.isnan(t[on_all]).any(), c["name"]  # values there
        p_all = np.broadcast_to((c["fdef_coord"] == vp.ALL_DEFINED)[:, None, None], c["p"].shape)
        assert (c["p"][p_all] == U).any() and np.isnan(c["p"][p_all]).any(), c["name"]
        for key in ("q_src", "ps", "p") + (("t_src", "p_src") if c["source"] == "planes" else ()):
            a = c[key]
            plain = vc.make(c["nlev"], c["ny"], c["nx"], c["from"], c["source"], factor=1.0 if c["scale"] is None else vr.SCALES[c["scale"]])[key]
            share = float((a.view(np.uint32) != plain.view(np.uint32)).mean())
            assert (0.015 < share < 0.08) if a.ndim == 3 else (0 < share < 0.12), (c["name"], key, share)  # (a plane has some hundred cells)
            assert a.ndim == 2 or np.isinf(a).any() or (np.abs(a) == vr.FLT_MAX).any(), (c["name"], key)


def moved(c, form, ref, mistake):
    """The outputs in which the mistake moves a stable value beyond the bound, or changes an undef cell."""
    with vp.mistaken(mistake):
        r = vc.run_restatement(c, form)
    seen = []
    for n in vp.OUTPUTS:
        e, g = ref.r0[n], r[n]
        st = ref.stable if e.ndim == 2 else np.broadcast_to(ref.stable, e.shape)
        m = st & (e != U) & (g != U)
        with np.errstate(all="ignore"):
            beyond = ~(np.abs(g.astype(np.float64) - e.astype(np.float64))[m] <= ref.bound(n)[m])
        if beyond.any() or ((g == U) != (e == U))[st].any():
            seen.append(n)
    return seen


@pytest.mark.parametrize("scale", list(vr.SCALES))
def test_which_mistakes_the_cases_of_a_seam_can_see(scale):
    for mistake in vp.MISTAKES:
        seen = set()
        for c in clean(scale):
            for form in vc.FORMS:
                seen |= set(moved(c, form, vr.reference(c["name"], form), mistake))
        want = OBSERVABLE[scale][mistake]
        print("%-5s %-45s moves %s" % (scale, mistake, sorted(seen) or "nothing"))
        if want:
            assert set(want) <= seen, (scale, mistake, sorted(seen))
        else:
            assert not seen, (scale, mistake, sorted(seen), "has become observable: say so in OBSERVABLE and in DESIGN.md")


def test_the_correct_restatement_moves_nothing():
    """`moved` on the restatement itself: what the test above sees is the mistake."""
    for c in clean("s-49") + clean("s116"):
        for form in vc.FORMS:
            ref = vr.reference(c["name"], form)
            r = vc.run_restatement(c, form)
            assert all(np.array_equal(r[n].view(np.uint32), ref.r0[n].view(np.uint32)) for n in vp.OUTPUTS)
    assert not vp._mistakes
