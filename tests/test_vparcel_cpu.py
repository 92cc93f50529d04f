"""CPU checks of mifc_vparcel_hlevels / mifc_vparcel_fields / mifc_vparcel_levels: the step arithmetic of their numpy
restatement (tests/vparcel_restate.py, the oracle of the GPU tests) against the compiled reference's showalterIndex, the
semantics on hand-worked columns, the stability of the shared cases under one-ulp changes of pi (the condition the GPU
tolerance rests on), that the entries are declared, bound and configured where the others are, and the front's
marshalling against a recording stub library."""
import ctypes
import glob
import math
import os
import re

import numpy as np
import pytest

import vparcel_cases as vc
import vparcel_restate as vp
from test_python_front_cpu import _data, _stub_context

F, D = np.float32, np.float64
U = vp.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, S_, N = vp.ALL_DEFINED, vp.SOME_DEFINED, vp.NONE_DEFINED


# ------------------------------------------------------------------------------------ the step is the reference's
def test_adjustment_is_showalterindex_bit_for_bit(ref):
    """showalterIndex (FieldCalculations.cc:872) lifts t850 dry to p500 and runs the seven trips there.  Fed the same
    tcl0, qcl and p, the restatement's adjust() must give the same tk500 - tcl / cp, bit for bit: 4 096 seeded cells and
    two pairs of levels, the cold ones leaving the table in the first trip (the reference's `break`)."""
    powf = ctypes.CDLL("libm.so.6").powf
    powf.restype, powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    pi = lambda p: F(vp.CP * F(powf(float(F(p) * vp.P0INV), float(vp.KAPPA))))  # noqa: E731  pi_from_p with the reference's powf
    rng = np.random.default_rng(5)
    ny, nx = 64, 64
    broke = 0
    for p500, p850 in ((500.0, 850.0), (300.0, 925.0)):
        t850 = rng.uniform(169.0, 312.0, (ny, nx)).astype(F)
        t500 = rng.uniform(200.0, 280.0, (ny, nx)).astype(F)
        rh850 = rng.uniform(0.0, 110.0, (ny, nx)).astype(F)
        ok, out, flag = ref.call("showalterIndex", nx, ny, t500, t850, rh850, p500, p850, 1)
        assert ok
        pi500, pi850 = pi(p500), pi(p850)
        dryadiabat = F(F(vp.CP * F(vp.CP / pi850)) * F(pi500 / vp.CP))  # :913
        rh = np.clip((0.01 * rh850.astype(D)).astype(F), F(0.02), F(1.0))
        x = vp.ewt_x(t850 - vp.T0)
        defined = (x > F(-1.0)) & (x < F(40.0))
        etd = (vp.ewt_value(np.where(defined, x, F(0.0))) * rh).astype(F)
        tcl0 = (dryadiabat * t850).astype(F).ravel()
        qcl0 = ((vp.EPS * etd).astype(F) / F(p850)).astype(F).ravel()
        pp = np.full(tcl0.shape, F(p500), F)
        first_ok, _ = vp.sat_test(tcl0, pp)
        broke += int((~first_ok & defined.ravel()).sum())
        tcl, qcl = vp.adjust(tcl0, qcl0, pp, np.ones(tcl0.shape, bool))
        mine = np.where(defined.ravel(), (t500.ravel() - (tcl / vp.CP).astype(F)).astype(F), U).reshape(ny, nx)
        assert (out == U).sum() == (~defined).sum()
        assert mine.tobytes() == out.tobytes(), int((mine.view(np.uint32) != out.view(np.uint32)).sum())
        assert (tcl[first_ok] != tcl0[first_ok]).any()
    assert broke > 50, broke


# ------------------------------------------------------------------------------------------- hand-worked columns
def column(p, t, q, **kw):
    """One column (ny = nx = 1), the pressure as a batch: the restatement's dict with scalars and tparcel[nlev]."""
    p, t = np.asarray(p, F), np.asarray(t, F)
    d = {}
    r = vp.fields(t[:, None, None], p[:, None, None], np.full((1, 1), q, F), diag=d, **kw)
    out = {n: (r[n][:, 0, 0] if n == "tparcel" else r[n][0, 0]) for n in vp.OUTPUTS}
    out["flags"], out["diag"] = r["flags"], {k: (v[:, 0, 0] if v.ndim == 3 else int(v[0, 0])) for k, v in d.items()}
    return out


P5 = [1000.0, 900.0, 750.0, 600.0, 450.0]


def test_dry_adiabatic_environment_has_no_buoyancy_below_the_lcl():
    dry = column(P5, [300.0] * 5, 1e-9)  # a parcel that never saturates: its curve is the dry adiabat through (1000 hPa, 300 K)
    assert dry["diag"]["lcl_pos"] == -1 and not dry["diag"]["adjusted"].any()
    assert dry["cape"] == 0 and not np.signbit(dry["cape"]) and dry["cin"] == U and dry["plcl"] == U and dry["plfc"] == U and dry["pel"] == U
    assert dry["flags"]["cape"] == A and dry["flags"]["cin"] == N and (dry["flags"]["tparcel"] == A).all()
    env = dry["tparcel"].copy()
    theta = env * (F(1000.0) / np.asarray(P5, F)) ** vp.KAPPA
    assert np.allclose(theta, 300.0, atol=2e-3)
    moist = column(P5, env, 0.008)  # the same environment: B is exactly zero at every point below the condensation level
    j = moist["diag"]["lcl_pos"]
    assert j == 2 and 750.0 < moist["plcl"] < 900.0, (j, moist["plcl"])
    assert moist["tparcel"][:j].tobytes() == env[:j].tobytes()
    assert (moist["tparcel"][j:] > env[j:]).all()  # above it the parcel follows the moist adiabat: warmer than the dry one
    assert moist["plfc"] == moist["plcl"] and moist["cin"] == 0 and moist["pel"] == U and moist["cape"] > 0  # B(LCL) > 0; B > 0 at the top


def test_isothermal_column_has_no_lfc():
    r = column(P5, [288.0] * 5, 0.009)
    assert r["diag"]["lcl_pos"] >= 1 and r["plcl"] != U and r["diag"]["lfc_pos"] == -1
    assert r["cape"] == 0 and not np.signbit(r["cape"]) and r["cin"] == U and r["plfc"] == U and r["pel"] == U
    assert (r["tparcel"][1:] < F(288.0)).all() and r["tparcel"][0] == (vp.CP * F(288.0)) / vp.CP
    assert r["flags"] == {**r["flags"], "cape": A, "cin": N, "plcl": A, "plfc": N, "pel": N}


def test_three_levels_by_hand():
    """Source saturated at 1000 hPa (the LCL is the source, B = 0 there), then 800 and 600 hPa with the environment 2 K
    warmer than the parcel at 800 (B1 ~ -2) and 3 K colder at 600 (B2 ~ +3).  With l = ln p:
      piece 0 -> 1: both B <= 0:   cin += (0 + B1) / 2 * (l0 - l1)
      piece 1 -> 2: up, w0 = B1 / (B1 - B2) ~ 0.4: the LFC at l1 + w0 (l2 - l1);
                    cin += B1 / 2 * w0 (l1 - l2), cape = B2 / 2 * (1 - w0) (l1 - l2)
      B2 > 0 at the last point: no EL.   cape and cin times Rd = 287."""
    p = [1000.0, 800.0, 600.0]
    first = column(p, [290.0, 250.0, 250.0], 0.05)
    tp = first["tparcel"]
    t = np.array([290.0, tp[1] + F(2.0), tp[2] - F(3.0)], F)
    r = column(p, t, 0.05)
    assert r["tparcel"].tobytes() == tp.tobytes() and r["diag"]["adjusted"].tolist() == [False, True, True]
    B1, B2 = float(tp[1]) - float(t[1]), float(tp[2]) - float(t[2])
    assert abs(B1 + 2) < 1e-4 and abs(B2 - 3) < 1e-4
    l0, l1, l2 = (math.log(x) for x in p)
    w0 = B1 / (B1 - B2)
    cin = 287.0 * ((0.0 + B1) * 0.5 * (l0 - l1) + B1 * 0.5 * (w0 * (l1 - l2)))
    cape = 287.0 * (B2 * 0.5 * ((1 - w0) * (l1 - l2)))
    assert r["plcl"] == F(1000.0) and r["diag"]["lcl_pos"] == 0 and r["diag"]["lfc_pos"] == 2
    assert r["cin"] == pytest.approx(cin, rel=1e-6) and r["cin"] < 0 and r["cape"] == pytest.approx(cape, rel=1e-6) and cape > 0
    assert r["plfc"] == pytest.approx(math.exp(l1 + w0 * (l2 - l1)), rel=1e-6) and 600 < r["plfc"] < 800
    assert r["pel"] == U and r["flags"]["pel"] == N
    # one more level, colder parcel: the EL between 600 and 450 hPa, and CAPE gains the triangle below it
    tp4 = column(p + [450.0], list(t) + [250.0], 0.05)["tparcel"]
    r4 = column(p + [450.0], list(t) + [tp4[3] + F(1.0)], 0.05)
    B3 = float(tp4[3]) - float(F(tp4[3] + F(1.0)))
    l3 = math.log(450.0)
    w1 = B2 / (B2 - B3)
    assert r4["pel"] == pytest.approx(math.exp(l2 + w1 * (l3 - l2)), rel=1e-6) and r4["diag"]["el_pos"] == 3
    assert r4["cape"] == pytest.approx(cape + 287.0 * (B2 * 0.5 * (w1 * (l2 - l3))), rel=1e-6) and r4["cin"] == r["cin"] and r4["plfc"] == r["plfc"]


def test_holes_and_the_source():
    base = dict(p=[1000.0, 850.0, 700.0, 500.0], t=[295.0, 285.0, 275.0, 255.0], q=0.012)
    good = column(**base)
    assert (good["tparcel"] != U).all() and good["cape"] != U
    for what, change in (("undef t", dict(t=[295.0, 285.0, U, 255.0])), ("NaN t", dict(t=[295.0, 285.0, np.nan, 255.0])),
                         ("pressure not falling", dict(p=[1000.0, 850.0, 850.0, 500.0])), ("NaN pressure", dict(p=[1000.0, 850.0, np.nan, 500.0])),
                         ("undef pressure", dict(p=[1000.0, 850.0, U, 500.0]))):
        r = column(**dict(base, **change))
        assert r["tparcel"][:2].tobytes() == good["tparcel"][:2].tobytes() and (r["tparcel"][2:] == U).all(), what  # undef from the hole on
        assert all(r[n] == U for n in vc.PLANES) and all(r["flags"][n] == N for n in vc.PLANES), what
    r = column(**dict(base, t=[295.0, 285.0, U, 255.0]), fdefined_in=A)  # a stored undef under ALL_DEFINED is a (very warm) value
    assert (r["tparcel"] != U).all() and r["cape"] != U
    for what, change in (("undef humidity", dict(q=U)), ("NaN humidity", dict(q=np.nan)), ("undef source level", dict(t=[U, 285.0, 275.0, 255.0])),
                         ("a source outside the table", dict(t=[400.0, 285.0, 275.0, 255.0]))):
        r = column(**dict(base, **change))
        assert (r["tparcel"] == U).all() and all(r[n] == U for n in vc.PLANES), what
    # the walk from the last level is the same column stored upside down; a source in mid-column leaves the levels in front alone
    down = column(base["p"][::-1], base["t"][::-1], base["q"], from_="last", src_level=3)
    assert down["tparcel"][::-1].tobytes() == good["tparcel"].tobytes() and all(down[n] == good[n] for n in vc.PLANES)
    mid = column(base["p"], base["t"], base["q"], src_level=1)
    assert mid["tparcel"][0] == U and mid["tparcel"][1] == (vp.CP * F(285.0)) / vp.CP and mid["flags"]["tparcel"].tolist() == [N, A, A, A]
    # a source given by planes: the walk begins at the first pressure below p_src
    plane = lambda v: np.full((1, 1), v, F)  # noqa: E731
    pl = column(base["p"], base["t"], base["q"], src_level=None, t_src=plane(290.0), p_src=plane(900.0))
    assert (pl["tparcel"][:1] == U).all() and (pl["tparcel"][1:] != U).all()
    same = column(base["p"], base["t"], base["q"], src_level=None, t_src=plane(285.0), p_src=plane(850.0))  # 850 is not below 850
    assert same["tparcel"][1] == U and same["tparcel"][2:].tobytes() == mid["tparcel"][2:].tobytes() and same["cape"] == mid["cape"]
    leaves = column([1000.0, 500.0, 100.0], [250.0, 230.0, 210.0], 1e-6)  # 250 K lifted dry to 100 hPa is below the table
    assert leaves["tparcel"][1] != U and leaves["tparcel"][2] == U and leaves["cape"] == U


def test_hybrid_and_levels_forms_state_their_pressure():
    t = np.full((3, 1, 2), 280.0, F)
    ps = np.array([[1000.0, U]], F)
    r = vp.hlevels(t, ps, [0.0, 50.0, 100.0], [1.0, 0.7, 0.3], np.full((1, 2), 0.004, F))
    f = vp.fields(t, np.array([1000.0, 750.0, 400.0], F)[:, None, None] * np.ones((1, 1, 2), F), np.full((1, 2), 0.004, F))
    assert r["tparcel"][:, 0, 0].tobytes() == f["tparcel"][:, 0, 0].tobytes() and (r["tparcel"][:, 0, 1] == U).all() and r["flags"]["cape"] == S_
    lv = vp.levels(t, [1000.0, 750.0, 400.0], np.full((1, 2), 0.004, F))
    assert lv["tparcel"].tobytes() == f["tparcel"].tobytes() and lv["cape"].tobytes() == f["cape"].tobytes()


# ------------------------------------------------------------------------------------------- stability of the cases
@pytest.mark.parametrize("name", vc.case_names())
def test_cases_are_stable_under_one_ulp_of_pi(name):
    """The condition on the inputs that the GPU tolerance rests on: at most 2 % of a case's cells change the undef-ness of
    an output, the piece that holds LCL, LFC or EL, or whether the adjustment ran at a level when every pi moves by one
    ulp in the patterns of the family; and no flag of any output changes."""
    c = vc.by_name(name)
    for form in vc.FORMS:
        ref = vc.reference(name, form)
        unstable = 1.0 - ref.stable.mean()
        print(name, form, "unstable cells: %.4f" % unstable)
        assert unstable <= 0.02, (name, form, unstable)
        for m in ref.members:
            for n in vp.OUTPUTS:
                assert np.array_equal(m["flags"][n], ref.r0["flags"][n]), (name, form, n)
        assert len(ref.members) == 6
    assert c["nlev"] in vc.NLEVS


def test_cases_reach_what_they_are_for():
    seen = {"never saturated": 0, "no lfc": 0, "B > 0 at the top": 0, "source saturated": 0, "left the table or met a hole": 0, "el": 0}
    pieces = {"lcl": set(), "lfc": set(), "el": set()}
    for c in vc.cases():
        ref = vc.reference(c["name"], "fld")
        r, d = ref.r0, ref.diag
        alive = r["cape"] != U
        seen["never saturated"] += int((alive & (r["plcl"] == U)).sum())
        seen["no lfc"] += int((alive & (r["plcl"] != U) & (r["plfc"] == U)).sum())
        seen["B > 0 at the top"] += int(((r["plfc"] != U) & (r["pel"] == U)).sum())
        seen["source saturated"] += int((alive & (d["lcl_pos"] == (0 if c["src_level"] is not None and c["source"] == "first" else -1)) & (r["plcl"] != U)).sum())
        seen["left the table or met a hole"] += int((~alive).sum())
        seen["el"] += int((r["pel"] != U).sum())
        if c["nlev"] == 12 and c["source"] == "first":
            for k in pieces:
                row = d[k + "_pos"][0]
                pieces[k] |= set(row[row >= 0].tolist())
    print(seen, pieces)
    assert all(v >= 20 for v in seen.values()), seen
    assert all(len(v) >= 2 for v in pieces.values()), pieces  # the levels move across a row


# ------------------------------------------------------------------------------- declared, bound, configured
def test_header_constants_and_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi
    from mi_fieldcalc_amd import vparcel

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_vparcel_hlevels", "mifc_vparcel_fields", "mifc_vparcel_levels", "mifc_last_vparcel_form"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert [len(capi.SIGNATURES["mifc_vparcel_" + k][1]) for k in ("hlevels", "fields", "levels")] == [27, 25, 24]
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bMIFC_VPARCEL_([A-Z_]+) = (\d+)\b", header)}
    assert enums == {"FROM_FIRST": 0, "FROM_LAST": 1}
    assert vparcel.VPARCEL_FROM == {"first": enums["FROM_FIRST"], "last": enums["FROM_LAST"]} == vp.FROM
    assert vparcel.VPARCEL_OUTPUTS == vp.OUTPUTS
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(csrc, "*"))) if '"MIFC_VPARCEL_CHUNK_MIB"' in open(p, errors="replace").read()]
    assert readers == ["mifc_env.hip"], readers
    host = open(os.path.join(csrc, "mifc_capi_vparcel.hip")).read()
    assert "getenv" not in host and re.search(r"vparcel_chunk_mib > 0 \? mifc::env\(\)\.vparcel_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_vparcel.hip") == 1 and makefile.count("mifc_capi_vparcel.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    kernel = open(os.path.join(csrc, "mifc_vparcel.hip")).read()
    assert kernel.count("__global__") == 1  # one kernel for both directions and both kinds of source


# ------------------------------------------------------------------------------- the front against a recording stub
class _Raw:
    """Wraps the stub library: keeps the raw C arguments of every entry call."""

    def __init__(self, lib):
        self.lib, self.raw = lib, []

    def __getattr__(self, name):
        entry = getattr(self.lib, name)

        def call(*cargs):
            vals = [v.value if isinstance(v, ctypes._SimpleCData) else v for v in cargs]
            self.raw.append((name, vals[1:]))
            return entry(*cargs)

        return call

    def seen(self):
        """The last vparcel call, decoded in header order."""
        name, a = self.raw[-1]
        w = self.lib.where
        nlev = a[2]
        ints = lambda addr, n: None if addr is None else list((ctypes.c_int * n).from_address(addr))  # noqa: E731
        floats = lambda addr: list((ctypes.c_float * nlev).from_address(addr))  # noqa: E731
        s = {"name": name, "head": a[:3], "t": w(a[3]), "fdefined_in": ints(a[4], nlev), "nargs": len(a)}
        if name == "mifc_vparcel_hlevels":
            s.update(coord=w(a[5]), fdef_ps=a[6], alevel=floats(a[7]), blevel=floats(a[8]))
            at = 9
        elif name == "mifc_vparcel_fields":
            s.update(coord=w(a[5]), fdef_coord=ints(a[6], nlev))
            at = 7
        else:
            s.update(levels=floats(a[5]))
            at = 6
        s.update(**{"from": a[at], "src_level": a[at + 1], "t_src": w(a[at + 2]), "fdef_tsrc": a[at + 3], "q_src": w(a[at + 4]), "fdef_qsrc": a[at + 5],
                    "p_src": w(a[at + 6]), "fdef_psrc": a[at + 7], "outs": [w(x) for x in a[at + 8:at + 14]], "out_addrs": list(a[at + 8:at + 14]), "undef": a[at + 15], "memkind": a[at + 16]})
        return s


def _front(rc=1):
    from mi_fieldcalc_amd import vparcel

    d = _data()
    ctx, lib = _stub_context(d, rc)
    raw = _Raw(lib)
    ctx._lib = raw
    return vparcel, d, ctx, raw


def test_front_marshals_the_hybrid_form_in_header_order():
    vparcel, d, ctx, raw = _front()
    r = vparcel.vparcel_hlevels(ctx, d["T"], d["PS"], [0.0, 10.0, 20.0], [1.0, 0.5, 0.0], d["XM"], src_level=2, from_="last", outputs=vp.OUTPUTS,
                                fdefined_in=[A, S_, A], fdef_ps=A, fdef_qsrc=A)
    s = raw.seen()
    assert s["name"] == "mifc_vparcel_hlevels" and s["head"] == [5, 4, 3] and s["t"] == ["T", 0] and s["coord"] == ["PS", 0] and s["fdef_ps"] == A
    assert s["alevel"] == [0.0, 10.0, 20.0] and s["blevel"] == [1.0, 0.5, 0.0] and s["fdefined_in"] == [A, S_, A]
    assert s["from"] == 1 and s["src_level"] == 2 and s["t_src"] is None and s["p_src"] is None and s["q_src"] == ["XM", 0]
    assert (s["fdef_tsrc"], s["fdef_qsrc"], s["fdef_psrc"]) == (S_, A, S_) and s["undef"] == float(U) and s["memkind"] == 0 and s["nargs"] == 26
    assert sorted(r) == sorted(vp.OUTPUTS + ("flags",)) and r["cape"].shape == (4, 5) and r["tparcel"].shape == (3, 4, 5) and r["cape"].dtype == np.float32
    assert s["out_addrs"] == [r[n].ctypes.data for n in vp.OUTPUTS] and len(set(s["out_addrs"])) == 6
    assert isinstance(r["flags"]["cape"], int) and r["flags"]["tparcel"].shape == (3,) and r["flags"]["tparcel"].dtype == np.int32


def test_front_passes_planes_subsets_and_out():
    vparcel, d, ctx, raw = _front()
    mine = d["OUT"][:20].reshape(4, 5)
    r = vparcel.vparcel_fields(ctx, d["T"], d["COORD"], d["XM"], src_level=None, t_src=d["LO"], p_src=d["HI"], outputs=("pel", "cape"), out={"pel": mine},
                               fdef_coord=[A, A, S_], fdef_tsrc=A, fdef_psrc=A)
    s = raw.seen()
    assert s["name"] == "mifc_vparcel_fields" and s["coord"] == ["COORD", 0] and s["fdef_coord"] == [A, A, S_] and s["fdefined_in"] is None
    assert s["src_level"] == -1 and s["from"] == 0 and s["t_src"] == ["LO", 0] and s["p_src"] == ["HI", 0] and s["q_src"] == ["XM", 0] and s["nargs"] == 24
    assert (s["fdef_tsrc"], s["fdef_qsrc"], s["fdef_psrc"]) == (A, S_, A)
    assert r["pel"] is mine and s["outs"][4] == ["OUT", 0] and s["out_addrs"][0] == r["cape"].ctypes.data and s["outs"][1:4] == [None] * 3
    assert s["outs"][5] is None and sorted(r) == ["cape", "flags", "pel"] and sorted(r["flags"]) == ["cape", "pel"]
    r = vparcel.vparcel_levels(ctx, d["T"], [900.0, 700.0, 500.0], d["XM"], outputs="tparcel", fdefined_in=A)
    s = raw.seen()
    assert s["name"] == "mifc_vparcel_levels" and s["levels"] == [900.0, 700.0, 500.0] and s["fdefined_in"] == [A, A, A] and s["nargs"] == 23
    assert s["src_level"] == 0 and s["outs"][:5] == [None] * 5 and s["out_addrs"][5] == r["tparcel"].ctypes.data and sorted(r) == ["flags", "tparcel"]
    with pytest.raises(ValueError, match="needs t_src, q_src and p_src"):
        vparcel.vparcel_levels(ctx, d["T"], [900.0, 700.0, 500.0], d["XM"], src_level=None, t_src=d["LO"])
    with pytest.raises(ValueError, match="q_src must have the shape"):
        vparcel.vparcel_levels(ctx, d["T"], [900.0, 700.0, 500.0], d["T"])
    with pytest.raises(ValueError, match="unknown output 'lcl'"):
        vparcel.vparcel_levels(ctx, d["T"], [900.0, 700.0, 500.0], d["XM"], outputs=("lcl",))
    with pytest.raises(ValueError, match=r"out\['pel'\] must have shape"):
        vparcel.vparcel_levels(ctx, d["T"], [900.0, 700.0, 500.0], d["XM"], outputs=("pel",), out={"pel": d["T"]})
    with pytest.raises(ValueError, match="one value per level"):
        vparcel.vparcel_levels(ctx, d["T"], [900.0, 700.0], d["XM"])
    with pytest.raises(ValueError, match="one .nlev, ny, nx. batch"):
        vparcel.vparcel_levels(ctx, d["F2"], [900.0, 700.0, 500.0], d["XM"])


def test_a_refused_call_raises_value_error_with_the_librarys_message():
    vparcel, d, ctx, raw = _front(rc=0)
    raw.lib.__dict__["mifc_last_error"] = lambda c: b"mifc_vparcel_levels: levels[1] <= 0"
    with pytest.raises(ValueError, match=r"mifc_vparcel_levels: levels\[1\] <= 0") as info:
        vparcel.vparcel_levels(ctx, d["T"], [900.0, -1.0, 500.0], d["XM"])
    assert isinstance(info.value, RuntimeError)  # what the Context methods raise for a refusal is caught by the same handler
