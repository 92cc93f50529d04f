"""CPU checks of mifc_pvort_hlevels / mifc_pvort_fields / mifc_pvort_levels: the semantics through their numpy
restatement (tests/pvort_restate.py, the oracle of the GPU tests) on hand-worked columns, every cause of an undefined
cell alone, the two identities that tie it to the reference's absvort and to the vertical derivative, an independent
float64 evaluation, a physical sanity case, that the entries are declared, bound and configured where the others are,
and the front's marshalling against a recording stub library."""
import glob
import os
import re

import numpy as np
import pytest

import pvort_restate as pv
import vderiv_restate as vd
from test_python_front_cpu import _data, _stub_context

U = pv.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, S_, N = pv.ALL_DEFINED, pv.SOME_DEFINED, pv.NONE_DEFINED
METHODS = (pv.CENTRED, pv.WEIGHTED)


def planes(nlev, centre, ny=3, nx=3, fill=None):
    """(nlev, ny, nx): level k is the constant centre[k] (or fill[k])."""
    a = np.empty((nlev, ny, nx), np.float32)
    a[:] = np.asarray(centre if fill is None else fill, np.float32).reshape(-1, 1, 1)
    a[:, 1, 1] = np.asarray(centre, np.float32)
    return a


def test_hand_worked_two_levels():
    u, v, th = planes(2, [3, 13]), planes(2, [2, 6]), planes(2, [300, 320])
    v[0, 1, 0], v[0, 1, 2] = 1, 5  # dx(v) = 0.25 * 4 = 1
    u[0, 0, 1], u[0, 2, 1] = 2, 4  # dy(u) = 0.25 * 2 = 0.5
    th[0, 1, 0], th[0, 1, 2] = 296, 304  # dx(th) = 2
    th[0, 0, 1], th[0, 2, 1] = 298, 310  # dy(th) = 3
    half = np.full((3, 3), 0.5, np.float32)
    f = np.full((3, 3), 1.5, np.float32)
    for method in METHODS:
        out, fd = pv.levels(u, v, th, [100, 300], half, half, f, method, scale=2.0)
        # D = difference / 200 on both levels (one side each); level 0: za = 1 - 0.5 + 1.5 = 2
        e0 = np.float32(2.0 * ((2.0 * (20 * (1.0 / 200)) - (4 * (1.0 / 200)) * 2.0) + (10 * (1.0 / 200)) * 3.0))
        e1 = np.float32(2.0 * (1.5 * (20 * (1.0 / 200))))  # level 1: the planes are constant, za = f
        assert abs(e0 - 0.62) < 1e-6 and abs(e1 - 0.3) < 1e-6
        assert (out[0] == e0).all() and (out[1] == e1).all() and (fd == A).all()  # the ring is the centre's copy
    out2, _ = pv.levels(u, v, th, [100, 300], half, half, None, scale=2.0)
    assert out2[0, 1, 1] == np.float32(2.0 * ((0.5 * 0.1 - 0.02 * 2.0) + 0.05 * 3.0))  # no f: za = zeta


def test_hand_worked_three_levels():
    zero = np.zeros((3, 3, 3), np.float32)
    th = planes(3, [300, 303, 312])
    one = np.ones((3, 3), np.float32)
    f = np.full((3, 3), 2, np.float32)
    out, fd = pv.levels(zero, zero, th, [100, 200, 400], one, one, f, pv.WEIGHTED)
    # level 1: w1 = 200 / (100 * 300), w2 = 100 / (200 * 300): 3 / 150 + 9 / 600 = 0.035
    e = [np.float32(2 * (3 * (1.0 / 100))), np.float32(2 * (3.0 * (200.0 / (100.0 * 300.0)) + 9.0 * (100.0 / (200.0 * 300.0)))), np.float32(2 * (9 * (1.0 / 200)))]
    assert [float(x) for x in out[:, 1, 1]] == [float(x) for x in e] and abs(e[1] - 0.07) < 1e-7 and (fd == A).all()
    out, fd = pv.levels(zero, zero, th, [100, 200, 400], one, one, f, pv.CENTRED)
    assert out[1, 0, 2] == np.float32(2 * (12 * (1.0 / 300)))


# ---------------------------------------------------------------------------------------------- every undef cause alone
def _seven(seed=2):
    """3 x 3 x 7: one interior cell, every neighbour in the ring."""
    rng = np.random.default_rng(seed)
    u, v, th = (rng.normal(0, 5, (7, 3, 3)).astype(np.float32) for _ in range(3))
    p = np.broadcast_to(np.array([100, 200, 300, 400, 550, 700, 900], np.float32).reshape(-1, 1, 1), (7, 3, 3)).copy()
    xm, ym, f = (rng.uniform(0.5, 2, (3, 3)).astype(np.float32) for _ in range(3))
    return u, v, th, p, xm, ym, f


def _undef_levels(out, fd):
    lv = [k for k in range(out.shape[0]) if (out[k] == U).all()]
    assert all((out[k] == U).all() or (out[k] != U).all() for k in range(out.shape[0]))  # the ring copies the one cell
    assert [int(x) for x in fd] == [N if k in lv else A for k in range(out.shape[0])]  # counted over the interior: one cell
    return lv


@pytest.mark.parametrize("method", METHODS)
def test_each_neighbour_alone(method):
    for field, (dy, dx) in [(1, (0, -1)), (1, (0, 1)), (0, (-1, 0)), (0, (1, 0)), (2, (0, -1)), (2, (0, 1)), (2, (-1, 0)), (2, (1, 0))]:
        for bad in (U, np.nan):
            c = _seven()
            c[field][3, 1 + dy, 1 + dx] = bad
            out, fd = pv.coord_fields(*c, method=method)
            assert _undef_levels(out, fd) == [3], (field, dy, dx)
    # what is no neighbour of the stencil plays no part: the corners, u left and right, v above and below
    c = _seven()
    for a in c[:3]:
        a[3, ::2, ::2] = U
    c[0][3, 1, ::2] = U
    c[1][3, ::2, 1] = U
    c[3][3, ::2, :] = U  # the coordinate of the neighbours
    c[3][3, 1, ::2] = np.nan
    out, fd = pv.coord_fields(*c, method=method)
    e, _ = pv.coord_fields(*_seven(), method=method)
    assert _undef_levels(out, fd) == [] and out.tobytes() == e.tobytes()


@pytest.mark.parametrize("method", METHODS)
def test_each_vertical_cause_alone(method):
    for field in range(3):
        c = _seven()
        c[field][3, 1, 1] = U  # the centre; the levels 2 and 4 keep one side
        assert _undef_levels(*pv.coord_fields(*c, method=method)) == [3]
        c = _seven()
        c[field][2, 1, 1] = c[field][4, 1, 1] = U  # no side at level 3
        assert _undef_levels(*pv.coord_fields(*c, method=method)) == [2, 3, 4]
    c = _seven()
    c[3][4, 1, 1] = c[3][2, 1, 1]  # zero spacing: c_4 == c_2 around level 3
    assert _undef_levels(*pv.coord_fields(*c, method=method)) == [3]
    c = _seven()
    c[3][3, 1, 1] = U  # the coordinate is not usable
    assert _undef_levels(*pv.coord_fields(*c, method=method)) == [3]
    c = _seven()
    c[3][3, 1, 1] = np.nan
    assert _undef_levels(*pv.coord_fields(*c, method=method, fdef_coord=[A] * 7)) == [3]
    c = _seven()
    c[3][3, 1, 1] = U
    out, fd = pv.coord_fields(*c, method=method, fdef_coord=[A] * 7)  # flagged ALL_DEFINED: undef is a value
    assert _undef_levels(out, fd) == ([] if method == pv.CENTRED else [3])  # (WEIGHTED: the two huge spacings cancel, a zero denominator)


def test_nan_through_an_all_defined_flag_is_a_value():
    c = _seven()
    c[0][3, 1, 1] = np.nan
    c[2][3, 0, 1] = np.nan  # a neighbour
    flags = np.full((3, 7), A)
    out, fd = pv.coord_fields(*c, method=pv.WEIGHTED, flags=flags)
    assert (fd == A).all() and np.isnan(out[2:5]).all() and not np.isnan(out[:2]).any() and not np.isnan(out[5:]).any()
    flags[:, 3] = S_
    out, fd = pv.coord_fields(*c, method=pv.WEIGHTED, flags=flags)
    assert [int(x) for x in fd] == [A, A, A, N, A, A, A] and (out[3] == U).all() and not np.isnan(out).any()  # (the levels 2 and 4 are one-sided now)


def test_the_count_is_over_the_interior():
    c = pv.pv_case(nlev=5, ny=6, nx=7, frac=0.0)
    args = [c[k] for k in ("u", "v", "th", "p", "xmapr", "ymapr", "fcoriolis")]
    for a in args[:3]:
        a[np.isnan(a)] = 1
    args[0][2, 2, 3] = U  # an interior centre: itself, and the dy neighbour of the cells above and below
    out, fd = pv.coord_fields(*args)
    assert [int(x) for x in fd] == [A, A, S_, A, A] and sorted(map(tuple, np.argwhere(out[2] == U))) == [(0, 3), (1, 3), (2, 3), (3, 3)]  # (row 0 copies row 1)
    args[0][2, 2, 3] = 1
    args[1][2, 1, 0] = U  # a ring cell that is the dx neighbour of cell (1, 1), which the ring copies
    out, fd = pv.coord_fields(*args)
    assert fd[2] == S_ and sorted(map(tuple, np.argwhere(out[2] == U))) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    args[1][2, 1, 0] = 1
    args[0][2, 0, 0] = args[1][2, 5, 6] = args[2][2, 0, 6] = U  # corners: no part
    out, fd = pv.coord_fields(*args)
    assert (fd == A).all() and not (out == U).any()


# ------------------------------------------------------------------------------------------------------ identities
def _identity_a_case(nlev=9, ny=6, nx=7, seed=11):
    rng = np.random.default_rng(seed)
    u, v = (rng.normal(0, 1, (nlev, ny, nx)).astype(np.float32) for _ in range(2))
    xm, ym, f = (rng.normal(0, 1, (ny, nx)).astype(np.float32) for _ in range(3))
    levs = (128.0 * np.arange(1, nlev + 1)).astype(np.float32)
    th = np.broadcast_to(levs.reshape(-1, 1, 1), (nlev, ny, nx)).copy()
    return u, v, th, levs, xm, ym, f


@pytest.mark.parametrize("method", METHODS)
def test_identity_a_absvort_of_every_level(oracle, method):
    """th = levels with power-of-two spacings: D_th is exactly 1, dx(th) = dy(th) = 0, so S = za: the reference's absvort,
    ring included."""
    u, v, th, levs, xm, ym, f = _identity_a_case()
    out, fd = pv.levels(u, v, th, levs, xm, ym, f, method)
    for k in range(u.shape[0]):
        ok, e, flag = oracle.call("absvort", u.shape[2], u.shape[1], u[k], v[k], xm, ym, f, fdefined=S_)
        assert ok and out[k].tobytes() == e.tobytes() and flag == fd[k] == A, k


@pytest.mark.parametrize("method", METHODS)
def test_identity_a_against_the_compiled_reference(ref, method):
    u, v, th, levs, xm, ym, f = _identity_a_case(seed=12)
    u[4, 2, 3] = v[4, 3, 1] = U
    out, fd = pv.levels(u, v, th, levs, xm, ym, f, method)
    for k in (0, 3, 5, 8):  # (level 4 has holes at cell centres, which absvort does not read)
        ok, e, flag = ref.call("absvort", u.shape[2], u.shape[1], u[k], v[k], xm, ym, f, fdefined=S_)
        assert ok and out[k].tobytes() == e.tobytes() and flag == fd[k] == A, k


@pytest.mark.parametrize("method", METHODS)
def test_identity_b_the_vertical_derivative_at_the_clamped_cell(method):
    """No horizontal part (xmapr = ymapr = 0) and f = 1: S = D_th, the result vderiv_restate's at the clamped cell."""
    c = pv.pv_case(nlev=9, ny=6, nx=7, seed=21)
    c["u"][~np.isfinite(c["u"]) | (c["u"] == U)] = 1  # (holes in u and v would make cells undef that vderiv of th defines)
    c["v"][~np.isfinite(c["v"]) | (c["v"] == U)] = 1
    zero, one = np.zeros((6, 7), np.float32), np.ones((6, 7), np.float32)
    th = c["th"].copy()
    th[:, :, ::6] = 7  # the neighbours are tested: keep them defined, the holes at the centres
    th[:, ::5, :] = 7
    th[3, 2, 3], th[5, 3, 2] = U, np.nan
    out, fd = pv.hlevels(c["u"], c["v"], th, c["ps"], c["alevel"], c["blevel"], zero, zero, one, method)
    e, _ = vd.hlevels(th[None], c["ps"], c["alevel"], c["blevel"], method)
    yc, xc = np.clip(np.arange(6), 1, 4), np.clip(np.arange(7), 1, 5)
    want = e[0][:, yc][:, :, xc]
    holes = np.zeros(th.shape, bool)  # a hole is a neighbour of four cells
    bad_th = ~np.isfinite(th) | (th == U)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        holes |= np.roll(bad_th, (dy, dx), axis=(1, 2))
    holes = holes[:, yc][:, :, xc]
    assert (out[holes] == U).all() and holes.sum() >= 8
    assert out[~holes].tobytes() == want[~holes].tobytes() and (want[~holes] != U).sum() > 200 and (want[~holes] == U).any()


def test_vertical_is_the_double_of_vderiv_restate():
    fields, ps, (al, bl), coord = vd.deriv_case()
    for method in METHODS:
        e, efd, ebad = vd.derivative(fields, coord, pv.is_defined(False, coord, U), method)
        for f in range(fields.shape[0]):
            r, bad = pv.vertical(fields[f], coord, pv.is_defined(False, coord, U), method)
            with np.errstate(all="ignore"):
                assert np.where(bad, U, r.astype(np.float32)).tobytes() == e[f].tobytes() and (bad == ebad[f]).all()


def _scratch_pv(u, v, th, c, xm, ym, f, method, scale):
    """The definition of include/mifc.h restated cell by cell in Python floats (doubles), without holes."""
    nlev, ny, nx = u.shape
    out = np.zeros((nlev, ny, nx), np.float32)

    def deriv(a, k, y, x):
        a, cc = a[:, y, x].astype(np.float64), c[:, y, x].astype(np.float64)
        if k == 0:
            return (a[1] - a[0]) * (1.0 / (cc[1] - cc[0]))
        if k == nlev - 1:
            return (a[k] - a[k - 1]) * (1.0 / (cc[k] - cc[k - 1]))
        if method == pv.CENTRED:
            return (a[k + 1] - a[k - 1]) * (1.0 / (cc[k + 1] - cc[k - 1]))
        h1, h2 = cc[k] - cc[k - 1], cc[k + 1] - cc[k]
        den = h1 + h2
        return (a[k] - a[k - 1]) * (h2 / (h1 * den)) + (a[k + 1] - a[k]) * (h1 / (h2 * den))

    for k in range(nlev):
        for y in range(ny):
            for x in range(nx):
                yc, xc = min(max(y, 1), ny - 2), min(max(x, 1), nx - 2)
                hx, hy = 0.5 * np.float64(xm[yc, xc]), 0.5 * np.float64(ym[yc, xc])
                dx = lambda a: hx * np.float64(a[k, yc, xc + 1] - a[k, yc, xc - 1])  # noqa: E731  (float32 difference)
                dy = lambda a: hy * np.float64(a[k, yc + 1, xc] - a[k, yc - 1, xc])  # noqa: E731
                za = (dx(v) - dy(u)) + np.float64(f[yc, xc])
                s = (za * deriv(th, k, yc, xc) - deriv(v, k, yc, xc) * dx(th)) + deriv(u, k, yc, xc) * dy(th)
                out[k, y, x] = np.float32(scale * s)
    return out


@pytest.mark.parametrize("method", METHODS)
def test_the_restatement_against_a_scratch_restatement(method):
    rng = np.random.default_rng(31)
    u, v, th = (rng.normal(0, 1, (9, 6, 7)).astype(np.float32) for _ in range(3))
    xm, ym, f = (rng.normal(0, 1, (6, 7)).astype(np.float32) for _ in range(3))
    p = (np.cumsum(rng.uniform(20, 90, (9, 6, 7)), axis=0)).astype(np.float32)
    out, fd = pv.coord_fields(u, v, th, p, xm, ym, f, method, scale=-3.5)
    assert out.tobytes() == _scratch_pv(u, v, th, p, xm, ym, f, method, -3.5).tobytes() and (fd == A).all()
    # the identities on the scratch restatement too
    u, v, th, levs, xm, ym, f = _identity_a_case(9, 6, 7, seed=32)
    c = np.broadcast_to(levs.reshape(-1, 1, 1), u.shape)
    s = _scratch_pv(u, v, th, c, xm, ym, f, method, 1.0)
    assert s.tobytes() == pv.levels(u, v, th, levs, xm, ym, f, method)[0].tobytes()
    zero, one = np.zeros((6, 7), np.float32), np.ones((6, 7), np.float32)
    th = rng.normal(300, 5, (9, 6, 7)).astype(np.float32)
    s = _scratch_pv(u, v, th, p, zero, zero, one, method, 1.0)
    e, _ = vd.coord_fields(th[None], p, method)
    assert s.tobytes() == e[0][:, np.clip(np.arange(6), 1, 4)][:, :, np.clip(np.arange(7), 1, 5)].tobytes()


@pytest.mark.parametrize("method", METHODS)
def test_independent_float64_evaluation_within_the_propagated_bound(method):
    """The same formula from the same float inputs with every difference in float64: the only differences are the float
    subtractions of the neighbours (2^-24 relative each) and the final rounding; the bound carries the factor 4."""
    c = pv.pv_case(nlev=9, ny=8, nx=10, seed=41, frac=0.0)
    u, v, th = c["u"], c["v"], c["th"]
    for a in (u, v, th):
        a[np.isnan(a)] = 1
    scale = -9.8e4
    terms = {}
    out, fd = pv.coord_fields(u, v, th, c["p"], c["xmapr"], c["ymapr"], c["fcoriolis"], method, scale, terms=terms)
    assert (fd == A).all()
    d = lambda a: a.astype(np.float64)  # noqa: E731
    hx, hy = 0.5 * d(c["xmapr"])[1:-1, 1:-1], 0.5 * d(c["ymapr"])[1:-1, 1:-1]
    dx = lambda a: hx * (d(a)[:, 1:-1, 2:] - d(a)[:, 1:-1, :-2])  # noqa: E731
    dy = lambda a: hy * (d(a)[:, 2:, 1:-1] - d(a)[:, :-2, 1:-1])  # noqa: E731
    Du, Dv, Dt = terms["Du"], terms["Dv"], terms["Dt"]  # (the vertical part is float64 in the definition already)
    za = (dx(v) - dy(u)) + d(c["fcoriolis"])[1:-1, 1:-1]
    want = scale * ((za * Dt - Dv * dx(th)) + Du * dy(th))
    bound = 2.0 ** -22 * abs(scale) * (np.abs(terms["za"] * Dt) + np.abs(terms["t2"]) + np.abs(terms["t3"]) + (np.abs(terms["dxv"]) + np.abs(terms["dyu"])) * np.abs(Dt))
    err = np.abs(d(out[:, 1:-1, 1:-1]) - want)
    print("largest error / bound", float((err / bound).max()))
    assert (err <= bound).all()


def test_sanity_icao_troposphere_at_rest():
    """ICAO: T = 288.15 - 6.5 K/km, p = 1013.25 (T / 288.15)^5.2559; theta = T (1000 / p)^0.2857.  At rest PV = -g f dtheta/dp."""
    levs = np.arange(300, 1001, 50, dtype=np.float32)
    t = 288.15 * (levs.astype(np.float64) / 1013.25) ** (1 / 5.2559)
    theta = (t * (1000.0 / levs) ** 0.2857).astype(np.float32)
    nlev = levs.size
    th = np.broadcast_to(theta.reshape(-1, 1, 1), (nlev, 4, 5)).copy()
    zero = np.zeros((nlev, 4, 5), np.float32)
    one = np.ones((4, 5), np.float32)
    f = np.full((4, 5), 1e-4, np.float32)
    for method in METHODS:
        out, fd = pv.levels(zero, zero, th, levs, one, one, f, method, scale=-9.8e4)
        print(method, "PVU", float(out.min()), float(out.max()))
        assert (fd == A).all() and (out > 0.2).all() and (out < 1.0).all()


# ------------------------------------------------------------------------------- declared, bound and configured
def test_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi
    from mi_fieldcalc_amd import pvort

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_pvort_hlevels", "mifc_pvort_fields", "mifc_pvort_levels", "mifc_last_pvort_form"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert [len(capi.SIGNATURES["mifc_pvort_" + k][1]) for k in ("hlevels", "fields", "levels")] == [21, 19, 18]
    assert all(capi.SIGNATURES["mifc_pvort_" + k][1][-5] == "d" for k in ("hlevels", "fields", "levels"))  # scale is a double
    assert "MIFC_PVORT_" not in header  # the methods are MIFC_VDERIV_*: no new enum
    assert pvort.PVU_SCALE == -9.8e4
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(csrc, "*"))) if '"MIFC_PVORT_CHUNK_MIB"' in open(p, errors="replace").read()]
    assert readers == ["mifc_env.hip"], readers
    host = open(os.path.join(csrc, "mifc_capi_pvort.hip")).read()
    assert "getenv" not in host and re.search(r"pvort_chunk_mib > 0 \? mifc::env\(\)\.pvort_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_pvort.hip") == 1 and makefile.count("mifc_capi_pvort.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    kernel = open(os.path.join(csrc, "mifc_pvort.hip")).read()
    assert kernel.count("__global__") == 1


# ------------------------------------------------------------------------------- the front against a recording stub
def _front(rc=1):
    from mi_fieldcalc_amd import pvort

    d = _data()
    ctx, lib = _stub_context(d, rc)
    return pvort, d, ctx, lib


def test_front_marshals_the_hybrid_form_in_header_order():
    pvort, d, ctx, lib = _front()
    out, fd = pvort.pvort_hlevels(ctx, d["B"], d["V"], d["T"], d["PS"], [0.0, 10.0, 20.0], [1.0, 0.5, 0.0], d["XM"], d["YM"], d["FCOR"], "weighted", -2.5,
                                  fdefined_in=[A, S_, A], fdef_ps=A)
    name, a = lib.calls[-1]
    assert name == "mifc_pvort_hlevels" and a[:3] == [5, 4, 3] and a[3:6] == [["B", 0], ["V", 0], ["T", 0]]
    assert a[6]["values"] == [A, A, A, S_, S_, S_, A, A, A] and a[7] == ["PS", 0] and a[8] == A
    assert a[9]["values"] == [0.0, 10.0, 20.0] and a[10]["values"] == [1.0, 0.5, 0.0]
    assert a[11:14] == [["XM", 0], ["YM", 0], ["FCOR", 0]] and a[14] == 1 and a[15] == -2.5
    assert a[17]["numpy"] == "int32" and a[17]["shape"] == [3] and a[18] == float(U) and a[19] == 0 and len(a) == 20
    assert out.shape == (3, 4, 5) and out.dtype == np.float32 and fd.shape == (3,) and fd.dtype == np.int32
    assert lib.where(out.ctypes.data) == "<other>" and a[16] == "<other>"


def test_front_null_fcoriolis_out_and_the_other_forms():
    pvort, d, ctx, lib = _front()
    o = d["OUT"][: 3 * 4 * 5].reshape(3, 4, 5)
    out, fd = pvort.pvort_fields(ctx, d["B"], d["V"], d["T"], d["COORD"], d["XM"], d["YM"], out=o)
    name, a = lib.calls[-1]
    assert name == "mifc_pvort_fields" and out is o and a[14] == ["OUT", 0] and a[7] == ["COORD", 0] and a[8] is None and a[6] is None
    assert a[9:12] == [["XM", 0], ["YM", 0], None] and a[12] == 0 and a[13] == 1.0 and len(a) == 18
    out, fd = pvort.pvort_fields(ctx, d["B"], d["V"], d["T"], d["COORD"], d["XM"], d["YM"], d["FCOR"], fdef_coord=[A, S_, A])
    assert lib.calls[-1][1][8]["values"] == [A, S_, A] and lib.calls[-1][1][11] == ["FCOR", 0]
    out, fd = pvort.pvort_levels(ctx, d["B"], d["V"], d["T"], [100.0, 200.0, 300.0], d["XM"], d["YM"], None, pv.WEIGHTED, scale=3)
    name, a = lib.calls[-1]
    assert name == "mifc_pvort_levels" and a[7]["values"] == [100.0, 200.0, 300.0] and a[8:11] == [["XM", 0], ["YM", 0], None] and a[11] == 1 and a[12] == 3.0
    assert len(a) == 17 and out.shape == (3, 4, 5)
    with pytest.raises(ValueError, match="out must have shape"):
        pvort.pvort_fields(ctx, d["B"], d["V"], d["T"], d["COORD"], d["XM"], d["YM"], out=d["OUT"][:20].reshape(4, 5))
    with pytest.raises(ValueError, match="xmapr must have the shape"):
        pvort.pvort_fields(ctx, d["B"], d["V"], d["T"], d["COORD"], d["COORD"], d["YM"])
    with pytest.raises(ValueError, match="every field must have the shape"):
        pvort.pvort_fields(ctx, d["B"], d["PS"], d["T"], d["COORD"], d["XM"], d["YM"])
    with pytest.raises(ValueError, match="one value per level"):
        pvort.pvort_levels(ctx, d["B"], d["V"], d["T"], [100.0, 200.0], d["XM"], d["YM"])


def test_potential_vorticity_forms_theta_and_calls_the_hybrid_entry():
    pvort, d, ctx, lib = _front()
    out, fd = pvort.potential_vorticity_hlevels(ctx, d["B"], d["V"], d["T"], d["PS"], [0.0, 10.0, 20.0], [1.0, 0.5, 0.0], d["XM"], d["YM"], d["FCOR"])
    (n1, a1), (n2, a2) = [call for call in lib.calls if "stream" not in call[0]][-2:]
    assert n1 == "mifc_hlevel_derived_batch" and a1[5] == ["T", 0] and a1[3] is None and a1[4] is None and a1[13] == 3  # hleveltemp, compute 3
    assert n2 == "mifc_pvort_hlevels" and a2[3:5] == [["B", 0], ["V", 0]] and a2[5] == a1[11] == "<other>"  # th is the batch's output
    assert a2[14] == 1 and a2[15] == -9.8 * 1e4 and a2[13] == ["FCOR", 0] and out.shape == (3, 4, 5)


def test_a_refused_call_raises_value_error_with_the_librarys_message():
    pvort, d, ctx, lib = _front(rc=0)
    lib.__dict__["mifc_last_error"] = lambda c: b"mifc_pvort_fields: scale is NaN"
    with pytest.raises(ValueError, match=r"mifc_pvort_fields: scale is NaN") as info:
        pvort.pvort_fields(ctx, d["B"], d["V"], d["T"], d["COORD"], d["XM"], d["YM"], scale=float("nan"))
    assert isinstance(info.value, RuntimeError)
