"""Numpy restatement of mifc_pvort_hlevels / mifc_pvort_fields / mifc_pvort_levels (include/mifc.h, "Ertel potential
vorticity of level batches"): the oracle of tests/test_gpu_pvort.py.  The coordinate in float32, the vertical
derivatives by the rules of vderiv_restate but kept in float64 (rule 2: the double r before its rounding), the
neighbour differences in float32, the products step by step in float64 (every ufunc rounds once, so nothing is
contracted).  The result of the interior cells is computed, the ring is taken from it by the clamped index."""
import numpy as np

from vderiv_restate import CENTRED, METHODS, WEIGHTED  # noqa: F401
from vinterp_restate import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, hybrid_coordinate, hybrid_levels, is_defined  # noqa: F401

FU, FV, FT = 0, 1, 2


def vertical(x, coord, coord_defined, method, flags=None, undef=UNDEF):
    """Rules 2 to 6 of mifc_vderiv_* for one field x float32 (nlev, ny, nx): (r float64 (nlev, ny, nx) -- the value
    before the rounding to float, garbage where bad --, bad bool (nlev, ny, nx): the rules leave the cell undef).  The
    same steps as vderiv_restate.derivative, which rounds r to float32 (tests/test_pvort_cpu.py holds the two together)."""
    x = np.asarray(x, np.float32)
    nlev, ny, nx = x.shape
    cells = ny * nx
    x = x.reshape(nlev, cells)
    c = np.broadcast_to(np.asarray(coord, np.float32), (nlev, ny, nx)).reshape(nlev, cells)
    undef = np.float32(undef)
    method = METHODS.get(method, method)
    fl = [SOME_DEFINED] * nlev if flags is None else list(np.asarray(flags).reshape(nlev))
    r = np.zeros((nlev, cells), np.float64)
    bad = np.ones((nlev, cells), bool)
    with np.errstate(all="ignore"):
        usable_c = np.broadcast_to(np.asarray(coord_defined, bool), (nlev, ny, nx)).reshape(nlev, cells) & ~np.isnan(c)
        d = c.astype(np.float64)
        zero, no = np.zeros(cells, np.float64), np.zeros(cells, bool)
        point = np.stack([usable_c[k] & is_defined(fl[k] == ALL_DEFINED, x[k], undef) for k in range(nlev)])
        xd = x.astype(np.float64)
        for k in range(nlev):
            lower = point[k - 1] & (c[k - 1] != c[k]) if k > 0 else no
            upper = point[k + 1] & (c[k + 1] != c[k]) if k < nlev - 1 else no
            dm, xm = (d[k - 1], xd[k - 1]) if k > 0 else (zero, zero)
            dp, xp = (d[k + 1], xd[k + 1]) if k < nlev - 1 else (zero, zero)
            if method == CENTRED:
                den = dp - dm
                w = 1.0 / den
                both = (xp - xm) * w
            else:
                h1, h2 = d[k] - dm, dp - d[k]
                den = h1 + h2
                w1, w2 = h2 / (h1 * den), h1 / (h2 * den)
                both = (xd[k] - xm) * w1 + (xp - xd[k]) * w2
            one_lower = (xd[k] - xm) * (1.0 / (d[k] - dm))
            one_upper = (xp - xd[k]) * (1.0 / (dp - d[k]))
            r[k] = np.where(lower & upper, both, np.where(lower, one_lower, one_upper))
            bad[k] = ~point[k] | ~(lower | upper) | (lower & upper & (den == 0))
    return r.reshape(nlev, ny, nx), bad.reshape(nlev, ny, nx)


def potential_vorticity(u, v, th, coord, coord_defined, xmapr, ymapr, fcoriolis=None, method=CENTRED, scale=1.0, flags=None, undef=UNDEF, terms=None):
    """u, v, th float32 (nlev, ny, nx); coord float32 broadcastable to that and coord_defined bool (rule 1 of vinterp);
    xmapr, ymapr, fcoriolis (ny, nx), fcoriolis None: the addition is absent; flags None (SOME_DEFINED) or (3, nlev) in the
    order u, v, th.  Returns (pv (nlev, ny, nx), flags_out int32 (nlev,)).  terms: a dict that receives the float64 terms
    of the interior cells (za, D_u, D_v, D_th, dxv, dyu, dxt, dyt, t1, t2, t3, S, bad)."""
    f = [np.asarray(a, np.float32) for a in (u, v, th)]
    nlev, ny, nx = f[0].shape
    assert nx >= 3 and ny >= 3 and nlev >= 2
    undef = np.float32(undef)
    fl = np.full((3, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(3, nlev)
    D, vbad = zip(*[vertical(f[j], coord, coord_defined, method, fl[j], undef) for j in range(3)])
    mid = (slice(None), slice(1, ny - 1), slice(1, nx - 1))

    def nb(a, dy, dx):
        return a[:, 1 + dy:ny - 1 + dy, 1 + dx:nx - 1 + dx]

    def ok(j, a):
        alld = (fl[j] == ALL_DEFINED).reshape(nlev, 1, 1)
        return alld | (~np.isnan(a) & (a != undef))

    with np.errstate(all="ignore"):
        hx = 0.5 * np.asarray(xmapr, np.float32)[1:-1, 1:-1].astype(np.float64)
        hy = 0.5 * np.asarray(ymapr, np.float32)[1:-1, 1:-1].astype(np.float64)
        vl, vr, ul, uh = nb(f[FV], 0, -1), nb(f[FV], 0, 1), nb(f[FU], -1, 0), nb(f[FU], 1, 0)
        tl, tr, td, tu = nb(f[FT], 0, -1), nb(f[FT], 0, 1), nb(f[FT], -1, 0), nb(f[FT], 1, 0)
        nb_ok = ok(FV, vl) & ok(FV, vr) & ok(FU, ul) & ok(FU, uh) & ok(FT, tl) & ok(FT, tr) & ok(FT, td) & ok(FT, tu)
        dxv = hx * (vr - vl).astype(np.float64)  # the difference in float32, the products in float64
        dyu = hy * (uh - ul).astype(np.float64)
        dxt = hx * (tr - tl).astype(np.float64)
        dyt = hy * (tu - td).astype(np.float64)
        zeta = dxv - dyu
        za = zeta if fcoriolis is None else zeta + np.asarray(fcoriolis, np.float32)[1:-1, 1:-1].astype(np.float64)
        Du, Dv, Dt = D[FU][mid], D[FV][mid], D[FT][mid]
        t1 = za * Dt
        t2 = Dv * dxt
        t3 = Du * dyt
        S = (t1 - t2) + t3
        r = (np.float64(scale) * S).astype(np.float32)
    bad = vbad[FU][mid] | vbad[FV][mid] | vbad[FT][mid] | ~nb_ok
    inner = np.where(bad, undef, r).astype(np.float32)
    if terms is not None:
        terms.update(za=za, Du=Du, Dv=Dv, Dt=Dt, dxv=dxv, dyu=dyu, dxt=dxt, dyt=dyt, t1=t1, t2=t2, t3=t3, S=S, bad=bad)
    yc = np.clip(np.arange(ny), 1, ny - 2) - 1
    xc = np.clip(np.arange(nx), 1, nx - 2) - 1
    out = inner[:, yc][:, :, xc]
    fd = np.array([classify(int(bad[k].sum()), (nx - 2) * (ny - 2)) for k in range(nlev)], np.int32)
    return np.ascontiguousarray(out), fd


def hlevels(u, v, th, ps, alevel, blevel, xmapr, ymapr, fcoriolis=None, method=CENTRED, scale=1.0, flags=None, fdef_ps=SOME_DEFINED, undef=UNDEF, terms=None):
    c = hybrid_coordinate(ps, alevel, blevel)
    psd = is_defined(fdef_ps == ALL_DEFINED, np.asarray(ps, np.float32), undef)
    return potential_vorticity(u, v, th, c, np.broadcast_to(psd, c.shape), xmapr, ymapr, fcoriolis, method, scale, flags, undef, terms)


def coord_fields(u, v, th, p, xmapr, ymapr, fcoriolis=None, method=CENTRED, scale=1.0, flags=None, fdef_coord=None, undef=UNDEF, terms=None):
    c = np.asarray(p, np.float32)
    fc = [SOME_DEFINED] * c.shape[0] if fdef_coord is None else list(fdef_coord)
    cdef = np.stack([is_defined(fc[k] == ALL_DEFINED, c[k], undef) for k in range(c.shape[0])])
    return potential_vorticity(u, v, th, c, cdef, xmapr, ymapr, fcoriolis, method, scale, flags, undef, terms)


def levels(u, v, th, levs, xmapr, ymapr, fcoriolis=None, method=CENTRED, scale=1.0, flags=None, undef=UNDEF, terms=None):
    """The coordinate is one constant per level: always defined (the call refuses a NaN level)."""
    c = np.asarray(levs, np.float32).reshape(-1, 1, 1)
    shape = np.asarray(u).shape
    return potential_vorticity(u, v, th, c, np.ones(shape, bool), xmapr, ymapr, fcoriolis, method, scale, flags, undef, terms)


# ---------------------------------------------------------------------------------------------- case generators
def pv_case(nlev=13, ny=9, nx=12, seed=3, undef=UNDEF, frac=0.02):
    """Wind, a potential temperature that rises with height (the levels top-down), ps, the levels, maps and f; `frac` of
    each field and of ps undefined, and a cell of every field NaN.  Returns a dict."""
    rng = np.random.default_rng(seed)
    alevel, blevel = hybrid_levels(nlev)

    def holes(a):
        a = a.copy()
        a[rng.random(a.shape) < frac] = undef
        return a

    ps = holes(rng.uniform(700, 1050, (ny, nx)).astype(np.float32))
    u = holes(rng.normal(10, 8, (nlev, ny, nx)).astype(np.float32))
    v = holes(rng.normal(0, 8, (nlev, ny, nx)).astype(np.float32))
    th = holes((rng.normal(0, 2, (nlev, ny, nx)) + np.linspace(420, 285, nlev).reshape(-1, 1, 1)).astype(np.float32))
    if nlev * ny * nx > 60:
        for j, a in enumerate((u, v, th)):
            a.reshape(-1)[7 + 11 * j] = np.nan
    p = hybrid_coordinate(np.where(ps == undef, np.float32(900), ps), alevel, blevel)
    p[:, ps == undef] = undef
    xm = rng.uniform(0.5e-5, 2e-5, (ny, nx)).astype(np.float32)
    ym = rng.uniform(0.5e-5, 2e-5, (ny, nx)).astype(np.float32)
    fc = rng.uniform(0.5e-4, 1.4e-4, (ny, nx)).astype(np.float32)
    levs = np.round(1000 * np.linspace(0.17, 1, nlev) ** 2).astype(np.float32)
    return dict(u=u, v=v, th=th, ps=ps, alevel=alevel, blevel=blevel, p=p, levels=levs, xmapr=xm, ymapr=ym, fcoriolis=fc)
