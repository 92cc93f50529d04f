"""Numpy restatement of mifc_vinterp_hlevels / mifc_vinterp_fields (include/mifc.h, "interpolation of level batches to
constant surfaces"): the oracle of tests/test_gpu_vinterp.py.  The coordinate in float32, the weight and the result step
by step in float64 (every ufunc rounds once, so nothing is contracted), the levels walked in index order.  Also the
case generators the CPU and GPU tests share."""
import numpy as np

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
LINEAR, LOG = 0, 1
UNDEF = np.float32(1.0e35)


def classify(n_undefined, n):
    """miutil::checkDefined, FieldDefined.cc:62-70."""
    if n_undefined == 0:
        return ALL_DEFINED
    return NONE_DEFINED if n_undefined == n else SOME_DEFINED


def is_defined(all_defined, x, undef):
    """FieldCalculations.h:42-50 on an array: an ALL_DEFINED flag switches the test off."""
    if all_defined:
        return np.ones(x.shape, bool)
    return ~np.isnan(x) & (x != np.float32(undef))


def hybrid_coordinate(ps, alevel, blevel):
    """p_hlevel, FieldCalculations.cc:303, per level: the float product rounded, then the float sum."""
    ps = np.asarray(ps, np.float32)
    a, b = np.asarray(alevel, np.float32), np.asarray(blevel, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([(a[k] + (b[k] * ps).astype(np.float32)).astype(np.float32) for k in range(a.size)])


def interpolate(fields, coord, coord_defined, targets, method, flags=None, undef=UNDEF, prefilter=None):
    """fields float32 (nf, nlev, ny, nx); coord float32 (nlev, ny, nx) and coord_defined bool of the same shape (rule 1);
    flags None (SOME_DEFINED) or (nf, nlev).  Returns (out (nf, nt, ny, nx), flags_out int32 (nf, nt)).  prefilter: not part
    of the definition -- a test's model of a filter in front of the bracket test, called as prefilter(k, t) and giving per
    cell whether the pair (k, k + 1) is looked at for target t at all."""
    x = np.asarray(fields, np.float32)
    nf, nlev, ny, nx = x.shape
    cells = ny * nx
    x = x.reshape(nf, nlev, cells)
    c = np.asarray(coord, np.float32).reshape(nlev, cells)
    cdef = np.asarray(coord_defined, bool).reshape(nlev, cells)
    undef = np.float32(undef)
    tg = np.asarray(targets, np.float32).ravel()
    fl = np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)
    out = np.full((nf, tg.size, cells), undef, np.float32)
    bad = np.ones((nf, tg.size, cells), bool)
    with np.errstate(all="ignore"):
        for t, ct in enumerate(tg):
            found = np.zeros(cells, bool)
            for k in range(nlev - 1):
                ck, ck1 = c[k], c[k + 1]
                lo, hi = np.minimum(ck, ck1), np.maximum(ck, ck1)  # a NaN comes through and fails both comparisons
                br = cdef[k] & cdef[k + 1] & (lo <= ct) & (ct <= hi) & ~found
                if prefilter is not None:
                    br &= prefilter(k, t)
                if not br.any():
                    continue
                found |= br
                dk, dk1 = ck.astype(np.float64), ck1.astype(np.float64)
                if method == LOG:
                    lk = np.log(dk)
                    w = (np.log(np.float64(ct)) - lk) / (np.log(dk1) - lk)
                    usable = lo > 0
                else:
                    w = (np.float64(ct) - dk) / (dk1 - dk)
                    usable = np.ones(cells, bool)
                for f in range(nf):
                    xk, xk1 = x[f, k], x[f, k + 1]
                    ok = is_defined(fl[f, k] == ALL_DEFINED, xk, undef) & is_defined(fl[f, k + 1] == ALL_DEFINED, xk1, undef) & usable
                    xd = xk.astype(np.float64)
                    v = (xd + w * (xk1.astype(np.float64) - xd)).astype(np.float32)
                    r = np.where(ok, np.where(ck == ck1, xk, v), undef)
                    out[f, t, br] = r[br]
                    bad[f, t, br] = ~ok[br]
    fd = np.array([[classify(int(bad[f, t].sum()), cells) for t in range(tg.size)] for f in range(nf)], np.int32)
    return out.reshape(nf, tg.size, ny, nx), fd


def hlevels(fields, ps, alevel, blevel, targets, method, flags=None, fdef_ps=SOME_DEFINED, undef=UNDEF, prefilter=None):
    c = hybrid_coordinate(ps, alevel, blevel)
    psd = is_defined(fdef_ps == ALL_DEFINED, np.asarray(ps, np.float32), undef)
    return interpolate(fields, c, np.broadcast_to(psd, c.shape), targets, method, flags, undef, prefilter)


def coord_fields(fields, coord, targets, method, flags=None, fdef_coord=None, undef=UNDEF, prefilter=None):
    c = np.asarray(coord, np.float32)
    fc = [SOME_DEFINED] * c.shape[0] if fdef_coord is None else list(fdef_coord)
    cdef = np.stack([is_defined(fc[k] == ALL_DEFINED, c[k], undef) for k in range(c.shape[0])])
    return interpolate(fields, c, cdef, targets, method, flags, undef, prefilter)


# ---------------------------------------------------------------------------------------------- case generators
MAIN_TARGETS = np.array([1000, 925, 850, 700, 500, 300, 100, 10, 0.5], np.float32)


def hybrid_levels(nlev=12):
    """eta = linspace(0.02, 1, nlev) ** 1.5, b = eta^2, a = 1000 (eta - eta^2): top-down, the ground last."""
    eta = np.linspace(0.02, 1, nlev) ** 1.5
    return (1000 * (eta - eta ** 2)).astype(np.float32), (eta ** 2).astype(np.float32)


def sprinkle(a, rng, frac, value):
    a = a.copy()
    a[rng.random(a.shape) < frac] = value
    return a


def main_case(nf=3, nlev=12, ny=9, nx=13, seed=1, undef=UNDEF, frac=0.03):
    """The main generator: ps uniform in 700..1050, 3 % of ps and of each field undefined."""
    rng = np.random.default_rng(seed)
    alevel, blevel = hybrid_levels(nlev)
    ps = sprinkle(rng.uniform(700, 1050, (ny, nx)).astype(np.float32), rng, frac, undef)
    fields = np.stack([sprinkle((rng.normal(0, 10, (nlev, ny, nx)) + 250 - 5 * f).astype(np.float32), rng, frac, undef) for f in range(nf)])
    return fields, ps, alevel, blevel


def targets_n(n, seed=5):
    """n targets between 1 and 1100 hPa, in no order (some above the top, some below the ground)."""
    return np.random.default_rng(seed).uniform(1, 1100, n).astype(np.float32)
