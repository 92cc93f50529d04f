"""Numpy restatement of mifc_vcumul_hlevels / mifc_vcumul_fields / mifc_vcumul_levels (include/mifc.h, "running vertical
integrals of level batches"): the oracle of tests/test_gpu_vcumul.py.  The coordinate in float32, g(c), the sum and the
result step by step in float64 (every ufunc rounds once, so nothing is contracted), the levels walked in the order of
the call.  No loop over cells.  The case generators are the ones of vinterp_restate."""
import numpy as np

from vinterp_restate import (ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, hybrid_coordinate, hybrid_levels,  # noqa: F401
                             is_defined, main_case, sprinkle)

LINEAR, LOG = 0, 1
FROM_FIRST, FROM_LAST = 0, 1
METHODS = {"linear": LINEAR, "log": LOG}
FROM = {"first": FROM_FIRST, "last": FROM_LAST}


def g_of(c, method):
    """Rule 1: (double)c, or its logarithm; with whether c is usable besides being defined."""
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        if method == LOG:
            return np.log(c.astype(np.float64)), c > 0
        return c.astype(np.float64), ~np.isnan(c)


def cumulate(fields, coord, coord_defined, method=LINEAR, from_=FROM_FIRST, start=None, fdef_start=SOME_DEFINED, base=None, fdef_base=None,
             scale=None, flags=None, undef=UNDEF, sums=None):
    """fields float32 (nf, nlev, ny, nx); coord float32 (nlev, ny, nx) or (nlev, 1, 1) and coord_defined bool like it
    (rule 1 of vinterp); start None or (ny, nx); base None or a sequence of nf planes (ny, nx) or None; fdef_base None or
    nf flags; scale None or nf factors; flags None (SOME_DEFINED) or (nf, nlev).  Returns (out (nf, nlev, ny, nx),
    flags_out int32 (nf, nlev)).  sums: a float64 array like out that receives S of every level."""
    x = np.asarray(fields, np.float32)
    nf, nlev, ny, nx = x.shape
    cells = ny * nx
    x = x.reshape(nf, nlev, cells)
    c = np.broadcast_to(np.asarray(coord, np.float32), (nlev, ny, nx)).reshape(nlev, cells)
    cdef = np.broadcast_to(np.asarray(coord_defined, bool), (nlev, ny, nx)).reshape(nlev, cells)
    undef = np.float32(undef)
    method, from_ = METHODS.get(method, method), FROM.get(from_, from_)
    fl = np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)
    out = np.full((nf, nlev, cells), undef, np.float32)
    bad = np.ones((nf, nlev, cells), bool)
    ssum = np.zeros((nf, nlev, cells), np.float64)
    order = list(range(nlev)) if from_ == FROM_FIRST else list(range(nlev - 1, -1, -1))  # rule 2
    with np.errstate(all="ignore"):
        g, ok = g_of(c, method)
        usable_c = cdef & ok  # rule 1
        cell_ok = np.ones(cells, bool)
        gs = None
        if start is not None:  # rule 4
            s = np.asarray(start, np.float32).reshape(cells)
            gs, sok = g_of(s, method)
            cell_ok = is_defined(fdef_start == ALL_DEFINED, s, undef) & sok
        for f in range(nf):
            alive = cell_ok.copy()
            b = None
            if base is not None and base[f] is not None:  # rule 6
                b = np.asarray(base[f], np.float32).reshape(cells)
                fb = SOME_DEFINED if fdef_base is None else np.asarray(fdef_base).reshape(-1)[f]
                alive &= is_defined(fb == ALL_DEFINED, b, undef) & ~np.isnan(b)
            sc = np.float64(1.0) if scale is None else np.float64(np.asarray(scale, np.float64).reshape(-1)[f])
            xd = x[f].astype(np.float64)
            S = np.zeros(cells, np.float64)
            for m, k in enumerate(order):
                alive = alive & usable_c[k] & is_defined(fl[f, k] == ALL_DEFINED, x[f, k], undef)  # rules 3 and 6
                if m == 0:
                    if gs is not None:
                        S = xd[k] * (g[k] - gs)  # rule 4
                else:
                    a = order[m - 1]
                    S = S + ((xd[a] + xd[k]) * 0.5) * (g[k] - g[a])  # rule 5
                p = sc * S
                r = (p if b is None else b.astype(np.float64) + p).astype(np.float32)  # rule 7
                out[f, k] = np.where(alive, r, undef)
                bad[f, k] = ~alive
                ssum[f, k] = S
    if sums is not None:
        sums[...] = ssum.reshape(sums.shape)
    fd = np.array([[classify(int(bad[f, k].sum()), cells) for k in range(nlev)] for f in range(nf)], np.int32)
    return out.reshape(nf, nlev, ny, nx), fd


def hlevels(fields, ps, alevel, blevel, method=LINEAR, from_=FROM_FIRST, flags=None, fdef_ps=SOME_DEFINED, undef=UNDEF, **kw):
    c = hybrid_coordinate(ps, alevel, blevel)
    psd = is_defined(fdef_ps == ALL_DEFINED, np.asarray(ps, np.float32), undef)
    return cumulate(fields, c, np.broadcast_to(psd, c.shape), method, from_, flags=flags, undef=undef, **kw)


def coord_fields(fields, coord, method=LINEAR, from_=FROM_FIRST, flags=None, fdef_coord=None, undef=UNDEF, **kw):
    c = np.asarray(coord, np.float32)
    fc = [SOME_DEFINED] * c.shape[0] if fdef_coord is None else list(fdef_coord)
    cdef = np.stack([is_defined(fc[k] == ALL_DEFINED, c[k], undef) for k in range(c.shape[0])])
    return cumulate(fields, c, cdef, method, from_, flags=flags, undef=undef, **kw)


def levels(fields, levs, method=LINEAR, from_=FROM_FIRST, flags=None, undef=UNDEF, **kw):
    """The coordinate is one constant per level: always defined (the call refuses a level that is not usable)."""
    x = np.asarray(fields, np.float32)
    c = np.asarray(levs, np.float32).reshape(-1, 1, 1)
    return cumulate(x, c, np.ones(c.shape, bool), method, from_, flags=flags, undef=undef, **kw)


def neighbours(got, exp):
    """got is exp or the float next to it, element by element (a NaN matches a NaN)."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    with np.errstate(all="ignore"):
        near = (got == exp) | (got == np.nextafter(exp, np.float32(np.inf))) | (got == np.nextafter(exp, np.float32(-np.inf)))
    return near | (np.isnan(got) & np.isnan(exp))


# ---------------------------------------------------------------------------------------------- case generators
def main_levels(nlev=12):
    """Pressure levels for the `levels` form, top-down, unevenly spaced."""
    return np.round(1000 * np.linspace(0.17, 1, nlev) ** 2).astype(np.float32)


def cumul_case(nf=3, nlev=12, ny=9, nx=13, seed=1, undef=UNDEF, frac=0.03):
    """main_case of vinterp_restate (positive fields around 250, 3 % of every field and of ps undefined) with the pressure
    of its levels as a coordinate batch, two start planes -- starts[FROM_FIRST] above the top level, starts[FROM_LAST] below
    the lowest one, so that a walk keeps its sign; some cells undefined, one not positive -- and base planes (some cells
    undefined)."""
    fields, ps, alevel, blevel = main_case(nf, nlev, ny, nx, seed, undef, frac)
    rng = np.random.default_rng(seed + 1000)
    coord = hybrid_coordinate(np.where(is_defined(False, ps, undef), ps, np.float32(900)), alevel, blevel)
    coord[:, ~is_defined(False, ps, undef)] = undef
    starts = np.stack([sprinkle(rng.uniform(lo, hi, (ny, nx)).astype(np.float32), rng, frac, undef) for lo, hi in ((0.5, 2.0), (1050, 1100))])
    starts.reshape(2, -1)[:, -1] = np.float32(-5.0)
    base = np.stack([sprinkle(rng.uniform(-50, 3000, (ny, nx)).astype(np.float32), rng, frac, undef) for _ in range(nf)])
    return fields, ps, (alevel, blevel), coord, starts, base
