"""Numpy restatement of mifc_vlayer_hlevels / mifc_vlayer_fields (include/mifc.h, "layer integrals, means and extremes
of level batches"): the oracle of tests/test_gpu_vlayer.py.  The coordinate in float32, the end values, the extent and
the accumulators step by step in float64 (every ufunc rounds once, so nothing is contracted), the pairs walked in index
order.  The case generators are the ones of vinterp_restate."""
import numpy as np

from vinterp_restate import (ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, hybrid_coordinate, hybrid_levels,  # noqa: F401
                             is_defined, main_case, sprinkle)

INTEGRAL, MEAN, MAX, MIN, COORD_OF_MAX, COORD_OF_MIN = 1, 2, 3, 4, 5, 6
ALL_PRODUCTS = [INTEGRAL, MEAN, MAX, MIN, COORD_OF_MAX, COORD_OF_MIN]
NAMES = {"integral": INTEGRAL, "mean": MEAN, "max": MAX, "min": MIN, "coord_of_max": COORD_OF_MAX, "coord_of_min": COORD_OF_MIN}
INF = np.float32(np.inf)


def layer(fields, coord, coord_defined, products, lo=-INF, hi=INF, flags=None, undef=UNDEF):
    """fields float32 (nf, nlev, ny, nx); coord float32 (nlev, ny, nx) and coord_defined bool of the same shape (rule 1 of
    vinterp); lo, hi: a number or an (ny, nx) array (a bound given as a field: tested per cell); flags None
    (SOME_DEFINED) or (nf, nlev).  Returns (out (nf, nproducts, ny, nx), flags_out int32 (nf, nproducts))."""
    x = np.asarray(fields, np.float32)
    nf, nlev, ny, nx = x.shape
    cells = ny * nx
    x = x.reshape(nf, nlev, cells)
    c = np.asarray(coord, np.float32).reshape(nlev, cells)
    undef = np.float32(undef)
    products = [NAMES.get(p, p) for p in products]
    fl = np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)
    with np.errstate(all="ignore"):
        # rule 1
        cell_bad = ~(np.asarray(coord_defined, bool).reshape(nlev, cells) & ~np.isnan(c)).all(axis=0)
        # rule 2
        bound = []
        for v in (lo, hi):
            if np.ndim(v) == 0:
                bound.append(np.full(cells, np.float32(v), np.float32))
            else:
                v = np.asarray(v, np.float32).reshape(cells)
                cell_bad |= np.isnan(v) | (v == undef)
                bound.append(v)
        L, H = bound
        cell_bad |= ~(L < H)
        # rules 3 to 6
        any_part = np.zeros(cells, bool)
        hole = np.zeros((nf, cells), bool)
        ext = np.zeros(cells, np.float64)
        acc = np.zeros((nf, cells), np.float64)
        mx, mn = np.zeros((nf, cells), np.float32), np.zeros((nf, cells), np.float32)
        cmx, cmn = np.zeros((nf, cells), np.float32), np.zeros((nf, cells), np.float32)
        for k in range(nlev - 1):
            ck, ck1 = c[k], c[k + 1]
            rising = ck <= ck1
            p, q = np.where(rising, ck, ck1), np.where(rising, ck1, ck)
            a, b = np.where(p >= L, p, L), np.where(q <= H, q, H)
            part = a < b
            if not part.any():
                continue
            dk, dk1 = ck.astype(np.float64), ck1.astype(np.float64)
            span = dk1 - dk
            d = b.astype(np.float64) - a.astype(np.float64)
            ext = np.where(part, ext + d, ext)
            first = part & ~any_part
            for f in range(nf):
                xk, xk1 = x[f, k], x[f, k + 1]
                ok = is_defined(fl[f, k] == ALL_DEFINED, xk, undef) & is_defined(fl[f, k + 1] == ALL_DEFINED, xk1, undef)
                hole[f] |= part & ~ok
                xd, xd1 = xk.astype(np.float64), xk1.astype(np.float64)
                diff = xd1 - xd
                v = []
                for e in (a, b):
                    w = (e.astype(np.float64) - dk) / span
                    v.append(np.where(e == ck, xd, np.where(e == ck1, xd1, xd + w * diff)))
                va, vb = v
                term = ((va + vb) * 0.5) * d
                acc[f] = np.where(part, acc[f] + term, acc[f])
                # the end nearer level k first, then the other
                cands = ((np.where(rising, va, vb).astype(np.float32), np.where(rising, a, b), first),
                         (np.where(rising, vb, va).astype(np.float32), np.where(rising, b, a), np.zeros(cells, bool)))
                for vf, e, init in cands:
                    up, down = part & (init | (vf > mx[f])), part & (init | (vf < mn[f]))
                    mx[f], cmx[f] = np.where(up, vf, mx[f]), np.where(up, e, cmx[f])
                    mn[f], cmn[f] = np.where(down, vf, mn[f]), np.where(down, e, cmn[f])
            any_part |= part
        cell_bad |= ~any_part
        value = {INTEGRAL: acc.astype(np.float32), MEAN: (acc / ext).astype(np.float32), MAX: mx, MIN: mn, COORD_OF_MAX: cmx, COORD_OF_MIN: cmn}
    bad = hole | cell_bad
    out = np.stack([np.where(bad, undef, value[p]) for p in products], axis=1).astype(np.float32)
    fd = np.array([[classify(int(bad[f].sum()), cells)] * len(products) for f in range(nf)], np.int32)
    return out.reshape(nf, len(products), ny, nx), fd


def hlevels(fields, ps, alevel, blevel, products, lo=-INF, hi=INF, flags=None, fdef_ps=SOME_DEFINED, undef=UNDEF):
    c = hybrid_coordinate(ps, alevel, blevel)
    psd = is_defined(fdef_ps == ALL_DEFINED, np.asarray(ps, np.float32), undef)
    return layer(fields, c, np.broadcast_to(psd, c.shape), products, lo, hi, flags, undef)


def coord_fields(fields, coord, products, lo=-INF, hi=INF, flags=None, fdef_coord=None, undef=UNDEF):
    c = np.asarray(coord, np.float32)
    fc = [SOME_DEFINED] * c.shape[0] if fdef_coord is None else list(fdef_coord)
    cdef = np.stack([is_defined(fc[k] == ALL_DEFINED, c[k], undef) for k in range(c.shape[0])])
    return layer(fields, c, cdef, products, lo, hi, flags, undef)


# the layers of the main case: open, two inside the column, one that reaches below the ground, one below every column
MAIN_LAYERS = [(-INF, INF), (300, 850), (500, 2000), (1060, 1100)]
