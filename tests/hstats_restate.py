"""Numpy restatement of mifc_hstats_levels (include/mifc.h, "horizontal statistics of level batches"): the oracle of
tests/test_gpu_hstats.py.  Two forms of rules 1-7: hstats(), vectorised over levels and rows with a loop over the at most
64 sequential steps of a partial and the six merge steps, and hstats_literal(), a cell-by-cell Python loop for tiny
shapes.  Every operation is one float64 operation (a numpy ufunc or a Python float operator rounds once), so the order
of the additions is the definition's."""
import numpy as np

from vinterp_restate import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, is_defined, sprinkle  # noqa: F401

SEGMENT, LANES, CELLS = 4096, 64, 4  # rule 3: cells of a segment, partials, consecutive cells of a trip
TRIPS = SEGMENT // (LANES * CELLS)
AREA, ROWS = 0, 1
MODES = {"area": AREA, "rows": ROWS}
MOMENTS, EXTREMES = 1, 2
N, W, S1, S2, MIN, MAX, IMIN, IMAX = range(8)


def _box(box, ny, nx):
    i0, i1, j0, j1 = (0, nx, 0, ny) if box is None else (int(b) for b in box)
    assert 0 <= i0 < i1 <= nx and 0 <= j0 < j1 <= ny
    return i0, i1, j0, j1


def _flags(flags, nf, nlev):
    return np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)


# Departures from the definition that a test may ask for by name (`mistakes`): what a kernel that is subtly wrong would
# compute.  tests/test_horizontal_range_cpu.py shows that the cases of tests/horizontal_range_cases.py tell each from the rules.
MISTAKES = ("masked by multiplication", "doubles flushed", "undef after the fact")


def flushed64(a):
    """Subnormal doubles replaced by zeros of their sign."""
    with np.errstate(invalid="ignore"):
        return np.where((a != 0) & (np.abs(a) < np.finfo(np.float64).tiny), np.copysign(0.0, a), a)


def cell_quantities(x, flag, y, flag_y, pivot, weight, fdef_weight, box, undef=UNDEF, mistakes=()):
    """Rules 1 and 2 for one level x (ny, nx): (included, d, w, q1, q2) over the whole level, float64; excluded cells
    carry w = q1 = q2 = +0.0 (d is whatever it is there).  mistakes: see hstats()."""
    undef = np.float32(undef)
    ny, nx = x.shape
    i0, i1, j0, j1 = box
    inc = np.zeros((ny, nx), bool)
    inc[j0:j1, i0:i1] = True
    inc &= is_defined(flag == ALL_DEFINED, x, undef)
    with np.errstate(all="ignore"):
        d = x.astype(np.float64)
        if y is not None:
            inc &= is_defined(flag_y == ALL_DEFINED, y, undef)
            d = d - y.astype(np.float64)
        d = d - np.float64(pivot)
        if weight is not None:
            inc &= is_defined(fdef_weight == ALL_DEFINED, weight, undef)
            w = weight.astype(np.float64)
        else:
            w = np.ones((ny, nx))
        if "doubles flushed" in mistakes:  # (a float widened to double is never a subnormal double: the pivot and the results are)
            d = flushed64(x.astype(np.float64) - (0.0 if y is None else y.astype(np.float64)))
            d = flushed64(d - flushed64(np.float64(pivot)))
        q1 = w * d
        q2 = q1 * d
        if "doubles flushed" in mistakes:
            q1 = flushed64(q1)
            q2 = flushed64(q1 * d)
        if "masked by multiplication" in mistakes:  # 0 * inf and 0 * NaN are NaN; 0 * -1 is -0.0
            m = inc.astype(np.float64)
            return inc, d, m * w, m * q1, m * q2
    zero = np.float64(0.0)
    return inc, d, np.where(inc, w, zero), np.where(inc, q1, zero), np.where(inc, q2, zero)


def segment_sums(q, i0, i1):
    """Rule 3 for q (..., nx), zero outside the included cells: the sums of the segments that the columns i0 .. i1 - 1
    touch, (..., nsegs)."""
    nx = q.shape[-1]
    s_lo, s_hi = i0 // SEGMENT, (i1 - 1) // SEGMENT
    nsegs = s_hi - s_lo + 1
    padded = np.zeros(q.shape[:-1] + (nsegs * SEGMENT,))
    lo, hi = s_lo * SEGMENT, min(nx, (s_hi + 1) * SEGMENT)
    padded[..., :hi - lo] = q[..., lo:hi]
    cells = padded.reshape(q.shape[:-1] + (nsegs, TRIPS, LANES, CELLS))
    with np.errstate(all="ignore"):
        p = np.zeros(q.shape[:-1] + (nsegs, LANES))
        for t in range(TRIPS):  # partial l: its cells in ascending column order, from +0.0
            for c in range(CELLS):
                p = p + cells[..., t, :, c]
        s = LANES // 2
        while s >= 1:  # P[t] = P[t] + P[t + s] for t < s
            p = p[..., :s] + p[..., s:2 * s]
            s //= 2
    return p[..., 0]


def combine(segs, mode):
    """Rule 4 for segs (..., nrows, nsegs): (..., nrows) or (..., 1)."""
    with np.errstate(all="ignore"):
        if mode == ROWS:
            acc = np.zeros(segs.shape[:-1])
            for s in range(segs.shape[-1]):
                acc = acc + segs[..., s]
            return acc
        flat = segs.reshape(segs.shape[:-2] + (-1,))
        acc = np.zeros(flat.shape[:-1])
        for s in range(flat.shape[-1]):
            acc = acc + flat[..., s]
        return acc[..., None]


def extremes(inc, d, box, mode):
    """Rule 6 for one level: (min, max, imin, imax) as float64 arrays of nrows values."""
    ny, nx = d.shape
    i0, i1, j0, j1 = box
    out = []
    for sign in (1, -1):
        start = np.inf * sign
        with np.errstate(all="ignore"):
            cand = np.where(inc & ~np.isnan(d), d, start)[j0:j1]
        idx = (np.arange(j0, j1)[:, None] * nx + np.arange(nx)[None, :]).astype(np.int64)
        if mode == AREA:
            cand, idx = cand.reshape(1, -1), idx.reshape(1, -1)
        at = np.argmin(cand, axis=1) if sign == 1 else np.argmax(cand, axis=1)  # the first of equal values
        rows = np.arange(cand.shape[0])
        val = cand[rows, at]
        hit = val != start
        out.append((np.where(hit, val, start), np.where(hit, idx[rows, at], -1).astype(np.float64)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def hstats(fields, minus=None, pivot=None, weight=None, box=None, mode=AREA, products=MOMENTS | EXTREMES, flags=None, flags_minus=None,
           fdef_weight=SOME_DEFINED, undef=UNDEF, fill=0.0, mistakes=()):
    """fields float32 (nf, nlev, ny, nx); minus None or like fields; pivot None or (nf, nlev) float64; weight None or
    float32 (ny, nx); box None or (i0, i1, j0, j1).  Returns (stats float64 (nf, nlev, nrows, 8), mean float32
    (nf, nlev, nrows), flags int32 (nf, nlev)); the slots of a group that is not in `products` hold `fill`.  mistakes: not
    part of the definition -- names from MISTAKES: "masked by multiplication" multiplies w, q1 and q2 of every cell by 1.0
    or 0.0 instead of selecting; "doubles flushed" takes every subnormal double of rule 2 for a zero; "undef after the
    fact" takes a mean equal to undef for a hole."""
    assert all(m in MISTAKES for m in mistakes), mistakes
    f = np.asarray(fields, np.float32)
    nf, nlev, ny, nx = f.shape
    mode = MODES.get(mode, mode)
    bx = _box(box, ny, nx)
    i0, i1, j0, j1 = bx
    nrows = 1 if mode == AREA else j1 - j0
    fl, flm = _flags(flags, nf, nlev), _flags(flags_minus, nf, nlev)
    pv = np.zeros((nf, nlev)) if pivot is None else np.asarray(pivot, np.float64).reshape(nf, nlev)
    y = None if minus is None else np.asarray(minus, np.float32)
    wt = None if weight is None else np.asarray(weight, np.float32)
    undef = np.float32(undef)
    stats = np.full((nf, nlev, nrows, 8), fill, np.float64)
    mean = np.full((nf, nlev, nrows), undef, np.float32)
    fd = np.zeros((nf, nlev), np.int32)
    for g in range(nf):
        q = [cell_quantities(f[g, k], fl[g, k], None if y is None else y[g, k], flm[g, k], pv[g, k], wt, fdef_weight, bx, undef, mistakes)
             for k in range(nlev)]
        inc, d = np.stack([c[0] for c in q]), np.stack([c[1] for c in q])
        if products & MOMENTS:
            count = inc[:, j0:j1].sum(axis=2).astype(np.float64)
            stats[g, :, :, N] = count.sum(axis=1, keepdims=True) if mode == AREA else count
            for slot, m in ((W, 2), (S1, 3), (S2, 4)):
                stats[g, :, :, slot] = combine(segment_sums(np.stack([c[m] for c in q])[:, j0:j1], i0, i1), mode)
            with np.errstate(all="ignore"):
                value = (pv[g][:, None] + stats[g, :, :, S1] / stats[g, :, :, W]).astype(np.float32)
            hole = (stats[g, :, :, N] == 0) | (stats[g, :, :, W] == 0.0)
            if "undef after the fact" in mistakes:
                hole = hole | (value == undef)
            mean[g] = np.where(hole, undef, value)
            for k in range(nlev):
                fd[g, k] = classify(int(hole[k].sum()), nrows)
        if products & EXTREMES:
            for k in range(nlev):
                stats[g, k, :, MIN], stats[g, k, :, MAX], stats[g, k, :, IMIN], stats[g, k, :, IMAX] = extremes(inc[k], d[k], bx, mode)
    return stats, mean, fd


def hstats_literal(fields, minus=None, pivot=None, weight=None, box=None, mode=AREA, flags=None, flags_minus=None, fdef_weight=SOME_DEFINED,
                   undef=UNDEF):
    """Rules 1-7 cell by cell in Python floats (IEEE doubles, one rounding per operator); both product groups."""
    f = np.asarray(fields, np.float32)
    nf, nlev, ny, nx = f.shape
    mode = MODES.get(mode, mode)
    i0, i1, j0, j1 = _box(box, ny, nx)
    nrows = 1 if mode == AREA else j1 - j0
    fl, flm = _flags(flags, nf, nlev), _flags(flags_minus, nf, nlev)
    undef = np.float32(undef)

    def defined(all_defined, v):
        return all_defined or (not np.isnan(v) and v != undef)

    stats = np.zeros((nf, nlev, nrows, 8), np.float64)
    mean = np.full((nf, nlev, nrows), undef, np.float32)
    fd = np.zeros((nf, nlev), np.int32)
    with np.errstate(all="ignore"):
        for g in range(nf):
            for k in range(nlev):
                p = 0.0 if pivot is None else float(np.asarray(pivot, np.float64).reshape(nf, nlev)[g, k])
                acc = [[0.0, 0.0, 0.0, 0.0, np.inf, -np.inf, -1.0, -1.0] for _ in range(nrows)]
                for j in range(j0, j1):
                    a = acc[0 if mode == AREA else j - j0]
                    for s in range(i0 // SEGMENT, (i1 - 1) // SEGMENT + 1):
                        part = [[np.float64(0.0)] * 3 for _ in range(LANES)]
                        for i in range(max(i0, s * SEGMENT), min(i1, (s + 1) * SEGMENT)):  # ascending: each partial sees its cells in order
                            x = f[g, k, j, i]
                            ok = defined(fl[g, k] == ALL_DEFINED, x)
                            d = np.float64(x)
                            if minus is not None:
                                y = np.float32(minus[g][k][j][i])
                                ok = ok and defined(flm[g, k] == ALL_DEFINED, y)
                                d = d - np.float64(y)
                            d = d - np.float64(p)
                            w = np.float64(1.0)
                            if weight is not None:
                                wv = np.float32(weight[j][i])
                                ok = ok and defined(fdef_weight == ALL_DEFINED, wv)
                                w = np.float64(wv)
                            if not ok:
                                continue
                            q1 = w * d
                            q2 = q1 * d
                            lane = part[(i // CELLS) % LANES]
                            lane[0], lane[1], lane[2] = lane[0] + w, lane[1] + q1, lane[2] + q2
                            a[N] += 1.0
                            if d < a[MIN]:
                                a[MIN], a[IMIN] = d, float(j * nx + i)
                            if d > a[MAX]:
                                a[MAX], a[IMAX] = d, float(j * nx + i)
                        step = LANES // 2
                        while step >= 1:
                            for t in range(step):
                                for m in range(3):
                                    part[t][m] = part[t][m] + part[t + step][m]
                            step //= 2
                        for m, slot in enumerate((W, S1, S2)):  # rule 4: both modes add the segment sums in row-major order
                            a[slot] = np.float64(a[slot]) + part[0][m]
                holes = 0
                for r in range(nrows):
                    stats[g, k, r] = acc[r]
                    if acc[r][N] == 0 or acc[r][W] == 0.0:
                        holes += 1
                    else:
                        mean[g, k, r] = np.float32(np.float64(p) + np.float64(acc[r][S1]) / np.float64(acc[r][W]))
                fd[g, k] = classify(holes, nrows)
    return stats, mean, fd


def same_bits64(a, b):
    """Bit for bit on float64, a NaN matching any NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    an, bn = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(an, bn) and np.array_equal(a[~an].view(np.uint64), b[~bn].view(np.uint64))


# ---------------------------------------------------------------------------------------------- case generators
def wide_fields(shape, seed, frac=0.03, undef=UNDEF):
    """float32(normal * 10^uniform(-6, 6)): values whose double sums depend on the order of the additions (float32 values
    of similar magnitude sum exactly in double, in any order, and cannot tell one tree from another); frac undefined."""
    rng = np.random.default_rng(seed)
    a = (rng.normal(0, 1, shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(np.float32)
    return sprinkle(a, rng, frac, np.float32(undef)) if frac else a


def wide_weight(ny, nx, seed, holes=0.0, undef=UNDEF):
    """Random float weights in [0.5, 2), `holes` of them undefined."""
    rng = np.random.default_rng(seed + 500)
    w = rng.uniform(0.5, 2.0, (ny, nx)).astype(np.float32)
    return sprinkle(w, rng, holes, np.float32(undef)) if holes else w


def main_case(nf=2, nlev=5, ny=9, nx=13, seed=1):
    """Fields, minus batches, a weight with holes, pivots and a box that cuts every side where the grid has room."""
    fields, minus = wide_fields((nf, nlev, ny, nx), seed), wide_fields((nf, nlev, ny, nx), seed + 100)
    weight = wide_weight(ny, nx, seed, 0.05)
    pivot = np.random.default_rng(seed + 200).normal(0, 100, (nf, nlev))
    box = (min(1, nx - 1), max(nx - 2, min(1, nx - 1) + 1), min(2, ny - 1), max(ny - 1, min(2, ny - 1) + 1))
    return fields, minus, weight, pivot, box


def extremes_case(nx=4100, ny=4):
    """One field of four levels whose extremes are ties and specials in different lanes, trips, segments and rows (nx > 4096:
    two segments).  Returns (fields (1, 4, ny, nx), flags (1, 4)).
    Level 0: the minimum -7 four times and the maximum 9e30 three times.  Level 1: all values in [1, 2) but zeros of both
    signs, -0.0 first in row 1, +0.0 first in row 2 and in the level.  Level 2: row 0 undefined throughout, +inf and -inf
    in row 3.  Level 3, flagged ALL_DEFINED: a NaN and a stored undef, which is a value there."""
    assert nx > SEGMENT + 3 and ny >= 4
    rng = np.random.default_rng(77)
    f = rng.uniform(1, 2, (1, 4, ny, nx)).astype(np.float32)
    for j, i in ((1, nx - 1), (1, 9), (2, 3), (1, 260)):
        f[0, 0, j, i] = -7
    for j, i in ((3, SEGMENT + 1), (0, 4000), (0, 255)):
        f[0, 0, j, i] = 9e30
    f[0, 1, 1, 17], f[0, 1, 1, SEGMENT] = -0.0, 0.0
    f[0, 1, 2, 5], f[0, 1, 2, 300] = 0.0, -0.0
    f[0, 1, 0, SEGMENT + 2] = 0.0
    f[0, 2, 0, :] = UNDEF
    f[0, 2, 3, 100], f[0, 2, 3, nx - 1] = np.inf, -np.inf
    f[0, 3, 2, 1000], f[0, 3, 1, 2] = np.nan, UNDEF
    return f, np.array([[SOME_DEFINED, SOME_DEFINED, SOME_DEFINED, ALL_DEFINED]], np.int32)
