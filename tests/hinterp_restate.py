"""Numpy restatement of mifc_hinterp_levels (include/mifc.h, "level batches sampled at arbitrary points"): the oracle of
tests/test_gpu_hinterp.py.  The position test, the cell and the fractions in float64 (exact), the interpolation step by
step in float64 (every ufunc rounds once, so nothing is contracted), the result rounded to float32 once."""
import numpy as np

from vinterp_restate import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, is_defined, sprinkle  # noqa: F401

NEAREST, BILINEAR, BICUBIC = 0, 1, 2
METHODS = {"nearest": NEAREST, "bilinear": BILINEAR, "bicubic": BICUBIC}
# the branch a (field, level, point) takes: rules 1, 4, 5, 6
POSITION_UNDEFINED, OUTSIDE, NEAREST_HIT, NEAREST_UNDEFINED, CUBIC, BILINEAR_UNDEFINED, ON_ROW, FULL_BILINEAR = range(8)
BRANCH_NAMES = ["position undefined", "outside", "nearest hit", "nearest undefined", "cubic", "bilinear undefined", "on a row or node (b == 0)",
                "full bilinear"]
# the branches a method can reach
REACHABLE = {NEAREST: [POSITION_UNDEFINED, OUTSIDE, NEAREST_HIT, NEAREST_UNDEFINED],
             BILINEAR: [POSITION_UNDEFINED, OUTSIDE, BILINEAR_UNDEFINED, ON_ROW, FULL_BILINEAR],
             BICUBIC: [POSITION_UNDEFINED, OUTSIDE, CUBIC, BILINEAR_UNDEFINED, ON_ROW, FULL_BILINEAR]}


def cubic_weights(t):
    """Rule 6: the Catmull-Rom weights of the columns i0 - 1 .. i0 + 2 (rows j0 - 1 .. j0 + 2), float64."""
    return [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, ((0.5 * t - 0.5) * t) * t]


# Departures from the definition that a test may ask for by name (`mistakes`): what a kernel that is subtly wrong would
# compute.  tests/test_horizontal_range_cpu.py shows that the cases of tests/horizontal_range_cases.py tell each from the rules.
MISTAKES = ("no select", "nearest in float", "no cubic on rows", "undef after the fact")


def sample(fields, xpos, ypos, method=BILINEAR, flags=None, undef=UNDEF, branches=None, mistakes=(), cells=None):
    """fields float32 (nf, nlev, ny, nx); xpos, ypos float32 of one shape S; flags None (SOME_DEFINED) or (nf, nlev).
    Returns (out (nf, nlev) + S, flags_out int32 (nf, nlev)).  branches: an int array like out that receives the branch of
    every output.  cells: a dict that receives rule 2 per point (i0, j0, a, b, usable).  mistakes: not part of the
    definition -- names from MISTAKES: "no select" reads column i0 + 1 and row j0 + 1 always (clamped to the grid) and
    adds a * (x10 - x00) and b * (r1 - r0) whether or not a, b are zero; "nearest in float" adds the 0.5 of rule 4 in float;
    "no cubic on rows" leaves rule 6 out where b == 0; "undef after the fact" takes a result equal to undef for a hole."""
    assert all(m in MISTAKES for m in mistakes), mistakes
    f = np.asarray(fields, np.float32)
    nf, nlev, ny, nx = f.shape
    xp, yp = np.asarray(xpos, np.float32), np.asarray(ypos, np.float32)
    where = xp.shape
    assert yp.shape == where
    xp, yp = xp.ravel(), yp.ravel()
    npos = xp.size
    undef = np.float32(undef)
    method = METHODS.get(method, method)
    assert method in (NEAREST, BILINEAR, BICUBIC)
    fl = np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)
    out = np.full((nf, nlev, npos), undef, np.float32)
    br = np.zeros((nf, nlev, npos), np.int64)
    fd = np.zeros((nf, nlev), np.int32)
    with np.errstate(all="ignore"):
        # rule 1
        pos_defined = is_defined(False, xp, undef) & is_defined(False, yp, undef)
        xd, yd = xp.astype(np.float64), yp.astype(np.float64)
        usable = pos_defined & (xd >= 0.0) & (xd <= float(nx - 1)) & (yd >= 0.0) & (yd <= float(ny - 1))
        xs, ys = np.where(usable, xd, 0.0), np.where(usable, yd, 0.0)  # (an unusable position computes on cell 0 and is thrown away)
        # rule 2
        i0, j0 = xs.astype(np.int64), ys.astype(np.int64)  # truncation
        a, b = xs - i0, ys - j0
        a0, b0 = a == 0, b == 0
        i1, j1 = i0 + ~a0, j0 + ~b0  # read only where needed: elsewhere the same column / row again
        inear, jnear = (xs + 0.5).astype(np.int64), (ys + 0.5).astype(np.int64)
        inside = ~(a0 & b0) & (i0 >= 1) & (i0 <= nx - 3) & (j0 >= 1) & (j0 <= ny - 3)
        select_a, select_b = a0, b0
        if "no select" in mistakes:
            i1, j1 = np.minimum(i0 + 1, nx - 1), np.minimum(j0 + 1, ny - 1)
            select_a, select_b = np.zeros_like(a0), np.zeros_like(b0)
        if "nearest in float" in mistakes:
            half = np.float32(0.5)
            inear, jnear = (xs.astype(np.float32) + half).astype(np.int64), (ys.astype(np.float32) + half).astype(np.int64)
            inear, jnear = np.minimum(inear, nx - 1), np.minimum(jnear, ny - 1)
        if "no cubic on rows" in mistakes:
            inside = inside & ~b0
        if cells is not None:
            cells.update(i0=i0, j0=j0, a=a, b=b, usable=usable)
        ci = [np.clip(i0 + n, 0, nx - 1) for n in (-1, 0, 1, 2)]  # (clipped only where the cubic rule does not apply)
        cj = [np.clip(j0 + m, 0, ny - 1) for m in (-1, 0, 1, 2)]
        wx, wy = cubic_weights(a), cubic_weights(b)
        for g in range(nf):
            for k in range(nlev):
                lev = f[g, k]
                all_defined = fl[g, k] == ALL_DEFINED
                if method == NEAREST:  # rule 4
                    v = lev[jnear, inear]
                    ok = is_defined(all_defined, v, undef)
                    res = v
                    branch = np.where(ok, NEAREST_HIT, NEAREST_UNDEFINED)
                else:  # rule 5
                    v00, v10, v01, v11 = lev[j0, i0], lev[j0, i1], lev[j1, i0], lev[j1, i1]
                    d00, d10, d01, d11 = (is_defined(all_defined, v, undef) for v in (v00, v10, v01, v11))
                    ok = d00 & (a0 | d10) & (b0 | d01) & (a0 | b0 | d11)
                    x00, x10, x01, x11 = (v.astype(np.float64) for v in (v00, v10, v01, v11))
                    r0 = np.where(select_a, x00, x00 + a * (x10 - x00))
                    r1 = np.where(select_a, x01, x01 + a * (x11 - x01))
                    res = np.where(select_b, r0, r0 + b * (r1 - r0)).astype(np.float32)
                    branch = np.where(ok, np.where(b0, ON_ROW, FULL_BILINEAR), BILINEAR_UNDEFINED)
                    if method == BICUBIC:  # rule 6
                        block = [[lev[cj[m], ci[n]] for n in range(4)] for m in range(4)]
                        cubic = inside.copy()
                        for m in range(4):
                            for n in range(4):
                                cubic &= is_defined(all_defined, block[m][n], undef)
                        s = [((wx[0] * block[m][0].astype(np.float64) + wx[1] * block[m][1].astype(np.float64)) + wx[2] * block[m][2].astype(np.float64))
                             + wx[3] * block[m][3].astype(np.float64) for m in range(4)]
                        rc = (((wy[0] * s[0] + wy[1] * s[1]) + wy[2] * s[2]) + wy[3] * s[3]).astype(np.float32)
                        res = np.where(cubic, rc, res)
                        ok = ok | cubic
                        branch = np.where(cubic, CUBIC, branch)
                bad = ~usable | ~ok
                if "undef after the fact" in mistakes:
                    bad = bad | (res == undef)
                out[g, k] = np.where(bad, undef, res)
                br[g, k] = np.where(~pos_defined, POSITION_UNDEFINED, np.where(~usable, OUTSIDE, branch))
                fd[g, k] = classify(int(bad.sum()), npos)  # rule 7
    if branches is not None:
        branches[...] = br.reshape(branches.shape)
    return out.reshape((nf, nlev) + where), fd


# ---------------------------------------------------------------------------------------------- case generators
def main_points(ny=9, nx=13, npos=600, seed=1, undef=UNDEF):
    """The positions of the main generator: uniform in [-0.5, n - 0.5) per axis (so some are outside), the first sixth
    with x rounded onto columns, the points from a twelfth to a quarter with y rounded onto rows (the overlap: nodes), one
    undef x, one NaN y and one point in the last corner, where the grid has room for them."""
    rng = np.random.default_rng(seed + 1000)
    x = rng.uniform(-0.5, nx - 0.5, npos).astype(np.float32)
    y = rng.uniform(-0.5, ny - 0.5, npos).astype(np.float32)
    on_col, row_from, row_to = npos // 6, npos // 12, npos // 4
    x[:on_col] = np.round(x[:on_col])
    y[row_from:row_to] = np.round(y[row_from:row_to])
    if npos >= 8:
        x[npos // 2] = undef
        y[npos // 2 + 1] = np.nan
        x[npos - 1], y[npos - 1] = nx - 1, ny - 1
    return x, y


def main_case(nf=1, nlev=1, ny=9, nx=13, npos=600, seed=1, undef=UNDEF, frac=0.03):
    """The main generator: fields N(280 - 5 f, 10) on a 9 x 13 grid with 3 % undefined cells, and main_points."""
    rng = np.random.default_rng(seed)
    fields = np.stack([sprinkle((rng.normal(0, 10, (nlev, ny, nx)) + 280 - 5 * f).astype(np.float32), rng, frac, undef) for f in range(nf)])
    x, y = main_points(ny, nx, npos, seed, undef)
    return fields, x, y
