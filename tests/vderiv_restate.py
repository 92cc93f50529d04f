"""Numpy restatement of mifc_vderiv_hlevels / mifc_vderiv_fields / mifc_vderiv_levels (include/mifc.h, "vertical
derivatives of level batches"): the oracle of tests/test_gpu_vderiv.py.  The coordinate in float32, the spacings, the
weights and the result step by step in float64 (every ufunc rounds once, so nothing is contracted), the magnitude in
float32.  The case generators are the ones of vinterp_restate, with extra cells for the branches they do not reach."""
import numpy as np

from vinterp_restate import (ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, hybrid_coordinate, hybrid_levels,  # noqa: F401
                             is_defined, main_case, sprinkle)

CENTRED, WEIGHTED = 0, 1
METHODS = {"centred": CENTRED, "weighted": WEIGHTED}
# the branch a (field, level, cell) takes: rules 2 to 6
CENTRE_UNDEFINED, NO_SIDE, LOWER_ONLY, UPPER_ONLY, BOTH_SIDES, ZERO_SPACING = range(6)
BRANCH_NAMES = ["centre undefined", "no side", "lower only", "upper only", "both sides", "zero spacing"]


def derivative(fields, coord, coord_defined, method, flags=None, undef=UNDEF, branches=None):
    """fields float32 (nf, nlev, ny, nx); coord float32 (nlev, ny, nx) and coord_defined bool of the same shape (rule 1 of
    vinterp); flags None (SOME_DEFINED) or (nf, nlev).  Returns (out (nf, nlev, ny, nx), flags_out int32 (nf, nlev), bad
    bool like out: the cells left undef).  branches: an int array like out that receives the branch of every output."""
    x = np.asarray(fields, np.float32)
    nf, nlev, ny, nx = x.shape
    cells = ny * nx
    x = x.reshape(nf, nlev, cells)
    c = np.broadcast_to(np.asarray(coord, np.float32), (nlev, ny, nx)).reshape(nlev, cells)
    undef = np.float32(undef)
    method = METHODS.get(method, method)
    fl = np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)
    out = np.full((nf, nlev, cells), undef, np.float32)
    bad = np.ones((nf, nlev, cells), bool)
    br = np.zeros((nf, nlev, cells), np.int64)
    with np.errstate(all="ignore"):
        usable_c = np.broadcast_to(np.asarray(coord_defined, bool), (nlev, ny, nx)).reshape(nlev, cells) & ~np.isnan(c)  # rule 1
        d = c.astype(np.float64)
        zero = np.zeros(cells, np.float64)
        no = np.zeros(cells, bool)
        for f in range(nf):
            point = np.stack([usable_c[k] & is_defined(fl[f, k] == ALL_DEFINED, x[f, k], undef) for k in range(nlev)])  # rule 2
            xd = x[f].astype(np.float64)
            for k in range(nlev):
                lower = point[k - 1] & (c[k - 1] != c[k]) if k > 0 else no  # rule 3
                upper = point[k + 1] & (c[k + 1] != c[k]) if k < nlev - 1 else no
                dm, xm = (d[k - 1], xd[k - 1]) if k > 0 else (zero, zero)
                dp, xp = (d[k + 1], xd[k + 1]) if k < nlev - 1 else (zero, zero)
                # rule 4
                if method == CENTRED:
                    den = dp - dm
                    w = 1.0 / den
                    both = (xp - xm) * w
                else:
                    h1, h2 = d[k] - dm, dp - d[k]
                    den = h1 + h2
                    w1, w2 = h2 / (h1 * den), h1 / (h2 * den)
                    both = (xd[k] - xm) * w1 + (xp - xd[k]) * w2
                # rule 5
                one_lower = (xd[k] - xm) * (1.0 / (d[k] - dm))
                one_upper = (xp - xd[k]) * (1.0 / (dp - d[k]))
                r = np.where(lower & upper, both, np.where(lower, one_lower, one_upper)).astype(np.float32)  # rule 7
                b = ~point[k] | ~(lower | upper) | (lower & upper & (den == 0))
                out[f, k] = np.where(b, undef, r)
                bad[f, k] = b
                br[f, k] = np.where(~point[k], CENTRE_UNDEFINED, np.where(lower & upper, np.where(den == 0, ZERO_SPACING, BOTH_SIDES),
                                                                          np.where(lower, LOWER_ONLY, np.where(upper, UPPER_ONLY, NO_SIDE))))
    if branches is not None:
        branches[...] = br.reshape(branches.shape)
    fd = np.array([[classify(int(bad[f, k].sum()), cells) for k in range(nlev)] for f in range(nf)], np.int32)
    return out.reshape(nf, nlev, ny, nx), fd, bad.reshape(nf, nlev, ny, nx)


def magnitude(out, bad, undef=UNDEF):
    """Rule 8: absval of the pairs (2j, 2j + 1) in float32, undef where either component was left undef."""
    nf, nlev, ny, nx = out.shape
    undef = np.float32(undef)
    with np.errstate(all="ignore"):
        a, b = out[0::2], out[1::2]
        m = np.sqrt((a * a + b * b).astype(np.float32)).astype(np.float32)
    mbad = bad[0::2] | bad[1::2]
    mag = np.where(mbad, undef, m).astype(np.float32)
    fd = np.array([[classify(int(mbad[j, k].sum()), ny * nx) for k in range(nlev)] for j in range(nf // 2)], np.int32).reshape(nf // 2, nlev)
    return mag, fd


def _finish(res, want_magnitude, undef):
    out, fd, bad = res
    if not want_magnitude:
        return out, fd
    mag, mfd = magnitude(out, bad, undef)
    return out, fd, mag, mfd


def hlevels(fields, ps, alevel, blevel, method=CENTRED, flags=None, fdef_ps=SOME_DEFINED, undef=UNDEF, magnitude=False, branches=None):
    c = hybrid_coordinate(ps, alevel, blevel)
    psd = is_defined(fdef_ps == ALL_DEFINED, np.asarray(ps, np.float32), undef)
    return _finish(derivative(fields, c, np.broadcast_to(psd, c.shape), method, flags, undef, branches), magnitude, undef)


def coord_fields(fields, coord, method=CENTRED, flags=None, fdef_coord=None, undef=UNDEF, magnitude=False, branches=None):
    c = np.asarray(coord, np.float32)
    fc = [SOME_DEFINED] * c.shape[0] if fdef_coord is None else list(fdef_coord)
    cdef = np.stack([is_defined(fc[k] == ALL_DEFINED, c[k], undef) for k in range(c.shape[0])])
    return _finish(derivative(fields, c, cdef, method, flags, undef, branches), magnitude, undef)


def levels(fields, levs, method=CENTRED, flags=None, undef=UNDEF, magnitude=False, branches=None):
    """The coordinate is one constant per level: always defined (the call refuses a NaN level)."""
    x = np.asarray(fields, np.float32)
    c = np.asarray(levs, np.float32).reshape(-1, 1, 1)
    return _finish(derivative(x, c, np.ones(x.shape[1:], bool), method, flags, undef, branches), magnitude, undef)


# ---------------------------------------------------------------------------------------------- case generators
def main_levels(nlev=12):
    """Pressure levels for the `levels` form, top-down, unevenly spaced."""
    return np.round(1000 * np.linspace(0.17, 1, nlev) ** 2).astype(np.float32)


def deriv_case(nf=3, nlev=12, ny=9, nx=13, seed=1, undef=UNDEF):
    """main_case of vinterp_restate and the pressure of its levels as a coordinate batch, with cells added for the
    branches the generator does not reach where the grid has room for them: a column folded around level 1 (zero
    spacing), a column with two equal neighbours and one with isolated levels (no side)."""
    fields, ps, alevel, blevel = main_case(nf, nlev, ny, nx, seed, undef)
    coord = hybrid_coordinate(np.where(is_defined(False, ps, undef), ps, np.float32(900)), alevel, blevel)
    coord[:, ~is_defined(False, ps, undef)] = undef
    cells = coord.reshape(nlev, -1)
    fl = fields.reshape(nf, nlev, -1)
    if cells.shape[1] >= 4 and nlev >= 3:
        cells[:, 0] = np.where(np.isnan(cells[:, 1]) | (cells[:, 1] == undef), np.float32(500), cells[:, 1])
        cells[2, 0] = cells[0, 0]  # folded: c_2 == c_0 around level 1
        fl[:, :3, 0] = np.float32(250)
        cells[:, 2] = np.where(np.isnan(cells[:, 3]) | (cells[:, 3] == undef), np.float32(500), cells[:, 3])
        cells[1, 2] = cells[0, 2]  # equal neighbours: level 0 has no side, level 1 only the upper one
        fl[:, :3, 2] = np.float32(260)
        fl[:, 0::2, 3] = undef  # every other level missing: the levels between have no side
    return fields, ps, (alevel, blevel), coord
