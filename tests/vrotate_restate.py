"""Numpy restatement of rule R of include/mifc.h ("vector pairs of level batches rotated"): the oracle of
tests/test_gpu_vrotate.py and tests/test_gpu_hinterp_vector.py.  Step by step as R1 to R4, in float64 (every ufunc rounds
once, so nothing is contracted; the products of two widened floats are exact), each result rounded to float32 once."""
import numpy as np

import hinterp_restate as hi
from vinterp_restate import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, is_defined, sprinkle  # noqa: F401

# why a pair result is a hole (the first cause that applies), or that it is computed
COMPUTED, COEFFICIENTS, U_HOLE, V_HOLE = range(4)


def rotate(fields, cosa, sina, flags=None, fdef_rot=SOME_DEFINED, undef=UNDEF, causes=None, holes=None):
    """fields float32 (2 * npairs, nlev) + S: u0, v0, u1, v1 ...; cosa, sina float32 of shape S; flags None (SOME_DEFINED)
    or (2 * npairs, nlev).  Returns (out like fields, flags_out int32 (2 * npairs, nlev)).  causes: an int array
    (npairs, nlev) + S that receives COMPUTED or the cause of the hole.  holes: a bool array like fields -- the components
    that are undefined, known from where they came from (sample_rotate) instead of tested by value and flag."""
    f = np.asarray(fields, np.float32)
    nf, nlev = f.shape[:2]
    where = f.shape[2:]
    assert nf % 2 == 0 and nf >= 2
    cf, sf = np.asarray(cosa, np.float32), np.asarray(sina, np.float32)
    assert cf.shape == where and sf.shape == where, (cf.shape, sf.shape, where)
    undef = np.float32(undef)
    fl = np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)
    out = np.empty_like(f)
    fd = np.zeros((nf, nlev), np.int32)
    why = np.zeros((nf // 2, nlev) + where, np.int64)
    n = int(np.prod(where, dtype=np.int64))
    with np.errstate(all="ignore"):
        # R1
        rot_defined = is_defined(fdef_rot == ALL_DEFINED, cf, undef) & is_defined(fdef_rot == ALL_DEFINED, sf, undef)
        c, s = cf.astype(np.float64), sf.astype(np.float64)
        for q in range(nf // 2):
            for k in range(nlev):
                u, v = f[2 * q, k], f[2 * q + 1, k]
                # R2: each component by its own flag
                if holes is None:
                    u_defined = is_defined(fl[2 * q, k] == ALL_DEFINED, u, undef)
                    v_defined = is_defined(fl[2 * q + 1, k] == ALL_DEFINED, v, undef)
                else:
                    u_defined, v_defined = ~holes[2 * q, k], ~holes[2 * q + 1, k]
                hole = ~rot_defined | ~u_defined | ~v_defined
                # R3
                ud, vd = u.astype(np.float64), v.astype(np.float64)
                cu, sv, su, cv = c * ud, s * vd, s * ud, c * vd
                ru = (cu - sv).astype(np.float32)
                rv = (su + cv).astype(np.float32)
                out[2 * q, k] = np.where(hole, undef, ru)
                out[2 * q + 1, k] = np.where(hole, undef, rv)
                # R4
                fd[2 * q, k] = fd[2 * q + 1, k] = classify(int(hole.sum()), n)
                why[q, k] = np.where(~rot_defined, COEFFICIENTS, np.where(~u_defined, U_HOLE, np.where(~v_defined, V_HOLE, COMPUTED)))
    if causes is not None:
        causes[...] = why
    return out, fd


SAMPLING_HOLES = (hi.POSITION_UNDEFINED, hi.OUTSIDE, hi.NEAREST_UNDEFINED, hi.BILINEAR_UNDEFINED)


def sample_rotate(fields, xpos, ypos, cosa, sina, method=hi.BILINEAR, flags=None, fdef_rot=SOME_DEFINED, undef=UNDEF, causes=None):
    """mifc_hinterp_vector_levels: hinterp_restate.sample of every component (rules 1 to 7, rounded to float), then rotate()
    of the (2 * npairs, nlev) + S result with the points' coefficients.  A component is undefined where the sampling left
    a hole (an unusable position, an undefined value that was needed): the holes are carried, not recognised by value, so a
    stored undef that a component flagged ALL_DEFINED hands through stays the value it is for the sampling."""
    f = np.asarray(fields, np.float32)
    where = np.asarray(xpos).shape
    br = np.zeros(f.shape[:2] + where, np.int64)
    sampled, _ = hi.sample(f, xpos, ypos, method, flags, undef, branches=br)
    return rotate(sampled, cosa, sina, None, fdef_rot, undef, causes, holes=np.isin(br, SAMPLING_HOLES))


# ---------------------------------------------------------------------------------------------- case generators
def coefficients(shape, seed=1, frac=0.03, undef=UNDEF, nan=True):
    """cos and sin of angles uniform in (-pi, pi], rounded to float32 (so c * c + s * s is only nearly one: the library does
    not normalise), `frac` of the cells or points with an undefined coefficient: undef in c, undef in s, and -- where
    there is room, with nan -- one NaN in each."""
    rng = np.random.default_rng(seed + 2000)
    angle = rng.uniform(-np.pi, np.pi, shape)
    c = sprinkle(np.cos(angle).astype(np.float32), rng, frac / 2, undef)
    s = sprinkle(np.sin(angle).astype(np.float32), rng, frac / 2, undef)
    if nan and c.size >= 8:
        c.reshape(-1)[c.size // 3] = np.nan
        s.reshape(-1)[(2 * c.size) // 3] = np.nan
    return c, s


def grid_case(npairs=1, nlev=5, ny=9, nx=13, seed=1, undef=UNDEF, frac=0.03):
    """The on-grid generator: u = N(5 + q, 10), v = N(-3 - q, 10) with `frac` undefined cells in each component and one NaN
    in each where there is room, and coefficients()."""
    rng = np.random.default_rng(seed)
    comps = []
    for q in range(npairs):
        for mean in (5.0 + q, -3.0 - q):
            a = sprinkle(rng.normal(mean, 10, (nlev, ny, nx)).astype(np.float32), rng, frac, undef)
            if a.size >= 8:
                a.reshape(-1)[(len(comps) + 1) * a.size // 9] = np.nan
            comps.append(a)
    c, s = coefficients((ny, nx), seed, frac, undef)
    return np.stack(comps), c, s


def point_case(npairs=1, nlev=1, ny=9, nx=13, npos=600, seed=1, undef=UNDEF, frac=0.03):
    """The sampling generator: hinterp_restate.main_case with 2 * npairs fields, and coefficients() at its points."""
    fields, x, y = hi.main_case(2 * npairs, nlev, ny, nx, npos, seed, undef, frac)
    c, s = coefficients((npos,), seed, frac, undef)
    return fields, x, y, c, s
