"""mifc_vparcel_* at scaled pressures and with the ends of the float range among its inputs: the cases that
tests/test_vparcel_range_cpu.py (what they reach, which mistakes they see) and tests/test_gpu_vparcel_range.py (the kernel)
share.  Numpy only.

The kernel of mifc_vparcel.hip has branches keyed on magnitude that pressures of 240 .. 1050 never reach.  A scaled case is
vparcel_cases.make with every pressure -- ps, alevel, the fields form's p, the levels, p_src -- times 2^s, and q_src from the
saturation value at the scaled pressure; the temperatures are those of the unscaled case.  With pressures of 0.24 .. 1.05
times 1000 * 2^s the levels of one column straddle:

  s    seam
  -96  p * p0inv = 2^-96: the second rescaling of pow_kappa_rare (mifc_device.h), low side
  -49  p_b = 2^-40: the trips' quotient by p_b leaves the shared reciprocal for the plain division; and cplr * qcl = 2^64: a1
       leaves the refined-reciprocal sequence
  -32  p * p0inv = 2^-32: the low end of pow_kappa's fast domain
   31  p_b = 2^40
   32  p * p0inv = 2^32: the high end of the fast domain
   78  cplr * qcl = 2^-64
   96  p * p0inv = 2^96: the second rescaling, high side
  116  qsat = eps * esat / p turns subnormal
  "pa" every pressure times 100: Pa handed over for hPa, the mistake a user makes

On the low side the parcel is what it is at ordinary pressures with q scaled up; CAPE, CIN and tparcel respond to the
quotients.  On the high side q is tiny, the parcel carries no latent heat: no LFC, cape 0, pel undef in every cell; what a
wrong quotient can still move is plcl and tparcel.

Two cases per scale (nlev 7 on 9 x 16, four cells per lane; nlev 12 on 9 x 13, one), directions and the three kinds of source
rotating, and one of 10 x 206 cells at s = -49.  "special" cases sprinkle the ends of the float range at 4 % into t, q_src,
t_src, p_src, ps and the fields form's p: +-0, +-2^-149, +-FLT_MAX, +-inf, both neighbours of 1e35, the temperatures one float
inside and one outside both ends of the saturation table, and on ALL_DEFINED levels a stored 1e35 and NaN."""
import functools

import numpy as np

import vparcel_cases as vc
import vparcel_restate as vp

F = np.float32
U = vp.UNDEF
A = vp.ALL_DEFINED
FLT_MAX, DENORM_MIN, INF = np.finfo(F).max, F(2.0) ** F(-149), F(np.inf)
UNDEF_BELOW, UNDEF_ABOVE = np.nextafter(U, F(0)), np.nextafter(U, INF)

SCALES = {"s-96": 2.0 ** -96, "s-49": 2.0 ** -49, "s-32": 2.0 ** -32, "s31": 2.0 ** 31, "s32": 2.0 ** 32, "s78": 2.0 ** 78, "s96": 2.0 ** 96,
          "s116": 2.0 ** 116, "pa": 100.0}
LOW_SIDE = ("s-96", "s-49", "s-32")  # the parcel carries latent heat: LFC, CAPE, EL exist
SPECIAL_RATE = 0.04
SPECIAL_SCALES = (None, "s-49", "s-32", "s31")  # None: unscaled


def table_edge_temperatures():
    """The float temperatures one inside and one outside both ends of the saturation table (the table covers -1 < x < 40
    of vparcel_restate.sat_test): found by bisection on the restatement's own test."""
    def ok(T):
        return bool(vp.sat_test((vp.CP * np.array([T], F)).astype(F), np.array([1000.0], F))[0][0])

    out = []
    for lo, hi in ((F(100.0), F(250.0)), (F(250.0), F(500.0))):  # ok changes once in each
        a, b = lo, hi
        while np.nextafter(a, b) != b:
            m = F((np.float64(a) + np.float64(b)) / 2)
            a, b = (m, b) if ok(m) == ok(a) else (a, m)
        out += [a, b]
    return np.array(out, F)


def _sprinkle(a, rng, rate, values):
    flat = a.reshape(-1)
    at = np.nonzero(rng.random(flat.size) < rate)[0]
    flat[at] = rng.choice(values, size=at.size)


def with_specials(c, seed):
    rng = np.random.default_rng(seed)
    ends = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX, np.inf, -np.inf, UNDEF_BELOW, UNDEF_ABOVE], F)
    temps = np.concatenate([ends, table_edge_temperatures()])
    stored = np.array([U, np.nan], F)
    out = dict(c, name=c["name"] + "_special")
    for key, values in (("t", temps), ("q_src", ends), ("t_src", temps), ("p_src", ends), ("ps", ends), ("p", ends)):
        if c[key] is None:
            continue
        a = np.array(c[key], F)
        _sprinkle(a, rng, SPECIAL_RATE, values)
        flags = {"t": c["fdefined_in"], "p": c["fdef_coord"]}.get(key)
        if flags is not None:
            for k in range(a.shape[0]):
                if flags[k] == A:  # values there
                    _sprinkle(a[k], rng, 0.01, stored)
        out[key] = a
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for i, (name, factor) in enumerate(SCALES.items()):
        for nlev, ny, nx, j in ((7, 9, 16, i), (12, 9, 13, i + 1)):
            c = vc.make(nlev, ny, nx, ("first", "last")[j % 2], vc.SOURCES[j % 3], factor=factor)
            out.append(dict(c, name="%s_%s" % (c["name"], name), scale=name))
    c = vc.make(7, 10, 206, "last", "first", factor=SCALES["s-49"])
    out.append(dict(c, name=c["name"] + "_s-49", scale="s-49"))
    for i, name in enumerate(SPECIAL_SCALES):
        nlev, ny, nx = ((7, 9, 16), (12, 9, 13))[i % 2]
        c = vc.make(nlev, ny, nx, ("last", "first")[i % 2], vc.SOURCES[(i + 2) % 3], factor=1.0 if name is None else SCALES[name])
        out.append(with_specials(dict(c, name="%s_%s" % (c["name"], name or "s0"), scale=name), SPECIAL_SEEDS[i]))
    for c in out:
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


# seeds of the sprinkling for which the restatement alone leaves at most 2 % of a case's cells unstable and no output
# wholly undef (tests/test_vparcel_range_cpu.py)
SPECIAL_SEEDS = (1, 2, 3, 4)


def case_names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


class Reference(vc.Reference):
    """vparcel_cases.Reference, with one more way for a cell to be unstable: a value that is NaN or infinite in R0 or in a
    member and not the same bits in all of them (a NaN is a NaN).  On the stable cells a value of R0 that is not finite is
    therefore what every member gives, and the GPU file asks the kernel for the same (the bound says nothing about it:
    |inf - inf| is no number)."""

    def __init__(self, c, form):
        super().__init__(c, form)
        stable = self.stable
        for n in vp.OUTPUTS:
            e = self.r0[n]
            for m in self.members:
                g = m[n]
                odd = ~np.isfinite(e) | ~np.isfinite(g)
                same = (e.view(np.uint32) == g.view(np.uint32)) | (np.isnan(e) & np.isnan(g))
                bad = odd & ~same
                stable = stable & ~(bad if bad.ndim == 2 else bad.any(axis=0))
        self.stable = stable


@functools.lru_cache(maxsize=None)
def reference(name, form):
    return Reference(by_name(name), form)
