"""Seeded cases that put the six column-walk families (mifc_vinterp_*, mifc_vlayer_*, mifc_vderiv_*, mifc_vcumul_*,
mifc_pvort_*, mifc_vregrid_*) at the ends of the float range (numpy only: no GPU, nothing read from the reference).
tests/test_column_range_cpu.py asserts on the CPU that the cases reach what they are meant to reach and that they tell a
flush to zero, a float intermediate and a key/float mismatch of the vinterp bracket from the definition;
tests/test_gpu_column_range.py runs them through the library.

A case is a dict:
  label    "<family>-<class>-<kind>-<method>[-<extra>][-nan-undef]-<nx>x<ny>x<nlev>": names the seam
  family   vinterp | vlayer | vderiv | vcumul | pvort | vregrid  kind    hybrid | field | levels
  method   the family's method (vlayer: None)                   klass   huge | tiny | mid
  undef    1e35, or NaN in the "-nan-undef" variant
  fields   float32 (nf, nlev, ny, nx); pvort: u, v, th          flags   int32 (nf, nlev): ALL_DEFINED and SOME_DEFINED mixed
  hybrid:  ps (ny, nx), ab = (alevel, blevel), fdef_c one flag  field:  coord (nlev, ny, nx), fdef_c int32[nlev]
  levels:  levs float32[nlev]
  extras   vinterp: targets | vlayer: lo, hi (numbers or (ny, nx) fields) | vcumul: from_, start, fdef_start, base, fdef_base,
           scale | pvort: xmapr, ymapr, fcoriolis, scale | vregrid: tcoord (nt, ny, nx), fdef_t int32[nt], method, from_, outside
           (what the call is run with; the case's own `method` names the rule its coordinate was drawn by)

What the ingredients are for:
  fields   per magnitude class a decade chosen so that the RESULT straddles the end of the range: `huge` differences
           overflow float but not double (vderiv, pvort: difference over a spacing of order 1; vcumul and vlayer's integral:
           x * dc, a lower decade so that the sums straddle FLT_MAX and do not saturate); `tiny` inputs are subnormal and the
           results lie around FLT_MIN; `mid` are ordinary.  6 % of every field are specials: +-0, +-2^-149, 1e-40, +-FLT_MIN,
           3e38, -FLT_MAX, +-inf, both neighbours of 1e35; on ALL_DEFINED levels also a stored 1e35 and NaN (values
           there), on SOME_DEFINED levels 3 % undef.
  coord    field: a monotone base with spacings of order 1 that crosses zero, 4 % specials: +0 / -0 pairs (equal
           neighbours), a spacing of one subnormal, +-FLT_MAX, +-inf, on ALL_DEFINED levels NaN and a stored 1e35, on
           SOME_DEFINED levels undef.  hybrid: levels with spacings of order 1, blevel[0] = 0 (0 * inf: a NaN that arithmetic
           makes), ps with subnormals, huge values, infinities, undef, NaN under ALL_DEFINED; the "-overflow" variant has an
           alevel of 2e38, so that alevel + blevel * ps leaves the float range for a finite ps.  levels: a subnormal
           spacing, a signed-zero pair, +-FLT_MAX and +-inf at the ends.
  LOG      (vinterp, vcumul) positive coordinates from subnormal to FLT_MAX with zeros, negatives and +inf sprinkled in;
           usable neighbours are bit-equal or at least 1e-3 apart in ln c (asserted here), and the fields have one sign, so
           that the families' "equal or the neighbouring float" rule and its derivation (docstrings of
           tests/test_gpu_vinterp.py and tests/test_gpu_vcumul.py: no cancellation) hold unchanged.

The rates and decades are tuned until the conditions asserted in tests/test_column_range_cpu.py hold: a case must not
degrade into comparing NaN with NaN or undef with undef.

vinterp_seam_cases() are cases of another kind, for the wave pre-filter of vinterp_kernel: see the section below.

vregrid re-uses vinterp's ingredients unchanged (make_fields, the coordinate and ps specials, the LOG coordinate rule; its
`levels` kind takes LEVELS_LINEAR_B and LEVELS_LOG) and adds per-cell targets: see "vregrid: the targets" below.  One set of
arrays (a "base") is run with every (method, from, outside): each combination is a case of its own that shares the
base's arrays.  A base drawn by the LOG rule is run with both methods.  A base drawn by the LINEAR rule is run with LINEAR, and
with LOG where at most half of the outputs are holes (log_runs_on_a_linear_base): its coordinates cross zero, MIFC_VINTERP_LOG
turns away every target <= 0 and every bracket with an end <= 0, and so the `levels` bases (LEVELS_LINEAR_B has one pair
above zero), the two-level base and the `field` bases under OUTSIDE_UNDEF come to 58 .. 99 % holes -- they would compare
undef with undef -- while the hybrid bases (17 .. 33 %) and the `field` bases under OUTSIDE_CLAMP (43 .. 50 %) run.
tests/test_column_range_cpu.py asserts both sides of that line, and that a double log() one ulp off moves nothing on the
LOG runs of the LINEAR bases either (between neighbours one float apart a target can only be an end: weight 0 or 1 under
any log()).  vregrid_seam_cases() and
vregrid_hand_columns() are for the wave interval of vregrid_kernel and for its clamp rule.
"""
import functools
import zlib

import numpy as np

import pvort_restate as pv
import vcumul_restate as vc
import vderiv_restate as vd
import vinterp_restate as vi
import vlayer_restate as vl
import vregrid_restate as vg

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = vi.ALL_DEFINED, vi.NONE_DEFINED, vi.SOME_DEFINED
UNDEF = vi.UNDEF
FAMILIES = ("vinterp", "vlayer", "vderiv", "vcumul", "pvort", "vregrid")
CLASSES = ("huge", "tiny", "mid")
NY, NX_VEC, NX_ODD, NLEV = 9, 68, 67, 7  # 612 cells: four per lane, three waves | 603: one per lane, a partial last wave
MIN_NLEV = {"vinterp": 2, "vlayer": 2, "vderiv": 2, "vcumul": 2, "pvort": 2, "vregrid": 2}

_F = np.float32
FLT_MAX, FLT_MIN, DENORM_MIN = np.finfo(np.float32).max, np.finfo(np.float32).tiny, _F(2.0) ** _F(-149)
INF = _F(np.inf)
UNDEF_BELOW, UNDEF_ABOVE = np.nextafter(UNDEF, _F(0)), np.nextafter(UNDEF, INF)

FIELD_SPECIALS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1e-40, FLT_MIN, -FLT_MIN, 3e38, -FLT_MAX, np.inf, -np.inf, UNDEF_BELOW, UNDEF_ABOVE],
                          np.float32)
# LOG: one sign (the neighbour rule is derived without cancellation); -0 is a zero
FIELD_SPECIALS_POSITIVE = np.array([0.0, -0.0, DENORM_MIN, 1e-40, FLT_MIN, 3e38, FLT_MAX, np.inf, UNDEF_BELOW, UNDEF_ABOVE], np.float32)
COORD_SPECIALS = np.array([FLT_MAX, -FLT_MAX, np.inf, -np.inf, DENORM_MIN, -DENORM_MIN, UNDEF_BELOW, UNDEF_ABOVE], np.float32)
COORD_SPECIALS_LOG = np.array([0.0, -0.0, -1.5, -DENORM_MIN, np.inf, DENORM_MIN, FLT_MIN, FLT_MAX, 1e-40], np.float32)
PS_SPECIALS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1e-40, FLT_MIN, 3e38, FLT_MAX, -FLT_MAX, np.inf, -np.inf, UNDEF_BELOW, UNDEF_ABOVE],
                       np.float32)
PS_SPECIALS_LOG = np.array([0.0, -0.0, DENORM_MIN, 1e-40, FLT_MIN, 3e38, FLT_MAX, -2.0, np.inf, UNDEF_BELOW], np.float32)
FIELD_RATE, COORD_RATE, UNDEF_RATE = 0.06, 0.04, 0.03

# centred: both infinities at the ends (a weighted derivative next to an infinite spacing is inf / inf, a level of NaN)
LEVELS_LINEAR = np.array([-np.inf, -1.0, -0.0, 0.0, DENORM_MIN, 1.25, np.inf], np.float32)
# pvort, centred: a zero derivative (1 / inf) times an infinite horizontal difference is NaN; one infinite end is enough of that
LEVELS_LINEAR_P = np.array([-FLT_MAX, -1.0, -0.0, 0.0, DENORM_MIN, 1.25, np.inf], np.float32)
# weighted: +-FLT_MAX at the ends; level 3 has two neighbours equal to it: no side, a level of undef (NONE_DEFINED)
LEVELS_LINEAR_B = np.array([-FLT_MAX, -0.5, 0.0, -0.0, 0.0, 0.75, FLT_MAX], np.float32)
# vcumul: an end of the range in front would send every later level of an ordinary field to infinity; it is walked last
LEVELS_CUMUL = np.array([-1.5, -0.75, -0.0, 0.0, DENORM_MIN, 1.25, FLT_MAX], np.float32)
LEVELS_LOG = np.array([DENORM_MIN, 1e-40, FLT_MIN, 1e-3, 40.0, FLT_MAX, np.inf], np.float32)  # +inf is walked last in either direction

# log10 of the field magnitudes of a `huge` case, per family and method (see the module docstring); tiny is the same everywhere
HUGE_DECADES = {
    ("vinterp", "linear"): (36.5, 38.5), ("vinterp", "log"): (36.5, 38.5),
    ("vlayer", None): (36.8, 38.5),
    ("vderiv", "centred"): (36.8, 38.5), ("vderiv", "weighted"): (36.8, 38.5),
    ("vcumul", "linear"): (36.3, 38.3), ("vcumul", "log"): (35.3, 37.2), ("vcumul", "log-hybrid"): (36.0, 38.0),
    ("pvort", "centred"): (36.8, 38.5), ("pvort", "weighted"): (36.8, 38.5),
    ("vregrid", "linear"): (36.5, 38.5), ("vregrid", "log"): (36.5, 38.5),  # vinterp's
}
TINY_DECADES = (-44.5, -37.6)


def _seed(label):
    return zlib.crc32(label.encode())


def _sprinkle(a, rng, rate, values):
    a = a.reshape(-1)
    at = np.nonzero(rng.random(a.size) < rate)[0]
    a[at] = rng.choice(values, size=at.size)
    return at


def make_flags(rng, nf, nlev):
    """ALL_DEFINED and SOME_DEFINED mixed, both present in every field's column of flags."""
    fl = rng.choice([ALL_DEFINED, SOME_DEFINED], size=(nf, nlev)).astype(np.int32)
    fl[:, 0] = SOME_DEFINED
    fl[:, nlev - 1] = ALL_DEFINED
    return fl


def make_fields(rng, klass, decades, nf, nlev, ny, nx, flags, undef, positive=False, smooth=None, centre=250.0):
    """(nf, nlev, ny, nx) of the class's magnitudes, the specials and the holes.  smooth: the relative horizontal
    variation of a field whose neighbour differences must stay finite (pvort's th); None: every value on its own."""
    shape = (nf, nlev, ny, nx)
    if klass == "mid":
        x = rng.normal(0, 10, shape) + centre - 5 * np.arange(nf).reshape(-1, 1, 1, 1)
    else:
        lo, hi = decades if klass == "huge" else TINY_DECADES
        if smooth is None:
            x = 10.0 ** rng.uniform(lo, hi, shape)
            sign = rng.choice([-1.0, 1.0], size=shape)
        else:
            x = 10.0 ** rng.uniform(lo, hi, (nf, nlev, 1, 1)) * (1 + smooth * rng.uniform(-1, 1, shape))
            sign = rng.choice([-1.0, 1.0], size=(nf, nlev, 1, 1))
        x = x if positive else x * sign
    x = np.minimum(np.maximum(x, -float(FLT_MAX)), float(FLT_MAX)).astype(np.float32)
    _sprinkle(x, rng, FIELD_RATE, FIELD_SPECIALS_POSITIVE if positive else FIELD_SPECIALS)
    for f in range(nf):
        for k in range(nlev):
            if flags[f, k] == ALL_DEFINED:  # values there
                _sprinkle(x[f, k], rng, 0.01, np.array([UNDEF, np.nan], np.float32))
            else:
                _sprinkle(x[f, k], rng, UNDEF_RATE, np.array([undef], np.float32))
    return x


def make_coord_flags(rng, nlev):
    fc = rng.choice([ALL_DEFINED, SOME_DEFINED], size=nlev).astype(np.int32)
    fc[0], fc[nlev - 1] = ALL_DEFINED, SOME_DEFINED
    return fc


def make_coord_linear(rng, nlev, ny, nx, fdef_c, undef):
    """Monotone per cell, spacings 0.5 .. 2, crossing zero; then the specials."""
    c = (rng.uniform(-6, -1, (1, ny, nx)) + np.cumsum(rng.uniform(0.5, 2, (nlev, ny, nx)), axis=0)).astype(np.float32)
    if nlev == 2:  # the one pair straddles zero
        c = np.stack([-rng.uniform(0.1, 1.5, (ny, nx)), rng.uniform(0.1, 1.5, (ny, nx))]).astype(np.float32)
    flat = c.reshape(nlev, -1)
    cells = flat.shape[1]
    _sprinkle(c, rng, COORD_RATE / 2, COORD_SPECIALS)
    for i in np.nonzero(rng.random(cells) < COORD_RATE * 2)[0]:  # pairs, one per chosen cell
        k = int(rng.integers(0, nlev - 1))
        what = int(rng.integers(0, 4))
        if what == 0:
            flat[k, i], flat[k + 1, i] = 0.0, -0.0  # equal neighbours of different bits
        elif what == 1:
            flat[k, i], flat[k + 1, i] = DENORM_MIN, -0.0  # a spacing of one subnormal ...
        elif what == 2:
            with np.errstate(over="ignore"):
                flat[k + 1, i] = np.nextafter(flat[k, i], INF)  # one ulp
        else:
            flat[k, i], flat[k + 1, i] = DENORM_MIN, -DENORM_MIN
        if what == 1 and k + 2 < nlev:
            flat[k + 2, i] = DENORM_MIN  # ... and a column folded around it: the two-sided spacing is zero
    _coord_holes(rng, c, fdef_c, undef)
    return c


def make_coord_log(rng, nlev, ny, nx, fdef_c, undef):
    """Positive and monotone per cell from subnormal to just below FLT_MAX in steps of 25 .. 30 in ln c (nlev 7); then
    zeros, negatives, +inf and the positive ends of the range."""
    g = rng.uniform(-102, -95, (1, ny, nx)) + np.cumsum(rng.uniform(25, 30, (nlev, ny, nx)), axis=0) - 25
    c = np.exp(g).astype(np.float32)
    _sprinkle(c, rng, COORD_RATE, COORD_SPECIALS_LOG)
    _coord_holes(rng, c, fdef_c, undef)
    return c


def _coord_holes(rng, c, fdef_c, undef):
    for k in range(c.shape[0]):
        if fdef_c[k] == ALL_DEFINED:
            _sprinkle(c[k], rng, 0.01, np.array([UNDEF, np.nan], np.float32))
        else:
            _sprinkle(c[k], rng, 0.01, np.array([undef], np.float32))


def make_hybrid(rng, nlev, ny, nx, fdef_ps, undef, log, overflow):
    """alevel, blevel with spacings of order 1 at ps 5 .. 9 (below 4.4 the two lowest levels cross) and blevel[0] = 0; ps
    with its specials."""
    eta = np.linspace(0.02, 1, nlev) ** 1.5
    a, b = (10 * (eta - eta ** 2)).astype(np.float32), (eta ** 2).astype(np.float32)
    b[0] = 0
    if overflow and nlev > 5:
        a[5] = 2e38  # 2e38 + 0.586 * 3e38 leaves the float range
    ps = rng.uniform(5, 9, (ny, nx)).astype(np.float32)
    _sprinkle(ps, rng, FIELD_RATE, PS_SPECIALS_LOG if log else PS_SPECIALS)
    if fdef_ps == ALL_DEFINED:
        _sprinkle(ps, rng, 0.02, np.array([UNDEF, np.nan], np.float32))
    else:
        _sprinkle(ps, rng, UNDEF_RATE, np.array([undef], np.float32))
    return ps, (a, b)


def assert_log_spacing(c, usable):
    """Neighbours that are both usable and positive are bit-equal or at least 1e-3 apart in ln c."""
    c = np.asarray(c, np.float32)
    with np.errstate(all="ignore"):
        g = np.log(c.astype(np.float64))
        for k in range(c.shape[0] - 1):
            both = usable[k] & usable[k + 1] & (c[k] > 0) & (c[k + 1] > 0) & np.isfinite(c[k]) & np.isfinite(c[k + 1]) & (c[k] != c[k + 1])
            assert (np.abs(g[k + 1] - g[k])[both] >= 1e-3).all(), "LOG: usable neighbours closer than 1e-3 in ln c"


def coordinate_of(case):
    """(coord float32 (nlev, ny, nx), usable-by-rule-1 bool) of a case of any kind."""
    f = case["fields"]
    nlev, ny, nx = f.shape[1:]
    if case["kind"] == "hybrid":
        c = vi.hybrid_coordinate(case["ps"], *case["ab"])
        d = np.broadcast_to(vi.is_defined(case["fdef_c"] == ALL_DEFINED, case["ps"], case["undef"]), c.shape)
    elif case["kind"] == "field":
        c = case["coord"]
        d = np.stack([vi.is_defined(case["fdef_c"][k] == ALL_DEFINED, c[k], case["undef"]) for k in range(nlev)])
    else:
        c = np.broadcast_to(case["levs"].reshape(-1, 1, 1), (nlev, ny, nx))
        d = np.ones(c.shape, bool)
    return np.ascontiguousarray(c), d


def as_field(case):
    """The `field` form of a hybrid or levels case: the same problem with the coordinate given as a batch.  hybrid: where
    ps is not defined the batch holds undef under SOME_DEFINED flags; under fdef_ps == ALL_DEFINED every level is flagged
    ALL_DEFINED (a coordinate that happens to be 1e35 is a value in both forms, a NaN one is unusable in both)."""
    c, d = coordinate_of(case)
    c = c.copy()
    nlev = c.shape[0]
    if case["kind"] == "hybrid" and case["fdef_c"] != ALL_DEFINED:
        assert not ((c == UNDEF) & d).any(), "a computed coordinate that equals undef"
        c[~d] = case["undef"]
        fdef = np.full(nlev, SOME_DEFINED, np.int32)
    else:
        fdef = np.full(nlev, ALL_DEFINED, np.int32)
    out = {k: v for k, v in case.items() if k not in ("ps", "ab", "levs")}
    out.update(kind="field", coord=c, fdef_c=fdef, label=case["label"] + "-as-field")
    return out


# ------------------------------------------------------------------------------------------------ the cases
def _spec(family, klass):
    """(kind, method, nx, nlev, nan_undef, extra) of the cases of a family and class: every kind and method, both widths,
    one "-nan-undef" variant; the family's minimum nlev once, in the mid class."""
    V, O = NX_VEC, NX_ODD
    if family == "vregrid":
        return _vregrid_spec(klass)
    if family == "vinterp":
        s = [("hybrid", "linear", V, NLEV, False, None), ("field", "linear", O, NLEV, False, None), ("field", "log", V, NLEV, False, None),
             ("hybrid", "log", O, NLEV, False, None), ("field", "linear", V, NLEV, True, None)]
    elif family == "vlayer":
        s = [("hybrid", None, V, NLEV, False, "open"), ("field", None, O, NLEV, False, "fltmax"), ("field", None, V, NLEV, False, "fields"),
             ("hybrid", None, O, NLEV, True, "fields"), ("field", None, O, NLEV, False, "open")]
        if klass == "mid":
            s.append(("field", None, V, NLEV, False, "subnormal"))
    elif family in ("vderiv", "pvort"):
        s = [("hybrid", "centred", V, NLEV, False, None), ("field", "weighted", O, NLEV, False, None), ("levels", "centred", O, NLEV, False, None),
             ("field", "centred", V, NLEV, True, None), ("hybrid", "weighted", O, NLEV, False, None), ("levels", "weighted", V, NLEV, False, "b")]
    else:
        s = [("hybrid", "linear", V, NLEV, False, "first"), ("field", "linear", O, NLEV, False, "last-full"), ("levels", "linear", O, NLEV, False, "first-full"),
             ("field", "log", V, NLEV, False, "first-full"), ("levels", "log", O, NLEV, False, "last"), ("hybrid", "log", V, NLEV, True, "last-full"),
             ("levels", "log", V, NLEV, False, "first")]
    if klass == "mid":
        kind, method, nx, _, _, extra = s[1]
        s.append((kind, method, nx, MIN_NLEV[family], False, extra))
        kind, method, nx, nlev, _, extra = s[0]
        s.append((kind, method, nx, nlev, False, (extra + "-" if extra else "") + "overflow"))
    return s


@functools.lru_cache(maxsize=None)
def cases(family, klass):
    out = [make_case(family, klass, *s) for s in _spec(family, klass)]
    assert len({c["label"] for c in out}) == len(out)
    return out


def all_cases():
    return [c for family in FAMILIES for klass in CLASSES for c in cases(family, klass)]


def make_case(family, klass, kind, method, nx, nlev, nan_undef, extra):
    if family == "vregrid":
        return make_vregrid_case(klass, kind, method, nx, nlev, nan_undef, extra)
    ny = NY
    parts = [family, klass, kind] + ([method] if method else []) + ([extra] if extra else []) + (["nan-undef"] if nan_undef else [])
    label = "-".join(parts) + "-%dx%dx%d" % (nx, ny, nlev)
    rng = np.random.default_rng(_seed(label))
    undef = _F(np.nan) if nan_undef else UNDEF
    log = method == "log"
    overflow = bool(extra) and extra.endswith("overflow")
    nf = 3 if family == "pvort" else 2
    flags = make_flags(rng, nf, nlev)
    decades = HUGE_DECADES.get((family, "log-hybrid" if (family == "vcumul" and log and kind == "hybrid") else method))
    case = dict(label=label, family=family, kind=kind, method=method, klass=klass, undef=undef, flags=flags, extras={})
    if family == "pvort":
        # u, v ordinary (their neighbour differences enter the vorticity), th of the class, horizontally coherent so that its
        # float neighbour differences stay finite; the vertical differences are the ones that leave the range
        uv = make_fields(rng, "mid", None, 2, nlev, ny, nx, flags[:2], undef, centre=5.0)
        th = make_fields(rng, klass, decades, 1, nlev, ny, nx, flags[2:], undef, smooth=None if klass == "mid" else 0.05)
        case["fields"] = np.concatenate([uv, th])
    else:
        case["fields"] = make_fields(rng, klass, decades, nf, nlev, ny, nx, flags, undef, positive=log)
    # the coordinate
    if kind == "hybrid":
        case["fdef_c"] = int(rng.choice([ALL_DEFINED, SOME_DEFINED]))
        case["ps"], case["ab"] = make_hybrid(rng, nlev, ny, nx, case["fdef_c"], undef, log, overflow)
    elif kind == "field":
        case["fdef_c"] = make_coord_flags(rng, nlev)
        case["coord"] = (make_coord_log if log else make_coord_linear)(rng, nlev, ny, nx, case["fdef_c"], undef)
    else:
        levs = LEVELS_LOG if log else LEVELS_CUMUL if family == "vcumul" else (LEVELS_LINEAR_B if extra == "b" else LEVELS_LINEAR_P if family == "pvort" else LEVELS_LINEAR)
        if family == "vcumul" and extra and extra.startswith("last"):
            levs = levs[::-1]  # the infinity is walked last
        case["levs"] = np.ascontiguousarray(levs[:nlev] if nlev < NLEV else levs)
    c, usable = coordinate_of(case)
    if log:
        assert_log_spacing(c, usable)
    ex = case["extras"]
    if family == "vinterp":
        row = min(2, nlev - 1)  # the target that is bit-equal to a stored coordinate: the first usable finite one of this level
        with np.errstate(invalid="ignore"):
            fit = usable[row] & np.isfinite(c[row]) & ((c[row] > 0) if log else True)
        assert fit.any(), label
        stored = c[row][fit][0]
        if log:
            ordinary = np.exp(rng.uniform(-90, 80, 8)) if kind == "field" else rng.uniform(0.05, 8, 8)
            t = np.concatenate([[DENORM_MIN, 1e-40, FLT_MIN, FLT_MAX, np.inf, stored], ordinary])
        else:
            lo, hi = (-0.3, 0.3) if nlev == 2 else (0.05, 7) if kind == "hybrid" else (-2, 6)
            t = np.concatenate([[0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX, np.inf, -np.inf, stored], rng.uniform(lo, hi, 7)])
        ex["targets"] = t.astype(np.float32)
        assert ex["targets"].size <= 16
    elif family == "vlayer":
        what = extra.replace("-overflow", "") if extra else "open"
        if what == "open":
            ex["lo"], ex["hi"] = -INF, INF
        elif what == "fltmax":
            ex["lo"], ex["hi"] = -FLT_MAX, FLT_MAX
        elif what == "subnormal":
            ex["lo"], ex["hi"] = _F(-0.0), DENORM_MIN
        else:
            lo = rng.uniform(-4, 0, (ny, nx)).astype(np.float32)
            hi = rng.uniform(1, 6, (ny, nx)).astype(np.float32)
            _sprinkle(lo, rng, 0.08, np.array([-np.inf, -FLT_MAX, -0.0, 0.0, -DENORM_MIN, UNDEF_BELOW, np.nan, undef, np.inf], np.float32))
            _sprinkle(hi, rng, 0.08, np.array([np.inf, FLT_MAX, DENORM_MIN, 0.0, UNDEF_ABOVE, np.nan, undef, -np.inf], np.float32))
            ex["lo"], ex["hi"] = lo, hi
    elif family == "vcumul":
        ex["from_"] = "last" if extra.startswith("last") else "first"
        if "full" in extra:
            first = c[0 if ex["from_"] == "first" else nlev - 1].reshape(ny, nx)
            if log:
                with np.errstate(all="ignore"):
                    start = np.where((first > 0) & np.isfinite(first), first * _F(0.25), _F(1e-3)).astype(np.float32)
                _sprinkle(start, rng, 0.05, np.array([0.0, -1.0, DENORM_MIN, FLT_MAX, np.inf, undef], np.float32))
                base = rng.uniform(1, 3000, (nf, ny, nx)).astype(np.float32)
                _sprinkle(base, rng, 0.05, np.array([0.0, DENORM_MIN, 3e38, np.inf, UNDEF_ABOVE, undef, np.nan], np.float32))
            else:
                start = (np.where(np.isfinite(first), first, _F(0)) + rng.uniform(-2, 2, (ny, nx))).astype(np.float32)
                _sprinkle(start, rng, 0.05, np.array([0.0, -0.0, DENORM_MIN, -FLT_MAX, FLT_MAX, np.inf, -np.inf, undef, np.nan, UNDEF_BELOW], np.float32))
                base = rng.uniform(-50, 3000, (nf, ny, nx)).astype(np.float32)
                if klass != "mid":
                    base = make_fields(rng, klass, decades, nf, 1, ny, nx, np.full((nf, 1), SOME_DEFINED), undef)[:, 0]
                _sprinkle(base, rng, 0.05, np.array([0.0, -0.0, DENORM_MIN, 3e38, -FLT_MAX, np.inf, -np.inf, UNDEF_ABOVE, undef, np.nan], np.float32))
            ex["start"], ex["fdef_start"] = start, int(rng.choice([ALL_DEFINED, SOME_DEFINED]))
            ex["base"], ex["fdef_base"] = [base[0], None], [ALL_DEFINED, SOME_DEFINED]
            ex["scale"] = [1.0, 0.5] if log else [1.0, -0.5]
    elif family == "vregrid":
        raise AssertionError("vregrid cases are made by make_vregrid_case")
    elif family == "pvort":
        xm = rng.uniform(0.5e-2, 2e-2, (ny, nx)).astype(np.float32)
        ym = rng.uniform(0.5e-2, 2e-2, (ny, nx)).astype(np.float32)
        for m in (xm, ym):
            _sprinkle(m, rng, 0.02, np.array([DENORM_MIN, 1e-40, FLT_MIN, 1e30, 3e38], np.float32))
        fc = rng.uniform(-1.0, 1.0, (ny, nx)).astype(np.float32)
        fc[ny // 2] = 0.0  # the equator
        _sprinkle(fc, rng, 0.05, FIELD_SPECIALS[:11])
        ex.update(xmapr=xm, ymapr=ym, fcoriolis=fc, scale=1e-30 if (klass == "mid" and kind == "field") else 1.0)
    for a in [case["fields"], case["flags"]] + [v for v in list(case.values()) + list(ex.values()) if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return case


# ------------------------------------------------------------------------------------------------ vinterp: the wave's interval
# vinterp_kernel looks at a pair of levels for a target only if the target lies in the interval that the pair spans over the
# whole WAVE (64 lanes of four cells on the 16-byte grid, of one cell off it), compared on integer keys; the cell's own test
# is a float compare.  The two can part only where the wave's minimum or maximum is itself a zero of either sign or a
# subnormal, or where an end of the float range is an end of the interval.  With coordinates drawn per cell that never
# happens, so these cases give a wave's worth of neighbouring cells the same column of coordinates: blocks of 256 cells
# (one wave on the grid, four off it), the rest of the grid a third block (a partial wave whose idle lanes walk cells 0 .. 3).
SEAM_BLOCK = 256
_D2 = _F(2) * DENORM_MIN
# columns of a `field` case; the pair that is the FIRST bracket of a target and ends on it:
SEAM_COLUMNS = {
    "A": [-np.inf, -FLT_MAX, -DENORM_MIN, -0.0, 1.5, 2.5, 3.5],  # (-inf, -FLT_MAX): -inf, -FLT_MAX; (-2^-149, -0.0): +-0
    "B": [_D2, DENORM_MIN, 0.0, -1.5, -2.5, FLT_MAX, np.inf],  # (2^-149, 2 * 2^-149): both; (+0.0, 2^-149): +-0; (.., FLT_MAX); (FLT_MAX, inf): inf
    "C": [-0.0, -0.0, 1.0, 2.0, 3.0, 4.0, 5.0],  # (-0.0, -0.0): +-0, and c_k == c_k+1
    "D": [-0.0, 0.0, -1.0, -2.0, -3.0, -4.0, -5.0],  # (-0.0, +0.0): +-0
    "Blog": [_D2, DENORM_MIN, 1e-3, 1.0, 50.0, FLT_MAX, np.inf],
    "Clog": [DENORM_MIN, _D2, 1e-3, 1.0, 50.0, FLT_MAX, np.inf],
}
# hybrid: alevel = (-0.0, 0, FLT_MAX, ...), blevel = (0.5, 1, 1, ...): levels 0 .. 2 are ps / 2 (-0.0 kept), ps, FLT_MAX + ps
SEAM_PS = {
    "A": -DENORM_MIN,  # (-0.0, -2^-149, FLT_MAX): the pair (-2^-149, -0.0)
    "B": _D2,  # (2^-149, 2 * 2^-149, FLT_MAX)
    "C": DENORM_MIN,  # (+0.0, 2^-149, FLT_MAX): half a subnormal rounds to zero
    "D": _F(-0.0),  # (-0.0, +0.0, FLT_MAX)
    "E": FLT_MAX,  # (FLT_MAX / 2, FLT_MAX, inf): the pair (FLT_MAX, inf)
}
SEAM_SPECS = [("field", "linear", NX_VEC, "ABD"), ("field", "linear", NX_ODD, "CDB"), ("hybrid", "linear", NX_VEC, "BAC"), ("hybrid", "linear", NX_ODD, "ACD"),
              ("hybrid", "linear", NX_VEC, "ACE"), ("field", "log", NX_VEC, "Blog,Clog,Blog"), ("field", "log", NX_ODD, "Clog,Blog,Clog")]
SEAM_TARGETS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX, np.inf, -np.inf, _D2, 1.25, -1.25, 2.75], np.float32)
SEAM_TARGETS_LOG = np.array([DENORM_MIN, _D2, 1e-40, FLT_MAX, np.inf, 0.5, 7.0], np.float32)


@functools.lru_cache(maxsize=None)
def vinterp_seam_cases():
    out = []
    for kind, method, nx, blocks in SEAM_SPECS:
        names = blocks.split(",") if "," in blocks else list(blocks)
        label = "vinterp-seam-%s-%s-%s-%dx%dx%d" % (kind, method, "".join(names), nx, NY, NLEV)
        rng = np.random.default_rng(_seed(label))
        cells = NY * nx
        block = np.minimum(np.arange(cells) // SEAM_BLOCK, 2)
        flags = make_flags(rng, 2, NLEV)
        fields = make_fields(rng, "mid", None, 2, NLEV, NY, nx, flags, UNDEF)
        case = dict(label=label, family="vinterp", kind=kind, method=method, klass="seam", undef=UNDEF, flags=flags, fields=fields, blocks=names,
                    extras=dict(targets=SEAM_TARGETS_LOG if method == "log" else SEAM_TARGETS))
        holes = np.arange(cells) % 37 == 11  # a few cells of every wave without a coordinate: carried as NaN through the wave's reduction
        if kind == "field":
            c = np.stack([np.array(SEAM_COLUMNS[n], np.float32) for n in names])[block].T.copy()  # (nlev, cells)
            c[1, holes] = UNDEF
            case.update(coord=c.reshape(NLEV, NY, nx), fdef_c=np.full(NLEV, SOME_DEFINED, np.int32))
        else:
            ps = np.array([SEAM_PS[n] for n in names], np.float32)[block]
            ps[holes] = UNDEF
            a = np.array([-0.0, 0.0, FLT_MAX, 1.0, 2.0, 3.0, 4.0], np.float32)
            b = np.array([0.5, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0], np.float32)
            case.update(ps=ps.reshape(NY, nx), ab=(a, b), fdef_c=SOME_DEFINED)
        for v in list(case.values()) + list(case["extras"].values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(case)
    return out


# ------------------------------------------------------------------------------------------------ vregrid: the targets
# Per cell and target plane one of five kinds (`tkind` of a case holds which):
#   0 on a level    the coordinate of a level of the cell's own column, bit for bit (weight 0 or 1, c_k == c_k+1 next to it)
#   1 midpoint      of two neighbouring levels, computed in double and rounded
#   2 beyond        below the smallest or above the largest usable coordinate of the column (for OUTSIDE_CLAMP); where that
#                   extreme is infinite the other side, where both are a midpoint
#   3 ordinary      a number drawn like vinterp's targets
#   4 special       +-0, +-2^-149, +-FLT_MAX, +-inf, NaN, 1e35 and both its neighbours; LOG bases: also -1.5
# fdef_t is ALL_DEFINED and SOME_DEFINED mixed; a stored 1e35 lies in planes of both.
TARGET_KINDS = ("on a level", "midpoint", "beyond", "ordinary", "special")
TARGET_SHARES = (0.25, 0.30, 0.20, 0.20, 0.05)
TARGET_SPECIALS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan, UNDEF, UNDEF_BELOW, UNDEF_ABOVE], np.float32)
TARGET_SPECIALS_LOG = np.concatenate([TARGET_SPECIALS, np.array([-1.5], np.float32)])
VREGRID_COMBOS = [(m, f, o) for m in ("linear", "log") for f in ("first", "last") for o in ("undef", "clamp")]
# planes per pass of vregrid_kernel: 15 at four cells per lane, 24 at one (mifc_capi_vregrid.hip, pass_targets); a base
# with one plane more takes two passes in that layout, so the found-mask and the slots in LDS are used again
VREGRID_NT, VREGRID_TB = 10, {4: 15, 1: 24}


def make_targets(rng, c, usable, nt, log, kind, undef):
    """(tcoord (nt, ny, nx), fdef_t, tkind) for the coordinate c (nlev, ny, nx) with its rule-1 mask."""
    nlev, ny, nx = c.shape
    cells = ny * nx
    cf = c.reshape(nlev, cells)
    uf = usable.reshape(nlev, cells) & ~np.isnan(cf)
    every = np.arange(cells)[None]
    what = rng.choice(len(TARGET_KINDS), size=(nt, cells), p=TARGET_SHARES)
    with np.errstate(all="ignore"):
        on_level = cf[rng.integers(0, nlev, (nt, cells)), every]
        k = rng.integers(0, nlev - 1, (nt, cells))
        mid = ((cf[k, every].astype(np.float64) + cf[k + 1, every].astype(np.float64)) * 0.5).astype(np.float32)
        cmin, cmax = np.where(uf, cf, INF).min(axis=0), np.where(uf, cf, -INF).max(axis=0)
        u = rng.uniform(0.5, 3, (nt, cells)).astype(np.float32)
        if log:
            below, above = np.nextafter(cmin * _F(0.5) + 0 * u, _F(0)), np.nextafter(cmax * _F(2) + 0 * u, INF)
        else:
            below, above = np.nextafter(cmin - u, -INF), np.nextafter(cmax + u, INF)
        can_below, can_above = np.isfinite(cmin) & ((cmin > 0) | (not log)), np.isfinite(cmax)
        side = rng.random((nt, cells)) < 0.5
        take_below = can_below[None] & (side | ~can_above[None])
        beyond = np.where(take_below, below, np.where(can_above[None], above, mid)).astype(np.float32)
        if log:
            ordinary = np.exp(rng.uniform(-90, 80, (nt, cells))) if kind != "hybrid" else rng.uniform(0.05, 8, (nt, cells))
        else:
            lo, hi = (-0.3, 0.3) if nlev == 2 else (0.05, 7) if kind == "hybrid" else (-2, 6)
            ordinary = rng.uniform(lo, hi, (nt, cells))
        special = rng.choice(TARGET_SPECIALS_LOG if log else TARGET_SPECIALS, size=(nt, cells))
    t = np.choose(what, [on_level, mid, beyond, ordinary.astype(np.float32), special]).astype(np.float32)
    fdef_t = rng.choice([ALL_DEFINED, SOME_DEFINED], size=nt).astype(np.int32)
    fdef_t[0], fdef_t[nt - 1] = SOME_DEFINED, ALL_DEFINED
    for p in (0, nt - 1):  # a stored 1e35 under both flag values
        at = rng.choice(cells, size=6, replace=False)
        t[p, at], what[p, at] = UNDEF, 4
    for p in range(nt):
        if fdef_t[p] == SOME_DEFINED:
            at = _sprinkle(t[p], rng, 0.01, np.array([undef], np.float32))
            what[p, at] = 4
    return t.reshape(nt, ny, nx), fdef_t, what.astype(np.int8).reshape(nt, ny, nx)


def log_runs_on_a_linear_base(kind, nlev, outside):
    """LOG on a base drawn by the LINEAR rule: where at most half of the outputs are holes (see the module docstring)."""
    return kind == "hybrid" or (kind == "field" and nlev == NLEV and outside == "clamp")


def _vregrid_spec(klass):
    V, O = NX_VEC, NX_ODD
    bases = [("hybrid", "linear", V, NLEV, False, VREGRID_TB[4] + 1, ""), ("field", "linear", O, NLEV, False, VREGRID_TB[1] + 1, ""),
             ("levels", "linear", O, NLEV, False, VREGRID_NT, ""), ("field", "log", V, NLEV, False, VREGRID_NT, ""), ("hybrid", "log", O, NLEV, False, VREGRID_NT, ""),
             ("levels", "log", V, NLEV, False, VREGRID_NT, ""), ("field", "linear", V, NLEV, True, VREGRID_NT, "")]
    if klass == "mid":
        bases += [("field", "linear", O, MIN_NLEV["vregrid"], False, VREGRID_NT, ""), ("hybrid", "linear", V, NLEV, False, VREGRID_NT, "-overflow")]
    return [(kind, rule, nx, nlev, nan_undef, "t%d.%s.%s.%s%s" % (nt, m, f, o, tail))
            for kind, rule, nx, nlev, nan_undef, nt, tail in bases for m, f, o in VREGRID_COMBOS
            if rule == "log" or m == "linear" or log_runs_on_a_linear_base(kind, nlev, o)]


@functools.lru_cache(maxsize=None)
def vregrid_base(klass, kind, rule, nx, nlev, nan_undef, nt, overflow):
    """The arrays that the combinations of one base share: fields, flags and the coordinate drawn exactly as make_case draws
    vinterp's, and the targets."""
    ny = NY
    label = "-".join(["vregrid", klass, kind, rule, "t%d" % nt] + (["overflow"] if overflow else []) + (["nan-undef"] if nan_undef else [])) + "-%dx%dx%d" % (nx, ny, nlev)
    rng = np.random.default_rng(_seed(label))
    undef = _F(np.nan) if nan_undef else UNDEF
    log = rule == "log"
    flags = make_flags(rng, 2, nlev)
    base = dict(family="vregrid", kind=kind, method=rule, klass=klass, undef=undef, flags=flags, base=label)
    base["fields"] = make_fields(rng, klass, HUGE_DECADES["vregrid", rule], 2, nlev, ny, nx, flags, undef, positive=log)
    if kind == "hybrid":
        base["fdef_c"] = int(rng.choice([ALL_DEFINED, SOME_DEFINED]))
        base["ps"], base["ab"] = make_hybrid(rng, nlev, ny, nx, base["fdef_c"], undef, log, overflow)
    elif kind == "field":
        base["fdef_c"] = make_coord_flags(rng, nlev)
        base["coord"] = (make_coord_log if log else make_coord_linear)(rng, nlev, ny, nx, base["fdef_c"], undef)
    else:
        base["levs"] = np.ascontiguousarray(LEVELS_LOG if log else LEVELS_LINEAR_B)
    c, usable = coordinate_of(base)
    if log:
        assert_log_spacing(c, usable)
    tcoord, fdef_t, tkind = make_targets(rng, c, usable, nt, log, kind, undef)
    base.update(tcoord=tcoord, fdef_t=fdef_t, tkind=tkind)
    for v in list(base.values()) + list(base.get("ab", ())):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return base


def make_vregrid_case(klass, kind, rule, nx, nlev, nan_undef, extra):
    overflow = extra.endswith("-overflow")
    nt, method, from_, outside = extra.replace("-overflow", "").split(".")
    base = vregrid_base(klass, kind, rule, nx, nlev, nan_undef, int(nt[1:]), overflow)
    label = "-".join(["vregrid", klass, kind, rule] + extra.split("-") + (["nan-undef"] if nan_undef else [])) + "-%dx%dx%d" % (nx, NY, nlev)
    case = {k: v for k, v in base.items() if k not in ("tcoord", "fdef_t")}
    case.update(label=label, extras=dict(tcoord=base["tcoord"], fdef_t=base["fdef_t"], method=method, from_=from_, outside=outside))
    return case


def vregrid_plain(case):
    """The case in the form of tests/vregrid_cases.py (what tests/test_vregrid_cpu.py hands to the rules header)."""
    kind, ex = case["kind"], case["extras"]
    out = dict(kind=kind, fields=case["fields"], tcoord=ex["tcoord"], flags=case["flags"], fdef_t=ex["fdef_t"], undef=case["undef"],
               coord=case["ps"] if kind == "hybrid" else case["coord"] if kind == "field" else case["levs"])
    if kind == "hybrid":
        out.update(ab=case["ab"], fdef_c=case["fdef_c"])
    elif kind == "field":
        out["fdef_c"] = case["fdef_c"]
    return out


# ------------------------------------------------------------------------------------------------ vregrid: the wave's interval
# vregrid_kernel skips a pair of levels where the interval [lo, hi] that the pair spans over the WAVE does not meet the
# interval [tmin, tmax] of the wave's usable targets of the pass: !(lo <= tmax && hi >= tmin), both reduced with fminf /
# fmaxf from [+inf, -inf].  The skip and the cell's own bracket test can part only where an end of the pair is itself the
# target and the wave's extreme on that side -- which per-cell random targets never make.  These cases give whole waves
# (blocks of 256 cells: one wave of four cells per lane, four waves of one) the same column of five levels
#   X, Ta, <hole>, Tb, Y        X <= Ta <= Tb <= Y
# and the targets Ta, Tb (and Ta again, with unusable targets sprinkled in): Ta is the smallest target of the wave and the
# upper end of the only pair that brackets it, Tb the largest and the lower end of its only pair.  The ends run through
# +-inf, +-FLT_MAX, +-FLT_MIN, +-2^-149 and zero, a zero level against the target of the other sign in both orders.
# Neighbouring blocks are far apart in value.  Three more blocks: targets that are all unusable; a lane whose coordinates are
# all NaN (stored, level 0 under an ALL_DEFINED flag) and one whose levels are undefined; one cell whose pairs are (-inf, +inf) (LOG: (2^-149, +inf)).
_Z = (_F(0.0), _F(-0.0))  # (level, target)
_ZR = (_F(-0.0), _F(0.0))
SEAM_ENDS = [(-INF, -FLT_MAX), (-FLT_MAX, -FLT_MIN), (-FLT_MIN, -DENORM_MIN), (-DENORM_MIN, _Z), (-DENORM_MIN, _ZR), (_Z, DENORM_MIN), (_ZR, DENORM_MIN),
             (DENORM_MIN, FLT_MIN), (FLT_MIN, FLT_MAX), (FLT_MAX, INF), (INF, INF), (-INF, -INF)]
SEAM_ENDS_LOG = [(_D2, FLT_MIN), (FLT_MIN, FLT_MAX), (FLT_MAX, INF), (INF, INF), (None, DENORM_MIN)]  # None: no pair below (LOG needs X > 0)
SEAM_EXTRA_BLOCKS = ("unusable targets", "a lane without levels", "a pair from -inf to +inf")
VREGRID_SEAM_NLEV, VREGRID_SEAM_NT = 5, 3


def _interleaved(n):
    half = (n + 1) // 2
    return [j // 2 + (half if j % 2 else 0) for j in range(n) if j // 2 + (half if j % 2 else 0) < n]


@functools.lru_cache(maxsize=None)
def vregrid_seam_bases():
    out = []
    for rule, ends in (("linear", SEAM_ENDS), ("log", SEAM_ENDS_LOG)):
        log = rule == "log"
        order = [ends[j] for j in _interleaved(len(ends))]
        nb = len(order) + len(SEAM_EXTRA_BLOCKS)
        nlev, nt, ny, nx = VREGRID_SEAM_NLEV, VREGRID_SEAM_NT, nb, SEAM_BLOCK
        label = "vregrid-seam-field-%s-%dx%dx%d" % (rule, nx, ny, nlev)
        rng = np.random.default_rng(_seed(label))
        flags = make_flags(rng, 2, nlev)
        fields = make_fields(rng, "mid", None, 2, nlev, ny, nx, flags, UNDEF, positive=log)
        c = np.empty((nlev, nb, SEAM_BLOCK), np.float32)
        t = np.empty((nt, nb, SEAM_BLOCK), np.float32)
        ordinary = np.array([1, 2, UNDEF, 3, 4], np.float32)
        with np.errstate(over="ignore"):
            for b, (ta, tb) in enumerate(order):
                (la, ta), (lb, tb) = (ta if isinstance(ta, tuple) else (ta, ta)), (tb if isinstance(tb, tuple) else (tb, tb))
                if la is None:  # the upper seam alone
                    col, ta = [UNDEF, UNDEF, UNDEF, lb, np.nextafter(_F(lb), INF)], tb
                else:
                    col = [np.nextafter(_F(la), -INF), la, UNDEF, lb, np.nextafter(_F(lb), INF)]
                c[:, b], t[:, b] = np.array(col, np.float32)[:, None], np.array([ta, tb, ta], np.float32)[:, None]
        for b in range(len(order), nb):
            c[:, b], t[:, b] = ordinary[:, None], np.array([2, 3, 2], np.float32)[:, None]
        b = len(order)
        t[:, b, :] = UNDEF
        t[1, b, ::3] = np.nan
        if log:
            t[2, b, ::5] = -1.0
        c[:, b + 1, 8:12] = np.nan  # a lane of four cells (four lanes of one) whose coordinates are all NaN: level 0 is flagged ALL_DEFINED,
        c[1:, b + 1, 16:20] = UNDEF  # so there the NaN is a stored value that is not usable; and one that is undef below a NaN
        c[0, b + 1, 16:20] = np.nan
        c[:, b + 2, 5] = np.array([DENORM_MIN if log else -np.inf, np.inf, UNDEF, DENORM_MIN if log else -np.inf, np.inf], np.float32)
        c, t = c.reshape(nlev, -1), t.reshape(nt, -1)
        i = np.arange(nb * SEAM_BLOCK)
        c[1, i % 37 == 11] = UNDEF  # a few cells of every wave lose their lower pair
        t[2, i % 41 == 7] = UNDEF  # and a few targets are not usable: NaN to the wave's reduction
        t[2, i % 41 == 19] = np.nan
        base = dict(family="vregrid", kind="field", method=rule, klass="seam", undef=UNDEF, flags=flags, fields=fields, base=label, blocks=order,
                    coord=c.reshape(nlev, ny, nx), fdef_c=np.array([ALL_DEFINED] + [SOME_DEFINED] * (nlev - 1), np.int32), tcoord=t.reshape(nt, ny, nx), fdef_t=np.full(nt, SOME_DEFINED, np.int32))
        for v in base.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(base)
    return out


@functools.lru_cache(maxsize=None)
def vregrid_seam_cases():
    """Every (from, outside) on the two seam bases, each with the method of its rule."""
    out = []
    for base in vregrid_seam_bases():
        for m, f, o in VREGRID_COMBOS:
            if m == base["method"]:
                case = {k: v for k, v in base.items() if k not in ("tcoord", "fdef_t")}
                case.update(label=base["base"].replace("-%d" % SEAM_BLOCK, "-%s.%s.%s-%d" % (m, f, o, SEAM_BLOCK), 1),
                            extras=dict(tcoord=base["tcoord"], fdef_t=base["fdef_t"], method=m, from_=f, outside=o))
                out.append(case)
    return out


# ------------------------------------------------------------------------------------------------ vregrid: columns by hand
# Rule 5 of mifc_vregrid_* (include/mifc.h) where the compares are at their ends, and rule 1 of the `levels` form (c_k =
# levels[k], the sign of a zero included).  Each column: coordinate, targets, and per `outside` the index of the level whose
# value is expected (None: undef); the values are x_k = k + 1.  The same in both directions.
HAND_COLUMNS = [
    # infinite extremes: ct < -inf and ct > +inf are false, the hole leaves no bracket
    dict(c=[-np.inf, UNDEF, np.inf], t=[5.0, -np.inf, np.inf, -FLT_MAX], undef=[None] * 4, clamp=[None] * 4),
    # a target of +-inf beyond finite extremes
    dict(c=[1, 2, 3], t=[np.inf, -np.inf], undef=[None, None], clamp=[2, 0]),
    dict(c=[3, 2, 1], t=[np.inf, -np.inf], undef=[None, None], clamp=[0, 2]),
    dict(c=[-FLT_MAX, 0, FLT_MAX], t=[np.inf, -np.inf], undef=[None, None], clamp=[2, 0]),
    # extremes tied between +0 and -0 at different levels: the lowest index
    dict(c=[-0.0, 3, 0.0, 7], t=[-1.0, -DENORM_MIN], undef=[None, None], clamp=[0, 0]),
    dict(c=[0.0, 3, -0.0, 7], t=[-1.0, -DENORM_MIN], undef=[None, None], clamp=[0, 0]),
    dict(c=[-5, 0.0, -3, -0.0], t=[1.0, DENORM_MIN], undef=[None, None], clamp=[1, 1]),
    dict(c=[-5, -0.0, -3, 0.0], t=[1.0, DENORM_MIN], undef=[None, None], clamp=[1, 1]),
    # a target equal to cmin / cmax that holes left without a bracket: not beyond, so undef
    dict(c=[1, UNDEF, 3], t=[1.0, 3.0, 0.5, 3.5], undef=[None] * 4, clamp=[None, None, 0, 2]),
    dict(c=[-0.0, UNDEF, DENORM_MIN], t=[0.0, DENORM_MIN, -DENORM_MIN, 2 * float(DENORM_MIN)], undef=[None] * 4, clamp=[None, None, 0, 2]),
]


def vregrid_hand_case(from_, outside):
    """The hand columns side by side as one `field` case (ny = 1), and the expected output (1, nt, 1, ncolumns)."""
    nlev, nt, n = max(len(h["c"]) for h in HAND_COLUMNS), max(len(h["t"]) for h in HAND_COLUMNS), len(HAND_COLUMNS)
    c, t = np.full((nlev, 1, n), UNDEF, np.float32), np.full((nt, 1, n), UNDEF, np.float32)
    x = np.broadcast_to(np.arange(1, nlev + 1, dtype=np.float32).reshape(1, nlev, 1, 1), (1, nlev, 1, n)).copy()
    want = np.full((1, nt, 1, n), UNDEF, np.float32)
    for i, h in enumerate(HAND_COLUMNS):
        c[:len(h["c"]), 0, i], t[:len(h["t"]), 0, i] = np.array(h["c"], np.float32), np.array(h["t"], np.float32)
        for j, k in enumerate(h[outside]):
            want[0, j, 0, i] = UNDEF if k is None else k + 1
    case = dict(label="vregrid-hand-%s-%s" % (from_, outside), family="vregrid", kind="field", method="linear", klass="hand", undef=UNDEF, fields=x,
                flags=np.full((1, nlev), SOME_DEFINED, np.int32), coord=c, fdef_c=np.full(nlev, SOME_DEFINED, np.int32),
                extras=dict(tcoord=t, fdef_t=np.full(nt, SOME_DEFINED, np.int32), method="linear", from_=from_, outside=outside))
    return case, want


def vregrid_zero_level_case(from_="first"):
    """`levels` form: c_k = levels[k] with the sign of a zero kept.  From the level -0 the target -0 has the weight
    (-0 - -0) / (1 - -0) = +0, and -0 + (+0) * (5 - -0) is +0; from a level +0 it would be -0 + (-0) * 5 = -0."""
    x = np.array([-0.0, 5.0], np.float32).reshape(1, 2, 1, 1) * np.ones((1, 1, 1, 3), np.float32)
    t = np.array([-0.0, 0.0, 1.0], np.float32).reshape(1, 1, 3)
    case = dict(label="vregrid-zero-level-" + from_, family="vregrid", kind="levels", method="linear", klass="hand", undef=UNDEF, fields=x,
                flags=np.full((1, 2), SOME_DEFINED, np.int32), levs=np.array([-0.0, 1.0], np.float32),
                extras=dict(tcoord=t, fdef_t=np.array([SOME_DEFINED], np.int32), method="linear", from_=from_, outside="undef"))
    return case, np.array([0.0, 0.0, 5.0], np.float32).reshape(1, 1, 1, 3)  # (the target +0: (+0 - -0) / 1 = +0 as well)


# ------------------------------------------------------------------------------------------------ the restatement of a case
def restate(case, mods=None, prefilter=None):
    """(out, flags_out) of the case by the family's restatement.  mods: the restatement modules to use instead (the CPU
    test's variants), a dict by family.  prefilter: vinterp only, see vinterp_restate.interpolate."""
    m = dict(vinterp=vi, vlayer=vl, vderiv=vd, vcumul=vc, pvort=pv, vregrid=vg)
    m.update(mods or {})
    family, kind, undef, ex = case["family"], case["kind"], case["undef"], case["extras"]
    x, fl = case["fields"], case["flags"]
    if family == "vregrid":
        how = (vg.LOG if ex["method"] == "log" else vg.LINEAR, vg.FROM_LAST if ex["from_"] == "last" else vg.FROM_FIRST,
               vg.OUTSIDE_CLAMP if ex["outside"] == "clamp" else vg.OUTSIDE_UNDEF)
        kw = {} if prefilter is None else dict(prefilter=prefilter)
        if kind == "hybrid":
            return m[family].hlevels(x, case["ps"], *case["ab"], ex["tcoord"], *how, fl, case["fdef_c"], ex["fdef_t"], undef, **kw)
        if kind == "field":
            return m[family].coord_fields(x, case["coord"], ex["tcoord"], *how, fl, case["fdef_c"], ex["fdef_t"], undef, **kw)
        return m[family].levels(x, case["levs"], ex["tcoord"], *how, fl, ex["fdef_t"], undef, **kw)
    if family == "vinterp":
        method = vi.LOG if case["method"] == "log" else vi.LINEAR
        if kind == "hybrid":
            return m[family].hlevels(x, case["ps"], *case["ab"], ex["targets"], method, fl, case["fdef_c"], undef, prefilter=prefilter)
        return m[family].coord_fields(x, case["coord"], ex["targets"], method, fl, case["fdef_c"], undef, prefilter=prefilter)
    if family == "vlayer":
        if kind == "hybrid":
            return m[family].hlevels(x, case["ps"], *case["ab"], vl.ALL_PRODUCTS, ex["lo"], ex["hi"], fl, case["fdef_c"], undef)
        return m[family].coord_fields(x, case["coord"], vl.ALL_PRODUCTS, ex["lo"], ex["hi"], fl, case["fdef_c"], undef)
    if family == "vderiv":
        if kind == "hybrid":
            return m[family].hlevels(x, case["ps"], *case["ab"], case["method"], fl, case["fdef_c"], undef)[:2]
        if kind == "field":
            return m[family].coord_fields(x, case["coord"], case["method"], fl, case["fdef_c"], undef)[:2]
        return m[family].levels(x, case["levs"], case["method"], fl, undef)[:2]
    if family == "vcumul":
        kw = {k: ex[k] for k in ("start", "fdef_start", "base", "fdef_base", "scale") if k in ex}
        if kind == "hybrid":
            return m[family].hlevels(x, case["ps"], *case["ab"], case["method"], ex["from_"], fl, case["fdef_c"], undef, **kw)
        if kind == "field":
            return m[family].coord_fields(x, case["coord"], case["method"], ex["from_"], fl, case["fdef_c"], undef, **kw)
        return m[family].levels(x, case["levs"], case["method"], ex["from_"], fl, undef, **kw)
    maps = (ex["xmapr"], ex["ymapr"], ex["fcoriolis"], case["method"], ex["scale"])
    if kind == "hybrid":
        return m[family].hlevels(x[0], x[1], x[2], case["ps"], *case["ab"], *maps, flags=fl, fdef_ps=case["fdef_c"], undef=undef)
    if kind == "field":
        return m[family].coord_fields(x[0], x[1], x[2], case["coord"], *maps, flags=fl, fdef_coord=case["fdef_c"], undef=undef)
    return m[family].levels(x[0], x[1], x[2], case["levs"], *maps, flags=fl, undef=undef)


_EXPECTED = {}


def expected(case):
    """The restatement of a case, computed once and read-only."""
    if case["label"] not in _EXPECTED:
        out, fd = restate(case)
        out.setflags(write=False)
        fd.setflags(write=False)
        _EXPECTED[case["label"]] = (out, fd)
    return _EXPECTED[case["label"]]


def widened(case, times):
    """The case tiled `times` times along y (columns are independent; pvort's rows are not: its seam rows differ and are
    computed anew): for the host call that needs more than one band."""
    def tile(a):
        a = np.asarray(a)
        reps = [1] * a.ndim
        reps[-2] = times
        return np.ascontiguousarray(np.tile(a, reps))
    out = dict(case, label=case["label"] + "-x%d" % times, fields=tile(case["fields"]))
    for k in ("ps", "coord"):
        if k in case:
            out[k] = tile(case[k])
    ex = dict(case["extras"])
    for k, v in ex.items():
        if isinstance(v, np.ndarray) and (v.ndim == 2 or k == "tcoord"):
            ex[k] = tile(v)
        elif k == "base":
            ex[k] = [None if b is None else tile(b) for b in v]
    out["extras"] = ex
    return out
