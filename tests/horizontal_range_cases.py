"""Seeded cases that put the horizontal families (mifc_hinterp_levels, mifc_hinterp_vector_levels, mifc_hstats_levels,
mifc_hremap_levels) at the ends of the float range (numpy only: no GPU, nothing read from the reference).
tests/test_horizontal_range_cpu.py asserts on the CPU that the cases reach what they are meant to reach and that they tell
the suspected mistakes (hinterp_restate.MISTAKES, hremap_restate.MISTAKES, hstats_restate.MISTAKES, a flush to zero, a float
intermediate) from the definition; tests/test_gpu_horizontal_range.py runs them through the library.

A case is a dict with label, family (hinterp | hvector | hremap | hstats), klass (huge | tiny | mid), undef, fields float32
(nf, nlev, ny, nx), flags int32 (nf, nlev) and
  hinterp  x, y float32[npos], method, marks {name: point}          hvector  the same with cosa, sina, fdef_rot (fields: u0, v0, u1, v1 ...)
  hremap   table (rowptr, col, w), mode, min_frac, marks {name: destination}
  hstats   minus, flags_minus, pivot, weight, fdef_weight, box (None where absent), mode, products

Magnitudes.  `huge`: 10^36.5 .. 10^38.5 with random signs, so that differences, products and sums leave the float range
but not the double range and results straddle FLT_MAX; `tiny`: 10^-44.5 .. 10^-37.6, subnormal inputs and results around
FLT_MIN; `mid`: N(280, 10).  Every class is sprinkled with +-0, +-2^-149, +-FLT_MIN, +-FLT_MAX, +-inf, both float
neighbours of 1e35, a stored 1e35 and NaN on levels flagged ALL_DEFINED and a stored undef on SOME_DEFINED levels -- where
the family's layout below leaves a cell free.

hinterp, grid 9 x 13 (rows x columns).  Rows 0..5 by columns 0..5 hold defined finite values only: every point of cell
1..3 by 1..3 takes the cubic rule at every level.  Rows 0..3 by columns 6..9 hold +-M in the sign pattern (-, +, +, -) by
(-, +, +, -), M = FLT_MAX in `huge`: the cubic rule overshoots to 1.5625 M at (7.5, 1.5), an infinity from finite inputs.
Rows 4..8 by columns 6..11 hold the corner scenarios (hinterp_scenario), the points that go with them are HINTERP_MARKS.
The rest of the grid is sprinkled with every special.  Points: wave 0 takes the cubic rule in no lane, wave 1 in every
lane, wave 2 in the even lanes while the odd ones hold inf or NaN in the corners their block is folded onto (column 12);
then the marks, the special positions of each axis against random ones and against each other, and random points.
"""
import functools
import zlib

import numpy as np

import hinterp_restate as hi
import hremap_restate as hr
import hstats_restate as hs
import vrotate_restate as vr

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = hi.ALL_DEFINED, hi.NONE_DEFINED, hi.SOME_DEFINED
UNDEF = hi.UNDEF
FAMILIES = ("hinterp", "hvector", "hremap", "hstats")
CLASSES = ("huge", "tiny", "mid")

_F = np.float32
FLT_MAX, FLT_MIN, DENORM_MIN = np.finfo(np.float32).max, np.finfo(np.float32).tiny, _F(2.0) ** _F(-149)
INF, NAN = _F(np.inf), _F(np.nan)
UNDEF_BELOW, UNDEF_ABOVE = np.nextafter(UNDEF, _F(0)), np.nextafter(UNDEF, INF)
TWICE_UNDEF = _F(2) * UNDEF  # exact: the midpoint of 0 and this, and half of it, is 1e35f bit for bit
assert _F(0.5 * float(TWICE_UNDEF)).view(np.uint32) == UNDEF.view(np.uint32)

FINITE_SPECIALS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, UNDEF_BELOW, UNDEF_ABOVE], np.float32)
SPECIALS = np.concatenate([FINITE_SPECIALS, np.array([np.inf, -np.inf], np.float32)])
HUGE_DECADES, TINY_DECADES = (36.5, 38.5), (-44.5, -37.6)


def _seed(label):
    return zlib.crc32(label.encode())


def _sprinkle(a, rng, rate, values, where=None):
    """Overwrites a share `rate` of a (of its cells `where`, a bool array like a) with draws from values."""
    flat = a.reshape(-1)
    pick = rng.random(flat.size) < rate
    if where is not None:
        pick &= np.broadcast_to(where, a.shape).reshape(-1)
    at = np.nonzero(pick)[0]
    flat[at] = rng.choice(values, size=at.size)


def magnitudes(rng, klass, shape, centre=280.0):
    if klass == "mid":
        return rng.normal(centre, 10, shape).astype(np.float32)
    lo, hi_ = HUGE_DECADES if klass == "huge" else TINY_DECADES
    x = 10.0 ** rng.uniform(lo, hi_, shape) * rng.choice([-1.0, 1.0], size=shape)
    return np.clip(x, -float(FLT_MAX), float(FLT_MAX)).astype(np.float32)


def mixed_flags(rng, nf, nlev, every=False):
    """ALL_DEFINED and SOME_DEFINED mixed: level 0 SOME_DEFINED and the last level ALL_DEFINED in every field."""
    if every:
        return np.full((nf, nlev), ALL_DEFINED, np.int32)
    fl = rng.choice([ALL_DEFINED, SOME_DEFINED], size=(nf, nlev)).astype(np.int32)
    fl[:, 0] = SOME_DEFINED
    fl[:, nlev - 1] = ALL_DEFINED
    return fl


def holes_and_values(x, rng, flags, rate, where=None, undef=UNDEF):
    """Per (field, level): a stored 1e35 and NaN where the flag is ALL_DEFINED (values there), a stored undef elsewhere."""
    for f in range(x.shape[0]):
        for k in range(x.shape[1]):
            if flags[f, k] == ALL_DEFINED:
                _sprinkle(x[f, k], rng, rate, np.array([UNDEF, np.nan], np.float32), where)
            else:
                _sprinkle(x[f, k], rng, rate, np.array([undef], np.float32), where)


# ====================================================================================================== hinterp
NY, NX, NPOS = 9, 13, 600
HINTERP_MARKS = {  # name: (x, y) of a point that goes with hinterp_scenario
    "overflow and back": (6.5, 4.0),        # -FLT_MAX + 0.5 * (FLT_MAX - -FLT_MAX) = 0: x10 - x00 leaves the float range
    "inf minus inf": (6.25, 5.0),           # inf + 0.25 * (inf - inf): a computed NaN, stored and not counted
    "node": (8.0, 4.0),                     # a == 0 and b == 0: inf, NaN, undef in the three corners that are not needed
    "on a column": (10.0, 4.5),             # a == 0: inf and NaN in column 11, which is not needed
    "on a row": (8.5, 6.0),                 # b == 0: undef and inf in row 7, which is not needed
    "zero weight times inf": (8.5, 2.0),    # b == 0, a != 0, inf in row j0 + 2: NaN by rule 6, finite by rule 5
    "overshoot": (7.5, 1.5),                # the cubic rule on the (-, +, +, -) pattern: 1.5625 M
    "equal to undef": (6.5, 8.0),           # 0 + 0.5 * (2e35f - 0) = 1e35f: a value
}


def hinterp_scenario(x, klass):
    """The designed cells of one level x (9, 13): see the module docstring."""
    m = {"huge": FLT_MAX, "tiny": _F(4) * DENORM_MIN, "mid": _F(300)}[klass]
    sg = np.array([-1, 1, 1, -1], np.float32)
    x[0:4, 6:10] = (sg[:, None] * sg[None, :]) * m
    x[4, 6], x[4, 7], x[4, 9], x[4, 11] = -FLT_MAX, FLT_MAX, INF, INF
    x[5, 6], x[5, 7], x[5, 8], x[5, 9], x[5, 11] = INF, INF, NAN, UNDEF, NAN
    x[7, 8], x[7, 9] = UNDEF, INF
    x[8, 6], x[8, 7] = 0.0, TWICE_UNDEF


def hinterp_free_cells():
    """Where every special may go: not the clean block, not the pattern and its column 10, not the scenario."""
    free = np.ones((NY, NX), bool)
    free[0:6, 0:6] = False
    free[0:4, 6:11] = False
    free[4:9, 6:12] = False
    return free


def hinterp_fields(rng, klass, nf, nlev, ny, nx, flags, vector=False):
    """vector: the fields are u0, v0, u1, v1 ...; the pattern of every v is a quarter as large, so that at the overshoot
    mark u leaves the float range and v does not: the rotation of (inf, finite) gives two infinities, of (inf, inf) a NaN."""
    x = magnitudes(rng, klass, (nf, nlev, ny, nx)) - (5 * np.arange(nf, dtype=np.float32).reshape(-1, 1, 1, 1) if klass == "mid" else 0)
    x = x.astype(np.float32)
    if (ny, nx) != (NY, NX):  # a degenerate grid: specials everywhere
        _sprinkle(x, rng, 0.08, SPECIALS)
        holes_and_values(x, rng, flags, 0.04)
        return x
    free = hinterp_free_cells()
    _sprinkle(x, rng, 0.06, FINITE_SPECIALS, ~free & (np.arange(NX) < 6))  # the clean block: defined finite specials
    _sprinkle(x, rng, 0.25, SPECIALS, free)
    holes_and_values(x, rng, flags, 0.10, free)
    for f in range(nf):
        for k in range(nlev):
            hinterp_scenario(x[f, k], klass)
            if f % 2:
                x[f, k, 0:4, 6:10] = x[f, k, 0:4, 6:10] * _F(0.25) if vector else -x[f, k, 0:4, 6:10]
            x[f, k, 0::2, 12] = INF if k % 2 else -INF  # the corners of the odd lanes of wave 2
            if flags[f, k] == ALL_DEFINED:
                x[f, k, 1::4, 12] = NAN
    return x


def axis_specials(n):
    """The positions of one axis of n nodes that the rules turn on."""
    v = [0.0, -0.0, DENORM_MIN, FLT_MIN, -DENORM_MIN, np.nextafter(_F(0.5), _F(0)), 0.5, np.nextafter(_F(0.5), _F(1)), np.inf, -np.inf, np.nan,
         UNDEF, FLT_MAX, -1.0, n - 0.5]
    for k in range(n):
        v += [np.nextafter(_F(k), -INF), k, np.nextafter(_F(k), INF)]  # the one above n - 1 is outside
        if k < n - 1:
            v += [k + 0.5, np.nextafter(_F(k + 0.5), _F(0))]
    return np.array(v, np.float32)


def hinterp_points(ny, nx, npos, seed, calm_share=0.9):
    """(x, y, marks): see the module docstring; on a degenerate grid the special positions and random points only."""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    marks = {}
    if (ny, nx) == (NY, NX):
        # wave 0: no lane takes the cubic rule -- cells of column 0 and of row 0, and nodes
        ring = np.arange(64) % 4
        xs.append(np.where(ring == 0, rng.uniform(0.1, 0.9, 64), np.where(ring == 1, rng.uniform(0, 8, 64), rng.integers(0, 6, 64))))
        ys.append(np.where(ring == 0, rng.uniform(0, 5, 64), np.where(ring == 1, rng.uniform(0.1, 0.9, 64), rng.integers(0, 6, 64))))
        # wave 1: every lane does (cells 1..3 by 1..3 of the clean block); eight on rows (b == 0), eight on columns (a == 0)
        for lanes in (np.ones(64, bool), np.arange(64) % 2 == 0):
            x = rng.integers(1, 4, 64) + rng.uniform(0.05, 0.95, 64)
            y = rng.integers(1, 4, 64) + rng.uniform(0.05, 0.95, 64)
            y[8:24:2], x[24:40:2] = np.floor(y[8:24:2]), np.floor(x[24:40:2])
            # wave 2: the odd lanes in the cells of columns 11 and 12, which the rule never reaches
            # (column 12 holds +-inf in the even rows: from row 7 the upper corners are finite and the result is an infinity;
            # from an even row it is inf - inf)
            xs.append(np.where(lanes, x, nx - 2 + rng.uniform(0.1, 0.9, 64)))
            ys.append(np.where(lanes, y, np.where(np.arange(64) % 8 == 1, rng.uniform(0, ny - 1, 64), 7 + rng.uniform(0.1, 0.9, 64))))
        for name, (x, y) in HINTERP_MARKS.items():
            marks[name] = sum(a.size for a in xs)
            xs.append(np.array([x]))
            ys.append(np.array([y]))
    sx, sy = axis_specials(nx), axis_specials(ny)

    def inside(n, m, calm=3.9):
        """m usable coordinates of an axis of n nodes, three in ten on a node; calm_share of them below `calm`, where the
        infinities of the scenario and of the free cells are out of reach of the cubic rule: cells 0..3 by 0..3, and
        rows 0 and 1 up to column 8 (the cases compare numbers, not NaN with NaN)."""
        near = np.where(rng.random(m) < calm_share, rng.uniform(0, min(n - 1, calm), m), rng.uniform(0, n - 1, m))
        return np.where(rng.random(m) < 0.3, np.floor(near), near)

    xs += [sx, inside(nx, sy.size)]
    ys += [inside(ny, sx.size, 1.9), sy]
    if nx > 1 and ny > 1:  # (on a degenerate grid nearly every special position of the short axis is outside)
        both = 48
        xs.append(sx[np.arange(both) % sx.size])
        ys.append(sy[(np.arange(both) * 7 + 3) % sy.size])
    x, y = np.concatenate(xs).astype(np.float32), np.concatenate(ys).astype(np.float32)
    rest = npos - x.size
    assert rest > 0, (npos, x.size)
    rx, ry = inside(nx, rest), inside(ny, rest)
    out = rest // 8  # an eighth of them around the grid: outside on one side or the other
    rx[:out], ry[:out] = rng.uniform(-0.5, nx - 0.5, out), rng.uniform(-0.5, ny - 0.5, out)
    return np.concatenate([x, rx.astype(np.float32)]), np.concatenate([y, ry.astype(np.float32)]), marks


def hinterp_case(klass, method, nf, nlev=7, ny=NY, nx=NX, npos=NPOS, every=False, family="hinterp", fdef_rot=SOME_DEFINED):
    label = "%s-%s-%s-%dx%dx%d-nf%d%s" % (family, klass, method, nx, ny, nlev, nf, "-untested" if every else "")
    rng = np.random.default_rng(_seed(label))
    flags = mixed_flags(rng, nf, nlev, every)
    vector = family == "hvector"
    # (a pair is NaN where either component is: the rotating entry keeps more of its points away from the infinities)
    x, y, marks = hinterp_points(ny, nx, npos, _seed(label) + 1, 0.97 if vector else 0.9)
    case = dict(label=label, family=family, klass=klass, undef=UNDEF, method=method,
                fields=hinterp_fields(rng, klass, nf, nlev, ny, nx, flags, vector), flags=flags, x=x, y=y, marks=marks)
    if family == "hvector":  # coefficients of every size: +-0, subnormal, of the size of FLT_MAX, and the undefined ones
        angle = rng.uniform(-np.pi, np.pi, npos)
        c, s = np.cos(angle).astype(np.float32), np.sin(angle).astype(np.float32)
        values = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1e-40, FLT_MAX, -FLT_MAX, 3e38, np.inf, -np.inf, np.nan, UNDEF], np.float32)
        for m, v in enumerate(values):  # each of them once in either, at a usable point of the cubic waves
            c[64 + 5 * m], s[66 + 5 * m] = v, v
        c[marks["overshoot"]], s[marks["overshoot"]] = 0.6, -0.8  # u' = 0.6 inf - -0.8 v = +inf, v' = -0.8 inf + 0.6 v = -inf
        case.update(cosa=c, sina=s, fdef_rot=fdef_rot)
    return case


def hinterp_clean_case():
    """Every position usable, every value defined, the levels tested: the flags come back ALL_DEFINED although one result
    is bit-equal to undef."""
    label = "hinterp-mid-bilinear-clean-13x9x2-nf1"
    rng = np.random.default_rng(_seed(label))
    fields = magnitudes(rng, "mid", (1, 2, NY, NX))
    fields[:, :, 8, 6], fields[:, :, 8, 7] = 0.0, TWICE_UNDEF
    x, y = rng.uniform(0, NX - 1, 70).astype(np.float32), rng.uniform(0, 6.9, 70).astype(np.float32)
    x[33], y[33] = HINTERP_MARKS["equal to undef"]
    return dict(label=label, family="hinterp", klass="mid", undef=UNDEF, method="bilinear", fields=fields, flags=np.full((1, 2), SOME_DEFINED, np.int32),
                x=x, y=y, marks={"equal to undef": 33})


@functools.lru_cache(maxsize=None)
def hinterp_cases(klass):
    if klass == "huge":
        return [hinterp_case(klass, "nearest", 2), hinterp_case(klass, "bilinear", 4), hinterp_case(klass, "bicubic", 3)]
    if klass == "tiny":
        return [hinterp_case(klass, "nearest", 1, every=True), hinterp_case(klass, "bilinear", 3), hinterp_case(klass, "bicubic", 4, every=True),
                hinterp_case(klass, "bicubic", 2)]
    return [hinterp_case(klass, "nearest", 3), hinterp_case(klass, "bilinear", 1, nlev=1), hinterp_case(klass, "bicubic", 2, nlev=2),
            hinterp_case(klass, "bicubic", 2, nlev=3, ny=1, npos=300), hinterp_case(klass, "bilinear", 2, nlev=3, nx=1, npos=300), hinterp_clean_case()]


@functools.lru_cache(maxsize=None)
def hvector_cases(klass):
    make = functools.partial(hinterp_case, family="hvector")
    if klass == "huge":
        return [make(klass, "bilinear", 4, fdef_rot=ALL_DEFINED), make(klass, "bicubic", 2)]
    if klass == "tiny":
        return [make(klass, "bicubic", 4, every=True, fdef_rot=ALL_DEFINED), make(klass, "nearest", 2)]
    return [make(klass, "nearest", 4, nlev=2), make(klass, "bilinear", 2, nlev=1, fdef_rot=ALL_DEFINED)]


# ====================================================================================================== hremap
NSRC, NDST = NY * NX, 200  # four slices of 64 destinations, the last one partial
# source cells with a designed value on every level of every field (flat indices; cell 0 is what the padding entries of
# an empty row name, and a row's first cell is what its own padding entries name: mifc_hremap_plan.h)
SRC = dict(pad0=0, one=1, max=2, nmax=3, inf=4, nan=5, und=6, den=7, min=8, twice_undef=9, big=10, four=11, a=12, b=13)
SRC_VALUES = dict(pad0=INF, one=1.0, max=FLT_MAX, nmax=-FLT_MAX, inf=INF, nan=NAN, und=UNDEF, den=DENORM_MIN, min=FLT_MIN, twice_undef=TWICE_UNDEF,
                  big=3e38, four=4.0, a=1.5, b=-2.5)
SAFE = np.arange(14, 60)  # cells that hold a defined value on every level: the rows of a slice without a bad entry draw from them
EPS53 = _F(2.0 ** -53)  # one double ulp of a sum in [0.5, 1)
MIN_FRAC_ROUNDS = 0.75 / (0.75 + float(_F(0.3)))  # times Wall = 0.75 + 0.3f the product is not exact: it rounds to 0.75 (asserted on the CPU)


def designed_rows():
    """name: (slice, [(source cell name, weight) ...]); the rows with an entry at `und` or `nan` have a bad entry on the
    levels that test (SOME_DEFINED)."""
    big = FLT_MAX
    return {
        # slice 0: no bad entry on any level
        "cancels": (0, [("max", big), ("one", 1.0), ("nmax", big)]),                # FLT_MAX^2 + 1 - FLT_MAX^2 = 0 in sequence
        "overflows": (0, [("max", 2.0)]),                                            # (float)S = +inf
        "overflows down": (0, [("nmax", 1.5), ("nmax", 0.5)]),                       # -inf
        "subnormal": (0, [("min", 0.25), ("den", 3.0)]),                             # (float)S subnormal
        "minus zero times inf": (0, [("inf", -0.0), ("a", 1.0)]),                    # NaN
        "equal to undef": (0, [("twice_undef", 0.5)]),                               # a value
        "short after inf": (0, [("inf", 1.0)]),                                      # its padding entries name the cell that holds inf
        "short after inf, negative": (0, [("inf", -DENORM_MIN), ("four", 1.0)]),
        "long": (0, [("a", 0.125)] * 12),                                            # the slice is as wide as this row
        "wall zero, no bad": (0, [("a", 1.0), ("b", -1.0)]),
        # slice 1: every row has a bad entry where the level tests
        "wdef cancels": (1, [("und", 1.0), ("a", 0.5), ("b", -0.5)]),                # Wdef == 0.0: a hole under RENORM
        "wall zero": (1, [("und", 1.0), ("a", 0.5), ("b", -1.5)]),                   # Wall == 0.0, Wdef = -1
        "equal at one": (1, [("und", 0.0), ("a", 0.75)]),                            # |Wdef| == 1 * |Wall|
        "one ulp short at one": (1, [("und", EPS53), ("a", 0.75)]),                  # Wall = 0.75 + 2^-53
        "equal where it rounds": (1, [("a", 0.75), ("und", 0.3)]),                   # need = fl(MIN_FRAC_ROUNDS * Wall) == 0.75
        "one ulp short where it rounds": (1, [("a", 0.75), ("b", -EPS53), ("und", 0.3), ("und", EPS53)]),  # the same Wall (ties to even)
        "renorm overflows": (1, [("und", 0.25), ("big", 1.0)]),                      # (3e38 / 1) * 1.25
        "renorm overflows, wdef tiny": (1, [("nan", 2.0), ("big", DENORM_MIN)]),     # Wdef = 2^-149, (S / Wdef) * 2 leaves the range
        "all bad": (1, [("und", 0.5), ("nan", 0.5)]),
        "short after nan": (1, [("nan", 1.0)]),
        "long with a bad entry": (1, [("b", 0.0625)] * 8 + [("und", 0.5)] + [("a", -0.0)] * 5),
        # slice 2: mixed
        "bad in the mix": (2, [("four", 0.5), ("und", 0.5)]),
        "good in the mix": (2, [("four", 0.5), ("one", 0.5)]),
        "idle lane divides zero by zero": (2, [("a", 0.5), ("b", -0.5), ("pad0", 0.0)]),  # no bad entry: RENORM's lanes compute 0 * inf / 0 here
    }


def hremap_table(rng):
    """(rowptr, col, w, marks): the designed rows at random places of their slices, random rows around them.  Slice 0: no
    entry at a cell that can be undefined; slice 1: every row has an entry at `und`; slices 2 and 3: anything."""
    rows = [None] * NDST
    marks = {}
    for name, (sl, entries) in designed_rows().items():
        while True:
            d = sl * 64 + int(rng.integers(0, 64))
            if rows[d] is None:
                break
        rows[d] = ([SRC[c] for c, _ in entries], [w for _, w in entries])
        marks[name] = d
    special_w = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MIN, -FLT_MIN, 3e38, -3e38], np.float32)
    for d in range(NDST):
        if rows[d] is not None:
            continue
        sl = d // 64
        n = int(rng.integers(0, 10)) if sl != 1 else int(rng.integers(1, 10))
        if d == 150:
            n = 17
        col = rng.choice(SAFE, n) if sl == 0 else rng.integers(0, NSRC, n)
        w = (rng.uniform(0.05, 1.0, n) / max(n, 1) * 2.0).astype(np.float32)
        w = np.where(rng.random(n) < 0.2, -w, w).astype(np.float32)
        if sl != 0:  # (slice 0 keeps ordinary weights around the designed rows: its results compare numbers)
            _sprinkle(w, rng, 0.08, special_w)
        if sl == 1:
            col[int(rng.integers(0, n))] = SRC["und"]
        rows[d] = (list(col), list(w))
    rows[30] = rows[30] if 30 in marks.values() else ([], [])
    rows[131] = rows[131] if 131 in marks.values() else ([], [])  # empty rows beside long ones
    lengths = np.array([len(r[0]) for r in rows])
    rowptr = np.zeros(NDST + 1, np.int32)
    np.cumsum(lengths, out=rowptr[1:])
    col = np.array([c for r in rows for c in r[0]], np.int32)
    w = np.array([v for r in rows for v in r[1]], np.float32)
    return rowptr, col, w, marks


def hremap_fields(rng, klass, nf, nlev, flags):
    x = magnitudes(rng, klass, (nf, nlev, NY, NX))
    flat = x.reshape(nf, nlev, NSRC)
    other = np.zeros(NSRC, bool)
    other[60:] = True
    _sprinkle(flat, rng, 0.06, FINITE_SPECIALS, np.arange(NSRC) >= 14)
    _sprinkle(flat, rng, 0.05, SPECIALS, other)
    holes_and_values(flat, rng, flags, 0.05, other)
    for name, cell in SRC.items():
        flat[:, :, cell] = SRC_VALUES[name]
    return x


def hremap_case(klass, mode, min_frac, nf, nlev, every=False):
    label = "hremap-%s-%s-%.3g-%dx%d-nf%d%s" % (klass, mode, min_frac, NDST, nlev, nf, "-untested" if every else "")
    rng = np.random.default_rng(_seed(label))
    flags = mixed_flags(rng, nf, nlev, every)
    rowptr, col, w, marks = hremap_table(np.random.default_rng(_seed("hremap-table-" + klass)))
    return dict(label=label, family="hremap", klass=klass, undef=UNDEF, mode=mode, min_frac=float(min_frac), fields=hremap_fields(rng, klass, nf, nlev, flags),
                flags=flags, table=(rowptr, col, w), marks=marks)


def hremap_clean_case():
    """No empty row, no undefined value, the levels tested: the flags come back ALL_DEFINED although one result is
    bit-equal to undef."""
    label = "hremap-mid-renorm-clean-70x2-nf1"
    rng = np.random.default_rng(_seed(label))
    rowptr, col, w = hr.table_from_lengths(rng.integers(1, 6, 70), NSRC, 5)
    col, w = col.copy(), w.copy()
    col[col == SRC["twice_undef"]] = 20
    d = 41
    col[rowptr[d]:rowptr[d + 1]], w[rowptr[d]:rowptr[d + 1]] = SRC["twice_undef"], 0.0
    w[rowptr[d]] = 0.5
    fields = magnitudes(rng, "mid", (1, 2, NY, NX))
    fields.reshape(1, 2, NSRC)[:, :, SRC["twice_undef"]] = TWICE_UNDEF
    return dict(label=label, family="hremap", klass="mid", undef=UNDEF, mode="renorm", min_frac=0.5, fields=fields, flags=np.full((1, 2), SOME_DEFINED, np.int32),
                table=(rowptr, col, w), marks={"equal to undef": d})


@functools.lru_cache(maxsize=None)
def hremap_cases(klass):
    if klass == "huge":
        return [hremap_case(klass, "strict", 0.0, 2, 7), hremap_case(klass, "renorm", MIN_FRAC_ROUNDS, 1, 13), hremap_case(klass, "renorm", 1.0, 3, 7),
                hremap_case(klass, "renorm", 0.0, 4, 7, every=True)]
    if klass == "tiny":
        return [hremap_case(klass, "strict", 0.0, 3, 13, every=True), hremap_case(klass, "renorm", 1.0, 4, 7), hremap_case(klass, "renorm", 0.0, 1, 7)]
    return [hremap_case(klass, "strict", 0.0, 1, 7), hremap_case(klass, "renorm", 0.0, 3, 7), hremap_case(klass, "renorm", MIN_FRAC_ROUNDS, 2, 13),
            hremap_case(klass, "strict", 0.0, 1, 13, every=True), hremap_case(klass, "renorm", 1.0, 2, 7, every=True), hremap_clean_case()]


# ====================================================================================================== hstats
WIDE, SMALL = (4, 4100), (9, 13)  # (ny, nx): two segments per row on the 16-byte grid | one short segment off it
# the columns of a wide row that are the first and last cell of a segment, lanes 0 and 63 of a trip, the first and last trip
WIDE_COLUMNS = [0, 3, 252, 255, 256, 3840, 3843, 4092, 4095, 4096, 4099]
WIDE_BOX, SMALL_BOX, EIGHT_CELLS = (5, 4098, 1, 4), (1, 12, 2, 8), (2, 6, 3, 5)  # (i0, i1, j0, j1); the first cuts both 16-byte groups at its ends


def hstats_fields(rng, klass, nf, nlev, shape, flags, plain):
    """The fields of one hstats case.  Finite specials at the seam columns of every row and sprinkled; the specials that
    poison a sum (NaN under ALL_DEFINED; +inf beside -inf) in the last level only, rows 1 and 2; a stored undef under
    ALL_DEFINED in its row 3; with `plain` (no minus, pivot or weight) its row 0 holds 1e35 throughout: a mean that is
    bit-equal to undef.  Level 0 of the last field: row 1 undefined throughout (N == 0)."""
    ny, nx = shape
    x = magnitudes(rng, klass, (nf, nlev, ny, nx))
    cols = WIDE_COLUMNS if nx > 4096 else [0, 3, 4, nx - 1]
    for f in range(nf):
        for k in range(nlev):
            # (tiny: the specials of the size of FLT_MAX and 1e35 in level 2 only -- elsewhere the means stay float denormals)
            values = FINITE_SPECIALS[:6] if klass == "tiny" and k != 2 else FINITE_SPECIALS
            _sprinkle(x[f, k], rng, 0.03, values)
            if flags[f, k] != ALL_DEFINED:
                _sprinkle(x[f, k], rng, 0.03, np.array([UNDEF], np.float32))
            for j in range(ny):
                for m, i in enumerate(cols):
                    x[f, k, j, i] = values[(m + 3 * j + k + f) % values.size]
    last = nlev - 1  # ALL_DEFINED in every field
    x[:, last, 1, nx // 3], x[:, last, 1, nx - 2] = NAN, UNDEF
    x[:, last, 2, 1], x[:, last, 2, nx - 3] = INF, -INF
    x[:, last, 3, nx // 2], x[:, last, 3, 2] = UNDEF, UNDEF
    if plain:
        x[:, last, 0, :] = UNDEF
    x[nf - 1, 0, 1, :] = UNDEF
    return x


def hstats_case(klass, shape, mode, products, nf, nlev=7, minus=False, weight=None, pivot=False, box=None, every=False):
    """weight: None | "holes" (SOME_DEFINED: undefined weights over poison, a cancelling row) | "values" (ALL_DEFINED: +-0,
    subnormal, inf and NaN as weights in the last row)."""
    ny, nx = shape
    label = "hstats-%s-%dx%d-%s-p%d-nf%d%s%s%s%s%s" % (klass, nx, ny, mode, products, nf, "-minus" if minus else "", "-w" + weight if weight else "",
                                                       "-pivot" if pivot else "", "-box%d" % box[0] if box else "", "-untested" if every else "")
    rng = np.random.default_rng(_seed(label))
    flags = mixed_flags(rng, nf, nlev, every)
    x = hstats_fields(rng, klass, nf, nlev, shape, flags, plain=not (minus or weight or pivot))
    case = dict(label=label, family="hstats", klass=klass, undef=UNDEF, fields=x, flags=flags, mode=mode, products=products, minus=None, flags_minus=None,
                pivot=None, weight=None, fdef_weight=SOME_DEFINED, box=box)
    poison = np.array([np.inf, -np.inf, np.nan, UNDEF], np.float32)
    if minus:
        fm = mixed_flags(rng, nf, nlev, every)
        y = magnitudes(rng, klass, x.shape)
        _sprinkle(y, rng, 0.03, FINITE_SPECIALS)
        for f in range(nf):
            for k in range(nlev):
                if fm[f, k] != ALL_DEFINED:
                    _sprinkle(y[f, k], rng, 0.02, np.array([UNDEF], np.float32))
        if klass == "huge" and nlev > 5:  # a mean that leaves the float range: +-3e38 - -+3e38 along row 0 of level 5
            sign = np.where(np.arange(nf) % 2 == 0, 1, -1).astype(np.float32).reshape(nf, 1)
            x[:, 5, 0, :], y[:, 5, 0, :] = sign * _F(3e38), -sign * _F(3e38)
        case.update(minus=y, flags_minus=fm)
    if weight == "holes":
        w = rng.uniform(0.5, 2.0, shape).astype(np.float32)
        gone = rng.random(shape) < 0.04
        gone[:, cols_of(nx)] = True
        gone[2, :] = False
        w[2, :] = np.where(np.arange(nx) % 2 == 0, 1.0, -1.0)  # W == 0.0 with N > 0 where every cell of the row is defined: a hole
        gone[2, nx - 1] = nx % 2 == 1  # (an even number of them)
        w[gone] = UNDEF
        case.update(weight=w)
    elif weight == "values":
        w = rng.uniform(0.5, 2.0, shape).astype(np.float32)
        _sprinkle(w[:ny - 1], rng, 0.02, np.array([DENORM_MIN, -DENORM_MIN, FLT_MIN, 0.0, -0.0, UNDEF], np.float32))  # finite: values
        _sprinkle(w[ny - 1], rng, 0.3, np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, DENORM_MIN], np.float32))
        for m, v in enumerate([DENORM_MIN, -DENORM_MIN, FLT_MIN, 0.0, -0.0, UNDEF]):  # each of them at least once
            w[m % (ny - 1), (3 * m + 1) % nx] = v
        w[ny - 1, :6] = [np.inf, -np.inf, np.nan, 0.0, -0.0, DENORM_MIN]
        case.update(weight=w, fdef_weight=ALL_DEFINED)
    if pivot:
        p = magnitudes(rng, klass, (nf, nlev)).astype(np.float64)
        if nlev >= 7:
            x[0, 0] = np.where(rng.random(shape) < 0.5, _F(0.0), _F(-0.0))  # d, q1, MIN and MAX are double denormals
            p[0, 0] = 1e-310
            p[0, 1] = 1e200  # q2 is inf in double
            p[0, 2], p[0, 3], p[nf - 1, 5] = np.inf, np.nan, -np.inf
            j, i = (box[2], box[0]) if box else (0, 0)
            p[nf - 1, 4] = np.nextafter(np.float64(x[nf - 1, 4, j, i]), np.inf)  # one double ulp from a stored value
        case.update(pivot=p)
    if weight == "holes":  # what an undefined weight excludes is inf, NaN or a stored undef on every level
        for f in range(nf):
            for k in range(nlev):
                x[f, k][gone] = rng.choice(poison, size=int(gone.sum()))
    if box:  # inf, NaN and a stored undef everywhere outside the box, on every level
        i0, i1, j0, j1 = box
        out = np.ones(shape, bool)
        out[j0:j1, i0:i1] = False
        for a in (x, case["minus"]):
            if a is not None:
                for f in range(nf):
                    for k in range(nlev):
                        a[f, k][out] = rng.choice(poison, size=int(out.sum()))
    return case


def cols_of(nx):
    """Columns with an undefined weight in every row: a seam column of each kind."""
    return [3, 255, 4095, 4096] if nx > 4096 else [3, 4]


def outside_overwritten(case, value=np.inf):
    """The case with everything outside its box overwritten by `value`: the same statistics."""
    i0, i1, j0, j1 = case["box"]
    c = dict(case, label=case["label"] + "-outside-inf")
    for name in ("fields", "minus"):
        if case[name] is not None:
            a = case[name].copy()
            keep = a[:, :, j0:j1, i0:i1].copy()
            a[...] = value
            a[:, :, j0:j1, i0:i1] = keep
            c[name] = a
    return c


@functools.lru_cache(maxsize=None)
def hstats_cases(klass):
    both = hs.MOMENTS | hs.EXTREMES
    if klass == "huge":
        return [hstats_case(klass, WIDE, "area", both, 3, minus=True, weight="holes", pivot=True, box=WIDE_BOX),
                hstats_case(klass, WIDE, "rows", hs.MOMENTS, 3, minus=True),
                hstats_case(klass, SMALL, "rows", both, 1, weight="values")]
    if klass == "tiny":
        return [hstats_case(klass, WIDE, "rows", both, 4),
                hstats_case(klass, SMALL, "area", both, 2, pivot=True, box=EIGHT_CELLS),
                hstats_case(klass, WIDE, "area", both, 1, weight="holes", box=WIDE_BOX)]
    return [hstats_case(klass, WIDE, "rows", both, 1, every=True),
            hstats_case(klass, SMALL, "rows", hs.EXTREMES, 3, minus=True, pivot=True, box=SMALL_BOX),
            hstats_case(klass, WIDE, "rows", hs.MOMENTS, 2, minus=True, weight="holes"),
            hstats_case(klass, WIDE, "rows", both, 2, pivot=True)]


# ====================================================================================================== all families
def cases(family, klass):
    return {"hinterp": hinterp_cases, "hvector": hvector_cases, "hremap": hremap_cases, "hstats": hstats_cases}[family](klass)


def restate(case, mistakes=()):
    """The restatement of the case's family on it.  hinterp, hvector, hremap: (out, flags); hstats: (stats, mean, flags), the
    slots of a product group that was not asked for NaN."""
    family = case["family"]
    if family == "hinterp":
        return hi.sample(case["fields"], case["x"], case["y"], case["method"], case["flags"], case["undef"], mistakes=mistakes)
    if family == "hvector":
        assert not mistakes
        return vr.sample_rotate(case["fields"], case["x"], case["y"], case["cosa"], case["sina"], hi.METHODS[case["method"]], case["flags"], case["fdef_rot"],
                                case["undef"])
    if family == "hremap":
        return hr.remap(case["fields"], *case["table"], case["mode"], case["min_frac"], case["flags"], case["undef"], mistakes=mistakes)
    return hs.hstats(case["fields"], case["minus"], case["pivot"], case["weight"], case["box"], case["mode"], case["products"], case["flags"],
                     case["flags_minus"], case["fdef_weight"], case["undef"], fill=np.nan, mistakes=mistakes)


_EXPECTED = {}


def expected(case):
    """restate(case), computed once per label and read-only."""
    if case["label"] not in _EXPECTED:
        res = restate(case)
        for a in res:
            a.setflags(write=False)
        _EXPECTED[case["label"]] = res
    return _EXPECTED[case["label"]]


def widened(case, times):
    """The case with its grid repeated `times` along y, so that it is large enough for a host call to be staged in more
    than one chunk of levels or band of rows.  hinterp, hvector, hremap: the points and the table stay where they are, in
    the first copy (a point beyond row 8 of the original is inside now).  hstats: the minus batches and the weight are
    repeated with the fields, the box stays.  The expected result is restated like every other."""
    c = dict(case, label="%s-rows-x%d" % (case["label"], times), fields=np.tile(case["fields"], (1, 1, times, 1)))
    if case["family"] == "hstats":
        c["minus"] = None if case["minus"] is None else np.tile(case["minus"], (1, 1, times, 1))
        c["weight"] = None if case["weight"] is None else np.tile(case["weight"], (times, 1))
    return c
