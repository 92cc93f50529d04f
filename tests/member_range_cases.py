"""Seeded cases at the ends of the float range for the entries that walk ensemble members: the five single-field reductions
(mifc_sumFields, mifc_meanValue, mifc_stddevValue, mifc_extremeValue, mifc_probability: family "single"),
mifc_ensemble_levels ("levels") and mifc_ensembleQuantiles ("quantiles").  Numpy only: tests/test_member_range_cpu.py
asserts what the cases hold and which mistakes they tell from the definition, tests/test_gpu_member_range.py runs them
through the library bit for bit against expected(case).

Classes: "huge" 10^36.5 .. 10^38.5 with random signs (every value above undef = 1e35 in magnitude), "tiny" 10^-44.5 .. 10^-37.6
(mostly subnormal), "mid" N(280, 10).  In plain huge data Welford's m2 is infinite or NaN in every cell and in plain tiny
data it is 0 in every cell, so the batches of the reductions keep their columns from WELFORD_FROM[klass] * nx on for
Welford: magnitudes of one decade around 10^WELFORD_DECADE[klass][nmem], where m2 straddles FLT_MAX (huge) or m2 / n the
smallest normal float (tiny).  The table was bisected per member count on the restatement (see welford_share).

Every class is sprinkled with +-0, +-2^-149, +-FLT_MIN, +-FLT_MAX, both float neighbours of 1e35 and +-inf; a stored 1e35
and NaN of both signs go to (member, level) pairs flagged ALL_DEFINED (values there), a stored undef to the others (a hole
there).  The rates fall with the member count, so that a cell meets about as many of them whatever the ensemble size.
Level 0 has every member SOME_DEFINED and level 1 every member ALL_DEFINED -- the designed cells of row 0 count on that --,
the levels after them mix the two with NONE_DEFINED members.

One variant per family has undef = NaN.  Its product lists leave extremeValue out: with undef = NaN nothing ever equals
undef, the running value starts as NaN and stays, and an output that is NaN in every cell compares nothing (that quirk is
on the ordinary data of tests/test_gpu_ensemble_levels.py)."""
import functools
import zlib

import numpy as np

import ensemble_restate as er
import quantile_restate as qr

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = er.ALL_DEFINED, er.NONE_DEFINED, er.SOME_DEFINED
UNDEF = er.UNDEF
FAMILIES = ("single", "levels", "quantiles")
CLASSES = ("huge", "tiny", "mid")

_F = np.float32
FLT_MAX, FLT_MIN, DENORM_MIN = np.finfo(np.float32).max, np.finfo(np.float32).tiny, _F(2.0) ** _F(-149)
INF, NAN = _F(np.inf), _F(np.nan)
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
UNDEF_BELOW, UNDEF_ABOVE = np.nextafter(UNDEF, _F(0)), np.nextafter(UNDEF, INF)
HALF_UNDEF, TWICE_UNDEF = _F(0.5) * UNDEF, _F(2) * UNDEF  # exact: two halves, and the mean of 0 and twice, are 1e35f bit for bit
assert (HALF_UNDEF + HALF_UNDEF).view(np.uint32) == UNDEF.view(np.uint32) and (TWICE_UNDEF / _F(2)).view(np.uint32) == UNDEF.view(np.uint32)
BELOW_100 = np.nextafter(_F(100), _F(0))

FINITE_SPECIALS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, UNDEF_BELOW, UNDEF_ABOVE], np.float32)
SMALL_SPECIALS = FINITE_SPECIALS[:6]
HUGE_DECADES, TINY_DECADES = (36.5, 38.5), (-44.5, -37.6)

# The Welford columns: from this share of nx on.  The plain columns in front of them are where sums and means of huge data
# overflow; stddevValue is infinite or NaN there (huge) or zero (tiny).
WELFORD_FROM = {"huge": 0.4, "tiny": 0.5}
# 10^d is the centre of the decade the Welford columns draw from, per member count: bisected on the restatement until
# about half of the cells of a batch with every member counted have an infinite m2 (huge) or a subnormal, nonzero m2 / n
# (tiny); welford_share(klass, nmem, d) is the function that was bisected, test_member_range_cpu.py holds it to 20 .. 80 %.
# A quarter of a decade below the entry the share is 0 %, a quarter above it 96 % and more (huge) or 4 % and less (tiny).
WELFORD_DECADE = {
    "huge": {7: 18.73, 8: 18.69, 9: 18.66, 16: 18.52, 17: 18.50, 32: 18.36, 33: 18.35, 51: 18.25, 64: 18.20, 65: 18.20, 70: 18.18},
    "tiny": {7: -19.08, 8: -19.09, 9: -19.10, 16: -19.11, 17: -19.11, 32: -19.12, 33: -19.12, 51: -19.12, 64: -19.13, 65: -19.13, 70: -19.13},
}
MEMBER_COUNTS = (7, 8, 9, 16, 17, 32, 33, 51, 64, 65, 70)

# expected number of sprinkled values per cell (over all members), by kind of batch: the reductions turn one NaN, or two
# infinities of opposite sign, into a NaN result, the quantiles need an infinity at a chosen rank in a tenth of their cells
RATES = {"reductions": dict(finite=0.6, inf=0.10, nan=0.08, hole=0.5, welford=0.15),
         "quantiles": dict(finite=0.8, inf=1.2, nan=0.10, hole=0.6, welford=0.0)}  # (no Welford columns)


def _seed(label):
    return zlib.crc32(label.encode())


def _sprinkle(a, rng, rate, values, where=None):
    """Overwrites a share `rate` of a (of its cells `where`, a bool array that broadcasts to a) with draws from values."""
    flat = a.reshape(-1)
    pick = rng.random(flat.size) < rate
    if where is not None:
        pick &= np.broadcast_to(where, a.shape).reshape(-1)
    at = np.nonzero(pick)[0]
    flat[at] = rng.choice(values, size=at.size)


def magnitudes(rng, klass, shape):
    if klass == "mid":
        return rng.normal(280.0, 10, shape).astype(np.float32)
    lo, hi = HUGE_DECADES if klass == "huge" else TINY_DECADES
    x = 10.0 ** rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], size=shape)
    return np.clip(x, -float(FLT_MAX), float(FLT_MAX)).astype(np.float32)


def welford_values(rng, decade, shape):
    return (10.0 ** rng.uniform(decade - 0.5, decade + 0.5, shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def welford_share(klass, nmem, decade, cells=4000, seed=1):
    """The share of cells whose Welford m2 is infinite (huge), or whose m2 / n is subnormal and not zero (tiny), with every
    member counted: what WELFORD_DECADE was bisected on."""
    x = welford_values(np.random.default_rng(seed), decade, (nmem, 1, 1, cells))
    (out, _), = er.statistics(x, None, ["stddev"])
    return float(np.isinf(out).mean()) if klass == "huge" else float(under_root_is_subnormal(out).mean())


def under_root_is_subnormal(out):
    """stddevValue is the root of a float quotient: the root of a subnormal is normal (2^-149 gives 2^-74.5), so whether
    m2 / n was subnormal and not zero is read from the result: 0 < out < sqrt(FLT_MIN) = 2^-63."""
    return (out > 0) & (out < _F(2.0) ** _F(-63))


def member_flags(rng, nmem, nlev):
    fl = rng.choice([ALL_DEFINED, SOME_DEFINED, SOME_DEFINED, NONE_DEFINED], size=(nmem, nlev), p=[0.4, 0.25, 0.25, 0.1]).astype(np.int32)
    fl[:, 0] = SOME_DEFINED
    if nlev > 1:
        fl[:, 1] = ALL_DEFINED
    return fl


def member_batch(label, klass, nmem, nlev, ny, nx, kind, undef=UNDEF):
    """-> (members float32 (nmem, nlev, ny, nx), flags int32 (nmem, nlev)) with the sprinkles; row 0 is free for designs."""
    rng = np.random.default_rng(_seed(label))
    flags = member_flags(rng, nmem, nlev)
    x = magnitudes(rng, klass, (nmem, nlev, ny, nx))
    rate = {k: v / nmem for k, v in RATES[kind].items()}
    plain = np.ones((ny, nx), bool)
    if kind == "reductions" and klass in WELFORD_FROM:
        first = int(np.ceil(WELFORD_FROM[klass] * nx))
        x[..., first:] = welford_values(rng, WELFORD_DECADE[klass][nmem], (nmem, nlev, ny, nx - first))
        plain[:, first:] = False
    quiet = rate["welford"] * nmem  # the Welford columns get this share of every rate: a NaN or an overflow there ends the cell
    for where, share in ((plain, 1.0), (~plain, quiet)):
        _sprinkle(x, rng, share * rate["finite"], FINITE_SPECIALS if share == 1.0 else SMALL_SPECIALS, where)
        _sprinkle(x, rng, share * rate["inf"], np.array([np.inf, -np.inf], np.float32), where)
        for j in range(nmem):
            for l in range(nlev):
                if flags[j, l] == ALL_DEFINED:
                    _sprinkle(x[j, l], rng, share * rate["nan"], np.array([UNDEF, NAN, NEG_NAN], np.float32), where)
                else:
                    _sprinkle(x[j, l], rng, share * rate["hole"], np.array([undef], np.float32), where)
    return x, flags


# ================================================================================================= the reductions
def probabilities():
    """Limits at the values where a comparison can go wrong: +-0 against -+0 members, 2^-149 between 0 and 2 * 2^-149,
    +-FLT_MAX against +-inf, +inf, NaN, the neighbours of 1e35; all six computes, 3 and 6 also with limits[0] > limits[1]."""
    d = float(DENORM_MIN)
    return [("probability", 1, [0.0]), ("probability", 2, [-0.0]), ("probability", 3, [0.0, 2 * d]), ("probability", 4, [float(FLT_MAX)]),
            ("probability", 5, [-float(FLT_MAX)]), ("probability", 6, [float(UNDEF_BELOW), float(UNDEF_ABOVE)]), ("probability", 1, [np.inf]),
            ("probability", 2, [np.nan]), ("probability", 3, [1.0, -1.0]), ("probability", 6, [float(FLT_MAX), -float(FLT_MAX)]),
            ("probability", 4, [float(UNDEF_BELOW)]), ("probability", 5, [d])]


def class_probabilities(klass):
    """Two limits inside the class's own range, so that the counts are not all 0 or all nmem."""
    mid = {"huge": 1.0e37, "tiny": 1.0e-41, "mid": 280.0}[klass]
    return [("probability", 1, [mid]), ("probability", 6, [-mid, mid])]


def flagged(name, nlev):
    """A sum / extreme product with its per-level in/out flags: SOME_DEFINED on level 0, ALL_DEFINED on level 1, mixed after."""
    fl = np.array([SOME_DEFINED, ALL_DEFINED, SOME_DEFINED, ALL_DEFINED, NONE_DEFINED] * (nlev // 5 + 1), np.int32)[:nlev]
    return (name, fl)


def full_list(klass, nlev, extremes=True):
    """Every statistic (for the single-field entries): the seven of the fixed slots and all probabilities."""
    names = ["sum", "max", "min", "argmax", "argmin"] if extremes else ["sum"]
    return [flagged(n, nlev) for n in names] + ["mean", "stddev"] + probabilities() + class_probabilities(klass)


def fifteen(klass, nlev):
    prob = probabilities()
    return [flagged("sum", nlev), "mean", "stddev"] + [flagged(n, nlev) for n in ("max", "min", "argmax", "argmin")] + prob[:6] + class_probabilities(klass)


def instance_lists(klass, nlev):
    """One product list per instantiation of launch_ensemble_levels: {welford} x {flagged} x {np 0, 1..3, 4..8} -- the key is
    (welford, flagged, np) as the 16-byte launch reports it; the list of stddev and probabilities alone takes the <1, 1, 3>
    detour -- and all fifteen products together."""
    p, own = probabilities(), class_probabilities(klass)
    fl = lambda n: flagged(n, nlev)  # noqa: E731
    return [
        ((0, 0, 0), ["mean"]),
        ((0, 0, 3), ["mean", p[0], own[0]]),
        ((0, 0, 8), [p[1], p[2], p[3], p[6], own[1]]),
        ((0, 1, 0), [fl("sum"), fl("max"), fl("argmin")]),
        ((0, 1, 3), [fl("min"), p[4]]),
        ((0, 1, 8), [fl("argmax"), "mean"] + p[5:11] + own),
        ((1, 0, 0), ["stddev"]),
        ((1, 1, 3), ["stddev", "mean", p[7], p[8], p[9]]),  # no flagged product: <true, false, 3> is not instantiated
        ((1, 0, 8), ["stddev", p[10], p[11], p[0], own[0]]),
        ((1, 1, 0), ["stddev", fl("sum")]),
        ((1, 1, 3), ["stddev", fl("max"), p[2], own[1]]),
        ((1, 1, 8), fifteen(klass, nlev)),
    ]


def _designs(nmem, klass):
    """The designed cells of row 0 of a reductions batch: name -> (level, column, member values).  Level 0: every member and
    every product flag SOME_DEFINED (a stored undef is a hole there, H); level 1: ALL_DEFINED (everything is a value)."""
    H, d, big, n = UNDEF, DENORM_MIN, FLT_MAX, nmem
    x = {"huge": _F(3.0e37), "tiny": _F(3.0e-42), "mid": _F(281.5)}[klass]

    def cell(head, fill, last=None):
        v = np.full(n, fill, np.float32)
        v[:len(head)] = head
        if last is not None:
            v[n - 1] = last
        return v

    return {
        "sum equals undef": (0, 0, cell([HALF_UNDEF, HALF_UNDEF], 0.0)),
        "mean equals undef": (0, 1, cell([TWICE_UNDEF, 0.0], H)),
        "inf then nan": (0, 2, cell([big, big, -INF], 0.0)),
        "cancels to x": (0, 3, cell([-big, big, x], 0.0)),
        "welford delta overflows": (0, 4, cell([-big, big], H)),
        "mean 3/2": (0, 5, cell([d, 2 * d], H)),
        "mean 5/2": (0, 6, cell([2 * d, 3 * d], H)),
        "mean 1/3": (0, 7, cell([d, 0.0, 0.0], H)),
        "-0 then +0": (0, 8, cell([-0.0, 0.0], H)),
        "+0 then -0": (0, 9, cell([0.0, -0.0], H)),
        "nan first, some": (0, 10, cell([NAN, 5.0, 7.0], H)),
        "undef first re-arms": (0, 11, cell([H, 3.0, 2.0, 4.0], H)),
        "limits": (0, 12, np.resize(np.array([0.0, -0.0, d, 2 * d, -d, big, -big, INF, -INF, NAN, UNDEF_BELOW, UNDEF_ABOVE, H], np.float32), n)),
        "nan first, all": (1, 0, cell([NAN, 5.0, 7.0], 1.0)),
        "undef is the running maximum": (1, 1, cell([1.0, H, 0.5], 0.25)),
        "undef is the last member": (1, 2, cell([1.0, 2.0], 1.5, last=H)),
        "maximum at the last member": (1, 3, cell([1.0], 1.0, last=9.0)),
        "maximum tied with member 0": (1, 4, cell([9.0], 1.0, last=9.0)),
        "limits, all": (1, 12, np.resize(np.array([0.0, -0.0, d, 2 * d, -d, big, -big, INF, -INF, NAN, UNDEF_BELOW, UNDEF_ABOVE, H], np.float32), n)),
    }


def reduction_marks(nmem, klass):
    """name -> (product name, level, column of row 0, the float32 the restatement must give there; NaN: any NaN)."""
    x = {"huge": _F(3.0e37), "tiny": _F(3.0e-42), "mid": _F(281.5)}[klass]
    last = _F(nmem - 1)
    limits = np.resize(np.arange(13), nmem)  # which of the thirteen values of the "limits" cells member j holds
    count = lambda *which: _F(np.isin(limits, which).sum())  # noqa: E731
    return {
        "sum equals undef: not a hole": ("sum", 0, 0, UNDEF),
        "mean equals undef: not a hole": ("mean", 0, 1, UNDEF),
        "FLT_MAX + FLT_MAX - inf": ("sum", 0, 2, NAN),
        "-FLT_MAX + FLT_MAX + x": ("sum", 0, 3, x),
        "Welford's delta overflows": ("stddev", 0, 4, NAN),
        "mean of 3 * 2^-149 over 2 rounds to even": ("mean", 0, 5, 2 * DENORM_MIN),
        "mean of 5 * 2^-149 over 2 rounds to even": ("mean", 0, 6, 2 * DENORM_MIN),
        "mean of 2^-149 over 3 rounds to zero": ("mean", 0, 7, _F(0.0)),
        "max of -0, +0 is the first": ("max", 0, 8, _F(-0.0)),
        "min of -0, +0 is the first": ("min", 0, 8, _F(-0.0)),
        "argmax of -0, +0 is the first": ("argmax", 0, 8, _F(0.0)),
        "argmin of -0, +0 is the first": ("argmin", 0, 8, _F(0.0)),
        "max of +0, -0 is the first": ("max", 0, 9, _F(0.0)),
        "min of +0, -0 is the first": ("min", 0, 9, _F(0.0)),
        "argmax of +0, -0 is the first": ("argmax", 0, 9, _F(0.0)),
        "argmin of +0, -0 is the first": ("argmin", 0, 9, _F(0.0)),
        "NaN as member 0 stays, SOME_DEFINED": ("max", 0, 10, NAN),
        "NaN as member 0 keeps index 0, SOME_DEFINED": ("argmin", 0, 10, _F(0.0)),
        "undef as member 0 is taken and re-arms: max": ("max", 0, 11, _F(4.0)),
        "undef as member 0 is taken and re-arms: argmin": ("argmin", 0, 11, _F(2.0)),
        "NaN as member 0 stays, ALL_DEFINED": ("min", 1, 0, NAN),
        "1e35 stored becomes the running maximum and re-arms": ("max", 1, 1, _F(0.5)),
        "1e35 stored as the last member is the maximum": ("max", 1, 2, UNDEF),
        "the maximum at member nmem - 1": ("argmax", 1, 3, last),
        "a maximum tied with member 0 keeps member 0": ("argmax", 1, 4, _F(0.0)),
        "a minimum everywhere tied keeps member 0": ("argmin", 1, 3, _F(0.0)),
        "above +0: -0 and +0 are not": ("probability 4 above FLT_MAX", 0, 12, count(7)),
        "between 0 and 2 * 2^-149: only 2^-149": ("probability 3 denormal", 0, 12, _F(np.float64(count(2)) / (nmem / 100.0))),
        "a stored undef of an ALL_DEFINED member is not counted": ("probability 1 above 0", 1, 12, _F(np.float64(count(2, 3, 5, 7, 10, 11)) / (nmem / 100.0))),
    }


# which product of full_list a mark's product name stands for
MARK_PRODUCTS = {"probability 4 above FLT_MAX": ("probability", 4, 0), "probability 3 denormal": ("probability", 3, 0), "probability 1 above 0": ("probability", 1, 0)}


def reduction_case(family, klass, nmem, ny, nx, products, nlev=3, undef=UNDEF, form=None, tag=""):
    label = "%s-%s-m%d-%dx%dx%d%s" % (family, klass, nmem, nlev, ny, nx, tag)
    data = "reductions-%s-m%d-%dx%dx%d-%r" % (klass, nmem, nlev, ny, nx, float(undef))  # single and levels share their batches
    x, flags = member_batch(data, klass, nmem, nlev, ny, nx, "reductions", undef)
    marks = {}
    if not np.isnan(undef) and nx >= 13 and nlev >= 2:
        for _, (lev, col, v) in _designs(nmem, klass).items():
            x[:, lev, 0, col] = v
        marks = reduction_marks(nmem, klass)
    return dict(family=family, klass=klass, label=label, members=x, flags=flags, undef=_F(undef), products=products, marks=marks, form=form or {})


# the grids: 12 x 20 the 16-byte form, 11 x 13 the scalar form of mifc_ensemble_levels (143 cells: 16-byte launch and scalar
# tail for a single-field entry), 9 x 21 = 189 cells = 47 lanes of four and one cell more
GRID16, GRID1, GRIDTAIL, GRIDTABLE = (12, 20), (11, 13), (9, 21), (6, 8)


@functools.lru_cache(maxsize=None)
def single_cases(klass):
    out = [reduction_case("single", klass, nmem, ny, nx, full_list(klass, 3), form=dict(c=4, tail=int(ny * nx % 4 != 0), inline=int(nmem <= 64)))
           for nmem, (ny, nx) in ((7, GRID16), (9, GRIDTAIL), (70, GRID1), (64, GRIDTAIL), (65, GRID16))]
    if klass == "mid":
        out.append(reduction_case("single", klass, 9, 12, 20, full_list(klass, 3, extremes=False), undef=NAN, tag="-nan-undef",
                                  form=dict(c=4, tail=0, inline=1)))
    return out


@functools.lru_cache(maxsize=None)
def levels_cases(klass):
    out = []

    def add(nmem, grid, lists, nlev=3, undef=UNDEF, tag=""):
        for k, (key, products) in enumerate(lists):
            c = 4 if grid[0] * grid[1] % 4 == 0 else 1
            w, f, np_ = key if c == 4 else (1, 1, 8)
            form = dict(entry="levels", c=c, welford=w, flagged=f, np=np_, inline=int(nmem <= 64 and nlev <= 64), launches=1, partials=0)
            out.append(reduction_case("levels", klass, nmem, grid[0], grid[1], products, nlev, undef, form, "%s-list%d" % (tag, k)))

    lists = instance_lists(klass, 3)
    add(7, GRID16, lists)
    add(9, GRID1, [lists[-1], lists[1], lists[7]])
    add(8, GRIDTAIL, [lists[-1]])
    add(64, GRID16, [lists[-1]])
    add(65, GRID16, [lists[-1], lists[5]])
    add(70, GRID1, [lists[-1]])
    add(70, GRID16, [lists[-1], lists[8]])
    add(8, GRIDTABLE, [((1, 1, 8), fifteen(klass, 65))], nlev=65, tag="-table")
    if klass == "mid":
        add(9, GRID16, [((1, 1, 8), [flagged("sum", 3), "mean", "stddev"] + probabilities()[:6]), ((1, 0, 0), ["stddev"])], undef=NAN, tag="-nan-undef")
    return out


# ================================================================================================= the quantiles
PERCENTILES = np.array([0.0, DENORM_MIN, 12.5, 30.0, 37.5, 50.0, 62.5, BELOW_100, 100.0], np.float32)
NEIGHBOUR_BASE = {"huge": _F(2.0e38), "tiny": _F(3.0e-42), "mid": _F(280.0)}


def _neighbours(klass, xor, negative):
    """Floats whose keys differ in their last two bits only: the key of the first ends in 00, min ^ max == xor (1, 2 or 3)."""
    b = NEIGHBOUR_BASE[klass].view(np.uint32) & np.uint32(0xFFFFFFFC)
    steps = {1: [0, 1], 2: [0, 2], 3: [0, 1, 2, 3]}[xor]
    v = np.array([b + np.uint32(s) for s in steps], np.uint32).view(np.float32)
    return -v if negative else v  # (the key of -v is ~bits: the same last two bits differ)


def quantile_designs(nmem, klass):
    """name -> (level, row, column, member values).  Level 0 (SOME_DEFINED: a stored undef is a hole, H) unless the name says all."""
    H, d, big, n = UNDEF, DENORM_MIN, FLT_MAX, nmem

    def of(values):
        return np.resize(np.asarray(values, np.float32), n)

    def few(values):
        v = np.full(n, H, np.float32)
        v[:len(values)] = values
        return v

    out = {}
    col = 0
    for negative in (False, True):
        for xor in (1, 2, 3):
            out["neighbours %s xor %d" % ("negative" if negative else "positive", xor)] = (0, 0, col, of(_neighbours(klass, xor, negative)))
            col += 1
    out["-0 and +0"] = (0, 0, 6, of([-0.0, 0.0]))
    out["around zero"] = (0, 0, 7, of([-d, -0.0, 0.0, d]))
    out["-FLT_MAX and FLT_MAX"] = (0, 0, 8, of([-big, big]))
    out["FLT_MAX and +inf"] = (0, 0, 9, of([big, INF]))
    out["-inf and +inf"] = (0, 0, 10, of([-INF, INF]))
    out["2^-149 and twice"] = (0, 0, 11, few([d, 2 * d]))
    out["no member counts"] = (0, 0, 12, few([]))
    out["one member counts"] = (0, 1, 0, few([NEIGHBOUR_BASE[klass]]))
    out["NaN at the top ranks, all"] = (1, 0, 0, of([NAN, NEG_NAN, 1.0, -1.0, 2.0]))
    out["1e35 counted, all"] = (1, 0, 1, of([H, 3.0e37, -3.0e37, 2.0e36]))
    return out


def quantile_case(klass, nmem, ny, nx, method, nlev=3, undef=UNDEF, tag=""):
    label = "quantiles-%s-m%d-%dx%dx%d-%s%s" % (klass, nmem, nlev, ny, nx, method, tag)
    data = "quantiles-%s-m%d-%dx%dx%d-%r" % (klass, nmem, nlev, ny, nx, float(undef))  # both methods on one batch
    x, flags = member_batch(data, klass, nmem, nlev, ny, nx, "quantiles", undef)
    flags = np.where(flags == NONE_DEFINED, SOME_DEFINED, flags).astype(np.int32)  # (the entry knows no NONE_DEFINED: as SOME_DEFINED)
    marks = {}
    if not np.isnan(undef) and nx >= 13:
        marks = quantile_designs(nmem, klass)
        for _, (lev, row, col, v) in marks.items():
            x[:, lev, row, col] = v
    form = dict(entry="quantiles", tier=sort_tier(nmem), inline=int(nmem <= 64 and nlev <= 64), launches=1, partials=0)
    return dict(family="quantiles", klass=klass, label=label, members=x, flags=flags, undef=_F(undef), percentiles=PERCENTILES, method=method,
                marks=marks, form=form)


def sort_tier(nmem):
    """quantile_tier of csrc/mifc_kernels.h: the capacity of the sorting network, 0 for the bisection."""
    return 8 if nmem <= 8 else 16 if nmem <= 16 else 32 if nmem <= 32 else 64 if nmem <= 64 else 0


@functools.lru_cache(maxsize=None)
def quantiles_cases(klass):
    out = []
    for nmem in MEMBER_COUNTS:
        grid = GRID1 if nmem in (9, 33) else GRID16
        for method in ("lower", "linear"):
            out.append(quantile_case(klass, nmem, grid[0], grid[1], method))
    for method in ("lower", "linear"):
        out.append(quantile_case(klass, 9, GRIDTABLE[0], GRIDTABLE[1], method, nlev=65, tag="-table"))
    if klass == "mid":
        out.append(quantile_case(klass, 9, 12, 20, "linear", undef=NAN, tag="-nan-undef"))
    return out


# ====================================================================================================== all families
def cases(family, klass):
    return {"single": single_cases, "levels": levels_cases, "quantiles": quantiles_cases}[family](klass)


def restate(case, mistakes=(), ranks=None):
    """single, levels: [(out (nlev, ny, nx), flags (nlev,))] per product; quantiles: (out (nq, nlev, ny, nx), flags (nlev,))."""
    if case["family"] == "quantiles":
        out, fd = qr.quantiles(case["members"], case["percentiles"], qr.LINEAR if case["method"] == "linear" else qr.LOWER, case["flags"], case["undef"],
                               mistakes=mistakes, ranks=ranks)
        return out, np.asarray(fd, np.int32)
    return er.statistics(case["members"], case["flags"], case["products"], case["undef"], mistakes=mistakes)


_EXPECTED = {}


def expected(case):
    """restate(case), computed once per label and read-only."""
    if case["label"] not in _EXPECTED:
        res = restate(case)
        for a in (res if case["family"] == "quantiles" else [a for pair in res for a in pair]):
            a.setflags(write=False)
        _EXPECTED[case["label"]] = res
    return _EXPECTED[case["label"]]


def widened(case, times):
    """The case with its grid repeated `times` along y, so that a host call stages it in more than one chunk.  The expected
    result is restated like every other."""
    return dict(case, label="%s-rows-x%d" % (case["label"], times), members=np.tile(case["members"], (1, 1, times, 1)), marks={})
