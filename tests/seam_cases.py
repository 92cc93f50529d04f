"""Seam cases for the pointwise catalogue and the elementwise thermodynamics: inputs placed ON the values at which the
device arithmetic changes its path -- table knots, class limits, `>=` thresholds, the switch between the two log series,
table-interval edges, the fast/slow switches of exp2_tab and pow_kappa -- and one or two float32 neighbours either side.
tests/cases.py draws uniform random fields, which land on none of these.

Same case-dict format as tests/cases.py.  Every case is one row (ny = 1) and comes in two lengths, a multiple of 4 (the
16-byte body of the pointwise kernel) and a multiple of 4 plus 3 in reversed order (seam values in the scalar tail too),
each under ALL_DEFINED and under SOME_DEFINED with a handful of undefined cells among the seams.

ModStall / MINCOG have tests/icing_cases.py; the stencils have no seams of this kind.  Pure numpy; nothing here needs a GPU.
"""
import itertools

import numpy as np

from cases import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
T0 = F(273.15)  # MetConstants.h:44
P0INV = F(1.0 / 1000.0)
KAPPA = F(287.0) / F(1004.0)  # float division, as the project's kappa
EPS = F(0.622)
# MetConstants.h:57-59, rounded to float as the reference stores it
EWT = np.array([.000034, .000089, .000220, .000517, .001155, .002472, .005080, .01005, .01921, .03553, .06356, .1111, .1891, .3139, .5088, .8070, 1.2540,
                1.9118, 2.8627, 4.2148, 6.1078, 8.7192, 12.272, 17.044, 23.373, 31.671, 42.430, 56.236, 73.777, 95.855, 123.40, 157.46, 199.26, 250.16,
                311.69, 385.56, 473.67, 578.09, 701.13, 845.28, 1013.25], np.float64).astype(F)
PLEVELTABLE = np.array([1000, 925, 850, 800, 700, 500, 400, 300, 250, 200, 150, 100, 70, 50, 30, 10], F)  # MetConstants.h:88-90
FLEVELTABLE = np.array([5, 25, 50, 65, 100, 185, 235, 300, 340, 385, 445, 530, 605, 675, 780, 1020], F)
CLASS_LIMITS = ([-40.0, -10.0, 0.0, 5.0, 20.0, 45.0], [-40.0, 45.0])  # the two tables of cases.catalogue_cases
MERTINS_CLASSES = (0.0, 0.8333, 2.0833, 4.375, 6.25)
POWER_EXPONENTS = (0.37, 2.0, -1.5, 0.5, 0.0, 1.0)
LIBM_OPS = ("logField", "log10Field", "expField", "pow10Field", "powerField")


def around(v, k=2):
    """v (as float32) and its k float32 neighbours on each side, ascending."""
    v = F(v)
    out, lo, hi = [v], v, v
    with np.errstate(over="ignore"):  # the neighbour above FLT_MAX is +inf
        for _ in range(k):
            lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
            out = [lo] + out + [hi]
    return np.array(out, F)


def cat(*parts):
    return np.concatenate([np.atleast_1d(np.asarray(p, F)).ravel() for p in parts]).astype(F)


def fill(n, *values):
    """n cells cycling through values."""
    return np.resize(np.asarray(values, F), n).astype(F)


def from_bits(b):
    return np.asarray(b, np.int64).astype(np.uint32).view(F)


# ---- float32 restatements of the lookups, for the searches and the coverage checks (the judges are the oracle and float64)
def ewt_x(tc):
    """x of MetConstants.h:65 for a float32 Celsius temperature."""
    return ((np.asarray(tc, F).astype(np.float64) + 100.0) * 0.2).astype(F)


def ewt_x_of_kelvin(tk):
    return ewt_x(np.asarray(tk, F) - T0)


def ewt_value(x):
    """e(T) for x inside the table, in float32 as the reference evaluates it."""
    x = np.asarray(x, F)
    l = np.clip(x.astype(np.int64), 0, 39)
    return (EWT[l] + (EWT[l + 1] - EWT[l]) * (x - l.astype(F))).astype(F)


def rh_fraction(rh100):
    """clamp_rh((float)(0.01 * rh)), FieldCalculations.cc:186-194."""
    r = (0.01 * np.asarray(rh100, F).astype(np.float64)).astype(F)
    return np.clip(r, F(0.02), F(1.0)).astype(F)


def knot_kelvin(k):
    """The Kelvin temperature whose x is exactly the integer k (tk - 273.15f is a rounded float subtraction, so this is a search)."""
    tc = F(5.0 * k - 100.0)
    guess = F(np.float64(tc) + np.float64(T0))
    for cand in around(guess, 8):
        if F(cand - T0) == tc and ewt_x(F(cand - T0)) == F(k):
            return cand
    raise AssertionError("no float32 Kelvin temperature reaches knot %d exactly" % k)


KNOTS = range(0, 41)
VALIDITY_ENDS = (-1, 40)  # ok() <=> -1 < x < 40


def table_kelvin():
    """Kelvin temperatures on every knot and both validity ends, two floats either side, then the special values."""
    parts = [around(knot_kelvin(k), 2) for k in range(-1, 41)]
    t = cat(*parts, [250.0, 288.3, 150.0, 400.0], [NAN, INF, -INF, 0.0, -0.0])
    x = ewt_x_of_kelvin(t)
    for k in range(-1, 41):
        assert np.any(x == F(k)) and np.any((x < F(k)) & (x > F(k - 1))) and np.any((x > F(k)) & (x < F(k + 1))), k
    return t


# ---- case plumbing
def _undef_positions(n, k):
    """A handful of cells, different for each field k of a case."""
    return sorted({(3 + 5 * k) % n, (n // 3 + k) % n, (n // 2 + 2 * k + 1) % n, (n - 2 - k) % n})


def variants(op, fields, make_args, tag, modes=(ALL_DEFINED, SOME_DEFINED)):
    """fields: equally long 1-D float32 arrays; make_args(fields) -> the case's args.  Returns the four cases."""
    n0 = len(fields[0])
    assert all(len(f) == n0 for f in fields), (op, tag, [len(f) for f in fields])
    n4 = (n0 + 3) // 4 * 4
    out = []
    for length, name in ((n4, "body"), (n4 + 3, "tail")):
        fs = [np.resize(f, length).astype(F) for f in fields]
        if name == "tail":
            fs = [f[::-1].copy() for f in fs]
        for mode in modes:
            gs = fs
            if mode == SOME_DEFINED:
                gs = []
                for k, f in enumerate(fs):
                    g = f.copy()
                    g[_undef_positions(length, k)] = UNDEF
                    gs.append(g)
            out.append(dict(op=op, nx=length, ny=1, args=make_args([g.reshape(1, length) for g in gs]), fdefined=mode, undef=UNDEF,
                            label="seam-%s%s-%s-%s" % (op, tag, name, "all" if mode == ALL_DEFINED else "some")))
    return out


# ---- saturation-pressure table: every operator that looks e(T) up, temperature taken directly (no power in front)
def table_cases():
    t = table_kelvin()
    n = len(t)
    tc = (t - T0).astype(F)
    rh = fill(n, 60.0, 100.0, 2.0, 35.5, 101.0, 0.5)
    q = fill(n, 0.003, 0.0001, 0.02)
    ps = fill(n, 1000.0, 850.0, 1013.25)
    p3 = fill(n, 850.0, 500.0, 300.0, 1000.0)
    mid = fill(n, 262.0, 255.5, 281.25)
    cs = []
    for c in (4,):  # t_thesat
        cs += variants("pleveltemp", [t], lambda f, c=c: [f[0], 850.0, "", c], str(c))
        cs += variants("hleveltemp", [t, ps], lambda f, c=c: [f[0], f[1], 12.5, 0.73, "", c], str(c))
        cs += variants("aleveltemp", [t, p3], lambda f, c=c: [f[0], f[1], "", c], str(c))
    for c in (1, 3, 5, 7, 9, 11):
        hp = q if c in (1, 7, 11) else rh
        cs += variants("plevelhum", [t, hp], lambda f, c=c: [f[0], f[1], 700.0, "", c], str(c))
        ha = q if c in (1, 5, 9) else rh
        cs += variants("hlevelhum", [t, ha, ps], lambda f, c=c: [f[0], f[1], f[2], 12.5, 0.73, "", c], str(c))
        cs += variants("alevelhum", [t, ha, p3], lambda f, c=c: [f[0], f[1], f[2], "", c], str(c))
    cs += variants("cvhum", [t, rh], lambda f: [f[0], f[1], "kelvin", 1], "1")
    cs += variants("cvhum", [t, rh], lambda f: [f[0], f[1], "", 2], "2")
    cs += variants("cvhum", [tc, rh], lambda f: [f[0], f[1], "", 3], "3")
    cs += variants("cvhum", [t, np.roll(t, 7)], lambda f: [f[0], f[1], "", 4], "4")
    cs += variants("cvhum", [np.roll(tc, 7), tc], lambda f: [f[0], f[1], "1", 5], "5")
    cs += variants("plevelthe", [t, rh], lambda f: [f[0], f[1], 850.0, 1], "1")
    for c in (3, 4, 5):
        cs += variants("plevelducting", [t, rh], lambda f, c=c: [f[0], f[1], 925.0, c], str(c))
    cs += variants("hlevelducting", [t, rh, ps], lambda f: [f[0], f[1], f[2], 12.5, 0.73, 3], "3")
    cs += variants("alevelducting", [t, rh, p3], lambda f: [f[0], f[1], f[2], 3], "3")
    cs += variants("kIndex", [mid, mid, rh, t, rh], lambda f: [f[0], f[1], f[2], f[3], f[4], 500.0, 700.0, 850.0, 1], "1-t850")
    cs += variants("kIndex", [mid, t, rh, mid, rh], lambda f: [f[0], f[1], f[2], f[3], f[4], 500.0, 700.0, 850.0, 1], "1-t700")
    cs += variants("ductingIndex", [t, rh], lambda f: [f[0], f[1], 850.0, 1], "1")
    cs += variants("showalterIndex", [mid, t, rh], lambda f: [f[0], f[1], f[2], 500.0, 850.0, 1], "1")
    return cs


# ---- inverse lookup: e == a table entry, one float either side, the clamp ends of the humidity, the powers of two
def _search_rh(l, target):
    """(tk, rh %) near knot l for which rh * e(tk) is target exactly, the float below it and the float above it.  The product
    of two floats does not reach every float, so several temperatures in bin l (each with its own e) are tried."""
    want = {np.nextafter(target, -INF): None, target: None, np.nextafter(target, INF): None}
    temps = [knot_kelvin(l)] + [t for t in around(knot_kelvin(l), 6) if F(l) < ewt_x_of_kelvin(t) < F(l + 1)]
    for tk in temps:
        et = ewt_value(ewt_x_of_kelvin(tk))
        guess = F(100.0 * np.float64(target) / np.float64(et))
        for cand in around(guess, 24):
            etd = F(rh_fraction(cand) * et)
            if etd in want and want[etd] is None:
                want[etd] = (tk, cand)
        if all(v is not None for v in want.values()):
            break
    return want


def inverse_pairs():
    """(tk, rh%) pairs, with the bookkeeping of what they reach: {"entry": {m: hits}, "power": {b: hits}}."""
    tk, rh = [], []
    reached = {"entry": {}, "power": {}}
    for l in range(0, 41):  # saturation at every knot: et == ewt[l] and the walk must not move
        tk.append(knot_kelvin(l))
        rh.append(F(100.0))
    for l in range(1, 40):
        for m in range(l - 1, max(l - 5, -1), -1):
            if np.float64(EWT[m]) / np.float64(EWT[l]) < 0.021:
                break
            for etd, cand in _search_rh(l, EWT[m]).items():
                if cand is not None:
                    tk.append(cand[0])
                    rh.append(cand[1])
                    reached["entry"].setdefault(m, set()).add(int(np.sign(np.float64(etd) - np.float64(EWT[m]))))
    for b in range(-14, 10):  # 2^b inside the table's range: the bin search starts from the binary exponent
        power = F(2.0) ** F(b)
        ls = [l for l in range(1, 40) if EWT[l] > power and np.float64(power) / np.float64(EWT[l]) > 0.021]
        for l in ls[:2]:
            for etd, cand in _search_rh(l, power).items():
                if cand is not None:
                    tk.append(cand[0])
                    rh.append(cand[1])
                    reached["power"].setdefault(b, set()).add(int(np.sign(np.float64(etd) - np.float64(power))))
    for t in (knot_kelvin(20), knot_kelvin(3), knot_kelvin(39), F(288.3), F(251.7)):  # clamp_rh ends
        for r in cat(around(2.0, 2), around(100.0, 2), [0.0, -5.0, 150.0, INF, -INF, NAN]):
            tk.append(t)
            rh.append(r)
    return np.array(tk, F), np.array(rh, F), reached


def inverse_cases():
    tk, rh, reached = inverse_pairs()
    for m in range(0, 39):
        assert reached["entry"].get(m) == {-1, 0, 1}, ("table entry %d is not reached exactly and from both sides" % m, reached["entry"].get(m))
    for b in range(-14, 10):
        assert reached["power"].get(b) == {-1, 0, 1}, ("2^%d is not reached exactly and from both sides" % b, reached["power"].get(b))
    n = len(tk)
    tc = (tk - T0).astype(F)
    ps = fill(n, 1000.0, 850.0)
    p3 = fill(n, 850.0, 500.0)
    mid = fill(n, 262.0, 255.5, 281.25)
    cs = []
    for c in (5, 9):
        cs += variants("plevelhum", [tk, rh], lambda f, c=c: [f[0], f[1], 700.0, "", c], "%d-inverse" % c)
    cs += variants("hlevelhum", [tk, rh, ps], lambda f: [f[0], f[1], f[2], 12.5, 0.73, "", 7], "7-inverse")
    cs += variants("alevelhum", [tk, rh, p3], lambda f: [f[0], f[1], f[2], "", 11], "11-inverse")
    cs += variants("cvhum", [tk, rh], lambda f: [f[0], f[1], "kelvin", 1], "1-inverse")
    cs += variants("cvhum", [tc, rh], lambda f: [f[0], f[1], "", 3], "3-inverse")
    cs += variants("kIndex", [mid, mid, fill(n, 40.0), tk, rh], lambda f: [f[0], f[1], f[2], f[3], f[4], 500.0, 700.0, 850.0, 1], "1-inverse850")
    cs += variants("kIndex", [mid, tk, rh, mid, fill(n, 40.0)], lambda f: [f[0], f[1], f[2], f[3], f[4], 500.0, 700.0, 850.0, 1], "1-inverse700")
    cs += variants("ductingIndex", [tk, rh], lambda f: [f[0], f[1], 850.0, 1], "1-inverse")
    # q -> Td: q == qsat makes the relative humidity exactly 1 and e exactly the knot's entry
    knots = np.array([knot_kelvin(l) for l in range(0, 40)], F)
    p = F(700.0)
    qsat = (EPS * EWT[:40] / p).astype(F)
    tq = np.repeat(knots, 5)
    qq = cat(*[around(v, 2) for v in qsat])
    cs += variants("plevelhum", [tq, qq], lambda f: [f[0], f[1], 700.0, "", 7], "7-saturated")
    cs += variants("alevelhum", [tq, qq, fill(len(tq), 700.0)], lambda f: [f[0], f[1], f[2], "", 5], "5-saturated")
    return cs


# ---- pressure2FlightLevel: the select chain
def flight_level_pressures():
    return cat(*[around(p, 2) for p in PLEVELTABLE], [1000.5, 1100.0, 2000.0, 3.0e38, 9.5, 5.0, 1.0, 1e-45, 0.0, -0.0, -5.0, INF, -INF, NAN, 612.5])


def flight_level_cases():
    return variants("pressure2FlightLevel", [flight_level_pressures()], lambda f: [f[0]], "")


# ---- values2classes: limits and the half-open range
def class_values(limits):
    return cat(*[around(v, 2) for v in limits], [-100.0, 100.0, 2.5, -0.0, 1e-45, -1e-45, NAN, INF, -INF])


def classes_cases():
    cs = []
    for limits, tag in zip(CLASS_LIMITS, ("-six", "-two")):
        cs += variants("values2classes", [class_values(limits)], lambda f, limits=limits: [f[0], list(limits)], tag)
    return cs


# ---- underCooledRain: precip >= precipMin, tk <= tkMax, snow <= precip * snowRateMax
UCR = dict(precipMin=0.5, snowRateMax=0.3, tcMax=1.0)


def undercooled_fields():
    tk_max = F(F(UCR["tcMax"]) + T0)
    precip, snow, tk = [], [], []
    for p, t in itertools.product(cat(around(UCR["precipMin"], 2), [2.0]), cat(around(tk_max, 2), [270.0])):
        for s in cat(around(F(p * F(UCR["snowRateMax"])), 2), [0.0]):
            precip.append(p)
            snow.append(s)
            tk.append(t)
    return np.array(precip, F), np.array(snow, F), np.array(tk, F)


def undercooled_cases():
    return variants("underCooledRain", list(undercooled_fields()), lambda f: [f[0], f[1], f[2], UCR["precipMin"], UCR["snowRateMax"], UCR["tcMax"]], "")


# ---- vesselIcingOverland / vesselIcingMertins: the ice-cover and freezing-point gates, the class ladder
def _freezing_point(sal):
    s = F(sal)
    return (-0.002 - 0.0524 * np.float64(s)) - 6.0e-5 * np.float64(F(s * s))


def _mertins_temps(ff, sst):
    sst = np.float64(F(sst))
    if ff < 17.2:
        return (-1.15 * sst - 4.3, -1.5 * sst - 10)
    if ff < 20.8:
        return (-0.6 * sst - 3.2, -1.05 * sst - 5.6, -1.75 * sst - 12.5)
    if ff < 28.5:
        return (-0.3 * sst - 2.6, -0.66 * sst - 3.32, -1.325 * sst - 7.651)
    return (-0.14 * sst - 2.28, -0.3 * sst - 2.6, -1.16 * sst - 5.22)


def icing_fields():
    rows = []  # airtemp, seatemp, u, v, sal, aice

    def add(air=-10.0, sst=2.0, u=15.0, v=0.0, sal=35.0, ice=0.1):
        rows.append((air, sst, u, v, sal, ice))

    for ice in cat(around(0.4, 2), [0.0, 0.39, 0.41, 1.0, -0.0, NAN]):  # the compare is in double: 0.4f > 0.4
        add(ice=ice)
    for sal in (5.0, 20.0, 35.0):
        for sst in cat(around(F(_freezing_point(sal)), 2), [-3.0]):
            add(sst=sst, sal=sal)
    for w in (10.8, 17.2, 20.8, 28.5):
        for u in around(w, 2):
            for air in (-1.0, -3.0, -6.0, -12.0, -25.0):
                add(air=air, u=u)
                add(air=air, u=0.0, v=-u)
    for w in (12.0, 18.0, 25.0, 30.0):
        for sst in (-1.0, 2.0, 6.0):
            temps = [-2.0] + [float(F(t)) for t in _mertins_temps(w, sst)]
            for t in temps:
                for air in around(t, 2):
                    add(air=air, sst=sst, u=w)
    return [np.array(col, F) for col in zip(*rows)]


def icing_cases(oracle=None):
    fields = icing_fields()
    cs = []
    for op in ("vesselIcingOverland", "vesselIcingMertins"):
        cs += variants(op, fields, lambda f: list(f), "")
    if oracle is not None:
        import cases as _cases

        ok, out, _ = _cases.run_cpu(oracle, [c for c in cs if c["op"] == "vesselIcingMertins"][0])
        assert ok and all(np.any(out == F(v)) for v in MERTINS_CLASSES), "a Mertins class does not occur"
    return cs


# ---- small branches
def _snow_fac(t):
    t = np.float64(F(t))
    ex = np.exp((t - 274.3) * 3.5)
    return F(F((1 - ex) / (1 + ex)) * F(0.13 / (0.02 + 0.1 * ((t - 252.0) / 20.0) * ((t - 252.0) / 20.0))))


def snow_fields():
    # fac(t) <= 1 keeps the water equivalent, above it multiplies: the two temperatures at which fac crosses 1
    grid = np.arange(200.0, 280.0, 1.0 / 64.0).astype(F)  # exact in float32
    fac = np.array([_snow_fac(t) for t in grid], F)
    cross = np.nonzero((fac[:-1] <= 1) != (fac[1:] <= 1))[0]
    assert len(cross) == 2, cross
    ts = cat(*[np.linspace(grid[i], grid[i + 1], 33).astype(F) for i in cross], [252.0, 274.3, 260.0, 300.0, 150.0, 1000.0])
    water, t2, td = [], [], []
    for w in cat(around(0.0, 2), [-1.0, -0.0, 5.0, 1e-38]):
        for t in (252.0, 274.3, 285.0):
            water.append(w), t2.append(t), td.append(t)
    for t in ts:
        water.append(3.0), t2.append(t), td.append(t)
    return np.array(water, F), np.array(t2, F), np.array(td, F)


def windcooling_fields(celsius):
    t, u, v = [], [], []
    for uu, vv in ((0.0, 0.0), (-0.0, 0.0), (1e-45, 0.0), (1e-20, 1e-20), (0.3, 0.4), (3.0, -4.0), (20.0, 0.0), (0.0, 1.5), (1e19, 1e19), (INF, 0.0)):
        ff = np.float64(F(np.float64(np.sqrt(F(F(uu) * F(uu) + F(vv) * F(vv)))) * 3.6))
        fp = ff ** 0.16 if np.isfinite(ff) else 1.0
        zero = (11.37 * fp - 13.12) / (0.6215 + 0.3965 * fp)  # d(tc) == 0
        for tc in cat(around(F(zero), 3), [-30.0, 0.0, 25.0]):
            t.append(tc if celsius else F(tc + T0)), u.append(uu), v.append(vv)
    return np.array(t, F), np.array(u, F), np.array(v, F)


SPECIALS = cat([0.0, -0.0, 1.0, -1.0, 3.5, NAN, INF, -INF, 1e-45, -1e-45])


def branch_cases():
    cs = variants("snow_in_cm", list(snow_fields()), lambda f: [f[0], f[1], f[2]], "")
    cs += variants("windCooling", list(windcooling_fields(False)), lambda f: [f[0], f[1], f[2], 1], "1")
    cs += variants("windCooling", list(windcooling_fields(True)), lambda f: [f[0], f[1], f[2], 2], "2")
    # division: zero divisors of either sign, the smallest subnormal, the ends of the normal range
    den = cat([0.0, -0.0, 1e-45, -1e-45], around(1.17549435e-38, 1), [1.0, -3.0, 3.0e38, INF, NAN])
    num = cat([1.0, 0.0, -0.0, -7.5, 1e-45, 3.0e38, INF, NAN])
    a, b = (np.array(x, F) for x in zip(*itertools.product(num, den)))
    for c in (1, 2, 3, 4):
        cs += variants("fieldOPERfield", [a, b], lambda f, c=c: [c, f[0], f[1]], str(c))
    for val in (2.5, 0.0, -0.0, 1e-45, 3.0e38):
        cs += variants("constantOPERfield", [den], lambda f, val=val: [4, val, f[0]], "4-%g" % val)
        cs += variants("fieldOPERconstant", [num], lambda f, val=val: [4, f[0], val], "4-%g" % val)
    # min / max: equal operands, zeros of either sign, NaN in either place
    a, b = (np.array(x, F) for x in zip(*itertools.product(SPECIALS, SPECIALS)))
    cs += variants("minvalueFields", [a, b], lambda f: [f[0], f[1]], "")
    cs += variants("maxvalueFields", [a, b], lambda f: [f[0], f[1]], "")
    for val in (0.0, -0.0, 3.5, float(INF)):
        cs += variants("minvalueFieldConst", [SPECIALS], lambda f, val=val: [f[0], val], "-%g" % val)
        cs += variants("maxvalueFieldConst", [SPECIALS], lambda f, val=val: [f[0], val], "-%g" % val)
    # replace*: the flag is an input, and so is a constant that equals undef
    field = cat(SPECIALS, [UNDEF, 2.0, UNDEF, np.nextafter(UNDEF, INF), np.nextafter(UNDEF, -INF)])
    for val, flag in itertools.product((float(UNDEF), -1.0, 0.0), (ALL_DEFINED, NONE_DEFINED, SOME_DEFINED)):
        cs += variants("replaceUndefined", [field], lambda f, val=val: [f[0], val], "-%g-flag%d" % (val, flag), modes=(flag,))
        cs += variants("replaceDefined", [field], lambda f, val=val: [f[0], val], "-%g-flag%d" % (val, flag), modes=(flag,))
    return cs


# ---- the libm class: logField / log10Field, expField / pow10Field, powerField
LOG_EDGE0 = 0x3f3504f3  # bits of sqrt(1/2) rounded up: where log2_tab's first interval starts


def log_arguments():
    rng = np.random.default_rng(20240607)
    edges = [LOG_EDGE0 + (i << 19) + (de << 23) + d for de in (-100, -20, -1, 0, 1, 30, 100) for i in range(17) for d in (-1, 0, 1)]
    return cat(around(1.0 - 1.0 / 32.0, 3), around(1.0 + 1.0 / 32.0, 3), around(1.0, 3), from_bits(edges),
               around(1.17549435e-38, 3), around(3.40282347e38, 3), [1e-45, 1e-40, 5.9e-39, 0.0, -0.0, -1.0, -1e-45, -INF, INF, NAN],
               from_bits(rng.integers(0x00800000, 0x7f800000, 3000)))  # log-uniform over the normal floats


def exp_arguments(base10):
    rng = np.random.default_rng(20240608 + int(base10))
    per_t = np.log10(2.0) if base10 else np.log(2.0)  # argument per unit of t = log2 of the result
    # 32 t an integer or a half-integer (the rint seam of exp2_tab), t from -150 to 128
    seam = cat(*[around(F(n / 64.0 * per_t), 1) for n in range(-9600, 8200, 37)])
    ends = [128.0, -126.0, -149.0, -150.0, 1000.0, -1000.0]  # overflow, smallest normal, smallest subnormal, rounds to zero, fast/slow switch
    lo, hi = (-46.0, 39.0) if base10 else (-104.0, 89.0)
    return cat(seam, *[around(F(t * per_t), 3) for t in ends], [0.0, -0.0, INF, -INF, NAN, 1e-45, -1e-45, 3.0e38, -3.0e38],
               rng.uniform(lo, hi, 1500))


def power_pairs_near_switch():
    """(base, exponent) with t = exponent * log2(base) around +-1000."""
    out = []
    for b, lg in ((8.0, 125.0), (8.0, -125.0), (-8.0, 125.0), (-8.0, -125.0), (10.0, 100.0), (-10.0, 100.0), (12.5, -80.0)):
        out.append((b, cat(around(F(2.0) ** F(lg), 3), around(F(2.0) ** F(lg * 0.999), 1), around(F(2.0) ** F(lg * 1.001), 1))))
    return out


def libm_cases():
    x = log_arguments()
    cs = variants("logField", [x], lambda f: [f[0]], "")
    cs += variants("log10Field", [x], lambda f: [f[0]], "")
    cs += variants("expField", [exp_arguments(False)], lambda f: [f[0]], "")
    cs += variants("pow10Field", [exp_arguments(True)], lambda f: [f[0]], "")
    for e in POWER_EXPONENTS:
        cs += variants("powerField", [x], lambda f, e=e: [f[0], e], "-%g" % e)
    for e, bases in power_pairs_near_switch():
        cs += variants("powerField", [bases], lambda f, e=e: [f[0], e], "-switch%g-%d" % (e, int(np.log2(np.float64(bases[3])))))
    return cs


# ---- pow_kappa: the 256 mantissa intervals, the ends of its fast domain, the rare path
def _pressures_reaching(x_target):
    """Pressures p with float32(p * p0inv) within two floats of x_target, by their distance from it in floats."""
    got = {}
    for cand in around(F(np.float64(x_target) / np.float64(P0INV)), 4):
        d = int(np.int64(F(cand * P0INV).view(np.uint32)) - np.int64(F(x_target).view(np.uint32)))
        if abs(d) <= 2 and d not in got:
            got[d] = cand
    return got


def kappa_edge_pressures(exponents=(-1, 0, -10)):
    """p * p0inv on the first float of each of the 256 mantissa intervals and the floats around it.  p -> float32(p * p0inv)
    skips about one float in 40 (the spacing of p * 0.001 is 1.024 spacings of the product) and the skipped patterns are the
    same at every exponent, so an edge itself may be out of reach: then the nearest floats on both sides stand for it -- what
    matters to the lookup is that the last floats of interval i - 1 and the first of interval i are both computed."""
    ps, reached = [], {}
    for e in exponents:
        for i in range(256):
            x = from_bits([((127 + e) << 23) | (i << 15)])[0]
            for d, p in _pressures_reaching(x).items():
                ps.append(p)
                reached.setdefault(i, set()).add(d)
    for i in range(256):
        assert reached[i] & {-2, -1} and reached[i] & {0, 1}, ("mantissa-interval edge %d is not approached from both sides" % i, reached.get(i))
    assert sum(1 for i in range(256) if 0 in reached[i]) >= 240
    return np.array(ps, F)


def kappa_rare_pressures():
    two = np.float64(2.0)
    parts = [around(F(two ** b * 1000.0), 3) for b in (-32, 32, -96, 96)]  # ends of the fast domain; the second rescaling of the rare path
    return cat(*parts, [1e-5, 1e-8, 1e-20, 1e-30, 1e-36, 1.2e-35, 1e-38, 1e-42, 1e-45, 1e13, 1e20, 1e30, 3.0e38, 0.0, -0.0, -1.0, -850.0, -1e-45, INF, -INF, NAN])


def kappa_cases():
    """aleveltemp, theta in kelvin out, with theta == 1.0f: the output IS pow_kappa(p * p0inv)."""
    p = cat(kappa_edge_pressures(), kappa_rare_pressures(), [1000.0, 850.0, 500.0, 1013.25, 150.0, 1040.0])
    return variants("aleveltemp", [np.ones(len(p), F), p], lambda f: [f[0], f[1], "kelvin", 2], "-bare-power")


def composite_fields():
    """theta, humidity fields and pressures for the operators that chain the power through the table."""
    p_edges = kappa_edge_pressures(exponents=(-1, 0))  # 500 .. 2000 hPa
    p_edges = p_edges[p_edges < 1100.0][::3]
    p = cat(p_edges, kappa_rare_pressures())
    theta = fill(len(p), 300.0, 285.5, 320.25)
    # temperatures at the table's validity ends: theta chosen so that theta * (p / p0)^kappa is the end, a few floats either side
    for pe in (500.0, 850.0):
        pw = np.float64(F(F(pe) * P0INV)) ** np.float64(KAPPA)
        for k in VALIDITY_ENDS + (0, 20):
            th = around(F(np.float64(knot_kelvin(k)) / pw), 3)
            theta, p = cat(theta, th), cat(p, fill(len(th), pe))
    n = len(p)
    return theta, p, fill(n, 60.0, 100.0, 2.0, 35.5), fill(n, 0.003, 0.0001, 0.02)


def composite_cases():
    th, p, rh, q = composite_fields()
    cs = []
    for c in (1, 2, 3, 5):
        cs += variants("hleveltemp", [th, p], lambda f, c=c: [f[0], f[1], 0.0, 1.0, "", c], "%d-theta" % c)
        cs += variants("aleveltemp", [th, p], lambda f, c=c: [f[0], f[1], "", c], "%d-theta" % c)
    for c in (2, 4, 6, 8):
        h = q if c in (2, 6) else rh
        cs += variants("hlevelhum", [th, h, p], lambda f, c=c: [f[0], f[1], f[2], 0.0, 1.0, "", c], "%d-theta" % c)
        cs += variants("alevelhum", [th, h, p], lambda f, c=c: [f[0], f[1], f[2], "", c], "%d-theta" % c)
    for c in (1, 2):
        cs += variants("hlevelthe", [th, q, p], lambda f, c=c: [f[0], f[1], f[2], 0.0, 1.0, c], "%d-theta" % c)
        cs += variants("alevelthe", [th, q, p], lambda f, c=c: [f[0], f[1], f[2], c], "%d-theta" % c)
    for c in (2, 4):
        h = q if c == 2 else rh
        cs += variants("hlevelducting", [th, h, p], lambda f, c=c: [f[0], f[1], f[2], 0.0, 1.0, c], "%d-theta" % c)
        cs += variants("alevelducting", [th, h, p], lambda f, c=c: [f[0], f[1], f[2], c], "%d-theta" % c)
    return cs


def composite_kelvin64(case):
    """float64 temperature theta * (p * p0inv)^kappa of a composite case (hlevel cases here use alevel = 0, blevel = 1)."""
    theta, p = np.asarray(case["args"][0], np.float64), np.asarray(case["args"][1 if case["op"].endswith("temp") else 2], F)
    with np.errstate(all="ignore"):
        return theta * np.power((p * P0INV).astype(np.float64), np.float64(KAPPA))


# ---- showalterIndex: the hand-expanded divisions
def showalter_cases():
    t850 = cat(*[around(knot_kelvin(k), 2) for k in (-1, 0, 1, 39, 40)], np.linspace(168.2, 215.0, 180), np.linspace(330.0, 373.14, 90), [288.3, 262.0])
    n = len(t850)
    t500 = fill(n, 252.0, 240.5, 265.25)
    rh = fill(n, 60.0, 100.0, 0.0, 2.0, 1e-30, 35.5, 1e-45, -0.0)
    cs = []
    # (p500, p850): ordinary; p500 outside (1e-6, 1e9) -> plain division by p500; pressures that put cplr * qcl outside [2^-64, 2^64)
    for p500, p850 in ((500.0, 850.0), (1e-7, 850.0), (2e9, 1e25), (1e-16, 1e-15), (1e30, 3.0e38), (1e-38, 1e-37)):
        for c in (1, 2):
            cs += variants("showalterIndex", [t500, t850, rh], lambda f, p500=p500, p850=p850, c=c: [f[0], f[1], f[2], p500, p850, c], "%d-%g-%g" % (c, p500, p850))
    return cs


# ---- abshum / seaSoundSpeed: the double polynomial paths
def abshum_temperatures():
    def t2(t):  # log2 of the exponential's value, as the kernel's switch sees it (float64 is close enough to bracket it)
        t = np.float64(t)
        v = 1 - t / 647.096
        s = -7.85951783 * v + 1.84408259 * v ** 1.5 - 11.7866497 * v ** 3 + 22.6807411 * v ** 3.5 - 15.9618719 * v ** 4 + 1.80122502 * v ** 7.5
        return 647.096 / t * s * 1.4426950408889634

    lo, hi = 1.0, 100.0  # t2 rises with t: bisect t2 == -1000
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if t2(mid) < -1000.0 else (lo, mid)
    switch = np.linspace(lo * 0.999, lo * 1.001, 41).astype(F)
    return cat(around(647.096, 3), [650.0, 700.0, 1000.0, 1e4, 1e10, 3.0e38, INF], switch, around(F(lo), 3),
               [1.0, 2.0, 5.0, 10.0, 20.0, 30.0, 50.0, 100.0, 200.0, 273.15, 300.0, 373.15, 500.0, 640.0], [0.0, -0.0, -10.0, 1e-45, 1e-38, NAN, -INF])


def polynomial_cases():
    t = abshum_temperatures()
    cs = variants("abshum", [t, fill(len(t), 60.0, 100.0, 0.0, 2.0)], lambda f: [f[0], f[1]], "")
    ts = cat(around(0.0, 2), around(273.15, 2), [-1.9, 4.0, 25.0, 300.0, -1e10, 1e10, 3.0e38, -3.0e38, 1e-45, INF, -INF, NAN])
    sal = cat(around(35.0, 2), [0.0, 5.0, 38.0, -0.0, 3.0e38, INF, NAN])
    a, b = (np.array(x, F) for x in zip(*itertools.product(ts, sal)))
    for c in (1, 2):
        cs += variants("seaSoundSpeed", [a, b], lambda f, c=c: [f[0], f[1], -75.0, c], str(c))
    return cs


FAMILIES = {
    "table": table_cases,
    "inverse": inverse_cases,
    "flightlevel": flight_level_cases,
    "classes": classes_cases,
    "undercooled": undercooled_cases,
    "icing": icing_cases,
    "branches": branch_cases,
    "libm": libm_cases,
    "kappa": kappa_cases,
    "composite": composite_cases,
    "showalter": showalter_cases,
    "polynomial": polynomial_cases,
}

_CACHE = {}


def family(name):
    """The cases of one family; generated once and shared (callers must not modify the arrays)."""
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name]()
    return _CACHE[name]


def all_cases():
    return [c for name in FAMILIES for c in family(name)]
