"""What the cases of tests/member_range_cases.py hold, without a GPU: (a) the numpy restatement of the five ensemble
reductions equals the CPU checker (and the reference itself, where built) bit for bit on every case of the single-field
entries and of mifc_ensemble_levels, flags included; (b) the quantile cases reach the key distances, member counts and
interpolation weights they are for; (c) enough results of every class lie where the class is meant to put them, and a NaN --
which matches any NaN -- never takes more than a third of a product; (d) each suspected mistake (the MISTAKES of
ensemble_restate.py and quantile_restate.py) changes the bits of the cases; (e) every designed cell gives what its mark says.

(c), stddevValue in tiny data: the result is the root of a float quotient and the root of a subnormal float is a normal one
(sqrt(2^-149) = 2^-74.5), so no stddevValue result is subnormal.  What is measured is the quotient under the root, read from
the result: 0 < result < sqrt(FLT_MIN) = 2^-63."""
import numpy as np
import pytest

import ensemble_restate as er
import member_range_cases as mc
import quantile_restate as qr
from test_gpu_ensemble_levels import expected as checker_expected

GROUPS = [(family, klass) for family in ("single", "levels") for klass in mc.CLASSES]
MIN_CELLS = 8

# (d) the classes in which a mistake changes the bits of at least MIN_CELLS cells of one case (measured on the restatements;
# the single-field cases carry every product, so they stand for the reductions)
SHOWS = {
    "reductions": {
        "double accumulators": ("huge", "tiny", "mid"),
        "welford contracted": ("huge", "tiny", "mid"),
        "reciprocal": ("huge", "tiny", "mid"),
        "fmax": ("huge", "tiny", "mid"),
        "first maximum lost": ("huge", "tiny", "mid"),
        "flushed": ("huge", "tiny", "mid"),
        "hole by magnitude": ("huge", "tiny", "mid"),
        "probability tests is_def": ("huge", "tiny", "mid"),
    },
    "quantiles": {
        "linear in float": ("huge", "tiny", "mid"),
        "linear contracted": ("huge",),  # in tiny and mid data the exact product changes the rounded sum in fewer than MIN_CELLS cells
        "lerp": ("huge", "tiny", "mid"),
        "zeros equal": ("huge", "tiny", "mid"),
        "flushed": ("huge", "tiny", "mid"),
        "prefix one bit short": ("huge", "tiny", "mid"),
    },
}


def differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


def shares(out):
    out = np.asarray(out)
    finite = np.isfinite(out) & (out != 0)
    return dict(finite=finite.mean(), infinite=np.isinf(out).mean(), nan=np.isnan(out).mean(), zero=(out == 0).mean(),
                subnormal=(finite & (np.abs(out) < mc.FLT_MIN)).mean())


# ------------------------------------------------------------------------------------------------ (a)
def against_checker(cpu, case):
    exp = mc.expected(case)
    for p, (out, fd) in zip(case["products"], exp):
        e, efd = checker_expected(cpu, case["members"], case["flags"], p, case["undef"])
        what = (case["label"], er.name_of(p), p[1:] if er.name_of(p) == "probability" else None)
        assert differing(out, e) == 0, what + (differing(out, e), "cells")
        assert list(fd) == efd, what + (list(fd), efd)


@pytest.mark.parametrize("family,klass", GROUPS)
def test_restatement_is_the_checker_bit_for_bit(oracle, family, klass):
    for case in mc.cases(family, klass):
        against_checker(oracle, case)


@pytest.mark.parametrize("family,klass", GROUPS)
def test_restatement_is_the_reference_bit_for_bit(ref, family, klass):
    for case in mc.cases(family, klass):
        against_checker(ref, case)


def test_single_interface_of_the_restatement(oracle):
    """single(): the spelling of the five functions one by one, on one level of a case."""
    case = mc.cases("single", "mid")[0]
    x, fl = case["members"][:, 2], case["flags"][:, 2]
    fields, fin = list(x), [int(v) for v in fl]
    ny, nx = x.shape[1:]
    for name, args, kw in (("sumFields", (), dict(fdefined=mc.ALL_DEFINED)), ("meanValue", (fin,), {}), ("stddevValue", (fin,), {}),
                           ("extremeValue", (), dict(fdefined=mc.SOME_DEFINED)), ("probability", (fin, [280.0]), {})):
        short = {"sumFields": "sum", "meanValue": "mean", "stddevValue": "stddev", "extremeValue": "extreme", "probability": "probability"}[name]
        lead = (3,) if name == "extremeValue" else (2,) if name == "probability" else ()
        ok, e, fd = oracle.call(name, nx, ny, *lead, fields, *args, **kw)
        got, gfd = er.single(short, fields, flags=fin, compute=lead[0] if lead else 0, limits=[280.0], fdefined=kw.get("fdefined", mc.SOME_DEFINED))
        assert ok and differing(got, e) == 0 and gfd == fd, name


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("klass", mc.CLASSES)
def test_quantile_cases_reach_what_they_are_for(klass):
    seen = {"bisection": set(), "network": set()}
    weights = {}
    for case in mc.cases("quantiles", klass):
        ranks = {}
        mc.restate(case, ranks=ranks)
        nmem = case["members"].shape[0]
        n, dist = ranks["n"], ranks["kmin"] ^ ranks["kmax"]
        side = "bisection" if nmem > 64 else "network"
        # counted members, not members: a cell of the bisection with fewer than 65 counted ones says nothing about n > 64
        seen[side] |= {int(d) for d in dist[(n > 64) if nmem > 64 else ((n > 1) & (n <= 64))].ravel()}
        if case["method"] == "linear":
            t = ranks["t"][:, n > 0]
            zero, other = weights.setdefault(case["form"]["tier"], [False, False])
            weights[case["form"]["tier"]] = [zero or bool((t == 0).any()), other or bool((t != 0).any())]
        assert (n == 0).any() and (n == 1).any() or not case["marks"], case["label"]
    for side, got in seen.items():
        assert got >= {1, 2, 3, 0xFFFFFFFF}, (side, sorted(got)[:8])  # 0xffffffff: -0 and +0, every bit of the key differs
    assert weights == {tier: [True, True] for tier in (8, 16, 32, 64, 0)}, weights


def test_percentiles_and_member_counts():
    p = mc.PERCENTILES
    assert p[0] == 0 and p[1] == mc.DENORM_MIN and p[-1] == 100 and p[-2] < 100 and np.nextafter(p[-2], np.float32(200)) == 100
    assert {12.5, 30.0, 50.0, 37.5, 62.5} <= set(float(v) for v in p)
    assert (9 - 1) * 37.5 / 100 == 3 and (9 - 1) * 62.5 / 100 == 5  # t == 0 off the ends
    for klass in mc.CLASSES:
        assert {c["members"].shape[0] for c in mc.cases("quantiles", klass)} == set(mc.MEMBER_COUNTS)
        assert {c["form"]["tier"] for c in mc.cases("quantiles", klass)} == {8, 16, 32, 64, 0}
        assert {c["form"]["inline"] for c in mc.cases("quantiles", klass)} == {0, 1}
        big = [c for c in mc.cases("quantiles", klass) if c["members"].shape[0] > 64]
        assert big and all(c["members"][0, 0].size <= 240 for c in big)  # the bisection rereads every member per bit


# ------------------------------------------------------------------------------------------------ (c)
def by_product(klass):
    """product name -> every result of it in the class (the reductions), "LINEAR" -> those of the linear quantile cases."""
    got = {}
    for family in ("single", "levels"):
        for case in mc.cases(family, klass):
            for p, (out, _) in zip(case["products"], mc.expected(case)):
                got.setdefault(er.name_of(p), []).append(out.ravel())
    got["LINEAR"] = [mc.expected(c)[0].ravel() for c in mc.cases("quantiles", klass) if c["method"] == "linear"]
    return {k: np.concatenate(v) for k, v in got.items()}


def test_huge_results_are_finite_and_infinite():
    got = by_product("huge")
    for name in ("sum", "mean", "stddev", "LINEAR"):
        s = shares(got[name])
        assert s["finite"] >= 0.10 and s["infinite"] >= 0.10, (name, s)


def test_tiny_results_are_subnormal():
    got = by_product("tiny")
    for name in ("mean", "LINEAR"):
        s = shares(got[name])
        assert s["subnormal"] >= 0.10, (name, s)
    assert mc.under_root_is_subnormal(got["stddev"]).mean() >= 0.10  # (see the module's docstring)
    assert shares(got["stddev"])["subnormal"] == 0
    assert np.sqrt(np.float64(mc.DENORM_MIN)).astype(np.float32) >= mc.FLT_MIN


@pytest.mark.parametrize("klass", mc.CLASSES)
def test_no_product_of_a_case_is_nan_in_more_than_a_third_of_its_cells(klass):
    for family in mc.FAMILIES:
        for case in mc.cases(family, klass):
            exp = mc.expected(case)
            outs = [("quantiles", exp[0])] if family == "quantiles" else [(er.name_of(p), o) for p, (o, _) in zip(case["products"], exp)]
            for name, out in outs:
                assert np.isnan(out).mean() <= 1 / 3, (case["label"], name, float(np.isnan(out).mean()))


def test_welford_decades():
    """The table of the module: per member count about half of the cells on either side of FLT_MAX (m2, huge) and of
    FLT_MIN (m2 / n, tiny); the plain data of the two classes give nothing there."""
    for klass, table in mc.WELFORD_DECADE.items():
        assert set(table) == set(mc.MEMBER_COUNTS)
        for nmem, decade in table.items():
            assert 0.2 <= mc.welford_share(klass, nmem, decade) <= 0.8, (klass, nmem, decade, mc.welford_share(klass, nmem, decade))
    rng = np.random.default_rng(3)
    (huge, _), = er.statistics(mc.magnitudes(rng, "huge", (9, 1, 1, 2000)), None, ["stddev"])
    (tiny, _), = er.statistics(mc.magnitudes(rng, "tiny", (9, 1, 1, 2000)), None, ["stddev"])
    assert not np.isfinite(huge).any() and (tiny == 0).all()


def test_every_class_holds_the_specials():
    for klass in mc.CLASSES:
        for family in mc.FAMILIES:
            x = np.concatenate([c["members"].ravel() for c in mc.cases(family, klass) if not np.isnan(c["undef"])])
            bits = set(np.unique(x.view(np.uint32)).tolist())
            for v in list(mc.FINITE_SPECIALS) + [mc.INF, -mc.INF, mc.UNDEF, mc.NAN, mc.NEG_NAN]:
                assert int(np.float32(v).view(np.uint32)) in bits, (klass, family, v)
        if klass == "huge":
            plain = mc.magnitudes(np.random.default_rng(1), "huge", 1000)
            assert (np.abs(plain) > mc.UNDEF).all()
    for family in mc.FAMILIES:
        assert sum(bool(np.isnan(c["undef"])) for klass in mc.CLASSES for c in mc.cases(family, klass)) >= 1, family


def test_levels_lists_cover_every_instantiation():
    lists = mc.instance_lists("mid", 3)
    keys = [k for k, _ in lists]
    assert set(keys) == {(w, f, n) for w in (0, 1) for f in (0, 1) for n in (0, 3, 8)} - {(1, 0, 3)} and len(set(keys)) == 11
    assert len(lists[-1][1]) == 15
    for (w, f, n), products in lists:
        names = [er.name_of(p) for p in products]
        nprob = names.count("probability")
        asked = (int("stddev" in names), int(any(k in names for k in ("sum", "max", "min", "argmax", "argmin"))), 0 if nprob == 0 else 3 if nprob <= 3 else 8)
        assert asked == (w, f, n) or (asked == (1, 0, 3) and (w, f, n) == (1, 1, 3)), (products, asked)
    assert sum(k == (1, 1, 3) for k in keys) == 2  # one of them is the list without a flagged product (checked above)
    for klass in mc.CLASSES:
        forms = {(c["form"]["c"], c["form"]["welford"], c["form"]["flagged"], c["form"]["np"]) for c in mc.cases("levels", klass)}
        assert forms == {(4,) + k for k in set(keys)} | {(1, 1, 1, 8)}
        assert {c["form"]["inline"] for c in mc.cases("levels", klass)} == {0, 1}
        assert any(c["members"].shape[1] == 65 for c in mc.cases("levels", klass))


# ------------------------------------------------------------------------------------------------ (d)
def test_the_tables_name_every_mistake():
    assert set(SHOWS["reductions"]) == set(er.MISTAKES) and set(SHOWS["quantiles"]) == set(qr.MISTAKES)
    assert "tiny" in SHOWS["reductions"]["flushed"] and "tiny" in SHOWS["quantiles"]["flushed"] and "huge" in SHOWS["reductions"]["hole by magnitude"]
    assert set(SHOWS["reductions"]["fmax"]) == set(mc.CLASSES) == set(SHOWS["quantiles"]["zeros equal"])


@pytest.mark.parametrize("kind,mistake", [(k, m) for k in SHOWS for m in SHOWS[k]])
def test_each_mistake_changes_the_bits(kind, mistake):
    family = "single" if kind == "reductions" else "quantiles"
    for klass in SHOWS[kind][mistake]:
        most = 0
        for case in mc.cases(family, klass):
            exp, got = mc.expected(case), mc.restate(case, mistakes=(mistake,))
            if family == "quantiles":
                most = max(most, differing(got[0], exp[0]))
            else:
                most = max(most, sum(differing(g, e) for (g, _), (e, _) in zip(got, exp)))
            if most >= MIN_CELLS:
                break
        assert most >= MIN_CELLS, (mistake, klass, most)


def test_default_of_the_quantile_restatement_is_unchanged():
    case = mc.cases("quantiles", "mid")[1]
    out, _ = qr.quantiles(case["members"], case["percentiles"], qr.LINEAR, case["flags"])
    again, _ = qr.quantiles(case["members"], case["percentiles"], qr.LINEAR, case["flags"], mistakes=())
    assert differing(out, again) == 0 and differing(out, mc.expected(case)[0]) == 0
    with pytest.raises(AssertionError):
        qr.quantiles(case["members"], [50.0], qr.LINEAR, mistakes=("no such mistake",))
    with pytest.raises(AssertionError):
        er.statistics(case["members"], None, ["mean"], mistakes=("no such mistake",))


# ------------------------------------------------------------------------------------------------ (e)
def product_of_mark(case, name):
    if name in mc.MARK_PRODUCTS:
        _, compute, nth = mc.MARK_PRODUCTS[name]
        return [k for k, p in enumerate(case["products"]) if er.name_of(p) == "probability" and p[1] == compute][nth]
    return [er.name_of(p) for p in case["products"]].index(name)


@pytest.mark.parametrize("klass", mc.CLASSES)
def test_every_mark_of_the_reductions_is_met(klass):
    marked = [c for c in mc.cases("single", klass) if c["marks"]]
    assert len(marked) >= 3
    for case in marked:
        exp = mc.expected(case)
        for mark, (name, lev, col, want) in case["marks"].items():
            got = exp[product_of_mark(case, name)][0][lev, 0, col]
            assert (np.isnan(want) and np.isnan(got)) or got.view(np.uint32) == np.float32(want).view(np.uint32), (case["label"], mark, got, want)
        # a sum and a mean that equal undef are written and not counted as holes: without any hole on a level of them alone
        # the flag would be ALL_DEFINED
        x = case["members"][:, :1, :1]
        (s_out, s_fd), = er.statistics(x[..., 0:1], None, ["sum"])
        (m_out, m_fd), = er.statistics(x[..., 1:2], None, ["mean"])
        assert s_out.ravel()[0] == mc.UNDEF and m_out.ravel()[0] == mc.UNDEF and s_fd[0] == mc.ALL_DEFINED and m_fd[0] == mc.ALL_DEFINED


@pytest.mark.parametrize("klass", mc.CLASSES)
def test_every_mark_of_the_quantiles_is_met(klass):
    F = np.float32
    for case in mc.cases("quantiles", klass):
        if not case["marks"]:
            continue
        ranks = {}
        out, _ = mc.restate(case, ranks=ranks)
        nmem, nlev, ny, nx = case["members"].shape
        n, dist = ranks["n"].reshape(nlev, ny, nx), (ranks["kmin"] ^ ranks["kmax"]).reshape(nlev, ny, nx)
        p = {float(v): k for k, v in enumerate(case["percentiles"])}
        for mark, (lev, row, col, values) in case["marks"].items():
            at, cell = (lev, row, col), out[:, lev, row, col]
            what = (case["label"], mark, cell)
            if mark.startswith("neighbours"):
                assert dist[at] == int(mark[-1]) and n[at] == nmem, what
                assert ((cell >= values.min()) & (cell <= values.max())).all(), what  # at most three floats to choose from
                assert cell[0] == values.min() and cell[-1] == values.max(), what
            elif mark == "-0 and +0":
                assert dist[at] == 0xFFFFFFFF and np.signbit(cell[0]) and not np.signbit(cell[-1]) and (cell == 0).all(), what
            elif mark == "around zero":
                assert cell[0] == -mc.DENORM_MIN and cell[-1] == mc.DENORM_MIN, what
            elif mark == "-FLT_MAX and FLT_MAX":
                assert cell[0] == -mc.FLT_MAX and cell[-1] == mc.FLT_MAX and np.isfinite(cell).all(), what  # b - a is finite in double only
            elif mark == "FLT_MAX and +inf":
                assert cell[0] == mc.FLT_MAX and cell[-1] == mc.INF and not np.isnan(cell[[0, -1]]).any(), what
            elif mark == "-inf and +inf":
                assert cell[0] == -mc.INF and cell[-1] == mc.INF, what
            elif mark == "2^-149 and twice":
                assert n[at] == 2 and cell[p[50.0]] == 2 * mc.DENORM_MIN, what  # LINEAR: 1.5 * 2^-149 rounds to even; LOWER: rank int(2 * 0.5) = 1
                assert cell[0] == mc.DENORM_MIN and cell[-1] == 2 * mc.DENORM_MIN, what
            elif mark == "no member counts":
                assert n[at] == 0 and (cell == case["undef"]).all(), what
            elif mark == "one member counts":
                assert n[at] == 1 and (cell == values[0]).all(), what
            elif mark == "NaN at the top ranks, all":
                assert n[at] == nmem and np.isnan(cell[-1]) and not np.isnan(cell[0]), what
            elif mark == "1e35 counted, all":
                assert n[at] == nmem and cell[0] == F(-3.0e37) and cell[-1] == F(3.0e37), what  # 1e35 is one of the values in between
            else:
                raise AssertionError("a mark without a test: %s" % mark)
