"""The range cases of the horizontal families (tests/horizontal_range_cases.py) on the CPU: every case goes through the
numpy restatements and must reach what its class is for without degrading into comparing NaN with NaN or undef with undef;
every seam the cases are built around must be there; each suspected mistake -- a flush to zero, a float intermediate, and
the named departures of hinterp_restate.MISTAKES, hremap_restate.MISTAKES and hstats_restate.MISTAKES -- must change the
cases aimed at it; and a handful of one-point, one-row and one-cell inputs, worked out here in plain Python floats from the
sentences of include/mifc.h, pin the restatements themselves.

The conditions are the generator's contract, not measurements: its rates and placements are tuned until they hold.

Bounds and exemptions that are set here, and where they come from:
  * hvector is held to the bounds of hinterp, case by case: at most 10 % of NaN, at most half holes.
  * `huge` hinterp: an infinity from finite inputs is asked of BICUBIC only.  A bilinear result lies between its corners up
    to one rounding in double, which the rounding to float cannot carry past FLT_MAX, and NEAREST computes nothing.
  * "greater in place of greater or equal" cannot show at min_frac == 0: |Wdef| > 0 fails only for Wdef == 0.0, which is a
    hole by its own clause.  The RENORM cases with min_frac 1 and MIN_FRAC_ROUNDS carry that seam.
"""
import contextlib
from fractions import Fraction

import numpy as np
import pytest

import hinterp_restate as hi
import horizontal_range_cases as hc
import hremap_restate as hr
import hstats_restate as hs
import vrotate_restate as vr
from test_column_range_cpu import _NarrowNumpy, flushed

A, N, S = hc.ALL_DEFINED, hc.NONE_DEFINED, hc.SOME_DEFINED
U = hc.UNDEF
F = np.float32
FLT_MAX, FLT_MIN, DEN = hc.FLT_MAX, hc.FLT_MIN, hc.DENORM_MIN
INF, NAN = hc.INF, hc.NAN
DBL_MIN = np.finfo(np.float64).tiny
GROUPS = [(family, klass) for family in hc.FAMILIES for klass in hc.CLASSES]
EVERY = [c for family, klass in GROUPS for c in hc.cases(family, klass)]


def ids(case):
    return case["label"]


def of(family, klass=None, **match):
    return [c for c in EVERY if c["family"] == family and klass in (None, c["klass"]) and all(c.get(k) == v for k, v in match.items())]


def full_grid(c):
    return c["fields"].shape[2:] == (hc.NY, hc.NX) and "clean" not in c["label"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def is_undef(out):
    return bits(np.asarray(out, np.float32)) == bits(U)


def differs(a, b):
    """Some output differs in bits (a NaN matches any NaN), or some flag does; over the arrays of a restatement's result."""
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype.kind == "f":
            if ((bits(x) != bits(y)) & ~(np.isnan(x) & np.isnan(y))).any():
                return True
        elif not np.array_equal(x, y):
            return True
    return False


def subnormal(a):
    return (a != 0) & (np.abs(a) < (FLT_MIN if a.dtype == np.float32 else DBL_MIN))


# ---------------------------------------------------------------------------------------------- what the cases reach
def test_the_number_of_cases():
    count = {(family, klass): len(hc.cases(family, klass)) for family, klass in GROUPS}
    assert count == {("hinterp", "huge"): 3, ("hinterp", "tiny"): 4, ("hinterp", "mid"): 6, ("hvector", "huge"): 2, ("hvector", "tiny"): 2,
                     ("hvector", "mid"): 2, ("hremap", "huge"): 4, ("hremap", "tiny"): 3, ("hremap", "mid"): 6, ("hstats", "huge"): 3,
                     ("hstats", "tiny"): 3, ("hstats", "mid"): 4}
    assert len({c["label"] for c in EVERY}) == len(EVERY)


def shares(case):
    """(NaN, hole, number) shares of the float results, and the numbers themselves."""
    res = hc.expected(case)
    out = res[1] if case["family"] == "hstats" else res[0]
    hole, nan = is_undef(out), np.isnan(out)
    return nan.mean(), hole.mean(), (~hole & ~nan).mean(), out[~hole & ~nan]


@pytest.mark.parametrize("case", of("hinterp") + of("hvector") + of("hremap"), ids=ids)
def test_point_and_row_cases_compare_numbers(case):
    nan, hole, number, values = shares(case)
    assert nan <= 0.10, (case["label"], nan)
    assert hole <= 0.5 and number >= 0.4, (case["label"], hole, number)
    if case["klass"] == "huge":
        assert (np.isfinite(values) & (np.abs(values) > 1e30)).any(), case["label"]
    if case["klass"] == "tiny":
        assert subnormal(values).mean() >= 0.2, (case["label"], subnormal(values).mean())
    out, fd = hc.expected(case)
    assert out.shape[:2] == case["flags"].shape == fd.shape


@pytest.mark.parametrize("case", of("hstats"), ids=ids)
def test_hstats_cases_compare_numbers(case):
    stats, mean, fd = hc.expected(case)
    if case["products"] & hs.MOMENTS:
        poisoned = np.isnan(stats[..., hs.S1]) | np.isnan(stats[..., hs.S2])
        assert 3 * poisoned.sum() <= poisoned.size, (case["label"], poisoned.mean())
        assert (~np.isnan(mean) & ~is_undef(mean)).mean() >= 0.5, case["label"]
    else:
        assert np.isnan(stats[..., :4]).all() and is_undef(mean).all()  # (not asked for: the fill)
    if case["products"] & hs.EXTREMES:
        assert not np.isnan(stats[..., 4:]).any() and (stats[..., hs.IMIN] >= 0).mean() > 0.8, case["label"]
        assert (np.abs(stats[..., hs.MIN]) != np.inf).mean() > 0.5
    else:
        assert np.isnan(stats[..., 4:]).all()


def test_huge_cases_give_both_infinities_from_finite_inputs():
    for c in of("hinterp", "huge", method="bicubic"):
        out, _ = hc.expected(c)
        br = np.zeros(out.shape, np.int64)
        hi.sample(c["fields"], c["x"], c["y"], c["method"], c["flags"], branches=br)
        p = c["marks"]["overshoot"]
        assert np.isfinite(c["fields"][:, :, 0:4, 6:10]).all() and (br[:, :, p] == hi.CUBIC).all()
        assert (out[0::2, :, p] == INF).all() and (out[1::2, :, p] == -INF).all(), c["label"]
    for c in of("hvector", "huge", method="bicubic"):  # u leaves the float range at the mark, v does not: u' = +inf, v' = -inf
        out, _ = hc.expected(c)
        p = c["marks"]["overshoot"]
        sampled, _ = hi.sample(c["fields"], c["x"], c["y"], c["method"], c["flags"])
        assert np.isfinite(c["fields"][:, :, 0:4, 6:10]).all() and (c["cosa"][p], c["sina"][p]) == (F(0.6), F(-0.8))
        assert (sampled[0::2, :, p] == INF).all() and np.isfinite(sampled[1::2, :, p]).all()
        assert (out[0::2, :, p] == INF).all() and (out[1::2, :, p] == -INF).all(), c["label"]
    assert of("hvector", "huge", method="bicubic")
    for c in of("hremap", "huge"):
        out, _ = hc.expected(c)
        assert (out[:, :, c["marks"]["overflows"]] == INF).all() and (out[:, :, c["marks"]["overflows down"]] == -INF).all(), c["label"]
    seen = set()
    for c in of("hstats", "huge"):
        if c["minus"] is not None and c["mode"] == "rows" and c["products"] & hs.MOMENTS:
            _, mean, _ = hc.expected(c)
            assert np.isfinite(c["fields"][:, 5, 0]).all() and np.isfinite(c["minus"][:, 5, 0]).all()
            seen |= {float(v) for v in mean[:, 5, 0]}
        stats, mean, _ = hc.expected(c)
        if c["products"] & hs.MOMENTS:
            assert (np.isfinite(mean) & (np.abs(mean) > 1e30) & ~is_undef(mean)).any(), c["label"]
    assert seen == {np.inf, -np.inf}


def test_tiny_hstats_cases_reach_double_denormals_and_float_denormal_means():
    small = [c for c in of("hstats", "tiny") if c["pivot"] is not None]
    assert small
    for c in small:
        stats, mean, _ = hc.expected(c)
        assert stats[0, 0, 0, hs.N] == 8 and stats[0, 0, 0, hs.S1] == -8e-310 and stats[0, 0, 0, hs.MIN] == -1e-310 == stats[0, 0, 0, hs.MAX]
        assert subnormal(stats[0, 0, 0, hs.S2:hs.S2 + 1]).all() or stats[0, 0, 0, hs.S2] == 0  # 1e-310^2 underflows: +0.0
    means = np.concatenate([hc.expected(c)[1].ravel() for c in of("hstats", "tiny") if c["products"] & hs.MOMENTS])
    means = means[~is_undef(means) & ~np.isnan(means)]
    assert subnormal(means).mean() >= 0.2, subnormal(means).mean()


# ---------------------------------------------------------------------------------------------- the seams are there
def sampled(c):
    out, fd = hc.expected(c)
    br, cells = np.zeros(out.shape, np.int64), {}
    hi.sample(c["fields"], c["x"], c["y"], c["method"], c["flags"], branches=br, cells=cells)
    return out, fd, br, cells


def test_hinterp_every_branch_of_every_method_occurs():
    for name, code in hi.METHODS.items():
        seen = set()
        for c in of("hinterp", method=name):
            seen |= set(np.unique(sampled(c)[2]))
        assert seen == set(hi.REACHABLE[code]), (name, seen)


def test_hinterp_positions_at_the_ends_of_every_cell():
    for c in [c for c in of("hinterp") if full_grid(c)]:
        x, y = c["x"], c["y"]
        for v, n in ((x, hc.NX), (y, hc.NY)):
            have = set(bits(v))
            want = [0.0, -0.0, DEN, -DEN, FLT_MIN, 0.5, np.nextafter(F(0.5), F(0)), np.nextafter(F(0.5), F(1)), np.inf, -np.inf, U,
                    np.nextafter(F(n - 1), INF), np.nextafter(F(n - 1), F(0)), n - 1]
            want += [k + 0.5 for k in range(n - 1)] + [np.nextafter(F(k), INF) for k in range(n)] + [np.nextafter(F(k), -INF) for k in range(n)]
            assert all(int(bits(F(w))) in have for w in want) and np.isnan(v).any(), c["label"]
        _, _, br, _ = sampled(c)
        outside = [int(np.nonzero(bits(x) == bits(F(w)))[0][0]) for w in (-DEN, np.nextafter(F(hc.NX - 1), INF), np.inf)]
        assert (br[:, :, outside] == hi.OUTSIDE).all()
        assert 600 == x.size and x.size % 64 != 0 and x.size > 2 * 256
    # 0.49999997f + 0.5 is exact in double and truncates to 0; in float it rounds to 1.0
    below = np.nextafter(F(0.5), F(0))
    assert int(float(below) + 0.5) == 0 and int(below + F(0.5)) == 1


def test_hinterp_waves_without_with_and_with_some_cubic_lanes():
    cases = [c for c in of("hinterp", method="bicubic") if full_grid(c)]
    assert len(cases) >= 3
    for c in cases:
        out, _, br, cells = sampled(c)
        cubic = br == hi.CUBIC
        assert not cubic[:, :, 0:64].any() and cubic[:, :, 64:128].all(), c["label"]
        assert cubic[:, :, 128:192:2].all() and not cubic[:, :, 129:192:2].any(), c["label"]
        on_rows = (cells["b"][64:128] == 0) & (cells["a"][64:128] != 0)
        assert on_rows.sum() >= 8 and ((cells["a"][64:128] == 0) & (cells["b"][64:128] != 0)).sum() >= 8
        # the corners that the odd lanes' blocks are folded onto hold inf or NaN, on every level
        i0, j0 = cells["i0"][129:192:2], cells["j0"][129:192:2]
        corners = np.stack([c["fields"][:, :, j0 + dj, i0 + di] for dj in (0, 1) for di in (0, 1)])
        assert (~np.isfinite(corners)).any(axis=0).mean(axis=2).min() >= 0.75, c["label"]


def test_hinterp_corner_scenarios():
    done = set()
    for c in [c for c in of("hinterp") if full_grid(c) and c["method"] != "nearest"]:
        out, fd, br, cells = sampled(c)
        m, f = c["marks"], c["fields"]
        bilinear = c["method"] == "bilinear"
        tested = c["flags"] == S
        # inf - inf at a needed corner: a computed NaN, not a hole
        p = m["inf minus inf"]
        assert np.isnan(out[:, :, p]).all() and not np.isin(br[:, :, p], vr.SAMPLING_HOLES).any()
        # x10 - x00 leaves the float range and comes back
        p = m["overflow and back"]
        with np.errstate(over="ignore"):
            assert F(FLT_MAX) - F(-FLT_MAX) == INF and cells["a"][p] == 0.5 and cells["b"][p] == 0
        if bilinear:
            assert (bits(out[:, :, p]) == 0).all()
            # a corner that is not needed holds inf, NaN or undef and does not reach the result, tested or not
            for name, (dj, di) in (("node", (1, 1)), ("on a column", (0, 1)), ("on a row", (1, 0))):
                p = m[name]
                i0, j0 = cells["i0"][p], cells["j0"][p]
                assert np.isfinite(out[:, :, p]).all() and not is_undef(out[:, :, p]).any(), (c["label"], name)
                other = f[:, :, j0 + dj, i0 + di]
                assert (~np.isfinite(other) | is_undef(other)).all(), (c["label"], name)
            assert (bits(out[:, :, m["node"]]) == bits(f[:, :, 4, 8])).all()
            assert (bits(out[:, :, m["equal to undef"]]) == bits(U)).all() and (br[:, :, m["equal to undef"]] == hi.ON_ROW).all()
            assert np.isfinite(out[:, :, m["zero weight times inf"]]).all()
            done.add("bilinear")
        else:
            p = m["zero weight times inf"]
            assert cells["b"][p] == 0 and cells["a"][p] != 0 and (f[:, :, 4, 9] == INF).all()
            assert (br[:, :, p] == hi.CUBIC).all() and np.isnan(out[:, :, p]).all(), c["label"]
            done.add("bicubic")
        if tested.any() and (~tested).any():
            done.add("both flags")
    assert done == {"bilinear", "bicubic", "both flags"}
    clean = [c for c in of("hinterp") if "clean" in c["label"]][0]
    out, fd = hc.expected(clean)
    assert (fd == A).all() and is_undef(out[:, :, clean["marks"]["equal to undef"]]).all() and is_undef(out).sum() == 2


def test_hvector_coefficients_of_every_kind():
    for c in of("hvector"):
        for v in (c["cosa"], c["sina"]):
            assert np.isnan(v).any() and np.isinf(v).any() and subnormal(v).any() and (np.abs(v) >= 3e38).any() and (bits(v) == bits(F(-0.0))).any()
            assert is_undef(v).any(), c["label"]
    assert {c["fdef_rot"] for c in of("hvector")} == {A, S}
    assert {c["fields"].shape[0] for c in of("hvector")} == {2, 4} and {c["method"] for c in of("hvector")} == set(hi.METHODS)


def row_sums(c, f, k, d):
    """Rule 2 of mifc_hremap_levels for one destination in Python floats: (S, Wdef, Wall, nbad, entries)."""
    rowptr, col, w = c["table"]
    src = c["fields"].reshape(c["fields"].shape[:2] + (-1,))[f, k]
    every = c["flags"][f, k] == A
    s = wdef = wall = 0.0
    nbad = 0
    with np.errstate(all="ignore"):
        for e in range(rowptr[d], rowptr[d + 1]):
            x, we = src[col[e]], float(w[e])
            wall = wall + we
            if every or not (np.isnan(x) or x == U):
                s, wdef = s + np.float64(we) * np.float64(x), wdef + we
            else:
                nbad += 1
    return float(s), wdef, wall, nbad, int(rowptr[d + 1] - rowptr[d])


def levels_of(c):
    """(a tested (field, level), an untested one) of the case, None where it has none."""
    t, u = np.argwhere(c["flags"] == S), np.argwhere(c["flags"] == A)
    return (tuple(t[0]) if len(t) else None), (tuple(u[0]) if len(u) else None)


def test_hremap_designed_rows():
    main = [c for c in of("hremap") if "clean" not in c["label"]]
    assert {c["fields"].shape[1] for c in main} == {7, 13} and {c["fields"].shape[0] for c in main} == {1, 2, 3, 4}
    assert {(c["mode"], c["min_frac"]) for c in main} == {("strict", 0.0), ("renorm", 0.0), ("renorm", 1.0), ("renorm", hc.MIN_FRAC_ROUNDS)}
    done = set()
    for c in main:
        rowptr, col, w = c["table"]
        m = c["marks"]
        length = np.diff(rowptr)
        assert rowptr.size == 201 and (length == 0).any() and length.max() == 17
        assert all(int(bits(F(v))) in set(bits(w)) for v in (0.0, -0.0, DEN, -DEN, FLT_MIN, -FLT_MIN, 3e38, -3e38, FLT_MAX)) and np.isfinite(w).all()
        out, fd = hc.expected(c)
        tested, untested = levels_of(c)
        f, k = tested or untested
        # the sums
        s, _, _, _, _ = row_sums(c, f, k, m["cancels"])
        assert s == 0.0 and float(FLT_MAX) * float(FLT_MAX) + 1.0 == float(FLT_MAX) * float(FLT_MAX) and bits(out[f, k, m["cancels"]]) == 0
        assert subnormal(out[:, :, m["subnormal"]]).all()
        assert np.isnan(out[:, :, m["minus zero times inf"]]).all()
        assert is_undef(out[:, :, m["equal to undef"]]).all() and row_sums(c, f, k, m["equal to undef"])[3] == 0
        # the padding entries of a short row name a cell that holds inf (NaN), in a slice wider than the row
        pad, width = hr.padding_columns(rowptr, col)
        for name, cell in (("short after inf", "inf"), ("short after inf, negative", "inf"), ("short after nan", "nan")):
            assert pad[m[name]] == hc.SRC[cell] and width[m[name]] >= 12 > length[m[name]], name
        assert (out[:, :, m["short after inf"]] == INF).all() and (out[:, :, m["short after inf, negative"]] == -INF).all()
        flat = c["fields"].reshape(c["fields"].shape[:2] + (-1,))
        assert (flat[:, :, 0] == INF).all() and (pad[length == 0] == 0).all()
        if untested:
            assert np.isnan(out[untested][m["short after nan"]])
        # the slices: none, every and some of the rows have a bad entry where the level tests
        if tested:
            nbad = np.array([row_sums(c, f, k, d)[3] for d in range(200)])
            assert (nbad[:64] == 0).all() and (nbad[64:128] > 0).all() and 0 < (nbad[128:192] > 0).sum() < 64, c["label"]
            _, wdef, wall, nb, n = row_sums(c, f, k, m["wdef cancels"])
            assert wdef == 0.0 and 0 < nb < n and wall == 1.0
            _, wdef, wall, nb, n = row_sums(c, f, k, m["wall zero"])
            assert wall == 0.0 and wdef == -1.0 and nb == 1
            assert row_sums(c, f, k, m["wall zero, no bad"])[2] == 0.0
            # the min_frac test, with equality and one ulp short of it
            _, wdef, wall, nb, _ = row_sums(c, f, k, m["equal at one"])
            assert wdef == wall == 0.75 and nb == 1
            _, wdef, wall, nb, _ = row_sums(c, f, k, m["one ulp short at one"])
            assert wdef == 0.75 and wall == np.nextafter(0.75, 1.0) and nb == 1
            _, wdef, wall, nb, _ = row_sums(c, f, k, m["equal where it rounds"])
            need = hc.MIN_FRAC_ROUNDS * wall
            assert wdef == 0.75 == need and Fraction(hc.MIN_FRAC_ROUNDS) * Fraction(wall) != Fraction(need) and nb == 1
            _, wdef2, wall2, nb, _ = row_sums(c, f, k, m["one ulp short where it rounds"])
            assert wdef2 == np.nextafter(0.75, 0.0) and wall2 == wall and nb == 2
            s, wdef, wall, _, _ = row_sums(c, f, k, m["renorm overflows"])
            assert np.isfinite(s) and F((s / wdef) * wall) == INF
            s, wdef, wall, _, _ = row_sums(c, f, k, m["renorm overflows, wdef tiny"])
            assert wdef == float(DEN) and np.isfinite(s) and F((s / wdef) * wall) == INF
            if c["mode"] == "renorm":
                got = out[f, k]
                assert is_undef(got[m["wdef cancels"]]) and is_undef(got[m["all bad"]])
                # (Wdef / Wall is 0.8 in the one row and 2^-150 in the other)
                assert (got[m["renorm overflows"]] == INF) == (c["min_frac"] < 0.8) and (got[m["renorm overflows, wdef tiny"]] == INF) == (c["min_frac"] == 0)
                done.add(c["min_frac"])
                if c["min_frac"] == 1.0:
                    assert not is_undef(got[m["equal at one"]]) and is_undef(got[m["one ulp short at one"]])
                if c["min_frac"] == hc.MIN_FRAC_ROUNDS:
                    assert not is_undef(got[m["equal where it rounds"]]) and is_undef(got[m["one ulp short where it rounds"]])
    assert done == {0.0, 1.0, hc.MIN_FRAC_ROUNDS}
    clean = [c for c in of("hremap") if "clean" in c["label"]][0]
    out, fd = hc.expected(clean)
    assert (fd == A).all() and is_undef(out[:, :, clean["marks"]["equal to undef"]]).all() and is_undef(out).sum() == 2


def test_hremap_strict_and_renorm_agree_where_no_entry_is_bad():
    for c in [c for c in of("hremap", mode="renorm") if "clean" not in c["label"]]:
        strict = hr.remap(c["fields"], *c["table"], "strict", 0.0, c["flags"])[0]
        out, _ = hc.expected(c)
        same = (bits(out) == bits(strict)) | (np.isnan(out) & np.isnan(strict))
        assert same[:, :, :64].all() and same[c["flags"] == A].all() and same.all() == (c["flags"] == A).all(), c["label"]


def test_hstats_shapes_options_and_seams():
    cases = of("hstats")
    assert {c["fields"].shape[2:] for c in cases} == {hc.WIDE, hc.SMALL} and {c["fields"].shape[0] for c in cases} == {1, 2, 3, 4}
    assert {c["fields"].shape[1] for c in cases} == {7}
    assert {(c["mode"], c["products"]) for c in cases} == {("area", 3), ("rows", 3), ("rows", 1), ("rows", 2)}
    for key in ("minus", "weight", "pivot", "box"):
        assert {c[key] is None for c in cases} == {True, False}, key
    assert {c["fdef_weight"] for c in cases if c["weight"] is not None} == {A, S}
    assert any((c["flags"] == A).all() for c in cases)
    for c in cases:
        x, (ny, nx) = c["fields"], c["fields"].shape[2:]
        stats, mean, fd = hc.expected(c)
        if nx > hs.SEGMENT and c["box"] is None and c["weight"] is None and c["pivot"] is None and c["minus"] is None:
            for i in hc.WIDE_COLUMNS:  # the first and last cell of a segment, lanes 0 and 63, the first and last trip
                assert i // 4 % 64 in (0, 63) and np.isin(bits(x[:, 1:6, :, i]), bits(hc.FINITE_SPECIALS)).all()
            assert {4095, 4096} <= set(hc.WIDE_COLUMNS) and {0, 15} <= {i % 4096 // 256 for i in hc.WIDE_COLUMNS}
            if c["products"] & hs.EXTREMES:
                assert np.isin(stats[..., hs.IMAX] % nx, hc.WIDE_COLUMNS).any() and np.isin(stats[..., hs.IMIN] % nx, hc.WIDE_COLUMNS).any()
        if c["box"]:  # nothing but inf, NaN and undef outside the box; the wide box cuts the 16-byte groups at both ends
            i0, i1, j0, j1 = c["box"]
            out = np.ones((ny, nx), bool)
            out[j0:j1, i0:i1] = False
            assert (~np.isfinite(x[:, :, out]) | is_undef(x[:, :, out])).all() and out.any()
            for kind in (np.isnan, np.isinf, is_undef):
                assert kind(x[:, :, out]).any()
            if nx > hs.SEGMENT:
                assert i0 % 4 and i1 % 4 and i0 // 4 == 1 and i1 > hs.SEGMENT
        if c["weight"] is not None and c["fdef_weight"] == S:  # what an undefined weight excludes is inf, NaN or undef
            gone = is_undef(c["weight"])
            assert gone.any() and (~np.isfinite(x[:, :, gone]) | is_undef(x[:, :, gone])).all()
            assert gone[:, hc.cols_of(nx)].all() or gone[[0, 1, 3]][:, hc.cols_of(nx)].all()
            if c["mode"] == "rows" and c["products"] & hs.MOMENTS:  # cancelling weights: W == 0.0 with N > 0, a hole
                last = x.shape[1] - 1
                assert (stats[:, last, 2, hs.W] == 0).all() and (stats[:, last, 2, hs.N] > 0).all() and is_undef(mean[:, last, 2]).all()
                assert (fd[:, last] == S).all()
        if c["weight"] is not None and c["fdef_weight"] == A:
            w = c["weight"]
            assert np.isnan(w).any() and np.isinf(w).any() and subnormal(w).any() and (bits(w) == bits(F(-0.0))).any() and is_undef(w).any()
            assert np.isfinite(w[:ny - 1]).all()  # the poisoning weights in the last row only
        if c["pivot"] is not None:
            p = c["pivot"]
            assert p[0, 0] == 1e-310 and p[0, 1] == 1e200 and p[0, 2] == np.inf and np.isnan(p[0, 3]) and p[-1, 5] == -np.inf
            j, i = (c["box"][2], c["box"][0]) if c["box"] else (0, 0)
            assert p[-1, 4] == np.nextafter(np.float64(x[-1, 4, j, i]), np.inf)
            if c["products"] & hs.MOMENTS and c["minus"] is None:
                assert (stats[0, 1, :, hs.S2] == np.inf).all()  # (x - 1e200)^2 is inf in double
    # a mean that is bit-equal to undef with N > 0 is a value and leaves the flag alone; a row of undefined cells is a hole
    plain = [c for c in cases if c["mode"] == "rows" and c["weight"] is None and c["pivot"] is None and c["minus"] is None]
    assert len(plain) >= 2
    for c in plain:
        stats, mean, fd = hc.expected(c)
        last = c["fields"].shape[1] - 1
        assert is_undef(mean[:, last, 0]).all() and (stats[:, last, 0, hs.N] == 4100).all() and (fd[:, last] == A).all(), c["label"]
        assert np.isnan(mean[:, last, 1]).all() and np.isnan(stats[:, last, 2, hs.S1]).all()  # NaN; +inf beside -inf
        if (c["flags"][-1, 0] == S):
            assert stats[-1, 0, 1, hs.N] == 0 and is_undef(mean[-1, 0, 1]) and fd[-1, 0] == S


# ---------------------------------------------------------------------------------------------- the cases discriminate
def restate_flushing(case):
    c = {k: flushed(v) for k, v in case.items()}
    if case["family"] == "hremap":
        c["table"] = (case["table"][0], case["table"][1], flushed(case["table"][2]))
    return tuple(flushed(a) for a in hc.restate(c))


@pytest.mark.parametrize("case", [c for c in EVERY if c["klass"] == "tiny"], ids=ids)
def test_a_flush_to_zero_shows_in_every_tiny_case(case):
    assert differs(restate_flushing(case), hc.expected(case)), case["label"]


@contextlib.contextmanager
def float_intermediates():
    mods = (hi, hr, hs, vr)
    try:
        for m in mods:
            m.np = _NarrowNumpy()
        yield
    finally:
        for m in mods:
            m.np = np


def test_the_narrowing_variant_is_the_restatement_where_nothing_leaves_the_float_range():
    """On small integers, halves and quarters every difference, sum and product is exact in float: the variant and the
    restatement agree, so what the next test sees is the rounding and nothing else."""
    x = ((np.arange(2 * 3 * 5 * 6, dtype=np.float32).reshape(2, 3, 5, 6) * 5) % 7)
    flags = np.full((2, 3), S, np.int32)
    px, py = np.array([0.5, 1.25, 3.0, 4.5], np.float32), np.array([1.0, 2.5, 0.75, 3.5], np.float32)
    rowptr, col, w = np.array([0, 2, 3, 6]), np.array([0, 7, 29, 3, 4, 5]), np.array([0.5, 0.25, 1.0, 2.0, 1.0, 0.125], np.float32)
    small = [dict(family="hinterp", fields=x, x=px, y=py, method="bilinear", flags=flags, undef=U),
             dict(family="hvector", fields=x, x=px, y=py, method="bilinear", flags=flags, undef=U, cosa=np.full(4, 0.5, np.float32),
                  sina=np.full(4, -0.25, np.float32), fdef_rot=S),
             dict(family="hremap", fields=x, table=(rowptr, col, w), mode="strict", min_frac=0.0, flags=flags, undef=U),
             dict(family="hstats", fields=x, minus=x[::-1], flags_minus=flags, pivot=np.full((2, 3), 2.0), weight=np.full((5, 6), 0.5, np.float32),
                  fdef_weight=S, box=None, mode="rows", products=3, flags=flags, undef=U)]
    for c in small:
        plain = hc.restate(c)
        with float_intermediates():
            narrow = hc.restate(c)
        assert not differs([np.asarray(a) for a in narrow], plain), c["family"]
        big = dict(c, fields=(c["fields"].astype(np.float64) * 1e38 - 3e38).astype(np.float32))
        with float_intermediates():
            narrow = hc.restate(big)
        assert differs([np.asarray(a) for a in narrow], hc.restate(big)), c["family"]


@pytest.mark.parametrize("case", [c for c in EVERY if c["klass"] == "huge"], ids=ids)
def test_a_float_intermediate_shows_in_every_huge_case(case):
    with float_intermediates():
        narrow = hc.restate(case)
    assert differs([np.asarray(a) for a in narrow], hc.expected(case)), case["label"]


def mistaken(case, name):
    return differs(hc.restate(case, mistakes=(name,)), hc.expected(case))


def test_the_mistakes_are_named_once():
    assert set(hi.MISTAKES) | set(hr.MISTAKES) | set(hs.MISTAKES) == {
        "no select", "nearest in float", "no cubic on rows", "undef after the fact", "padding added as zero", "greater in place of greater or equal",
        "masked by multiplication", "doubles flushed"}


@pytest.mark.parametrize("case", [c for c in of("hinterp") if full_grid(c)], ids=ids)
def test_hinterp_mistakes_show(case):
    if case["method"] == "nearest":
        assert mistaken(case, "nearest in float"), case["label"]
        assert not mistaken(case, "no select") and not mistaken(case, "no cubic on rows")  # (rule 4 has neither)
    else:
        assert mistaken(case, "no select"), case["label"]
        assert not mistaken(case, "nearest in float")
        assert mistaken(case, "no cubic on rows") == (case["method"] == "bicubic"), case["label"]


@pytest.mark.parametrize("case", [c for c in of("hremap") if "clean" not in c["label"]], ids=ids)
def test_hremap_mistakes_show(case):
    assert mistaken(case, "padding added as zero"), case["label"]
    tests_min_frac = case["mode"] == "renorm" and case["min_frac"] > 0 and (case["flags"] == S).any()
    assert mistaken(case, "greater in place of greater or equal") == tests_min_frac, case["label"]


@pytest.mark.parametrize("case", of("hstats"), ids=ids)
def test_hstats_mistakes_show(case):
    moments = bool(case["products"] & hs.MOMENTS)
    if moments and (case["box"] or (case["weight"] is not None and case["fdef_weight"] == S)):
        assert mistaken(case, "masked by multiplication"), case["label"]
    if case["pivot"] is not None and case["klass"] == "tiny":
        assert mistaken(case, "doubles flushed"), case["label"]
    elif case["pivot"] is None:
        assert not mistaken(case, "doubles flushed"), case["label"]  # (floats widened to double and their sums are no double denormals)


def test_a_result_taken_for_a_hole_after_the_fact_shows_in_every_family():
    clean = [c for c in EVERY if "clean" in c["label"]]
    plain = [c for c in of("hstats") if c["mode"] == "rows" and c["weight"] is None and c["pivot"] is None and c["minus"] is None]
    assert {c["family"] for c in clean} == {"hinterp", "hremap"} and plain
    for c in clean + plain:
        wrong = hc.restate(c, mistakes=("undef after the fact",))
        assert not np.array_equal(wrong[-1], hc.expected(c)[-1]), c["label"]  # the flags: the values are undef either way


# ---------------------------------------------------------------------------------------------- pins to include/mifc.h
def one_level(rows):
    return np.array(rows, np.float32)[None, None]


def test_header_hinterp_bilinear_selects_and_does_not_multiply_by_zero():
    # rule 5: r0 = a == 0 ? x00 : x00 + a * (x10 - x00); b == 0: the result is (float)r0
    f = one_level([[-0.0, np.inf, 3.0], [np.nan, U, -np.inf]])
    out, fd = hi.sample(f, [0.0, 2.0, 2.0], [0.0, 0.0, 0.5], hi.BILINEAR, [[A]])
    assert bits(out[0, 0, 0]) == bits(F(-0.0)) and out[0, 0, 1] == 3.0  # a node returns the node bit for bit, whatever lies beside it
    r0, r1 = 3.0, float("-inf")  # a == 0: r0 = x00, r1 = x01
    assert out[0, 0, 2] == F(r0 + 0.5 * (r1 - r0)) == -INF and fd[0, 0] == A
    # the same nodes under a testing flag: the corners that are not needed are not looked at
    out, fd = hi.sample(f, [0.0, 2.0], [0.0, 0.0], hi.BILINEAR, [[S]])
    assert bits(out[0, 0, 0]) == bits(F(-0.0)) and out[0, 0, 1] == 3.0 and fd[0, 0] == A


def test_header_hinterp_double_arithmetic_at_the_ends_of_the_range():
    big = float(FLT_MAX)
    f = one_level([[-FLT_MAX, FLT_MAX], [0.0, hc.TWICE_UNDEF], [np.inf, np.inf], [DEN, -DEN]])
    out, fd = hi.sample(f, [0.5, 0.5, 0.25, 0.25], [0.0, 1.0, 2.0, 3.0], hi.BILINEAR, [[S]])
    assert bits(out[0, 0, 0]) == bits(F(-big + 0.5 * (big - -big))) == 0  # FLT_MAX - -FLT_MAX is finite in double
    assert bits(out[0, 0, 1]) == bits(U) == bits(F(0.0 + 0.5 * (float(hc.TWICE_UNDEF) - 0.0)))  # a computed result equal to undef ...
    assert np.isnan(out[0, 0, 2])  # inf + 0.25 * (inf - inf)
    d = float(DEN)
    assert out[0, 0, 3] == F(d + 0.25 * (-d - d)) and bits(out[0, 0, 3]) in (bits(DEN), 0)
    assert fd[0, 0] == A  # ... and a computed NaN are not counted (rule 7)


def test_header_hinterp_nearest_adds_the_half_in_double():
    f = one_level([[1.0, 2.0, 3.0]])
    below, above = np.nextafter(F(0.5), F(0)), np.nextafter(F(1.5), F(2))
    out, _ = hi.sample(f, [below, 0.5, above, -0.0], [0.0, -0.0, 0.0, 0.0], hi.NEAREST)
    assert [int(float(v) + 0.5) for v in (below, F(0.5), above, F(-0.0))] == [0, 1, 2, 0]
    assert list(out[0, 0]) == [1.0, 2.0, 3.0, 1.0]


def test_header_hinterp_cubic_rule_on_a_row_multiplies_by_its_zero_weights():
    # rule 6 applies when a != 0 || b != 0: with b == 0 the weights of the rows are 0, 1, 0, 0 and 0 * inf is NaN
    f = np.arange(25, dtype=np.float32).reshape(1, 1, 5, 5)
    f[0, 0, 3, 2] = np.inf  # row j0 + 2
    t = 0.5
    wy = [((-0.5 * 0.0 + 1.0) * 0.0 - 0.5) * 0.0, ((1.5 * 0.0 - 2.5) * 0.0) * 0.0 + 1.0, ((-1.5 * 0.0 + 2.0) * 0.0 + 0.5) * 0.0, ((0.5 * 0.0 - 0.5) * 0.0) * 0.0]
    wx = [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t, ((0.5 * t - 0.5) * t) * t]
    assert wy == [0.0, 1.0, 0.0, 0.0] and wx == [-0.0625, 0.5625, 0.5625, -0.0625]
    s = [((wx[0] * float(f[0, 0, m, 0]) + wx[1] * float(f[0, 0, m, 1])) + wx[2] * float(f[0, 0, m, 2])) + wx[3] * float(f[0, 0, m, 3]) for m in range(4)]
    with np.errstate(invalid="ignore"):
        rc = ((np.float64(wy[0]) * s[0] + wy[1] * s[1]) + wy[2] * s[2]) + np.float64(wy[3]) * s[3]
    out, fd = hi.sample(f, [1.5], [1.0], hi.BICUBIC)
    assert np.isnan(rc) and np.isnan(out[0, 0, 0]) and fd[0, 0] == A
    out, _ = hi.sample(f, [1.5], [1.0], hi.BILINEAR)
    assert out[0, 0, 0] == 6.5
    # an overshoot: an infinity from finite inputs
    sg = np.array([-1, 1, 1, -1], np.float32)
    g = ((sg[:, None] * sg[None, :]) * FLT_MAX)[None, None]
    row = 0.0625 * float(FLT_MAX) + 0.5625 * float(FLT_MAX) + 0.5625 * float(FLT_MAX) + 0.0625 * float(FLT_MAX)
    assert row == 1.25 * float(FLT_MAX) and F(1.25 * row) == INF
    out, fd = hi.sample(g, [1.5], [1.5], hi.BICUBIC)
    assert out[0, 0, 0] == INF and fd[0, 0] == A


def test_header_hremap_sequential_double_sums():
    big = float(FLT_MAX)
    f = one_level([[FLT_MAX, 1.0, -FLT_MAX, np.inf, -0.0, hc.TWICE_UNDEF, U, 3e38]])
    rowptr = np.array([0, 3, 5, 6, 7, 8, 10, 12], np.int32)
    col = np.array([0, 1, 2, 3, 1, 4, 5, 0, 6, 1, 6, 7], np.int32)
    w = np.array([FLT_MAX, 1.0, FLT_MAX, -0.0, 1.0, 1.0, 0.5, 2.0, 0.0, 0.75, 1.0, 0.5], np.float32)
    out, fd = hr.remap(f, rowptr, col, w, hr.STRICT, 0.0, [[A]])
    assert bits(out[0, 0, 0]) == bits(F((0.0 + big * big) + 1.0 * 1.0 + big * -big)) == 0  # the 1 is lost in FLT_MAX^2, in this order
    assert np.isnan(out[0, 0, 1])  # -0 * inf
    assert bits(out[0, 0, 2]) == 0  # rule 6: -0.0 comes back as +0.0 (0.0 + 1 * -0.0)
    assert bits(out[0, 0, 3]) == bits(U) and out[0, 0, 4] == INF and fd[0, 0] == A  # computed: a value, an overflow of (float)S
    # RENORM where the level tests: rows 5 and 6 have the stored undef for a bad entry
    out, fd = hr.remap(f, rowptr, col, w, hr.RENORM, 1.0, [[S]])
    s, wdef, wall = 0.75 * 1.0, 0.75, 0.0 + 0.75
    assert abs(wdef) >= 1.0 * abs(wall) and out[0, 0, 5] == F((s / wdef) * wall) == 0.75  # equality keeps the row
    s, wdef, wall = 0.5 * float(F(3e38)), 0.5, 1.5
    assert not abs(wdef) >= 1.0 * abs(wall) and bits(out[0, 0, 6]) == bits(U)
    out, _ = hr.remap(f, rowptr, col, w, hr.RENORM, 0.25, [[S]])
    assert out[0, 0, 6] == F((s / wdef) * wall) == INF and fd[0, 0] == S


def test_header_hstats_double_denormals_and_excluded_cells():
    # rule 2 with pivot 1e-310 on eight zeros of both signs: d, q1, S1, MIN and MAX are double denormals
    f = one_level([[np.inf, 0.0, -0.0, 0.0, -0.0, np.nan], [U, -0.0, 0.0, 0.0, -0.0, -np.inf]])
    p = 1e-310
    s1 = 0.0
    for x in (0.0, -0.0, 0.0, -0.0, -0.0, 0.0, 0.0, -0.0):
        s1 = s1 + 1.0 * (x - p)
    assert s1 == -8e-310
    stats, mean, fd = hs.hstats(f, pivot=[[p]], box=(1, 5, 0, 2), flags=[[A]])
    assert list(stats[0, 0, 0]) == [8.0, 8.0, s1, 0.0, -p, -p, 1.0, 1.0]  # q2 = (-1e-310)^2 underflows; the first cell of the box wins the tie
    assert bits(mean[0, 0, 0]) == bits(F(p + s1 / 8.0)) == 0 and fd[0, 0] == A
    lit = hs.hstats_literal(f, pivot=[[p]], box=(1, 5, 0, 2), flags=[[A]])
    assert hs.same_bits64(lit[0], stats)
    # q2 is inf in double at pivot 1e200; an infinite pivot gives d = -inf and a NaN mean (inf + -inf), which is not a hole
    stats, mean, fd = hs.hstats(f, pivot=[[1e200]], box=(1, 5, 0, 2), flags=[[A]])
    assert stats[0, 0, 0, hs.S1] == -8e200 and stats[0, 0, 0, hs.S2] == np.inf and mean[0, 0, 0] == 0.0
    stats, mean, fd = hs.hstats(f, pivot=[[np.inf]], box=(1, 5, 0, 2), flags=[[A]])
    assert stats[0, 0, 0, hs.S1] == -np.inf and np.isnan(mean[0, 0, 0]) and fd[0, 0] == A
    # -inf < +inf: the first cell is the minimum; -inf > -inf is false: a d equal to the starting infinity is never selected
    assert list(stats[0, 0, 0, hs.MIN:]) == [-np.inf, -np.inf, 1.0, -1.0]


def test_header_hstats_a_mean_equal_to_undef_and_cancelling_weights():
    f = one_level([[U, U, U], [1.0, 2.0, np.inf]])
    stats, mean, fd = hs.hstats(f, mode=hs.ROWS, flags=[[A]])
    assert float(U) + float(U) + float(U) == 3 * float(U)
    assert stats[0, 0, 0, hs.N] == 3 and bits(mean[0, 0, 0]) == bits(U) and mean[0, 0, 1] == INF and fd[0, 0] == A
    w = np.array([[1.0, -1.0, U], [0.5, -0.0, U]], np.float32)
    stats, mean, fd = hs.hstats(f, mode=hs.ROWS, weight=w, flags=[[A]])  # the inf sits under an undefined weight
    assert list(stats[0, 0, :, hs.N]) == [2, 2] and list(stats[0, 0, :, hs.W]) == [0.0, 0.5]
    assert bits(mean[0, 0, 0]) == bits(U) and mean[0, 0, 1] == F(0.0 + (0.5 * 1.0 + -0.0 * 2.0) / 0.5) == 1.0 and fd[0, 0] == S
