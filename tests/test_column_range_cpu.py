"""The range cases of the column-walk families (tests/column_range_cases.py) on the CPU: every case goes through the numpy
restatements and must not have degraded into comparing NaN with NaN or undef with undef; the cases must tell three
plausible wrong kernels from the definition, and the seam cases of vinterp a wave filter whose integer keys part from the
float compare (on a model of that filter); and a handful of hand-computed columns pin the restatements themselves to the
sentences of include/mifc.h that the cases are about.

The conditions are the generator's contract, not measurements: its rates and decades are tuned until they hold.

One condition has an exemption that follows from the arithmetic: a `huge` vinterp case cannot produce an infinity from
finite inputs.  Its result is (float)(x_k + w * (x_k+1 - x_k)) with 0 <= w <= 1 (the target lies in the bracket; the
quotient of two doubles of which the numerator is the smaller one in magnitude does not round above 1), so it lies
between the two finite floats x_k and x_k+1 up to one rounding in double, which the rounding to float cannot carry past
FLT_MAX.  For vinterp the overflow is in the intermediate x_k+1 - x_k, which leaves the float range and not the double
one: the float-intermediate variant below shows that the cases see it."""
import contextlib

import numpy as np
import pytest

import column_range_cases as cr
import pvort_restate as pv
import vcumul_restate as vc
import vderiv_restate as vd
import vinterp_restate as vi
import vlayer_restate as vl

A, N, S = cr.ALL_DEFINED, cr.NONE_DEFINED, cr.SOME_DEFINED
U = cr.UNDEF
F = np.float32
FLT_MAX, FLT_MIN, DEN = cr.FLT_MAX, cr.FLT_MIN, cr.DENORM_MIN
INF = F(np.inf)
GROUPS = [(family, klass) for family in cr.FAMILIES for klass in cr.CLASSES]


def is_undef(out, undef):
    return np.isnan(out) if np.isnan(undef) else out == F(undef)


def finite_inputs(case):
    """bool, broadcastable to the outputs: every input the output can depend on is finite (an undef of 1e35 is).  The
    extras at the cell; the fields and the coordinate down the whole column (vinterp, vlayer), at the level and its two
    neighbours (vderiv, pvort: and there at the eight cells around it) or at the levels walked so far (vcumul)."""
    family, f = case["family"], case["fields"]
    nlev = f.shape[1]
    c, _ = cr.coordinate_of(case)
    lev = np.isfinite(f).all(axis=0) & np.isfinite(c)  # (nlev, ny, nx)
    cell = np.ones(f.shape[2:], bool)
    for k, v in case["extras"].items():
        for a in (v if k == "base" else [v]):
            if isinstance(a, np.ndarray) and a.ndim == 2:
                cell &= np.isfinite(a)
    if family in ("vinterp", "vlayer"):
        return (lev.all(axis=0) & cell)[None, None]
    if family == "vcumul":
        order = slice(None) if case["extras"]["from_"] == "first" else slice(None, None, -1)
        walked = np.zeros_like(lev)
        walked[order] = np.logical_and.accumulate(lev[order], axis=0)
        return (walked & cell)[None]
    near = lev.copy()
    near[1:] &= lev[:-1]
    near[:-1] &= lev[1:]
    near &= cell
    if family == "vderiv":
        return near[None]
    ny, nx = cell.shape
    pad = np.zeros((nlev, ny + 2, nx + 2), bool)
    pad[:, 1:-1, 1:-1] = near
    ok = np.logical_and.reduce([pad[:, 1 + dy:ny + 1 + dy, 1 + dx:nx + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    yc, xc = np.clip(np.arange(ny), 1, ny - 2), np.clip(np.arange(nx), 1, nx - 2)
    return ok[:, yc][:, :, xc]  # a ring cell is a copy of the interior cell next to it


def shares(case):
    """The shares of all outputs that are NaN (and not undef), finite and not undef, +-inf from finite inputs, finite
    above 1e37 in magnitude, subnormal."""
    out, fd = cr.expected(case)
    und = is_undef(out, case["undef"])
    nan = np.isnan(out) & ~und
    fin = np.isfinite(out) & ~und
    with np.errstate(invalid="ignore"):
        inf = np.isinf(out) & finite_inputs(case)
        if case["family"] == "vinterp":
            inf &= np.isfinite(case["extras"]["targets"]).reshape(1, -1, 1, 1)
        big = fin & (np.abs(out) > 1e37)
        sub = fin & (out != 0) & (np.abs(out) < FLT_MIN)
    return dict(nan=nan.mean(), finite=fin.mean(), inf=inf.mean(), big=big.mean(), subnormal=sub.mean(), all_inf=np.isinf(out).mean())


@pytest.mark.parametrize("family,klass", GROUPS)
def test_cases_reach_what_they_are_meant_to_reach(family, klass):
    for case in cr.cases(family, klass):
        s = shares(case)
        print("%-60s %s" % (case["label"], "  ".join("%s %.1f %%" % (k, 100 * v) for k, v in s.items())))
        assert s["nan"] <= 0.10, (case["label"], s)
        assert s["finite"] >= 0.30, (case["label"], s)
        if klass == "huge":
            assert s["big"] >= 0.01, (case["label"], s)
            if family != "vinterp":  # see the module docstring
                assert s["inf"] >= 0.01, (case["label"], s)
        if klass == "tiny":
            assert s["subnormal"] >= 0.05, (case["label"], s)


def test_the_shapes_and_ingredients_of_the_cases():
    for family in cr.FAMILIES:
        mine = [c for klass in cr.CLASSES for c in cr.cases(family, klass)]
        shapes = {c["fields"].shape[1:] for c in mine}
        assert {(cr.NLEV, 9, 68), (cr.NLEV, 9, 67)} <= shapes and any(s[0] == cr.MIN_NLEV[family] for s in shapes), family
        assert {c["kind"] for c in mine} == ({"hybrid", "field"} if family in ("vinterp", "vlayer") else {"hybrid", "field", "levels"}), family
        assert any(np.isnan(c["undef"]) for c in mine) and any(c["label"].endswith("overflow-68x9x7") for c in mine), family
        for c in mine:
            fl = c["flags"]
            assert set(np.unique(fl)) == {A, S}, c["label"]
            x = c["fields"]
            on_all = np.broadcast_to((fl == A)[:, :, None, None], x.shape)
            if x.shape[1] == cr.NLEV:
                assert (x[on_all] == U).any() and np.isnan(x[on_all]).any(), c["label"]  # values there
                for v in (0.0, DEN, FLT_MIN, F(3e38), INF, cr.UNDEF_BELOW, cr.UNDEF_ABOVE):
                    assert (x == F(v)).any(), (c["label"], v)
                assert (np.signbit(x) & (x == 0)).any(), c["label"]
            if family == "vinterp":
                assert c["extras"]["targets"].size <= 16
    # the overflow variant: a finite ps whose coordinate is infinite
    c = [c for c in cr.cases("vderiv", "mid") if "overflow" in c["label"]][0]
    coord, _ = cr.coordinate_of(c)
    assert (np.isinf(coord) & np.isfinite(c["ps"])).any() and (np.isnan(coord[0]) & np.isinf(c["ps"])).any()  # and 0 * inf on level 0


def test_every_vderiv_branch_and_every_output_flag_occurs():
    for klass in cr.CLASSES:
        seen = set()
        for c in cr.cases("vderiv", klass):
            br = np.zeros(c["fields"].shape, np.int64)
            cr.restate(c, dict(vderiv=_Branches(br)))
            mine = set(np.unique(br).tolist())
            if c["kind"] == "field" and c["fields"].shape[1] == cr.NLEV:
                assert mine == set(range(len(vd.BRANCH_NAMES))), (c["label"], [vd.BRANCH_NAMES[b] for b in sorted(mine)])
            seen |= mine
        assert seen == set(range(len(vd.BRANCH_NAMES))), klass
    flags = set()
    for c in cr.all_cases():
        flags |= set(np.unique(cr.expected(c)[1]).tolist())
    assert flags == {A, N, S}


class _Branches:
    """vderiv_restate with the branches of every output written into `br`."""

    def __init__(self, br):
        self.br = br

    def hlevels(self, *a):
        return vd.hlevels(*a, branches=self.br)

    def coord_fields(self, *a):
        return vd.coord_fields(*a, branches=self.br)

    def levels(self, *a):
        return vd.levels(*a, branches=self.br)


# ---------------------------------------------------------------------------------------------- the cases discriminate
def differs(a, b):
    """Some output differs in bits (a NaN matches any NaN), or some flag does."""
    (x, fx), (y, fy) = a, b
    return bool(((x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))).any()) or not np.array_equal(fx, fy)


def flushed(a):
    """Subnormal floats replaced by zeros of their sign, as a code object built with denormals flushed would read and
    write them."""
    if isinstance(a, (list, tuple)):
        return type(a)(flushed(v) for v in a)
    if not isinstance(a, np.ndarray) or a.dtype != np.float32:
        return a
    with np.errstate(invalid="ignore"):
        return np.where((a != 0) & (np.abs(a) < FLT_MIN), np.copysign(F(0), a), a).astype(np.float32)


def restate_flushing(case):
    c = {k: flushed(v) for k, v in case.items()}
    c["extras"] = {k: flushed(v) for k, v in case["extras"].items()}
    out, fd = cr.restate(c)
    return flushed(out), fd


@pytest.mark.parametrize("family", cr.FAMILIES)
def test_a_flush_to_zero_shows_in_every_tiny_case(family):
    for case in cr.cases(family, "tiny"):
        assert differs(restate_flushing(case), cr.expected(case)), case["label"]


class _Narrow(np.ndarray):
    """An array whose double differences, sums and products are rounded to float: what a kernel computes that keeps an
    intermediate in a float register.  Everything derived from it by a ufunc is one too."""

    def __array_ufunc__(self, ufunc, method, *inputs, **kw):
        args = [np.asarray(a) if isinstance(a, _Narrow) else a for a in inputs]
        if "out" in kw:
            kw["out"] = tuple(np.asarray(o) if isinstance(o, _Narrow) else o for o in kw["out"])
        r = getattr(ufunc, method)(*args, **kw)
        if isinstance(r, np.ndarray):
            if r.dtype == np.float64 and ufunc in (np.subtract, np.add, np.multiply):
                with np.errstate(all="ignore"):
                    r = r.astype(np.float32).astype(np.float64)
            r = r.view(_Narrow)
        return r


class _NarrowNumpy:
    """numpy, except that asarray hands out _Narrow arrays: put in the place of a restatement's `np`, the fields and
    the coordinate it converts carry the float rounding through its arithmetic."""

    def __getattr__(self, name):
        return getattr(np, name)

    def asarray(self, a, dtype=None):
        return np.asarray(a, dtype).view(_Narrow)

    def where(self, *a):  # a selection among narrowed values is one
        r = np.where(*a)
        return r.view(_Narrow) if isinstance(r, np.ndarray) else r


@contextlib.contextmanager
def float_intermediates():
    mods = (vi, vl, vd, vc, pv)
    try:
        for m in mods:
            m.np = _NarrowNumpy()
        yield
    finally:
        for m in mods:
            m.np = np


@pytest.mark.parametrize("family", cr.FAMILIES)
def test_the_narrowing_variant_is_the_restatement_where_nothing_leaves_the_float_range(family):
    """On small integers over unit spacings every difference, sum and product is exact in float (the weights are 0.5 and
    1): the variant and the restatement of every family agree, so what the next test sees is the rounding and nothing
    else -- and a restatement that converts its inputs in a way the variant does not follow fails here, with an error or a
    difference on the second case below, not silently."""
    nlev, ny, nx = 4, 3, 5
    x = (np.arange(3 * nlev * ny * nx, dtype=np.float32).reshape(3, nlev, ny, nx) * 5) % 7
    case = dict(label=family + "-exact", family=family, kind="field", klass="mid", undef=U, method=None, fields=x[:2],
                flags=np.full((3 if family == "pvort" else 2, nlev), S, np.int32), fdef_c=np.full(nlev, S, np.int32),
                coord=np.broadcast_to(np.arange(nlev, dtype=np.float32).reshape(nlev, 1, 1), (nlev, ny, nx)).copy(), extras={})
    if family == "vinterp":
        case.update(method="linear", extras=dict(targets=np.array([0.5, 1.5, 2.0], np.float32)))
    elif family == "vlayer":
        case["extras"] = dict(lo=F(0.5), hi=F(2.5))
    elif family == "vderiv":
        case["method"] = "weighted"
    elif family == "vcumul":
        case.update(method="linear", extras=dict(from_="last"))
    else:
        one = np.ones((ny, nx), np.float32)
        case.update(method="centred", fields=x, extras=dict(xmapr=2 * one, ymapr=2 * one, fcoriolis=one, scale=1.0))
    plain = cr.restate(case)
    with float_intermediates():
        narrow = cr.restate(case)
    assert np.isfinite(plain[0]).all() and not differs((np.asarray(narrow[0]), narrow[1]), plain), family
    # and the narrowing does reach this family's arithmetic: the same problem with fields of -3e38 .. 3e38 comes out different
    big = dict(case, fields=(case["fields"].astype(np.float64) * 1e38 - 3e38).astype(np.float32))
    with float_intermediates():
        narrow = cr.restate(big)
    assert differs((np.asarray(narrow[0]), narrow[1]), cr.restate(big)), family


@pytest.mark.parametrize("family", cr.FAMILIES)
def test_a_float_intermediate_shows_in_every_huge_case(family):
    for case in cr.cases(family, "huge"):
        with float_intermediates():
            out, fd = cr.restate(case)
        assert differs((np.asarray(out), fd), cr.expected(case)), case["label"]


def restate_dropping_small_targets(case):
    """The vinterp bracket test with the targets dropped for which an integer key compare and the float compare could
    part: +-0 (two keys for one value unless -0 is folded) and the subnormals (zeros to a flushing compare).  They are
    reported as not found."""
    out, fd = (a.copy() for a in cr.restate(case))
    t = case["extras"]["targets"]
    small = np.abs(t) < FLT_MIN
    out[:, small] = case["undef"]
    fd[:, small] = N
    return out, fd


def test_a_bracket_that_loses_zero_and_subnormal_targets_shows_in_every_vinterp_case():
    n = 0
    for klass in cr.CLASSES:
        for case in cr.cases("vinterp", klass):
            assert differs(restate_dropping_small_targets(case), cr.expected(case)), case["label"]
            n += 1
    assert n >= 15


# ---------------------------------------------------------------------------------------------- the wave filter of vinterp
def _key(x):
    """vinterp_key (csrc/mifc_kernels.h) of float32 values: integers in the order of the floats, -0 below +0."""
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7fffffff, b)


def _unkey(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 0, k ^ 0x7fffffff, k).astype(np.int32).view(np.float32)


def wave_filter(case, v, device_fold=True, host_fold=True, flush=False):
    """A model of the pre-filter of vinterp_kernel (csrc/mifc_vinterp.hip) as prefilter(k, t) of vinterp_restate: per wave
    of 64 lanes with v cells each, the minimum and the maximum of the pair (k, k + 1) over the wave's cells (a cell without a
    usable pair counts as the empty interval; the idle lanes of the last wave walk cells 0 .. v - 1), both `+ 0.f` and turned
    into keys; target t is looked at where its key, of `ct + 0.f` as the host makes it, lies between them.  device_fold /
    host_fold = False leave a `+ 0.f` out, flush = True lets the reduction flush a subnormal end to zero."""
    c, usable = cr.coordinate_of(case)
    nlev = c.shape[0]
    c = np.where(usable, c, F(np.nan)).reshape(nlev, -1)
    n = c.shape[1]
    t = case["extras"]["targets"]
    tkey = _key(t + F(0) if host_fold else t)
    per_wave = 64 * v
    first = np.arange(0, n, per_wave)
    allowed = np.zeros((nlev - 1, t.size, n), bool)

    def end(keys):
        x = _unkey(keys)
        if flush:
            x = np.where((x != 0) & (np.abs(x) < FLT_MIN), np.copysign(F(0), x), x).astype(np.float32)
        return _key(x + F(0) if device_fold else x)

    for k in range(nlev - 1):
        pair = ~(np.isnan(c[k]) | np.isnan(c[k + 1]))
        ka, kb = _key(c[k]), _key(c[k + 1])
        lo = np.where(pair, np.minimum(ka, kb), _key(INF))
        hi = np.where(pair, np.maximum(ka, kb), _key(-INF))
        wlo, whi = np.minimum.reduceat(lo, first), np.maximum.reduceat(hi, first)
        if n % per_wave:  # the idle lanes
            wlo[-1], whi[-1] = min(wlo[-1], lo[:v].min()), max(whi[-1], hi[:v].max())
        wlo, whi = np.repeat(end(wlo), per_wave)[:n], np.repeat(end(whi), per_wave)[:n]
        allowed[k] = (tkey[:, None] >= wlo[None]) & (tkey[:, None] <= whi[None])
    return lambda k, t: allowed[k, t]


BROKEN_FILTERS = {"the device without its + 0.f": dict(device_fold=False), "the host without its + 0.f": dict(host_fold=False),
                  "a reduction that flushes subnormals": dict(flush=True)}


def test_the_wave_filter_as_the_kernel_has_it_changes_nothing():
    """The model with both folds and no flush rejects no pair that a cell brackets: on every vinterp case and in both wave
    layouts the filtered restatement is the restatement.  What the next test sees is the broken filter and nothing else."""
    mine = [c for klass in cr.CLASSES for c in cr.cases("vinterp", klass)] + cr.vinterp_seam_cases()
    for case in mine:
        for v in (4, 1):
            assert not differs(cr.restate(case, prefilter=wave_filter(case, v)), cr.expected(case)), (case["label"], v)


def test_a_wave_filter_that_parts_from_the_float_compare_shows_in_every_seam_case():
    """Each of the three ways in which the integer keys of the wave and the float compare of the cell can part -- the
    device's or the host's `+ 0.f` missing, a flush in the fminf / fmaxf reduction -- changes at least one output of every
    seam case, in the layout of four cells per lane (256 cells per wave) and of one (64).  The LOG cases have no zero among
    their coordinates or targets: there only the flush can show."""
    for case in cr.vinterp_seam_cases():
        for v in (4, 1):
            for name, how in BROKEN_FILTERS.items():
                if case["method"] == "log" and "flush" not in name:
                    continue
                assert differs(cr.restate(case, prefilter=wave_filter(case, v, **how)), cr.expected(case)), (case["label"], v, name)


def test_the_seam_cases_bracket_first_on_the_pairs_they_are_about():
    """In every block a whole wave's worth of cells finds the end targets of its pair with a defined result."""
    for case in cr.vinterp_seam_cases():
        out, fd = cr.expected(case)
        found = (out[0] != U).reshape(out.shape[1], -1)  # (nt, cells)
        t = case["extras"]["targets"]
        ends = (np.abs(t) <= 2 * DEN) | (np.abs(t) >= FLT_MAX)  # the targets that are an end of some pair
        for b in range(3):
            cells = slice(b * cr.SEAM_BLOCK, min((b + 1) * cr.SEAM_BLOCK, found.shape[1]))
            assert found[ends][:, cells].mean(axis=1).max() > 0.8, (case["label"], b)
        assert (fd == S).any()


def test_a_target_is_bit_equal_to_a_usable_coordinate_in_every_vinterp_case():
    for klass in cr.CLASSES:
        for case in cr.cases("vinterp", klass):
            c, usable = cr.coordinate_of(case)
            bits = set(case["extras"]["targets"].view(np.uint32).tolist())
            assert np.isin(c[usable & np.isfinite(c)].view(np.uint32), list(bits)).any(), case["label"]


# ---------------------------------------------------------------------------------------------- the header, by hand
def column(*levels):
    """Values down one column as a (1, nlev, 1, 1) field batch."""
    return np.array(levels, np.float32).reshape(1, -1, 1, 1)


def coord(*levels):
    return np.array(levels, np.float32).reshape(-1, 1, 1)


def test_header_vderiv_a_computed_nan_or_infinity_is_a_value():
    """Rule 7 of mifc_vderiv_*: "The result is (float)r.  A computed NaN or infinity is a value: not undef, not counted." """
    out, fd = vd.coord_fields(column(-3e38, 3e38), coord(0, 1))[:2]  # (3e38 - -3e38) * (1 / 1) = 6e38 in double
    assert np.isposinf(out).all() and (fd == A).all()
    out, fd = vd.coord_fields(column(np.inf, np.inf, 1), coord(0, 1, 2), flags=[[A, A, A]])[:2]
    assert np.isnan(out[0, 0]) and np.isneginf(out[0, 1]) and np.isneginf(out[0, 2]) and (fd == A).all()  # inf - inf; (1 - inf) * (1 / 2)
    # a subnormal input and a subnormal result, exact: (2^-149 - 0) * (1 / 0.5) = 2^-148; a spacing of one subnormal:
    # 1 * (1 / 2^-149) = 2^149 in double, infinity in float
    out, fd = vd.coord_fields(column(0, DEN), coord(0, 0.5))[:2]
    assert (out == F(2.0) ** F(-148)).all() and (out != 0).all()
    out, fd = vd.coord_fields(column(0, 1, 5), coord(-0.0, DEN, DEN))[:2]  # level 2 has no side: c_2 == c_1
    assert np.isposinf(out[0, :2]).all() and out[0, 2] == U and list(fd[0]) == [A, A, N]
    # 0 * inf comes from an infinite coordinate: (x_1 - x_0) * (1 / inf) is 0 for finite values, NaN for an infinite difference
    out, fd = vd.levels(column(1, 2, -np.inf), [0, np.inf, 1], flags=[[A, A, A]])[:2]
    assert out[0, 0, 0, 0] == 0 and np.isnan(out[0, 2, 0, 0]) and (fd == A).all()


def test_header_is_defined_at_the_floats_next_to_undef_and_under_all_defined():
    """Rule 2 of mifc_vderiv_* / rule 3 of mifc_vinterp_*: is_defined(flag == ALL_DEFINED, x, undef); a stored undef or NaN
    under ALL_DEFINED is a value, the floats next to undef are values under any flag."""
    x = column(cr.UNDEF_BELOW, cr.UNDEF_ABOVE)
    out, fd = vd.coord_fields(x, coord(0, 2))[:2]
    r = F((np.float64(cr.UNDEF_ABOVE) - np.float64(cr.UNDEF_BELOW)) * 0.5)
    assert (out == r).all() and r > 0 and (fd == A).all()
    out, fd = vd.coord_fields(column(U, 0), coord(0, 2))[:2]
    assert (out == U).all() and (fd == N).all()
    out, fd = vd.coord_fields(column(U, 0), coord(0, 2), flags=[[A, S]])[:2]
    assert (out == F(-0.5e35)).all() and (fd == A).all()
    out, fd = vd.coord_fields(column(np.nan, 0), coord(0, 2), flags=[[A, S]])[:2]
    assert np.isnan(out).all() and (fd == A).all()
    out, fd = vi.coord_fields(column(1, 3), coord(U, 0).reshape(2, 1, 1), [0.5e35], vi.LINEAR, fdef_coord=[A, S])
    assert out[0, 0, 0, 0] == 2 and fd[0, 0] == A  # a stored 1e35 coordinate under ALL_DEFINED brackets
    out, fd = vi.coord_fields(column(1, 3), coord(U, 0).reshape(2, 1, 1), [0.5e35], vi.LINEAR)
    assert out[0, 0, 0, 0] == U and fd[0, 0] == N


def test_header_vinterp_bracket_at_the_ends_of_the_range():
    """Rule 2 of mifc_vinterp_*: min(c_k, c_k+1) <= ct <= max(c_k, c_k+1) in float; "A NaN coordinate (which can only get
    in through an ALL_DEFINED flag) fails both comparisons and never brackets"; rule 5: c_k == c_k+1: x_k bit for bit."""
    x = column(1, 3)
    for c, t, want in (((-0.0, DEN), 0.0, 1), ((0.0, DEN), -0.0, 1), ((-DEN, 0.0), -0.0, 3), ((-DEN, DEN), 0.0, 2), ((0.0, -0.0), 0.0, 1),
                       ((0.0, -0.0), -0.0, 1), ((-FLT_MAX, FLT_MAX), FLT_MAX, 3), ((-np.inf, np.inf), -np.inf, None), ((1, np.inf), np.inf, None),
                       ((np.inf, np.inf), np.inf, 1), ((-np.inf, 0), -FLT_MAX, None), ((DEN, 2 * float(DEN)), DEN, 1), ((0, DEN), -DEN, U),
                       ((np.nan, 1), 1.0, U), ((1, np.nan), 1.0, U), ((FLT_MAX, np.inf), -np.inf, U)):
        out, fd = vi.coord_fields(x, coord(*c), [t], vi.LINEAR, fdef_coord=[A, A])
        got = out[0, 0, 0, 0]
        if want is None:  # (ct - c_k) / (c_k+1 - c_k) is inf / inf or (-inf - -inf) / ...: found, and a NaN that is a value
            assert np.isnan(got) and fd[0, 0] == A, (c, t, got)
        else:
            assert got == F(want) and fd[0, 0] == (N if want == U else A), (c, t, got)


def test_header_vlayer_a_computed_nan_or_infinity_is_not_counted():
    """Rule 7 of mifc_vlayer_*: "A computed NaN or infinity is not counted"; rule 6: the extremes are a level's value."""
    out, fd = vl.coord_fields(column(3e38, 3e38), coord(0, 4), vl.ALL_PRODUCTS)
    integral, mean, mx, mn, cmx, cmn = out[0, :, 0, 0]
    assert np.isposinf(integral) and mean == F(3e38) and mx == mn == F(3e38) and cmx == cmn == 0 and (fd == A).all()  # 1.2e39 in double
    out, fd = vl.coord_fields(column(np.inf, -np.inf), coord(0, 4), vl.ALL_PRODUCTS, flags=[[A, A]])
    assert np.isnan(out[0, :2, 0, 0]).all() and np.isposinf(out[0, 2, 0, 0]) and np.isneginf(out[0, 3, 0, 0]) and (fd == A).all()
    # a layer of one subnormal: (-0.0, 2^-149) is a layer since -0.0 < 2^-149; the integral 2 * 2^-149 is exact
    out, fd = vl.coord_fields(column(2, 2), coord(-1, 1), [vl.INTEGRAL, vl.MEAN], F(-0.0), DEN)
    assert out[0, 0, 0, 0] == 2 * DEN and out[0, 1, 0, 0] == 2 and (fd == A).all()


def test_header_vcumul_a_computed_nan_or_infinity_is_a_value():
    """Rule 7 of mifc_vcumul_*: "A computed NaN or infinity is a value: not undef, not counted." """
    out, fd = vc.coord_fields(column(3e38, 3e38, -3e38), coord(0, 2, 4))
    assert list(out[0, :, 0, 0]) == [0, INF, INF] and (fd == A).all()  # S stays 6e38 in double: (3e38 - 3e38) * 0.5 * 2 adds zero
    out, fd = vc.coord_fields(column(1, 1, 1), coord(0, np.inf, np.inf))
    assert out[0, 0, 0, 0] == 0 and np.isposinf(out[0, 1, 0, 0]) and np.isnan(out[0, 2, 0, 0]) and (fd == A).all()  # inf + 1 * (inf - inf)
    out, fd = vc.coord_fields(column(DEN, DEN), coord(0, 1))  # a subnormal result, exact
    assert out[0, 1, 0, 0] == DEN
    out, fd = vc.levels(column(1, 1), [DEN, FLT_MAX], vc.LOG)  # ln FLT_MAX - ln 2^-149
    assert out[0, 1, 0, 0] == F(np.log(np.float64(FLT_MAX)) - np.log(np.float64(DEN))) and (fd == A).all()


def test_header_pvort_a_computed_nan_or_infinity_is_a_value():
    """Rule 5 of mifc_pvort_*: "(float)(scale * S).  A computed NaN or infinity is a value: not undef, not counted." """
    z = np.zeros((2, 3, 3), np.float32)
    th = np.stack([np.full((3, 3), -3e38, np.float32), np.full((3, 3), 3e38, np.float32)])
    m = np.zeros((3, 3), np.float32)
    f = np.full((3, 3), 0.75, np.float32)
    out, fd = pv.coord_fields(z, z, th, np.broadcast_to(coord(0, 1), (2, 3, 3)), m, m, f)  # za = 0.75, D_th = 6e38: 4.5e38
    assert np.isposinf(out).all() and (fd == A).all()
    out, fd = pv.coord_fields(z, z, th, np.broadcast_to(coord(0, 1), (2, 3, 3)), m, m, f, scale=0.5)  # the double S is finite
    assert (out == F(0.5 * (0.75 * 6e38))).all() and (fd == A).all()
    out, fd = pv.coord_fields(z, z, th, np.broadcast_to(coord(0, 1), (2, 3, 3)), m, m, np.full((3, 3), np.inf, np.float32), scale=0.0)
    assert np.isnan(out).all() and (fd == A).all()  # 0 * inf


def test_header_hybrid_coordinate_in_float():
    """Rule 1 of mifc_vinterp_*: "float product, then float sum"; the coordinate is defined where ps is, whatever its value:
    one that overflows is +inf, 0 * inf is a NaN that is not usable (rule 1 of mifc_vderiv_*)."""
    a, b = np.array([1e38, 2e38, 1.0], np.float32), np.array([0.0, 0.75, 1.0], np.float32)
    ps = np.array([[3e38, np.inf, DEN]], np.float32)
    c = vi.hybrid_coordinate(ps, a, b)
    assert c[0, 0, 0] == F(1e38) and np.isposinf(c[1, 0, 0]) and c[2, 0, 0] == F(3e38)  # 2e38 + 2.25e38 leaves the float range
    assert np.isnan(c[0, 0, 1]) and np.isposinf(c[1:, 0, 1]).all()
    assert c[1, 0, 2] == F(2e38) and c[2, 0, 2] == 1  # the subnormal product is absorbed by alevel
    x = np.arange(9, dtype=np.float32).reshape(1, 3, 1, 3)
    out, fd = vd.hlevels(x, ps, a, b)[:2]
    # cell 1: level 0 is NaN (not usable), levels 1 and 2 are both +inf: equal, so no side takes part anywhere
    assert (out[0, :, 0, 1] == U).all() and list(fd[0]) == [S, S, S]
    # cell 0: level 1 is +inf: (x_1 - x_0) * (1 / inf) = 0, and level 1 between 1e38 and 3e38 takes both sides
    assert out[0, 0, 0, 0] == 0 and out[0, 1, 0, 0] == F((6.0 - 0.0) * (1.0 / (np.float64(F(3e38)) - np.float64(F(1e38)))))


def test_header_levels_form_is_the_field_form():
    """mifc_vderiv_levels: "c_k = levels[k], always defined": the same rules on a constant coordinate, the weights included."""
    for klass in cr.CLASSES:
        for family in ("vderiv", "vcumul", "pvort"):
            for c in cr.cases(family, klass):
                if c["kind"] == "levels":
                    assert not differs(cr.restate(cr.as_field(c)), cr.expected(c)), c["label"]


def test_hybrid_form_is_the_field_form_of_its_coordinate():
    for c in cr.all_cases():
        if c["kind"] == "hybrid":
            assert not differs(cr.restate(cr.as_field(c)), cr.expected(c)), c["label"]
