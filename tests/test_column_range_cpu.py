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
import vregrid_restate as vg
from test_vregrid_cpu import header_run, shim  # noqa: F401  (the rules header of vregrid through the host compiler)

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
    if family == "vregrid":
        return (lev.all(axis=0) & cell)[None, None] & np.isfinite(case["extras"]["tcoord"])[None]
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
            if family not in ("vinterp", "vregrid"):  # see the module docstring (vregrid: the same result, or a copy of a level)
                assert s["inf"] >= 0.01, (case["label"], s)
        if klass == "tiny":
            assert s["subnormal"] >= 0.05, (case["label"], s)
        if family == "vregrid":  # at most half holes
            out, _ = cr.expected(case)
            assert is_undef(out, case["undef"]).mean() <= 0.5, case["label"]


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
    mods = (vi, vl, vd, vc, pv, vg)
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
    elif family == "vregrid":
        planes = np.broadcast_to(np.array([0.5, 1.5, 2.0], np.float32).reshape(3, 1, 1), (3, ny, nx)).copy()
        case.update(method="linear", extras=dict(tcoord=planes, fdef_t=np.full(3, S, np.int32), method="linear", from_="last", outside="clamp"))
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


# ---------------------------------------------------------------------------------------------- vregrid: targets, interval, clamp
def vregrid_bases():
    """One case per base (set of arrays): its first combination."""
    seen = {}
    for klass in cr.CLASSES:
        for case in cr.cases("vregrid", klass):
            seen.setdefault(case["base"], case)
    return list(seen.values())


def test_vregrid_every_kind_of_target_is_in_every_base_and_every_combination_is_run():
    bases = vregrid_bases()
    assert len(bases) == 7 * 3 + 2
    for case in bases:
        ex, label = case["extras"], case["base"]
        t, what = ex["tcoord"], case["tkind"]
        log = case["method"] == "log"
        c, usable = cr.coordinate_of(case)
        usable = usable & ~np.isnan(c)
        assert all((what == j).mean() > 0.02 for j in range(len(cr.TARGET_KINDS))), label
        assert set(np.unique(ex["fdef_t"])) == {A, S}, label
        for flag in (A, S):  # a stored 1e35 under both flag values
            assert (t[ex["fdef_t"] == flag] == U).any(), label
        with np.errstate(invalid="ignore"):
            # on a level: bit for bit; and some column has c_k == c_k+1 with a target on it
            on = what == 0
            assert (np.isin(t.view(np.uint32), c[usable].view(np.uint32)) & on).mean() > 0.1, label
            equal = usable[:-1] & usable[1:] & (c[:-1] == c[1:])
            assert equal.any() or log or case["kind"] == "hybrid", label  # (the LOG rule and the hybrid levels draw no equal neighbours)
            assert ((t[:, None] == c[None, :-1]) & equal[None]).any() or equal.mean() < 0.002, label
            # beyond both extremes of the column
            cmin, cmax = np.where(usable, c, INF).min(axis=0), np.where(usable, c, -INF).max(axis=0)
            assert ((t < cmin) & (what == 2)).mean() > 0.02 and ((t > cmax) & (what == 2)).mean() > (-1 if "levels-log" in label else 0.02), label  # (LEVELS_LOG ends on +inf)
            for v in (0.0, DEN, -DEN, FLT_MAX, -FLT_MAX, INF, -INF, cr.UNDEF_BELOW, cr.UNDEF_ABOVE):
                assert (t == F(v)).any(), (label, v)
            assert np.isnan(t).any() and (np.signbit(t) & (t == 0)).any(), label
            if log:
                assert (t == F(-1.5)).any() and ((t <= 0) & (what != 4)).mean() < 0.25, label  # (half of 2^-149, below LEVELS_LOG, is 0)
        combos = {(c2["extras"]["method"], c2["extras"]["from_"], c2["extras"]["outside"]) for klass in cr.CLASSES for c2 in cr.cases("vregrid", klass) if c2["base"] == label}
        nlev = case["fields"].shape[1]
        assert combos == {cb for cb in cr.VREGRID_COMBOS if log or cb[0] == "linear" or cr.log_runs_on_a_linear_base(case["kind"], nlev, cb[2])}, label
        # LOG on a base of the LINEAR rule is left out exactly where more than half of its outputs would be holes (its
        # coordinates cross zero): the combinations that run are held to a half by the test above, the others exceed it
        for cb in cr.VREGRID_COMBOS:
            if cb not in combos:
                out, _ = cr.restate(dict(case, extras=dict(ex, method=cb[0], from_=cb[1], outside=cb[2])))
                assert is_undef(out, case["undef"]).mean() > 0.5, (label, cb)
    # per class one base takes two passes in each layout
    for klass in cr.CLASSES:
        nts = {(c2["fields"].shape[3] % 4 == 0, c2["extras"]["tcoord"].shape[0]) for c2 in cr.cases("vregrid", klass)}
        assert (True, cr.VREGRID_TB[4] + 1) in nts and (False, cr.VREGRID_TB[1] + 1) in nts, klass


def vregrid_filter(case, v, mistake=None):
    c, usable = cr.coordinate_of(case)
    ex = case["extras"]
    return vg.wave_interval_filter(c, usable, ex["tcoord"], vg.LOG if ex["method"] == "log" else vg.LINEAR, ex["fdef_t"], case["undef"], v=v,
                                   tb=cr.VREGRID_TB[v], mistake=mistake)


def test_vregrid_the_wave_interval_as_the_kernel_has_it_changes_nothing():
    """The model of the skip -- [min, max] per wave from [+inf, -inf], a NaN passed by, both compares closed -- turns away
    no pair that a cell brackets: on every range case and seam case, in both layouts, the filtered restatement is the
    restatement.  In the seam cases it does skip."""
    mine = [c for klass in cr.CLASSES for c in cr.cases("vregrid", klass)] + cr.vregrid_seam_cases()
    for case in mine:
        for v in (4, 1):
            look, skipped = vregrid_filter(case, v)
            assert not differs(cr.restate(case, prefilter=look), cr.expected(case)), (case["label"], v)
            assert skipped > 0 or case["klass"] != "seam", (case["label"], v)


LOSING_FILTERS = [m for m in vg.FILTER_MISTAKES if m != "reductions start from +-FLT_MAX"]


def test_vregrid_a_wave_interval_that_parts_from_the_cell_compare_loses_a_target_in_every_seam_case():
    """A strict compare on either side, a reduction that flushes subnormals (the targets' or the pairs', one without the
    other), a min / max that hands a NaN on: each changes at least one output of every seam case, in both layouts.  Making
    either side of the kernel's skip test strict, or building the reductions from an instruction that flushes or that
    returns NaN, fails tests/test_gpu_column_range.py on these cases."""
    for case in cr.vregrid_seam_cases():
        for v in (4, 1):
            for mistake in LOSING_FILTERS:
                look, _ = vregrid_filter(case, v, mistake)
                assert differs(cr.restate(case, prefilter=look), cr.expected(case)), (case["label"], v, mistake)


def test_vregrid_reductions_started_from_flt_max_only_widen_the_interval():
    """A minimum started from +FLT_MAX instead of +inf can only come out smaller, a maximum from -FLT_MAX only larger: both
    intervals of the skip test grow, a pair that was looked at still is, and no output can change -- on no case at all.
    What the wrong start costs is pairs that are looked at in vain (never more skipped than with the right start); no test
    of outputs can see it, and none here claims to."""
    for case in [c for klass in cr.CLASSES for c in cr.cases("vregrid", klass)] + cr.vregrid_seam_cases():
        for v in (4, 1):
            look, skipped = vregrid_filter(case, v, "reductions start from +-FLT_MAX")
            assert not differs(cr.restate(case, prefilter=look), cr.expected(case)), (case["label"], v)
            assert skipped <= vregrid_filter(case, v)[1], (case["label"], v)


def test_vregrid_seam_cases_end_their_pairs_on_the_wave_extremes():
    """In every seam block the smallest target of the wave is the upper end of the one pair that brackets it and the largest
    the lower end of its pair; both are found with a defined result in most cells; the block of unusable targets is undef."""
    for base in cr.vregrid_seam_bases():
        c, t = base["coord"], base["tcoord"]
        nb = len(base["blocks"])
        for b, (ta, tb) in enumerate(base["blocks"]):
            with np.errstate(invalid="ignore"):
                usable_t = np.where((t[:, b] == U) | np.isnan(t[:, b]), np.nan, t[:, b])
                lo, hi = np.nanmin(usable_t), np.nanmax(usable_t)
                assert hi == c[3, b].min() == c[3, b].max(), (base["base"], b)  # the lower end of the pair (3, 4)
                if ta is not None:  # the upper end of the pair (0, 1), where a hole has not taken it
                    assert lo == c[1, b][c[1, b] != U].max() == c[1, b][c[1, b] != U].min() and (c[1, b] != U).mean() > 0.9, (base["base"], b)
        for case in cr.vregrid_seam_cases():
            if case["base"] != base["base"]:
                continue
            out, fd = cr.expected(case)
            found = out[0] != U
            assert found[:2, :nb].mean() > 0.8 and not found[:, nb].any() and (fd == S).all(), case["label"]
            if case["method"] == "linear":  # the cell whose pair is (-inf, +inf): inf / inf (LOG: (2^-149, +inf), weight 0)
                assert np.isnan(out[:, :, nb + 2, 5]).any(), case["label"]


def test_vregrid_log_results_move_by_one_float_step_at_most_when_log_is_an_ulp_off():
    """The allowance of MIFC_VINTERP_LOG on the range and seam cases, established as tests/test_vregrid_cpu.py does it for
    the ordinary ones: with every double log() moved by one ulp -- up, down, each its own way -- no undef cell and no flag
    changes, no result moves by more than one float step and at most 1 % of the compared results move at all."""
    # each value its own way, but the same value always the same way: a device's log() is a function
    coin = lambda v: (np.asarray(v, np.float64).view(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63) != 0  # noqa: E731
    finite = lambda v, to: np.where(np.isfinite(np.log(v)), np.nextafter(np.log(v), to), np.log(v))  # noqa: E731  (log(inf) is inf on any device)
    moves = {"up": lambda v: finite(v, np.inf), "down": lambda v: finite(v, -np.inf),
             "mixed": lambda v: finite(v, np.where(coin(v), np.inf, -np.inf))}
    worst, n = 0.0, 0
    for case in [c for klass in cr.CLASSES for c in cr.cases("vregrid", klass)] + cr.vregrid_seam_cases():
        if case["extras"]["method"] != "log":
            continue
        exp, efd = cr.expected(case)
        for name, moved in moves.items():
            got, gfd = cr.restate(case, dict(vregrid=_MovedLog(moved)))
            assert np.array_equal(gfd, efd) and np.array_equal(got == U, exp == U), (case["label"], name)
            d = (exp != U) & ~(np.isnan(got) & np.isnan(exp))
            steps = np.abs(got.view(np.int32)[d].astype(np.int64) - exp.view(np.int32)[d].astype(np.int64))
            assert steps.max() <= 1 and (steps != 0).mean() <= 0.01, (case["label"], name, int(steps.max()), float((steps != 0).mean()))
            worst = max(worst, float((steps != 0).mean()))
        n += 1
    print("LOG cases %d, largest share of results moved by a log() one ulp off: %.4f %%" % (n, 100 * worst))
    assert n == 3 * 12 + 4 + 28  # the LOG bases, the seam cases, LOG on the bases of the LINEAR rule


class _MovedLog:
    """vregrid_restate with another double logarithm."""

    def __init__(self, log):
        self.log = log

    def hlevels(self, *a, **kw):
        return vg.hlevels(*a, log=self.log, **kw)

    def coord_fields(self, *a, **kw):
        return vg.coord_fields(*a, log=self.log, **kw)

    def levels(self, *a, **kw):
        return vg.levels(*a, log=self.log, **kw)


def same_or_neighbour(case, got, gfd, exp, efd, label):
    """The compare of tests/test_gpu_vregrid.py without its import of torch: LINEAR bit for bit, LOG the neighbour rule."""
    assert np.array_equal(gfd, efd), label
    if case["extras"]["method"] == "linear":
        assert not differs((got, gfd), (exp, efd)), label
        return
    und = is_undef(exp, case["undef"])
    assert np.array_equal(is_undef(got, case["undef"]), und), label
    d = ~und & ~(np.isnan(got) & np.isnan(exp))
    steps = np.abs(got.view(np.int32)[d].astype(np.int64) - exp.view(np.int32)[d].astype(np.int64))
    assert steps.size == 0 or (steps.max() <= 1 and (steps != 0).mean() <= 0.01), label


@pytest.mark.parametrize("klass", cr.CLASSES + ("seam",))
def test_vregrid_rules_header_on_the_range_and_seam_cases(shim, klass):  # noqa: F811
    """mifc_vregrid_rules.h, the text the kernel is built from, compiled with the host compiler and walked cell by cell
    (tests/host/vregrid_rules_driver.h) gives what the restatement gives on every range and seam case."""
    for case in (cr.vregrid_seam_cases() if klass == "seam" else cr.cases("vregrid", klass)):
        ex = case["extras"]
        got, gfd = header_run(shim, cr.vregrid_plain(case), ex["method"], ex["from_"], ex["outside"])
        exp, efd = cr.expected(case)
        same_or_neighbour(case, got, gfd, exp, efd, case["label"])


def test_vregrid_clamp_rule_at_the_ends_of_its_compares(shim):  # noqa: F811
    """Rule 5 of mifc_vregrid_* by hand (column_range_cases.HAND_COLUMNS): infinite extremes (ct < -inf is false: undef), a
    target of +-inf beyond finite extremes, extremes tied between +0 and -0 at different levels (the lowest index, in both
    directions), a target equal to an extreme that holes left without a bracket (undef, not clamped) -- the restatement
    and the rules header both give the hand-written result."""
    for from_ in ("first", "last"):
        for outside in ("undef", "clamp"):
            case, want = cr.vregrid_hand_case(from_, outside)
            out, fd = cr.restate(case)
            assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (from_, outside, out, want)
            got, gfd = header_run(shim, cr.vregrid_plain(case), "linear", from_, outside)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(gfd, fd), (from_, outside)
    # the extremes themselves, as the walk in either direction leaves them: (kmin, kmax)
    out = np.zeros(2, np.int32)
    for col, want in (([-0.0, 3, 0.0, 7], (0, 3)), ([0.0, 3, -0.0, 7], (0, 3)), ([-5, 0.0, -3, -0.0], (0, 1)), ([-5, -0.0, -3, 0.0], (0, 1)),
                      ([-INF, np.nan, INF], (0, 2)), ([INF, -INF, INF, -INF], (1, 0)), ([DEN, -DEN, DEN, -DEN], (1, 0)), ([FLT_MAX, INF, FLT_MAX], (0, 1))):
        c = np.asarray(col, np.float32)
        for descending in (0, 1):
            shim.mifc_test_vregrid_extremes(c.ctypes.data, c.size, descending, out.ctypes.data)
            assert tuple(out) == want, (col, descending, tuple(out))


def test_vregrid_levels_form_keeps_the_sign_of_a_zero_level(shim):  # noqa: F811
    """Rule 1: "mifc_vregrid_levels: c_k = levels[k]".  The sign of a zero level reaches the result through the weight."""
    for from_ in ("first", "last"):
        case, want = cr.vregrid_zero_level_case(from_)
        out, fd = cr.restate(case)
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), (from_, out)
        got, _ = header_run(shim, cr.vregrid_plain(case), "linear", from_, "undef")
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (from_, got)
        plus = dict(case, levs=np.array([0.0, 1.0], np.float32))
        assert np.signbit(cr.restate(plus)[0][0, 0, 0, 0]) and not np.signbit(out[0, 0, 0, 0])  # the level +0 gives -0: the case tells them apart


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
        for family in ("vderiv", "vcumul", "pvort", "vregrid"):
            for c in cr.cases(family, klass):
                if c["kind"] == "levels":
                    assert not differs(cr.restate(cr.as_field(c)), cr.expected(c)), c["label"]


def test_hybrid_form_is_the_field_form_of_its_coordinate():
    for c in cr.all_cases():
        if c["kind"] == "hybrid":
            assert not differs(cr.restate(cr.as_field(c)), cr.expected(c)), c["label"]
