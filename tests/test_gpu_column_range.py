"""The column-walk families (mifc_vinterp_*, mifc_vlayer_*, mifc_vderiv_*, mifc_vcumul_*, mifc_pvort_*, mifc_vregrid_*) at the
ends of the float range on the GPU: every case of tests/column_range_cases.py through the library, compared with the numpy restatement
by the family's own rule (the `compare` of the family's GPU test file): bit for bit, a NaN matching any NaN, flags equal;
for the LOG methods the restatement's float or its neighbour, undef cells and flags exact.  What the cases hold and why
they would show a flush to zero, a float intermediate or a bracket that loses a target is asserted on the CPU in
tests/test_column_range_cpu.py.

Per case: device memory on the 16-byte grid, device memory one float past it (one cell per lane on the same data: not a
bit may change), host memory in one band; per family one case widened along y through the host path with the family's
MIFC_*_CHUNK_MIB at 1, which takes more than one band.  The inputs are unchanged after each call and the floats around a
device output are intact.

mifc_vregrid_* takes four cells per lane only where MIFC_VREGRID_V asks for it: its tests set it to 4, so that the batch
on the grid at width 68 runs in that layout (15 target planes per pass) and everything else one cell per lane (24)."""
import numpy as np
import pytest

import column_range_cases as cr
import test_gpu_pvort as tpv
import test_gpu_vcumul as tvc
import test_gpu_vderiv as tvd
import test_gpu_vinterp as tvi
import test_gpu_vlayer as tvl
import test_gpu_vregrid as tvg
import vlayer_restate as vl

pytestmark = pytest.mark.gpu

A, N, S = cr.ALL_DEFINED, cr.NONE_DEFINED, cr.SOME_DEFINED
SENTINEL = -4242.5
GROUPS = [(family, klass) for family in cr.FAMILIES for klass in cr.CLASSES]
PAD = {"aligned": 64, "offset": 65}  # floats in front of a device array: 64 keeps the 16-byte grid, 65 leaves it


def compare(case, got, gfd, exp, efd, label):
    family = case["family"]
    if family == "vinterp":
        tvi.compare(got, exp, gfd, efd, case["method"], case["undef"], label)
    elif family == "vlayer":
        tvl.compare(got, exp, gfd, efd, label)
    elif family == "vderiv":
        tvd.compare(got, exp, gfd, efd, label)
    elif family == "vcumul":
        tvc.compare(got, exp, gfd, efd, tvc.vc.METHODS[case["method"]], label)
    elif family == "vregrid":
        tvg.compare(got, exp, gfd, efd, case["extras"]["method"], case["undef"], label)
    else:
        tpv.compare(got, exp, gfd, efd, label)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def call(ctx, case, where, out_shape, form=None):
    """One call on the case with its arrays in host memory (where = "host") or on the device as guarded views ("aligned",
    "offset"), the output a view into a sentinel-filled tensor.  Asserts that no input has changed and that the sentinel
    around the output is intact.  Returns (out as numpy, flags)."""
    import torch

    device = where != "host"
    kept = []

    def put(a):
        if a is None or not isinstance(a, np.ndarray) or a.ndim < 2:
            return a
        p = tpv.guarded(a, PAD[where]) if device else np.array(a, np.float32)
        kept.append((p, a))
        return p

    family, kind, ex, undef = case["family"], case["kind"], case["extras"], case["undef"]
    f = put(case["fields"])
    kw = dict(fdefined_in=case["flags"], undef=undef)
    room = None
    if device:
        n, pad = int(np.prod(out_shape)), PAD[where]
        room = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float32, device="cuda")
        kw["out"] = room[pad:pad + n].view(out_shape)
    if kind == "hybrid":
        head, kw["fdef_ps"] = (put(case["ps"]), case["ab"][0], case["ab"][1]), case["fdef_c"]
    elif kind == "field":
        head, kw["fdef_coord"] = (put(case["coord"]),), case["fdef_c"]
    else:
        head = (case["levs"],)
    name = {"hybrid": "hlevels", "field": "fields", "levels": "levels"}[kind]
    if family == "vinterp":
        out, fd = getattr(ctx, "vinterp_" + name)(f, *head, ex["targets"], method=case["method"], **kw)
    elif family == "vlayer":
        out, fd = getattr(ctx, "vlayer_" + name)(f, *head, vl.ALL_PRODUCTS, put(ex["lo"]), put(ex["hi"]), **kw)
    elif family == "vderiv":
        out, fd = getattr(ctx, "vderiv_" + name)(f, *head, case["method"], None, **kw)
    elif family == "vcumul":
        more = {k: ex[k] for k in ("scale", "fdef_start", "fdef_base") if k in ex}
        if "start" in ex:
            more.update(start=put(ex["start"]), base=[put(b) for b in ex["base"]])
        out, fd = getattr(tvc.front(), "vcumul_" + name)(ctx, f, *head, case["method"], ex["from_"], **more, **kw)
    elif family == "vregrid":
        out, fd = getattr(tvg.front(), "vregrid_" + name)(ctx, f, *head, put(ex["tcoord"]), method=ex["method"], from_=ex["from_"], outside=ex["outside"],
                                                           fdef_tcoord=ex["fdef_t"], **kw)
        nx, nt = case["fields"].shape[3], ex["tcoord"].shape[0]
        seen = tvg.front().last_vregrid_form(ctx)
        want = {"method": ex["method"], "from": ex["from_"], "outside": ex["outside"], "coord": kind}
        if form and "v" in form and device:  # MIFC_VREGRID_V = 4 is set: four cells per lane on the grid
            v4 = 4 if nx % 4 == 0 and PAD[where] % 4 == 0 else 1
            want.update(v=v4, tb=cr.VREGRID_TB[v4], passes=-(-nt // cr.VREGRID_TB[v4]))
        assert {k: seen[k] for k in want} == want, (case["label"], where, seen, want)
    else:
        out, fd = getattr(tpv.front(), "pvort_" + name)(ctx, f[0], f[1], f[2], *head, put(ex["xmapr"]), put(ex["ymapr"]), put(ex["fcoriolis"]),
                                                        case["method"], scale=ex["scale"], **kw)
        nx = case["fields"].shape[3]
        v4 = 4 if nx % 4 == 0 and (not device or PAD[where] % 4 == 0) else 1
        want = {"v": v4, "kind": kind, "method": case["method"], "tile": "%dx%d" % (tpv.LANES_X * v4, tpv.TY), "launches": 1, "bands": 1}
        want.update(form or {})
        want = {k: v for k, v in want.items() if v is not None}
        seen = tpv.front().last_pvort_form(ctx)
        assert {k: seen[k] for k in want} == want, (case["label"], where, seen, want)
    if device:
        torch.cuda.synchronize()
        assert out is kw["out"], (case["label"], where)
        assert (room[:pad] == SENTINEL).all().item() and (room[pad + n:] == SENTINEL).all().item(), (case["label"], where, "the sentinel around the output")
        out = out.cpu().numpy()
    assert tuple(out.shape) == tuple(out_shape), (case["label"], where)
    for p, a in kept:
        assert same_bits(p.cpu().numpy() if device else p, a), (case["label"], where, "an input has changed")
    return out, np.asarray(fd)


def check(ctx, case, where, form=None):
    exp, efd = cr.expected(case)
    got, gfd = call(ctx, case, where, exp.shape, form)
    compare(case, got, gfd.reshape(efd.shape), exp, efd, (case["label"], where))
    return got, gfd


def four_cells_per_lane(mifc_env, family):
    """vregrid: ask for four cells per lane where the batch allows; the form that `call` then expects of a device call."""
    if family != "vregrid":
        return None
    mifc_env("MIFC_VREGRID_V", 4)
    return {"v": 4}


@pytest.mark.parametrize("family,klass", GROUPS)
def test_range_cases_in_device_and_host_memory(gpu_ctx, mifc_env, family, klass):
    form = four_cells_per_lane(mifc_env, family)
    for case in cr.cases(family, klass):
        on_grid, fd = check(gpu_ctx, case, "aligned", form)
        off_grid, ofd = check(gpu_ctx, case, "offset", form)
        # one cell per lane on the same data (LOG as well: the same log() of the same doubles)
        assert ((on_grid.view(np.uint32) == off_grid.view(np.uint32)) | (np.isnan(on_grid) & np.isnan(off_grid))).all(), (case["label"], "off the grid")
        assert np.array_equal(fd, ofd), case["label"]
        check(gpu_ctx, case, "host")


def test_vinterp_where_the_interval_of_a_wave_ends_on_a_target(gpu_ctx):
    """The seam cases of the wave pre-filter (column_range_cases.vinterp_seam_cases): whole waves of cells whose pair of
    levels ends on +-0, a subnormal or an end of the float range that is itself a target.  tests/test_column_range_cpu.py
    shows on a model of the filter that a missing `+ 0.f` on either side or a flushing reduction changes these cases, in
    the layout of four cells per lane (on the grid, and the staged host band) and of one (off the grid, and width 67)."""
    for case in cr.vinterp_seam_cases():
        on_grid, fd = check(gpu_ctx, case, "aligned")
        off_grid, ofd = check(gpu_ctx, case, "offset")
        assert ((on_grid.view(np.uint32) == off_grid.view(np.uint32)) | (np.isnan(on_grid) & np.isnan(off_grid))).all(), (case["label"], "off the grid")
        assert np.array_equal(fd, ofd), case["label"]
        check(gpu_ctx, case, "host")


def test_vregrid_where_the_interval_of_a_wave_ends_on_a_target(gpu_ctx, mifc_env):
    """The seam cases of the wave skip (column_range_cases.vregrid_seam_cases): whole waves whose smallest / largest usable
    target is the end of the one pair that brackets it, the ends at +-0, +-2^-149, +-FLT_MIN, +-FLT_MAX and +-inf; a wave
    without a usable target, a lane without levels, a pair from -inf to +inf.  tests/test_column_range_cpu.py shows on a
    model of the skip that a strict compare on either side, a flush in one of the reductions or a NaN that comes through
    one changes these cases, in the layout of four cells per lane (on the grid) and of one (off it)."""
    form = four_cells_per_lane(mifc_env, "vregrid")
    for case in cr.vregrid_seam_cases():
        on_grid, fd = check(gpu_ctx, case, "aligned", form)
        off_grid, ofd = check(gpu_ctx, case, "offset", form)
        assert ((on_grid.view(np.uint32) == off_grid.view(np.uint32)) | (np.isnan(on_grid) & np.isnan(off_grid))).all(), (case["label"], "off the grid")
        assert np.array_equal(fd, ofd), case["label"]
        check(gpu_ctx, case, "host")
    mifc_env("MIFC_VREGRID_V", None)  # and as the library chooses by itself
    for case in cr.vregrid_seam_cases():
        check(gpu_ctx, case, "aligned")


def test_vregrid_clamp_rule_and_zero_level_by_hand(gpu_ctx):
    """The hand-written columns of rule 5 (infinite extremes, targets of +-inf, extremes tied between +0 and -0, a target on
    an extreme that holes left without a bracket) and the `levels` form with a level of -0, whose sign reaches the result."""
    for from_ in ("first", "last"):
        for outside in ("undef", "clamp"):
            case, want = cr.vregrid_hand_case(from_, outside)
            efd = cr.restate(case)[1]
            for where in ("aligned", "offset", "host"):
                got, gfd = call(gpu_ctx, case, where, want.shape)
                assert same_bits(got, want) and np.array_equal(gfd.reshape(efd.shape), efd), (case["label"], where, got, want, gfd, efd)
        case, want = cr.vregrid_zero_level_case(from_)
        efd = cr.restate(case)[1]
        for where in ("aligned", "host"):
            got, gfd = call(gpu_ctx, case, where, want.shape)
            assert same_bits(got, want) and np.array_equal(gfd.reshape(efd.shape), efd), (case["label"], where, got, want, gfd, efd)


@pytest.mark.parametrize("family", cr.FAMILIES)
def test_the_coordinate_forms_of_one_problem_give_the_same_bits(gpu_ctx, family):
    """hybrid against the field form on the batch alevel + blevel * ps; levels against the field form on a batch filled
    from the levels.  In the levels form of vcumul LOG the host takes the logarithm (include/mifc.h), the device does in
    the field form: there the family's neighbour rule holds between the two, everywhere else the bits are the same."""
    n = 0
    for klass in cr.CLASSES:
        for case in cr.cases(family, klass):
            if case["kind"] == "field":
                continue
            twin = cr.as_field(case)
            exp, efd = cr.expected(case)
            got, gfd = call(gpu_ctx, case, "aligned", exp.shape)
            tgot, tfd = call(gpu_ctx, twin, "aligned", exp.shape)
            label = (case["label"], "against its field form")
            if case["kind"] == "levels" and case["method"] == "log":
                compare(case, got, gfd.reshape(efd.shape), tgot, tfd.reshape(efd.shape), label)
            else:
                assert ((got.view(np.uint32) == tgot.view(np.uint32)) | (np.isnan(got) & np.isnan(tgot))).all() and np.array_equal(gfd, tfd), label
            n += 1
    assert n >= 7


# The whole problem of the widened case -- its planes of 180 rows, before any padding -- is larger than the MiB (asserted), so
# a call that honours the budget takes at least two bands; where the entry reports its launches (vcumul, pvort) that is read
# back as well.  The level-batch entries of vinterp, vlayer and vderiv report no band count.
BAND_CASES = {"vinterp": ("huge", 1), "vlayer": ("tiny", 2), "vderiv": ("huge", 1), "vcumul": ("tiny", 1), "pvort": ("huge", 3), "vregrid": ("tiny", 11)}


@pytest.mark.parametrize("family", cr.FAMILIES)
def test_host_call_in_more_than_one_band(gpu_ctx, mifc_env, family):
    mifc_env("MIFC_%s_CHUNK_MIB" % family.upper(), 1)
    klass, j = BAND_CASES[family]
    wide = cr.widened(cr.cases(family, klass)[j], 20)
    assert wide["kind"] == "field" and wide["fields"].shape[2] == 180, wide["label"]
    exp, efd = cr.restate(wide)
    arrays = [wide["fields"], wide["coord"], exp] + [a for v in wide["extras"].values() for a in (v if isinstance(v, list) else [v])
                                                     if isinstance(a, np.ndarray) and a.ndim >= 2]
    assert 4 * sum(a.size for a in arrays) > 2 ** 20, (wide["label"], "fits one band")
    got, gfd = call(gpu_ctx, wide, "host", exp.shape, form={"bands": None, "launches": None})
    compare(wide, got, gfd.reshape(efd.shape), exp, efd, (wide["label"], "bands"))
    if family == "pvort":
        seen = tpv.front().last_pvort_form(gpu_ctx)
        assert seen["bands"] >= 2 and seen["launches"] == seen["bands"], seen
    if family == "vcumul":  # two fields: one launch per band
        seen = tvc.front().last_vcumul_form(gpu_ctx)
        assert seen["launches"] >= 2, seen
    if family == "vregrid":  # 25 target planes: two passes per band
        seen = tvg.front().last_vregrid_form(gpu_ctx)
        assert seen["passes"] == 2 and seen["launches"] >= 4, seen
    # the bands against the one-launch device call itself
    dev, dfd = call(gpu_ctx, wide, "aligned", exp.shape)
    assert ((got.view(np.uint32) == dev.view(np.uint32)) | (np.isnan(got) & np.isnan(dev))).all() and np.array_equal(gfd, dfd), (wide["label"], "bands against the device call")


def _all_computed(family):
    """A case whose results on some level are all infinities or NaN that the arithmetic made, every flag ALL_DEFINED."""
    ny, nx, nlev = 9, 67, 3
    big = np.float32(3e38)
    sign = np.array([1, -1, 1], np.float32).reshape(1, nlev, 1, 1)
    x = np.broadcast_to(big * sign, (2, nlev, ny, nx)).copy()
    coord = np.broadcast_to(np.array([0, 0.5, 1], np.float32).reshape(nlev, 1, 1), (nlev, ny, nx)).copy()
    case = dict(label=family + "-all-computed", family=family, kind="field", klass="huge", undef=cr.UNDEF, fields=x, coord=coord,
                flags=np.full((2, nlev), A, np.int32), fdef_c=np.full(nlev, A, np.int32), method=None, extras={})
    if family == "vinterp":  # an interpolation of finite values is finite: +inf and -inf stored under ALL_DEFINED, inf + w * -inf
        case["fields"] = np.broadcast_to(np.float32(np.inf) * sign, (2, nlev, ny, nx)).copy()
        case.update(method="linear", extras=dict(targets=np.array([0.25, 0.75], np.float32)))
    elif family == "vlayer":
        case["fields"] = np.full((2, nlev, ny, nx), big, np.float32)  # the integral of 3e38 over 4
        case["coord"] = coord * np.float32(4)
        case["extras"] = dict(lo=-cr.INF, hi=cr.INF)
    elif family == "vderiv":
        case["method"] = "weighted"
    elif family == "vcumul":
        case["fields"] = np.full((2, nlev, ny, nx), big, np.float32)
        case["coord"] = coord * np.float32(4)
        case.update(method="linear", extras=dict(from_="first"))
    elif family == "vregrid":  # as vinterp; the second plane lies beyond the column and is clamped to a level of +inf
        case["fields"] = np.broadcast_to(np.float32(np.inf) * sign, (2, nlev, ny, nx)).copy()
        planes = np.broadcast_to(np.array([0.25, 7.0], np.float32).reshape(2, 1, 1), (2, ny, nx)).copy()
        case.update(method="linear", extras=dict(tcoord=planes, fdef_t=np.full(2, A, np.int32), method="linear", from_="last", outside="clamp"))
    else:
        z = np.zeros((2, nlev, ny, nx), np.float32)
        case["fields"] = np.concatenate([z, x[:1]])
        case["flags"] = np.full((3, nlev), A, np.int32)
        m = np.zeros((ny, nx), np.float32)
        case.update(method="centred", extras=dict(xmapr=m, ymapr=m, fcoriolis=np.full((ny, nx), 0.75, np.float32), scale=1.0))
    return case


@pytest.mark.parametrize("family", cr.FAMILIES)
def test_a_level_of_computed_nan_or_infinity_comes_back_all_defined(gpu_ctx, family):
    case = _all_computed(family)
    exp, efd = cr.restate(case)
    planes = exp.reshape(-1, exp.shape[-2] * exp.shape[-1])
    assert (~np.isfinite(planes)).all(axis=1).any() and (planes != cr.UNDEF).all() and (efd == A).all(), (family, efd)
    for where in ("aligned", "offset", "host"):
        got, gfd = call(gpu_ctx, case, where, exp.shape)
        compare(case, got, gfd.reshape(efd.shape), exp, efd, (case["label"], where))
        assert (gfd == A).all(), (family, where, gfd)
