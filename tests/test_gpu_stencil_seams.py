"""The stencil operators at the ends of the float range, kernel form by kernel form.

The cases of tests/stencil_seam_cases.py (Coriolis parameters that are zero, denormal, huge, infinite or NaN; map factors around
2^-125 and at both ends of the range; fields whose differences overflow, cancel to inf - inf, are denormal or signed zeros;
partials near sqrt(FLT_MAX) and sqrt(FLT_MIN)) go through every kernel form that restates the point formulas.  Each result is
compared per level and bit for bit (a NaN for a NaN) with the oracle's single-field call, the output flags must be equal, and
the form the launch took is asserted (mifc_last_stencil_form).  tests/test_stencil_seams_cpu.py pins the oracle to the
compiled reference on the same cases.

Forms and how they are reached (13 rows, 3 levels flagged ALL, SOME, SOME; widths 68, 260 and the ragged 258):
  one-input operators   single field: scalar_oneshot (default), scalar_rows (MIFC_SCALAR_ROWS_R), cell (MIFC_FORCE_CELL_KERNEL),
                        flat4 (width 258; gradient 1 has the cell kernel only); level batch: scalar_split
                        (MIFC_LEVELWALK_MIN_UNITS=1), scalar_levelwalk (and MIFC_VORTDIV_SPLIT=0), scalar_split_ragged (258)
  wind operators, Jacobian   single field: wind_oneshot (K=1), wind_oneshot_tiles (K=2; not the Jacobian, which has no tiles),
                        wind_rows (R=8), cell, flat4; level batch: wind_split, wind_levelwalk (one output, or the pair under
                        MIFC_VORTDIV_SPLIT=0; absvort and the Jacobian then walk rows: wind_rows), wind_split_ragged, wind_split_ff
  advection             advection_oneshot, advection_split, advection_split_ragged, cell
  thermalFrontParameter, plevelqvector   fused2 (also with 5-row bands) and two_stage_passes
  shapiro2_filter       shapiro_fused with rows in registers and in LDS, shapiro_sweeps
Batches are device-resident; each family also goes through host memory once.

Not reached: none of the listed forms is left out.  The case with undef = NaN under SOME_DEFINED is declined by the
level-walking and split-role forms (their test is one compare per value); there the result is compared and the form is not
asserted.
"""
import numpy as np
import pytest

import cases
import gpu_util
import stencil_seam_cases as sc

pytestmark = pytest.mark.gpu

ALL = sc.ALL_DEFINED
SINGLE = [op for op, spec in sc.OPS.items() if len(spec[0]) == 1]  # operators with a single-field entry of their own

_EXPECT = {}  # (op, nx) -> [(case, outputs per level, flags per level)], the oracle's, computed once
_DEVICE = {}  # label -> the case with its arrays on the GPU


def expected(oracle, op, nx):
    if (op, nx) not in _EXPECT:
        rows = []
        for case in sc.cases_for(op, nx):
            outs, flags, ok = sc.expect(oracle, case)
            assert ok, case["label"]
            for level in outs:
                for a in level:
                    a.setflags(write=False)
            rows.append((case, outs, flags))
        _EXPECT[(op, nx)] = rows
    return _EXPECT[(op, nx)]


def on_device(case):
    import torch

    if case["label"] not in _DEVICE:
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).cuda()  # noqa: E731  (a copy: the cases are read-only)
        _DEVICE[case["label"]] = dict(case, fields=[up(a) for a in case["fields"]], xm=up(case["xm"]), ym=up(case["ym"]), fc=up(case["fc"]))
    return _DEVICE[case["label"]]


def to_host(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def same(case, l, got, want, got_flag, want_flag, form):
    what = (case["label"], "level %d" % l, form)
    g = to_host(got)
    if not cases.same_bits(g, want, nan_payload=False):
        bad = np.nonzero((g.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(g) & np.isnan(want)))
        j, i = int(bad[0][0]), int(bad[1][0])
        raise AssertionError("%s: %d cells differ; first at (%d, %d): got %r, the oracle %r" % (what, len(bad[0]), j, i, g[j, i], want[j, i]))
    assert got_flag == want_flag, (what, got_flag, want_flag)


def form_of(case, form):
    """The form to assert: none for the NaN-undef case where the form tests with one compare."""
    nan_undef = case["undef"] != case["undef"]
    return None if nan_undef and form and ("split" in form or "levelwalk" in form) else form


def check_single_field(ctx, oracle, ops, widths, form, device=True):
    """Every case of `ops` through the single-field entries, level by level."""
    for op in ops:
        for nx in widths:
            for case, outs, flags in expected(oracle, op, nx):
                d = on_device(case) if device else case
                want_form = form(op, nx) if callable(form) else form
                for l in range(case["nlev"]):
                    (name, args), = sc.oracle_calls(d, l)
                    res = getattr(ctx, name)(*args, fdefined=int(case["flags"][l]), undef=case["undef"])
                    assert res is not None, case["label"]
                    gpu_util.check_form(ctx, want_form, what=(case["label"], l))
                    got = res[0] if isinstance(res[0], tuple) else (res[0],)
                    for k, g in enumerate(got):
                        same(case, l, g, outs[l][k], res[1], flags[l][k], want_form)


def run_levels(ctx, case, d):
    """One case through its level-batch entry: (outputs as a list of (nlev, ny, nx) arrays, flags per level)."""
    op, f = case["op"], d["fields"]
    kw = dict(fdefined=case["flags"], undef=case["undef"])
    if op in ctx.OPS:
        f1 = f[1] if len(f) > 1 else None
        res = ctx.stencil_levels(op, f[0], f1, d["xm"], d["ym"], d["fc"] if sc.OPS[op][2] else None, **kw)
        assert res is not None, case["label"]
        (o0, o1), fo = res
        return [o0] + ([o1] if o1 is not None else []), fo
    if op == "advection":
        res = ctx.stencil_levels_ex("advection", f[0], f[1], f[2], d["xm"], d["ym"], scalar=case["hours"], **kw)
    elif op == "thermalFrontParameter":
        res = ctx.stencil_levels_ex(op, f[0], xmapr=d["xm"], ymapr=d["ym"], **kw)
    elif op == "shapiro2_filter":
        res = ctx.stencil_levels_ex(op, f[0], **kw)
    else:
        res = ctx.stencil_levels_ex("plevelqvector", f[0], f[1], None, d["xm"], d["ym"], d["fc"], level_scalars=case["pres"], compute=case["compute"], **kw)
    assert res is not None, case["label"]
    return [res[0]], res[1]


def check_levels(ctx, oracle, ops, widths, form, device=True):
    for op in ops:
        for nx in widths:
            for case, outs, flags in expected(oracle, op, nx):
                got, fo = run_levels(ctx, case, on_device(case) if device else case)
                want_form = form_of(case, form(op, nx) if callable(form) else form)
                if isinstance(want_form, tuple):
                    assert gpu_util.run_is_forced() or ctx.last_stencil_form() in want_form, (case["label"], ctx.last_stencil_form(), want_form)
                else:
                    gpu_util.check_form(ctx, want_form, what=case["label"])
                for l in range(case["nlev"]):
                    for k, g in enumerate(got):
                        same(case, l, to_host(g)[l], outs[l][k], fo[l], flags[l][k], want_form)


# ------------------------------------------------------------------------------------------------ one-input operators
@pytest.mark.parametrize("form", ["scalar_oneshot", "scalar_rows", "cell", "flat4"])
def test_one_input_operators_single_field(gpu_ctx, oracle, mifc_env, form):
    widths = (258,) if form == "flat4" else (68, 260)
    if form == "scalar_rows":
        mifc_env("MIFC_SCALAR_ROWS_R", "2")
    if form == "cell":
        mifc_env("MIFC_FORCE_CELL_KERNEL", "1")
        widths = (68, 258)
    if form != "flat4":
        check_single_field(gpu_ctx, oracle, sc.FAMILIES["scalar"], widths, form)
        return
    # a ragged width outside the split-role form: the flat kernel -- but for gradient 1, which has the cell kernel only, and,
    # through the single-field entries, the two wind components, which pass the one map factor they use
    check_single_field(gpu_ctx, oracle, sc.FAMILIES["scalar"], widths,
                       lambda op, nx: "cell" if op in ("gradient1", "plevelgwind_xcomp", "plevelgwind_ycomp") else "flat4")
    mifc_env("MIFC_RAGGED_SPLIT", "0")
    check_levels(gpu_ctx, oracle, sc.FAMILIES["scalar"], widths, lambda op, nx: "cell" if op == "gradient1" else "flat4")


@pytest.mark.parametrize("form", ["scalar_split", "scalar_levelwalk", "scalar_split_ragged"])
def test_one_input_operators_level_batch(gpu_ctx, oracle, mifc_env, form):
    mifc_env("MIFC_LEVELWALK_MIN_UNITS", "1")
    if form == "scalar_levelwalk":
        mifc_env("MIFC_VORTDIV_SPLIT", "0")
    if form == "scalar_split_ragged":
        mifc_env("MIFC_RAGGED_SPLIT", "1")
    check_levels(gpu_ctx, oracle, sc.FAMILIES["scalar"], (258,) if form == "scalar_split_ragged" else (68, 260), form)


# ------------------------------------------------------------------------------------- wind operators and the Jacobian
WIND_SINGLE = ("relvort", "divergence", "absvort", "jacobian")
WIND_LEVELS = ("vortdiv", "relvort", "divergence", "absvort", "jacobian")


@pytest.mark.parametrize("form,tune", [("wind_oneshot", "K=1"), ("wind_oneshot_tiles", "K=2"), ("wind_rows", "R=8"), ("cell", None), ("flat4", None)])
def test_wind_operators_single_field(gpu_ctx, oracle, mifc_env, form, tune):
    if tune:
        mifc_env("MIFC_VORTDIV_TUNE", tune)
    if form == "cell":
        mifc_env("MIFC_FORCE_CELL_KERNEL", "1")
    ops = tuple(op for op in WIND_SINGLE if not (op == "jacobian" and form == "wind_oneshot_tiles"))
    check_single_field(gpu_ctx, oracle, ops, (258,) if form == "flat4" else (68, 258) if form == "cell" else (68, 260), form)
    if form == "flat4":  # the fused pair has no single-field entry: a ragged batch kept off the split-role form
        mifc_env("MIFC_RAGGED_SPLIT", "0")
        check_levels(gpu_ctx, oracle, WIND_LEVELS, (258,), form)


def test_wind_operators_single_field_default_choice(gpu_ctx, oracle):
    """Without any switch a single small field takes the one-shot form."""
    check_single_field(gpu_ctx, oracle, WIND_SINGLE, (260,), "wind_oneshot")


@pytest.mark.parametrize("how", ["split", "nosplit", "ragged"])
def test_wind_operators_level_batch(gpu_ctx, oracle, mifc_env, how):
    mifc_env("MIFC_LEVELWALK_MIN_UNITS", "1")
    if how == "nosplit":
        mifc_env("MIFC_VORTDIV_SPLIT", "0")
    if how == "ragged":
        mifc_env("MIFC_RAGGED_SPLIT", "1")

    def form(op, nx):
        if how == "ragged":
            return "wind_split_ragged"
        if how == "nosplit":
            return "wind_rows" if op in ("absvort", "jacobian") else "wind_levelwalk"
        return "wind_split" if op in ("vortdiv", "absvort", "jacobian") else "wind_levelwalk"

    check_levels(gpu_ctx, oracle, WIND_LEVELS, (258,) if how == "ragged" else (68, 260), form)


@pytest.mark.parametrize("nx", [68, 260])
def test_vortdiv_ff_three_outputs(gpu_ctx, oracle, mifc_env, nx):
    """Vorticity, divergence and the wind speed in one pass (wind_split_ff): sqrtf(u*u + v*v) overflows and underflows here."""
    import torch

    import mi_fieldcalc_amd as fc

    mifc_env("MIFC_LEVELWALK_MIN_UNITS", "1")
    for case, outs, flags in expected(oracle, "vortdiv_ff", nx):
        d = on_device(case)
        u, v = d["fields"]
        rv, dg, ff = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)
        cnt = torch.full((case["nlev"],), 99, dtype=torch.int64, device="cuda")
        cnt_ff = torch.full((case["nlev"],), 99, dtype=torch.int64, device="cuda")
        assert gpu_ctx.vortdiv_ff_levels_enqueue(u, v, d["xm"], d["ym"], rv, dg, ff, fdefined=case["flags"], undef=case["undef"], n_undefined=cnt,
                                                 n_undefined_ff=cnt_ff), case["label"]
        want_form = form_of(case, "wind_split_ff")
        gpu_util.check_form(gpu_ctx, want_form, what=case["label"])
        torch.cuda.synchronize()
        c, cf = cnt.cpu().numpy(), cnt_ff.cpu().numpy()
        n = nx * case["ny"]
        for l in range(case["nlev"]):
            tested = case["flags"][l] != ALL
            f_st = fc.classify(int(c[l]), n - 2 * nx) if tested else ALL
            f_ff = fc.classify(int(cf[l]), n) if tested else ALL
            for k, (g, f) in enumerate(((rv, f_st), (dg, f_st), (ff, f_ff))):
                same(case, l, to_host(g)[l], outs[l][k], f, flags[l][k], want_form)


# ---------------------------------------------------------------------------------------------------------- advection
@pytest.mark.parametrize("form", ["advection_oneshot", "advection_split", "advection_split_ragged", "cell"])
def test_advection(gpu_ctx, oracle, mifc_env, form):
    if form == "advection_oneshot":  # the single-field entry, and a batch kept off the split-role kernel
        check_single_field(gpu_ctx, oracle, ("advection",), (68, 260), form)
        mifc_env("MIFC_VORTDIV_SPLIT", "0")
        check_levels(gpu_ctx, oracle, ("advection",), (260,), form)
    elif form == "cell":
        check_single_field(gpu_ctx, oracle, ("advection",), (258,), form)
        mifc_env("MIFC_FORCE_CELL_KERNEL", "1")
        check_single_field(gpu_ctx, oracle, ("advection",), (68,), form)
    else:
        mifc_env("MIFC_LEVELWALK_MIN_UNITS", "1")
        check_levels(gpu_ctx, oracle, ("advection",), (258,) if form == "advection_split_ragged" else (68, 260), form)


# ------------------------------------------------------------------------- thermalFrontParameter and plevelqvector
TWO_STAGE = sc.FAMILIES["tfp"] + sc.FAMILIES["qvector"]


@pytest.mark.parametrize("how", ["fused", "fused-band5", "passes"])
def test_two_stage_operators(gpu_ctx, oracle, mifc_env, how):
    """The one-launch form (fused2; fused2_redo where a level of thermalFrontParameter is repaired pass by pass) and the
    pass-by-pass form, as a batch and through the single-field entries."""
    mifc_env("MIFC_FUSED2", "0" if how == "passes" else "1")
    if how == "fused-band5":
        mifc_env("MIFC_FUSED2_BAND", "5")
    form = "two_stage_passes" if how == "passes" else ("fused2", "fused2_redo")
    check_levels(gpu_ctx, oracle, TWO_STAGE, sc.NX_FORMS if how != "fused-band5" else (260,), form)
    if how != "fused-band5":
        check_single_field(gpu_ctx, oracle, TWO_STAGE, (68,), None if how == "fused" else form)


# ------------------------------------------------------------------------------------------------------ shapiro2_filter
@pytest.mark.parametrize("how", ["registers", "lds", "sweeps"])
def test_shapiro_filter(gpu_ctx, oracle, mifc_env, how):
    """Sums that overflow in one order of addition and not in another: f[i-1] + f[i+1] first, as the reference has it."""
    mifc_env("MIFC_SHAPIRO_FUSED", "0" if how == "sweeps" else "1")
    mifc_env("MIFC_SHAPIRO_REGS", "0" if how == "lds" else "1")
    form = "shapiro_sweeps" if how == "sweeps" else "shapiro_fused"
    widths = (68, 260) if how == "lds" else sc.NX_FORMS  # the LDS form takes multiples of four only
    check_levels(gpu_ctx, oracle, ("shapiro2_filter",), widths, form)
    check_single_field(gpu_ctx, oracle, ("shapiro2_filter",), (68,), form)


# ---------------------------------------------------------------------------------------------------------- host memory
@pytest.mark.parametrize("family", sorted(f for f in sc.FAMILIES if f != "wind_ff"))  # (the three-output entry takes device tensors only)
def test_from_host_memory(gpu_ctx, oracle, family):
    """Each family once with its arrays in host memory: the batch entry (staged or piped by the library), the form it picks by
    default not asserted."""
    ops = sc.FAMILIES[family][:1] if family != "scalar" else ("gradient4", "plevelgvort")
    check_levels(gpu_ctx, oracle, ops, (68,), None, device=False)
    check_single_field(gpu_ctx, oracle, [op for op in ops if op in SINGLE], (258,), None, device=False)
