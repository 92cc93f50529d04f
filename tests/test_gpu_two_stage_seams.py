"""thermalFrontParameter, plevelqvector and shapiro2_filter at the seams of their host drivers (csrc/mifc_capi_twostage.hip):
which route a call takes (mifc_last_stencil_form: fused2 | fused2_redo | two_stage_passes | shapiro_fused | shapiro_sweeps),
the widths around what the one-launch kernels take, the two flag groups of a batch and their level list, the repair of a
level inside a batch, the in-place filter, the per-level pressures and the refusals.  Every result is compared per level and
bit for bit with the oracle's single-field call, flags included; the grids are tiny on purpose (the routes depend on widths,
flags and switches, not on size)."""
import numpy as np
import pytest

import cases
import gpu_util

pytestmark = pytest.mark.gpu

ALL, SOME = cases.ALL_DEFINED, cases.SOME_DEFINED
UNDEF = cases.UNDEF
SENTINEL = np.float32(-4242.5)
PRESSURES = np.array([1000.0, 850.0, 700.0, 500.0, 300.0], np.float32)  # one per level, all different
OPS = ["tfp", "q1", "q2", "q3", "q4", "shapiro"]

# the route under default switches, by width: the two-stage kernel takes nx >= 8 except a ragged width with nx % 240 == 1;
# the filter's register form takes any width from 8 on, its tile form multiples of four from 4 on
TWO_STAGE_ROUTE = {4: "two_stage_passes", 8: "fused2", 9: "fused2", 240: "fused2", 241: "two_stage_passes", 244: "fused2"}
SHAPIRO_ROUTE = {4: "shapiro_fused", 8: "shapiro_fused", 9: "shapiro_fused", 240: "shapiro_fused", 241: "shapiro_fused", 244: "shapiro_fused"}


# ---------------------------------------------------------------------------------------------------------------- data
_GRIDS = {}
_REFERENCE = {}  # (op, nx, ny, level tag, flag) -> the oracle's single-field result, computed once


def grid(nx, ny):
    """Map factors, Coriolis parameter and a pool of levels of one grid: 'c<l>' clean, 'h<l>' with undefined values."""
    import mi_fieldcalc_amd.synth as synth

    if (nx, ny) not in _GRIDS:
        xm, ym, fc = synth.grid_maps(nx, ny)
        _GRIDS[(nx, ny)] = dict(nx=nx, ny=ny, xm=xm, ym=ym, fc=fc, levels={})
    return _GRIDS[(nx, ny)]


def level(g, tag):
    """One level of the pool: (z, t).  'h': an undefined value in the middle (all a grid of a few columns can take without
    losing every result to it) and, from 16 columns on, one in the first row, one next to the last column and a NaN in the
    last column; 'p': a plateau (|grad| == 0, rejected by thermalFrontParameter whatever the flag says)."""
    import mi_fieldcalc_amd.synth as synth

    if tag not in g["levels"]:
        nx, ny = g["nx"], g["ny"]
        z = synth.scalar_field(nx, ny, 900 + 7 * int(tag[1:]) + nx)
        if tag[0] == "h":
            z[ny // 2, nx // 2] = UNDEF
            if nx >= 16:
                z[0, 1] = UNDEF
                z[ny - 2, nx - 1] = np.nan
                z[1, nx - 2] = UNDEF
        elif tag[0] == "p":
            z[ny // 3:, : max(3, nx // 2)] = np.float32(5432.0)
        bad = (z == UNDEF) | np.isnan(z)
        with np.errstate(all="ignore"):
            t = np.where(bad, z, np.float32(250.0) + np.float32(0.05) * (z - np.float32(5500.0))).astype(np.float32)
        g["levels"][tag] = (z, t)
    return g["levels"][tag]


def batch(g, tags):
    zs, ts = zip(*(level(g, tag) for tag in tags))
    return np.stack(zs), np.stack(ts)


def reference(oracle, g, op, z, t, tag, flag, p, xm=None, key=None):
    """The oracle's single-field call for one level: (field, flag)."""
    nx, ny = g["nx"], g["ny"]
    key = (op, nx, ny, tag, int(flag), float(p) if op[0] == "q" else 0.0, key)
    if key not in _REFERENCE:
        xm_ = g["xm"] if xm is None else xm
        if op == "tfp":
            res = oracle.call("thermalFrontParameter", nx, ny, z, xm_, g["ym"], fdefined=int(flag))
        elif op == "shapiro":
            res = oracle.call("shapiro2_filter", nx, ny, z, fdefined=int(flag))
        else:
            res = oracle.call("plevelqvector", nx, ny, z, t, xm_, g["ym"], g["fc"], float(p), int(op[1]), fdefined=int(flag))
        assert res[0], key
        res[1].setflags(write=False)
        _REFERENCE[key] = (res[1], res[2])
    return _REFERENCE[key]


def mover(device):
    """(to where the call reads it, back to numpy)"""
    if not device:
        return (lambda a: a), (lambda a: a)
    import torch

    return (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()), (lambda a: a.cpu().numpy())


def route_of(op, nx, routes=None):
    if routes and op in routes:
        return routes[op]
    if routes and ("two_stage" if op != "shapiro" else "filter") in routes:
        return routes["two_stage" if op != "shapiro" else "filter"]
    return SHAPIRO_ROUTE[nx] if op == "shapiro" else TWO_STAGE_ROUTE[nx]


def run_batch(ctx, g, op, z, t, flags, device, pres=PRESSURES, xm=None, out0=None):
    """One operator over a batch through mifc_stencil_levels_ex: (out as numpy, flags out, route)."""
    to, back = mover(device)
    nlev = z.shape[0]
    xm_ = g["xm"] if xm is None else xm
    if out0 is None:
        out0 = to(np.full(z.shape, SENTINEL, np.float32))
    if op == "tfp":
        res = ctx.stencil_levels_ex("thermalFrontParameter", to(z), xmapr=to(xm_), ymapr=to(g["ym"]), fdefined=flags, out0=out0)
    elif op == "shapiro":
        res = ctx.stencil_levels_ex("shapiro2_filter", to(z), fdefined=flags, out0=out0)
    else:
        res = ctx.stencil_levels_ex("plevelqvector", to(z), to(t), None, to(xm_), to(g["ym"]), to(g["fc"]), level_scalars=pres[:nlev],
                                    compute=int(op[1]), fdefined=flags, out0=out0)
    assert res is not None, op
    route = ctx.last_stencil_form()
    assert ctx.last_host_chunks() == (0, 0), op  # these operators are never piped
    return back(res[0]), res[1], route


def run_single(ctx, g, op, z, t, flag, device, p=700.0, xm=None):
    to, back = mover(device)
    xm_ = g["xm"] if xm is None else xm
    out = to(np.full(z.shape, SENTINEL, np.float32))
    if op == "tfp":
        res = ctx.thermalFrontParameter(to(z), to(xm_), to(g["ym"]), fdefined=int(flag), out=out)
    elif op == "shapiro":
        res = ctx.shapiro2_filter(to(z), fdefined=int(flag), out=out)
    else:
        res = ctx.plevelqvector(to(z), to(t), to(xm_), to(g["ym"]), to(g["fc"]), float(p), int(op[1]), fdefined=int(flag), out=out)
    assert res is not None, op
    return back(res[0]), res[1], ctx.last_stencil_form()


def check_batch(ctx, oracle, g, tags, flags, device, ops=OPS, routes=None, xm=None, key=None):
    """Every operator over the batch of the pool levels `tags`: per level the oracle's bits and flag, and the route."""
    z, t = batch(g, tags)
    flags = np.asarray(flags, np.int32)
    for op in ops:
        out, fo, route = run_batch(ctx, g, op, z, t, flags, device, xm=xm)
        for l, tag in enumerate(tags):
            e, f = reference(oracle, g, op, z[l], t[l], tag, flags[l], PRESSURES[l], xm=xm, key=key)
            assert cases.same_bits(out[l], e, nan_payload=False), (op, g["nx"], g["ny"], l, tag)
            assert fo[l] == f, (op, g["nx"], g["ny"], l, tag, fo[l], f)
        gpu_util.check_form(ctx, route_of(op, g["nx"], routes), what=(op, g["nx"], g["ny"], "batch"))


# ------------------------------------------------------------------------------------------------------------- widths
@pytest.mark.parametrize("ny", [3, 4, 9])
@pytest.mark.parametrize("nx", [4, 8, 9, 240, 241, 244])
def test_widths_around_the_one_launch_kernels(gpu_ctx, oracle, nx, ny):
    """Each width takes its route under default switches, as a mixed-flag batch and as a single field, and gives the oracle's
    bits either way."""
    g = grid(nx, ny)
    tags = ["h0", "c1", "p2", "c3", "h4"]
    flags = [SOME, ALL, SOME, ALL, SOME]
    check_batch(gpu_ctx, oracle, g, tags, flags, device=True)
    for op in OPS:
        for tag, flag in (("h0", SOME), ("c1", ALL)):
            z, t = level(g, tag)
            out, f, route = run_single(gpu_ctx, g, op, z, t, flag, device=True, p=PRESSURES[0])
            e, fe = reference(oracle, g, op, z, t, tag, flag, PRESSURES[0])
            assert cases.same_bits(out, e, nan_payload=False) and f == fe, (op, nx, ny, tag)
            gpu_util.check_form(gpu_ctx, route_of(op, nx), what=(op, nx, ny, "single"))


# ---------------------------------------------------------------------------------------------- batches and flag groups
FLAG_PATTERNS = {
    # pattern -> (pool levels, flags) of a five-level batch; shallower batches take the first levels
    "all": (["c0", "c1", "p2", "c3", "c4"], [ALL, ALL, ALL, ALL, ALL]),
    "some": (["h0", "c1", "h2", "p3", "h4"], [SOME, SOME, SOME, SOME, SOME]),
    "mixed": (["h0", "c1", "p2", "h3", "c4"], [SOME, ALL, ALL, SOME, SOME]),  # tested levels first and last
    "lying": (["h0", "h1", "c2", "h3", "h4"], [ALL, SOME, ALL, SOME, ALL]),  # undefined values under ALL_DEFINED: no tests
}


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("pattern", sorted(FLAG_PATTERNS))
@pytest.mark.parametrize("nlev", [1, 2, 5])
def test_batches_and_flag_groups(gpu_ctx, oracle, nlev, pattern, device):
    """Batches of 1, 2 and 5 levels from host and from device memory under the four flag patterns, at a ragged width on the
    one-launch kernels and at one on the pass-by-pass route.  A batch of one equals the single-field entry on the same data:
    bits, flag and route."""
    tags, flags = FLAG_PATTERNS[pattern]
    tags, flags = tags[:nlev], flags[:nlev]
    for nx, ny in ((9, 9), (241, 4)):
        g = grid(nx, ny)
        check_batch(gpu_ctx, oracle, g, tags, flags, device)
        if nlev == 1:
            z, t = batch(g, tags)
            for op in OPS:
                b_out, b_flag, b_route = run_batch(gpu_ctx, g, op, z, t, np.asarray(flags, np.int32), device)
                s_out, s_flag, s_route = run_single(gpu_ctx, g, op, z[0], t[0], flags[0], device, p=PRESSURES[0])
                assert cases.same_bits(b_out[0], s_out, nan_payload=True), (op, nx)
                assert b_flag[0] == s_flag and b_route == s_route, (op, nx, b_flag[0], s_flag, b_route, s_route)


@pytest.mark.parametrize("mixed", [True, False])
def test_a_batch_deeper_than_one_launch(gpu_ctx, oracle, mixed):
    """65 545 levels of 8 x 3 cells: grid.y ends at 65 535, so a flag group of more levels is split -- by the two-stage
    launcher, with a level list (mixed flags: three ALL_DEFINED levels, 65 542 tested ones) and without (one group), and by
    the filter's driver into slices with their own lists.  The levels around the seams and at both ends against the oracle."""
    nx, ny, nlev = 8, 3, 65545
    g = grid(nx, ny)
    pool = ["h0", "c1", "p2", "c3"]
    zp, tp = batch(g, pool)
    which = np.arange(nlev) % len(pool)
    z, t = zp[which], tp[which]
    flags = np.full(nlev, SOME, np.int32)
    if mixed:
        flags[[1, 3, 65541]] = ALL
    pres = PRESSURES[np.arange(nlev) % len(PRESSURES)]
    for op in OPS if mixed else ["tfp", "q2", "shapiro"]:
        out, fo, _ = run_batch(gpu_ctx, g, op, z, t, flags, device=True, pres=pres)
        for l in (0, 1, 2, 3, 65533, 65534, 65535, 65536, 65537, 65538, 65541, nlev - 1):
            e, f = reference(oracle, g, op, z[l], t[l], pool[which[l]], flags[l], pres[l])
            assert cases.same_bits(out[l], e, nan_payload=False), (op, l)
            assert fo[l] == f, (op, l, fo[l], f)
        if op == "shapiro":
            assert np.all(fo == ALL)


# ------------------------------------------------------------------------------------------------------ the repair rule
def nan_gradient_level(g):
    """cases.fused2_cases()'s nan-gradient recipe: every value defined, a NaN gradient (0 * inf) from defined inputs."""
    nx, ny = g["nx"], g["ny"]
    z, _ = level(g, "c9")
    zn, xn = z.copy(), g["xm"].copy()
    j, i = ny // 2, nx // 2
    zn[j, i - 1], zn[j, i + 1] = np.float32(-3.0e38), np.float32(3.0e38)
    xn[j, i] = np.float32(0.0)
    g["levels"]["n9"] = (zn, np.float32(250.0) + np.float32(0.05) * (zn - np.float32(5500.0)))
    return xn


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("nx,ny", [(8, 9), (9, 9), (244, 9)])
def test_a_level_repaired_inside_a_batch(gpu_ctx, oracle, nx, ny, device):
    """thermalFrontParameter's second pass is tested only if the first left something undefined (FieldCalculations.cc:2286): a
    SOME_DEFINED level without undefined values whose gradient is NaN goes again pass by pass (fused2_redo), between an
    ordinary tested level and an ALL_DEFINED one whose results the repair leaves alone.  Flagged ALL_DEFINED the same level
    needs no repair.  The single-field call takes the same two routes."""
    g = grid(nx, ny)
    xn = nan_gradient_level(g)
    tags = ["h0", "n9", "c1"]
    check_batch(gpu_ctx, oracle, g, tags, [SOME, SOME, ALL], device, ops=["tfp"], routes={"tfp": "fused2_redo"}, xm=xn, key="xn")
    check_batch(gpu_ctx, oracle, g, tags, [SOME, ALL, ALL], device, ops=["tfp"], routes={"tfp": "fused2"}, xm=xn, key="xn")
    check_batch(gpu_ctx, oracle, g, tags, [SOME, SOME, ALL], device, ops=["q1", "q4"], routes={"two_stage": "fused2"}, xm=xn, key="xn")
    z, t = level(g, "n9")
    for flag, want in ((SOME, "fused2_redo"), (ALL, "fused2")):
        out, f, route = run_single(gpu_ctx, g, "tfp", z, t, flag, device, xm=xn)
        e, fe = reference(oracle, g, "tfp", z, t, "n9", flag, 0.0, xm=xn, key="xn")
        assert cases.same_bits(out, e, nan_payload=False) and f == fe, (nx, flag)
        gpu_util.check_form(gpu_ctx, want, what=(nx, flag, "single"))


# ------------------------------------------------------------------------------------------------------------ switches
@pytest.mark.parametrize("nx,ny", [(8, 4), (9, 9)])
def test_switches_select_the_other_route(gpu_ctx, oracle, nx, ny, mifc_env):
    """MIFC_FUSED2=0, MIFC_SHAPIRO_FUSED=0 and MIFC_SHAPIRO_REGS=0 (at a width the filter's tile form takes, 8, and at one it
    does not, 9): the other route, the same bits, for batches and single fields."""
    g = grid(nx, ny)
    tags, flags = FLAG_PATTERNS["mixed"]

    def both(routes):
        check_batch(gpu_ctx, oracle, g, tags, flags, device=True, routes=routes)
        check_batch(gpu_ctx, oracle, g, tags[:1], flags[:1], device=False, routes=routes)
        for op in OPS:
            z, t = level(g, tags[3])
            out, f, route = run_single(gpu_ctx, g, op, z, t, SOME, device=True, p=PRESSURES[3])
            e, fe = reference(oracle, g, op, z, t, tags[3], SOME, PRESSURES[3])
            assert cases.same_bits(out, e, nan_payload=False) and f == fe, (op, nx)
            gpu_util.check_form(gpu_ctx, route_of(op, nx, routes), what=(op, nx, "single"))

    mifc_env("MIFC_FUSED2", "0")
    both({"two_stage": "two_stage_passes"})
    mifc_env("MIFC_FUSED2", None)
    mifc_env("MIFC_SHAPIRO_FUSED", "0")
    both({"filter": "shapiro_sweeps"})
    mifc_env("MIFC_SHAPIRO_FUSED", None)
    mifc_env("MIFC_SHAPIRO_REGS", "0")
    both({"filter": "shapiro_fused" if nx % 4 == 0 else "shapiro_sweeps"})


# ---------------------------------------------------------------------------------------------------- the filter in place
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("nx,ny", [(8, 4), (9, 9), (241, 3)])
def test_shapiro_in_place(gpu_ctx, oracle, nx, ny, fused, mifc_env):
    """field == fsmooth: a single field and a mixed-flag batch, on the one-launch route and sweep by sweep; the batch comes
    back in the caller's buffer."""
    import torch

    mifc_env("MIFC_SHAPIRO_FUSED", fused)
    want = "shapiro_fused" if fused == "1" else "shapiro_sweeps"
    g = grid(nx, ny)
    tags, flags = FLAG_PATTERNS["mixed"]
    z, t = batch(g, tags)
    dz = torch.from_numpy(z.copy()).cuda()
    out, fo = gpu_ctx.stencil_levels_ex("shapiro2_filter", dz, fdefined=np.asarray(flags, np.int32), out0=dz)
    gpu_util.check_form(gpu_ctx, want, what=(nx, "batch in place"))
    assert out.data_ptr() == dz.data_ptr() and np.all(fo == ALL)
    got = dz.cpu().numpy()
    for l, tag in enumerate(tags):
        e, _ = reference(oracle, g, "shapiro", z[l], t[l], tag, flags[l], 0.0)
        assert cases.same_bits(got[l], e, nan_payload=False), (nx, l)
    for l in (0, 1):
        d1 = torch.from_numpy(z[l].copy()).cuda()
        res = gpu_ctx.shapiro2_filter(d1, fdefined=int(flags[l]), out=d1)
        assert res is not None and res[0].data_ptr() == d1.data_ptr() and res[1] == ALL
        gpu_util.check_form(gpu_ctx, want, what=(nx, "single in place"))
        e, _ = reference(oracle, g, "shapiro", z[l], t[l], tags[l], flags[l], 0.0)
        assert cases.same_bits(d1.cpu().numpy(), e, nan_payload=False), (nx, l)


# ------------------------------------------------------------------------------------------------- per-level pressures
@pytest.mark.parametrize("nx,ny", [(9, 4), (241, 4)])
def test_qvector_pressures_follow_their_level(gpu_ctx, oracle, nx, ny):
    """A mixed-flag batch launches its levels in the order 1, 3, 0, 2, 4; the tables of the Q-vector's scalars are indexed by
    level.  Each level's result is the one of ITS pressure (and of no other level's: the pressures change the bits)."""
    g = grid(nx, ny)
    tags = ["h0", "c1", "h2", "c3", "h4"]
    flags = [SOME, ALL, SOME, ALL, SOME]
    check_batch(gpu_ctx, oracle, g, tags, flags, device=True, ops=["q1", "q2", "q3", "q4"])
    z, t = batch(g, tags)
    for op in ("q2", "q3"):
        own = reference(oracle, g, op, z[1], t[1], tags[1], ALL, PRESSURES[1])[0]
        other = reference(oracle, g, op, z[1], t[1], tags[1], ALL, PRESSURES[3])[0]
        assert not cases.same_bits(own, other, nan_payload=False)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(gpu_ctx):
    """A non-positive pressure in the middle of level_scalars, compute = 7 and nx = 2: refused (None through the Python front),
    the output buffer and the flags as they were."""
    from mi_fieldcalc_amd._batched import _BatchedOps

    nlev = 3

    def raw(op, nx, ny, pres, compute):
        """mifc_stencil_levels_ex on host arrays, the flag table the caller's own"""
        g = grid(nx if nx >= 3 else 8, ny)
        z = np.full((nlev, ny, nx), 5500.0, np.float32)
        z[:, 1, 1] = 5510.0
        maps = [np.ascontiguousarray(a[:, :nx]) for a in (g["xm"], g["ym"], g["fc"])]
        out = np.full((nlev, ny, nx), SENTINEL, np.float32)
        flags = np.array([SOME, ALL, 77], np.int32)  # 77: no flag value, so a rewritten table shows
        before = flags.copy()
        code = _BatchedOps.OPS_EX[op]
        gpu_ctx.set_stream(None)
        rc = gpu_ctx._call("mifc_stencil_levels_ex", [code, nx, ny, nlev, z, z.copy(), None, maps[0], maps[1], maps[2], pres, 0.0, compute, out, None,
                                                      flags, float(UNDEF), 0])
        assert rc == 0, (op, nx, compute)
        assert np.all(out == SENTINEL) and np.array_equal(flags, before), (op, nx, compute)
        front = gpu_ctx.stencil_levels_ex(op, z, z.copy() if op == "plevelqvector" else None, None, maps[0], maps[1], maps[2],
                                          level_scalars=pres, compute=compute, fdefined=before[:2].tolist() + [SOME], out0=out)
        assert front is None and np.all(out == SENTINEL), (op, nx, compute)

    good = np.array([850.0, 700.0, 500.0], np.float32)
    raw("plevelqvector", 9, 4, np.array([850.0, 0.0, 500.0], np.float32), 1)
    raw("plevelqvector", 9, 4, np.array([850.0, -700.0, 500.0], np.float32), 3)
    raw("plevelqvector", 9, 4, good, 7)
    for op in ("thermalFrontParameter", "plevelqvector", "shapiro2_filter"):
        raw(op, 2, 4, good, 1)
    # the single-field entries
    g = grid(9, 4)
    z, t = level(g, "c0")
    out = np.full(z.shape, SENTINEL, np.float32)
    assert gpu_ctx.plevelqvector(z, t, g["xm"], g["ym"], g["fc"], 0.0, 1, fdefined=SOME, out=out) is None
    assert gpu_ctx.plevelqvector(z, t, g["xm"], g["ym"], g["fc"], 700.0, 7, fdefined=SOME, out=out) is None
    two = np.zeros((4, 2), np.float32)
    out2 = np.full((4, 2), SENTINEL, np.float32)
    assert gpu_ctx.thermalFrontParameter(two, two, two, fdefined=SOME, out=out2) is None
    assert gpu_ctx.plevelqvector(two, two, two, two, two, 700.0, 1, fdefined=SOME, out=out2) is None
    assert gpu_ctx.shapiro2_filter(two, fdefined=SOME, out=out2) is None
    assert np.all(out == SENTINEL) and np.all(out2 == SENTINEL)
