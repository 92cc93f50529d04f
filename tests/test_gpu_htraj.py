"""Trajectories through a series of wind level batches on the GPU (mifc_htraj.hip, mifc_htraj_levels) against the
restatement (tests/htraj_restate.py): positions, traces and flags, every comparison for equality (a NaN matches a NaN) --
the definition is bit for bit, whatever the memory kind, the alignment or the staging.  The seeded cases are two full
workgroups and a tail; the seam cases (tests/htraj_cases.py) are a few particles each.  No test places a particle or a
pointer so as to provoke a fault: out-of-grid and NaN positions are ordinary inputs with a defined result, undef."""
import ctypes

import numpy as np
import pytest

import htraj_cases as hc
import htraj_restate as ht
from gpu_util import run_is_forced
from mi_fieldcalc_amd import htraj  # (without the feature the file fails here)

pytestmark = pytest.mark.gpu

A, S, N = ht.ALL_DEFINED, ht.SOME_DEFINED, ht.NONE_DEFINED
U = ht.UNDEF


def put(a, device, off_grid=False):
    """A numpy array as it is (host), or on the device -- off_grid: one float behind a 16-byte boundary."""
    import torch

    a = np.ascontiguousarray(a, np.float32)
    if not device:
        return a
    if not off_grid:
        return torch.from_numpy(a.copy()).cuda()  # (a copy: the shared cases are read-only)
    buf = torch.zeros(a.size + 5, dtype=torch.float32, device="cuda")
    skip = 1 + (-(buf.data_ptr() // 4) % 4)  # the first element 4 bytes behind the grid
    view = buf[skip:skip + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    assert view.data_ptr() % 16 == 4
    return view


def back(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def call(ctx, case, device, off_grid=False):
    """A case (the arguments of htraj_restate.run) through the front: (x, y, trace (ntrace, ...), flags) as numpy."""
    c = dict(case)
    nt = c["u"].shape[0]
    trace = c.pop("trace", None)
    tr = [] if trace is None else [[put(trace[f, j], device, off_grid) for j in range(nt)] for f in range(trace.shape[0])]
    res = htraj.trajectories(ctx, [put(c["u"][j], device, off_grid) for j in range(nt)], [put(c["v"][j], device, off_grid) for j in range(nt)], c["times"],
                             put(c["xmapr"], device, off_grid), put(c["ymapr"], device, off_grid), put(c["xpos"], device, off_grid),
                             put(c["ypos"], device, off_grid), start=c.get("j_start", 0), end=c.get("j_end", -1), nsub=c.get("nsub", 4), niter=c.get("niter", 2),
                             trace=tr, fdefined_in=c.get("fdefined_in"), fdef_map=c.get("fdef_map", S), fdef_trace=c.get("fdef_trace"), undef=c.get("undef", U))
    x = back(res["x"])
    t = np.stack([back(t) for t in res["trace"]]) if res["trace"] else np.zeros((0,) + x.shape, np.float32)
    return x, back(res["y"]), t, res["flags"]


def assert_same(got, exp, label):
    for name, g, e in zip(("x", "y", "trace", "flags"), got, exp):
        assert g.shape == e.shape and g.dtype == e.dtype, (label, name, g.shape, e.shape, g.dtype)
        if not ht.same(g, e):
            bits = np.uint32 if g.dtype == np.float32 else np.int32
            bad = np.argwhere((g.view(bits) != e.view(bits)) & ~((g != g) & (e != e)))
            first = tuple(int(b) for b in bad[0])
            raise AssertionError("%s: %d values of %s differ; first %s got %r expected %r" % (label, len(bad), name, first, g[first], e[first]))


def form(ctx, **expected_keys):
    """The launch shape of the last call, checked key by key -- unless the run forces a path."""
    got = htraj.last_htraj_form(ctx)
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


# ------------------------------------------------------------------------------------- the seeded and the seam cases
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nsub,niter", ht.SCHEMES)
@pytest.mark.parametrize("seed", ht.SEEDS)
def test_seeded_cases(gpu_ctx, seed, nsub, niter, device):
    args, exp = ht.seeded(seed, nsub, niter)
    assert_same(call(gpu_ctx, args, device), exp, ("seed", seed, nsub, niter, device))
    form(gpu_ctx, niter=niter, nsub=nsub, ntrace=2, tested=1, blocks=3, level_chunks=1, chunk=1, intervals=3, launches=3, staged=0 if device else 1)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", hc.NAMES)
def test_seam_cases(gpu_ctx, name, device):
    case = hc.cases()[name]
    assert_same(call(gpu_ctx, case, device), hc.expected(name), (name, device))
    nt, nlev = case["u"].shape[:2]
    intervals = abs((case["j_end"] % nt) - (case["j_start"] % nt))
    got = form(gpu_ctx, niter=case["niter"], nsub=case["nsub"], ntrace=0 if case["trace"] is None else case["trace"].shape[0], intervals=intervals,
               launches=intervals, blocks=1, level_chunks=nlev, chunk=1, staged=0 if device else 1)
    if name == "every flag ALL_DEFINED" and not run_is_forced():
        assert got["tested"] == 0


# ------------------------------------------------------------------------------------------------------- placement
@pytest.fixture(scope="module")
def tall():
    """Five levels of 150 x 120 cells with different winds, 70 particles, a trace field: 432 000 bytes of slice buffers and
    2 520 of slots per level -- two levels fit a MiB, the call takes three chunks."""
    rng = np.random.default_rng(77)
    nt, nlev, ny, nx, npos = 3, 5, 120, 150, 70
    u = ht.sprinkle(rng.uniform(-30, 30, (nt, nlev, ny, nx)).astype(np.float32), rng, 0.01, U)
    v = rng.uniform(-30, 30, (nt, nlev, ny, nx)).astype(np.float32)
    trace = ht.sprinkle(rng.normal(280, 10, (1, nt, nlev, ny, nx)).astype(np.float32), rng, 0.03, U)
    args = dict(u=u, v=v, times=np.array([0.0, 3600.0, 9000.0]), xmapr=(1.0e-4 * rng.uniform(0.9, 1.1, (ny, nx))).astype(np.float32),
                ymapr=(1.0e-4 * rng.uniform(0.9, 1.1, (ny, nx))).astype(np.float32), xpos=rng.uniform(0, nx - 1, npos).astype(np.float32),
                ypos=rng.uniform(0, ny - 1, npos).astype(np.float32), j_start=0, j_end=2, nsub=2, niter=1, trace=trace, undef=U)
    exp = ht.run(**args)
    alive = (exp[0][-1] != U).sum(axis=1)
    assert (alive > 5).all() and (alive < npos).all() and not ht.same(exp[0][2, 0], exp[0][2, 1])  # every level its own trajectories
    return args, exp


def test_device_memory_on_and_off_the_16_byte_grid(gpu_ctx, tall):
    args, exp = tall
    for off_grid in (False, True):
        assert_same(call(gpu_ctx, args, True, off_grid), exp, ("off grid", off_grid))
        form(gpu_ctx, blocks=1, level_chunks=5, chunk=1, intervals=2, launches=2, staged=0, tested=1, ntrace=1)
    args, exp = ht.seeded(ht.SEEDS[0], 3, 3)
    assert_same(call(gpu_ctx, args, True, True), exp, "seeded, off the grid")


def test_host_memory_in_several_level_chunks(gpu_ctx, mifc_env, tall):
    args, exp = tall
    assert_same(call(gpu_ctx, args, False), exp, "one chunk")
    form(gpu_ctx, staged=1, launches=2, level_chunks=5)
    mifc_env("MIFC_HTRAJ_CHUNK_MIB", 1)
    assert_same(call(gpu_ctx, args, False), exp, "a MiB")
    form(gpu_ctx, staged=3, launches=6, level_chunks=1, chunk=1, intervals=2)  # levels 0-1, 2-3, 4: the last chunk is one level
    back_args = dict(args, j_start=2, j_end=0)
    assert_same(call(gpu_ctx, back_args, False), ht.run(**back_args), "a MiB, backward")
    form(gpu_ctx, staged=3, launches=6)


def test_forced_levels_per_workgroup(gpu_ctx, mifc_env, tall):
    args, exp = tall
    for chunk in (1, 2, 5, 50):  # one level per workgroup, a remainder, one chunk, more than there are
        mifc_env("MIFC_HTRAJ_LEVEL_CHUNK", chunk)
        for device in (False, True):
            assert_same(call(gpu_ctx, args, device), exp, ("levels per workgroup", chunk, device))
            form(gpu_ctx, chunk=min(chunk, 5), level_chunks=-(-5 // min(chunk, 5)), launches=2)


# ------------------------------------------------------------------------------------------------------ properties
def test_a_level_of_a_batch_equals_the_call_on_that_level(gpu_ctx, tall):
    args, _ = tall
    whole = call(gpu_ctx, args, True)
    for k in range(5):
        one = call(gpu_ctx, dict(args, u=args["u"][:, k:k + 1], v=args["v"][:, k:k + 1], trace=args["trace"][:, :, k:k + 1]), True)
        assert_same(one, (whole[0][:, k:k + 1], whole[1][:, k:k + 1], whole[2][:, :, k:k + 1], whole[3][:, :, k:k + 1]), ("level", k))


def test_a_shuffle_of_the_particles_shuffles_the_results(gpu_ctx):
    args, exp = ht.seeded(ht.SEEDS[2], 3, 3)
    order = np.random.default_rng(3).permutation(args["xpos"].size)
    for device in (False, True):
        got = call(gpu_ctx, dict(args, xpos=args["xpos"][order], ypos=args["ypos"][order]), device)
        assert_same(got, (exp[0][..., order], exp[1][..., order], exp[2][..., order], exp[3]), ("shuffled", device))


def test_a_run_composes_from_its_intervals(gpu_ctx):
    args, exp = ht.seeded(ht.SEEDS[3], 3, 3)
    for device in (False, True):
        whole = call(gpu_ctx, dict(args, j_start=0, j_end=2), device)
        first = call(gpu_ctx, dict(args, j_start=0, j_end=1), device)
        rest = call(gpu_ctx, dict(args, xpos=first[0][1, 0], ypos=first[1][1, 0], j_start=1, j_end=2), device)
        assert_same(first, tuple(w[..., :2, :, :] for w in whole[:3]) + (whole[3][:, :2],), ("j0 -> j1", device))
        assert_same(rest, tuple(w[..., 1:, :, :] for w in whole[:3]) + (whole[3][:, 1:],), ("j1 -> j2", device))
        assert_same(whole, tuple(e[..., :3, :, :] for e in exp[:3]) + (exp[3][:, :3],), ("j0 -> j2", device))


def test_every_trace_slot_equals_hinterp_at_the_slot(gpu_ctx, tall):
    for args, label in ((tall[0], "tall"), (ht.seeded(ht.SEEDS[0], 1, 0)[0], "seeded"), (hc.cases()["backward"], "backward")):
        x, y, tr, fl = call(gpu_ctx, args, True)
        nt = args["u"].shape[0]
        j_start, j_end = (args.get("j_start", 0) % nt, args.get("j_end", -1) % nt)
        d = 1 if j_end > j_start else -1
        for f in range(tr.shape[0]):
            for n in range(x.shape[0]):
                for k in range(x.shape[1]):
                    plane = np.ascontiguousarray(args["trace"][f, j_start + n * d, k:k + 1])
                    s, sfl = gpu_ctx.hinterp_levels(plane, x[n, k], y[n, k], "bilinear", undef=args["undef"])
                    assert ht.same(s[0], tr[f, n, k]) and sfl[0] == fl[1 + f, n, k], (label, f, n, k)


# -------------------------------------------------------------------------------------------------------- refusals
def raw_call(ctx, device, fill=-4242.5, capture=False, **kw):
    """The C entry itself with pre-filled outputs: (return code or the RuntimeError's text, the outputs as numpy).
    capture: the call is made while a graph capture is open (device memory; nothing may synchronise inside it)."""
    import torch

    from mi_fieldcalc_amd import MEM_DEVICE
    from mi_fieldcalc_amd._args import _Arg, _pointer_table

    base = hc.small(21, nt=3, nlev=2, npos=9, ntrace=1)
    a = dict(nx=6, ny=5, nlev=2, nt=3, npos=9, ntrace=1, nslots=3, fdef_map=S, null=(), overlap=None, memkind=None)
    a.update({k: base[k] for k in ("times", "j_start", "j_end", "nsub", "niter", "undef")})
    a.update(kw)
    u, v, tr = ([put(base[name][j] if name != "trace" else base[name][0, j], device) for j in range(3)] for name in ("u", "v", "trace"))
    xm, ym, xp, yp = (put(base[name], device) for name in ("xmapr", "ymapr", "xpos", "ypos"))
    outs = [put(np.full((a["nslots"], 2, 9), fill, np.float32), device) for _ in range(3)]
    if a["overlap"] == "xres on u[1]":
        outs[0] = u[1].view(-1)[:54] if device else u[1].reshape(-1)[:54]
    if a["overlap"] == "tres[0] on yres":
        outs[2] = outs[1]
    if a["overlap"] == "yres on xpos0":
        xp = outs[1].view(-1)[:9] if device else outs[1].reshape(-1)[:9]
    fields = [_Arg(x) for x in u + v + tr + [xm, ym, xp, yp] + outs]
    addr = {name: _Arg(x).addr for name, x in (("xmapr", xm), ("ymapr", ym), ("xpos0", xp), ("ypos0", yp), ("xres", outs[0]), ("yres", outs[1]))}
    tu, tv, tt, to = (_pointer_table([_Arg(x).addr for x in xs]) for xs in (u, v, tr, outs[2:]))
    if "u[1]" in a["null"]:
        tu[1] = None
    if "trace[2]" in a["null"]:
        tt[2] = None
    if "tres[0]" in a["null"]:
        to[0] = None
    tables = {"u": ctypes.addressof(tu), "v": ctypes.addressof(tv), "trace": ctypes.addressof(tt), "tres": ctypes.addressof(to)}
    get = lambda name, value: None if name in a["null"] else value  # noqa: E731
    fd = np.full((2, a["nslots"], 2), -9, np.int32)
    times = None if a["times"] is None else np.ascontiguousarray(a["times"], np.float64)
    args = [a["nx"], a["ny"], a["nlev"], a["nt"], get("u", tables["u"]), get("v", tables["v"]), None, times, get("xmapr", addr["xmapr"]),
            get("ymapr", addr["ymapr"]), a["fdef_map"], a["npos"], get("xpos0", addr["xpos0"]), get("ypos0", addr["ypos0"]), a["j_start"], a["j_end"], a["nsub"],
            a["niter"], get("trace", tables["trace"]), None, a["ntrace"], get("xres", addr["xres"]), get("yres", addr["yres"]), get("tres", tables["tres"]),
            get("fdefined_out", fd), float(np.float32(a["undef"]))]
    def invoke():
        try:
            if capture:
                return ctx._call("mifc_htraj_levels", args + [MEM_DEVICE])
            if a["memkind"] is None:
                return ctx._launch("mifc_htraj_levels", fields, args)
            return ctx._call("mifc_htraj_levels", args + [a["memkind"]])
        except RuntimeError as err:
            return str(err)

    if capture:
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with ctx.graph_capture() as g:
            ctx.zero_counts_enqueue(counts)
            rc = invoke()
        g.close()
    else:
        rc = invoke()
    return rc, [back(o) for o in outs], fd


REFUSALS = [
    (dict(nt=1, j_end=0), "nt < 2"), (dict(nlev=0), "nlev < 1"), (dict(npos=0), "npos < 1"), (dict(nx=0), "nx < 1 or ny < 1"), (dict(ny=-1), "nx < 1 or ny < 1"),
    (dict(nx=(1 << 24) + 1), "nx or ny above 2^24"), (dict(nx=1 << 24, ny=128), "more than 2^31 - 1 cells per level"),
    (dict(j_start=3), "j_start or j_end outside 0..nt-1"), (dict(j_end=-1), "j_start or j_end outside 0..nt-1"), (dict(j_start=1, j_end=1), "j_start == j_end"),
    (dict(nsub=0), "nsub outside 1..64"), (dict(nsub=65), "nsub outside 1..64"), (dict(niter=-1), "niter outside 0..8"), (dict(niter=9), "niter outside 0..8"),
    (dict(ntrace=-1), "ntrace outside 0..4"), (dict(ntrace=5), "ntrace outside 0..4"), (dict(times=[0.0, np.inf, 2.0]), "a time of the used slices is not finite"),
    (dict(times=[0.0, np.nan, 2.0]), "a time of the used slices is not finite"), (dict(times=[0.0, 2.0, 2.0]), "the times of the used slices are not strictly increasing"),
    (dict(times=[2.0, 1.0, 0.0], j_start=2, j_end=0), "the times of the used slices are not strictly increasing"),
    (dict(undef=0.0), "undef is a position inside the grid"), (dict(undef=5.0), "undef is a position inside the grid"),
    (dict(times=None), "a null pointer (times)"), (dict(null=("u",)), "a null pointer (u, v,"), (dict(null=("xmapr",)), "a null pointer (u, v,"),
    (dict(null=("ypos0",)), "a null pointer (u, v,"), (dict(null=("yres",)), "a null pointer (u, v,"), (dict(null=("fdefined_out",)), "a null pointer (u, v,"),
    (dict(null=("trace",)), "a null pointer (trace or tres)"), (dict(null=("tres",)), "a null pointer (trace or tres)"),
    (dict(null=("u[1]",)), "a null pointer (u[1] or v[1])"), (dict(null=("trace[2]",)), "a null pointer (trace[2])"), (dict(null=("tres[0]",)), "a null pointer (tres[0])"),
    (dict(overlap="xres on u[1]"), "xres overlaps u[1]"), (dict(overlap="tres[0] on yres"), "overlaps"), (dict(overlap="yres on xpos0"), "yres overlaps xpos0"),
    (dict(memkind=7), "unknown memkind 7"),
]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_every_refusal_returns_0_writes_nothing_and_names_its_reason(gpu_ctx, device):
    for kw, reason in REFUSALS:
        rc, outs, fd = raw_call(gpu_ctx, device, **kw)
        assert isinstance(rc, str) and rc.startswith("mifc_htraj_levels: mifc_htraj_levels: ") and reason in rc, (kw, rc)
        if kw.get("overlap") is None:
            assert all((o == np.float32(-4242.5)).all() for o in outs) and (fd == -9).all(), kw
    # a null trace, tres and fdef_trace are fine without trace fields; times outside the used range are not looked at
    rc, outs, fd = raw_call(gpu_ctx, device, ntrace=0, null=("trace", "tres"))
    assert rc is True and (outs[2] == np.float32(-4242.5)).all() and not (outs[0] == np.float32(-4242.5)).any() and (fd[0] != -9).all() and (fd[1] == -9).all()
    rc, outs, fd = raw_call(gpu_ctx, device, times=[np.nan, 1.0, 2.0], j_start=1, j_end=2, nslots=2)
    assert rc is True and (fd != -9).all()
    rc, outs, fd = raw_call(gpu_ctx, device, undef=np.nan)
    assert rc is True
    # afterwards the calls run as ever
    args, exp = ht.seeded(ht.SEEDS[0], 1, 0)
    assert_same(call(gpu_ctx, args, device), exp, "after the refusals")


def test_refused_while_a_capture_is_open(gpu_ctx):
    rc, outs, fd = raw_call(gpu_ctx, True, capture=True)
    assert isinstance(rc, str) and "not available while a mifc_graph capture is open" in rc, rc
    assert all((o == np.float32(-4242.5)).all() for o in outs) and (fd == -9).all()
    rc, outs, fd = raw_call(gpu_ctx, True)  # afterwards the same call runs
    assert rc is True and not (outs[0] == np.float32(-4242.5)).any() and (fd != -9).all()
