"""Vector pairs sampled at arbitrary points and rotated in the same pass on the GPU (the ROTATE form of mifc_hinterp.hip,
mifc_hinterp_vector_levels) against the numpy restatement (tests/vrotate_restate.py: hinterp_restate.sample of every
component, then rule R): bit for bit (a NaN matches any NaN), flags equal, the three methods, host and device memory."""
import ctypes
import functools

import numpy as np
import pytest

import hinterp_restate as hi
import vinterp_restate as vi
import vrotate_restate as vr
from cases import same_bits
from gpu_util import run_is_forced

pytestmark = pytest.mark.gpu

MIXED = [hi.ALL_DEFINED, hi.SOME_DEFINED, hi.NONE_DEFINED]
NAMES = {code: name for name, code in hi.METHODS.items()}
METHODS = (("nearest", hi.NEAREST), (hi.BILINEAR, hi.BILINEAR), ("bicubic", hi.BICUBIC))  # (what the call is given: a name or a code, the restatement's)


def compare(got, exp, gfd, efd, label):
    assert got.shape == exp.shape, (label, got.shape, exp.shape)
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if not same_bits(got, exp, nan_payload=False):
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))


@functools.lru_cache(maxsize=None)
def base(npairs=1, nlev=5, ny=9, nx=13, npos=600, seed=1):
    case = vr.point_case(npairs, nlev, ny, nx, npos, seed)  # 3 % of the points with an undefined coefficient
    for a in case:
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def expected(npairs, nlev, ny, nx, npos, seed, code, flags=None, fdef_rot=vr.SOME_DEFINED):
    """The restatement of a base() case, computed once (flags: bytes of the int32 table, or None)."""
    fields, x, y, c, s = base(npairs, nlev, ny, nx, npos, seed)
    fl = None if flags is None else np.frombuffer(flags, np.int32).reshape(2 * npairs, nlev)
    return vr.sample_rotate(fields, x, y, c, s, code, fl, fdef_rot)


def run(ctx, case, method, device, flags=None, fdef_rot=vr.SOME_DEFINED, undef=hi.UNDEF, stacked=True):
    import torch

    fields, x, y, c, s = case
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    npairs = fields.shape[0] // 2
    f = put(fields.reshape((npairs, 2) + fields.shape[1:]))
    f = f if stacked else [(f[q, 0], f[q, 1]) for q in range(npairs)]
    res, fd = ctx.hinterp_vector_levels(f, put(x), put(y), put(c), put(s), method, fdefined_in=flags, fdef_rot=fdef_rot, undef=undef)
    res = res.cpu().numpy() if device else res
    return res.reshape((fields.shape[0], fields.shape[1]) + x.shape), fd.reshape(fields.shape[0], -1)


def check(ctx, key, method, device, flags=None, fdef_rot=vr.SOME_DEFINED, stacked=True, label=None):
    given, code = method
    got, fd = run(ctx, base(*key), given, device, flags, fdef_rot, stacked=stacked)
    exp, efd = expected(*key, code, None if flags is None else np.ascontiguousarray(flags, np.int32).tobytes(), fdef_rot)
    compare(got, exp, fd, efd, (label, code, "device" if device else "host"))


def form(ctx, **expected_keys):
    """The launch shape of the last call (the vector call reports through mifc_last_hinterp_form, nf = components per
    launch), checked key by key -- unless the run forces a path."""
    got = ctx.last_hinterp_form()
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("npairs", [1, 2, 3, 4])  # a launch takes 2 pairs, 1 with the bicubic method
def test_main_case_pairs_methods_and_memory(gpu_ctx, npairs, device):
    key = (npairs, 5, 9, 13, 600, 1)
    flags = np.random.default_rng(npairs).choice(MIXED, size=(2 * npairs, 5)).astype(np.int32)
    flags[0, :3], flags[1, :3] = MIXED, MIXED[::-1]
    for method in METHODS:
        check(gpu_ctx, key, method, device, stacked=(npairs != 3), label=("npairs", npairs))
        check(gpu_ctx, key, method, device, flags=flags, stacked=(npairs != 3), label=("npairs", npairs, "mixed flags"))
        per_launch = 2 if method[1] == hi.BICUBIC else 4
        form(gpu_ctx, method=NAMES[method[1]], nf=min(2 * npairs, per_launch), tested=1, launches=-(-2 * npairs // per_launch), blocks=3)
    exp, _ = expected(*key, hi.BILINEAR)
    assert (exp != hi.UNDEF).mean() >= 0.5


@pytest.mark.parametrize("npos", [1, 63, 64, 65, 256, 257, 1100])  # one lane, the wave seam, the workgroup seam, several workgroups
def test_points(gpu_ctx, npos):
    key = (2, 3, 9, 13, npos, 3)
    for device in (False, True):
        for method in METHODS:
            check(gpu_ctx, key, method, device, label=("npos", npos))
    form(gpu_ctx, blocks=-(-npos // 256))


@pytest.mark.parametrize("nlev", [1, 2, 3, 7])  # every remainder of the unroll
def test_levels(gpu_ctx, nlev):
    key = (2, nlev, 9, 13, 300, 4)
    flags = np.random.default_rng(nlev).choice(MIXED, size=(4, nlev)).astype(np.int32)
    for device in (False, True):
        for method in METHODS:
            check(gpu_ctx, key, method, device, flags=flags, label=("nlev", nlev))
    form(gpu_ctx, blocks=2, chunk=min(nlev, 2), level_chunks=-(-nlev // 2))  # (hinterp_plan, unchanged)


@pytest.mark.parametrize("shape", [(1, 13), (9, 1)], ids=["13x1", "1x9"])
def test_degenerate_grids(gpu_ctx, shape):
    ny, nx = shape
    key = (1, 3, ny, nx, 300, 5)
    fields, x, y, c, s = base(*key)
    zero = np.zeros_like(x)  # and points that are inside: on the one row / column
    on_the_line = (fields, x if ny == 1 else zero, zero if ny == 1 else y, c, s)
    for device in (False, True):
        for method in METHODS:
            check(gpu_ctx, key, method, device, label=shape)
            got, fd = run(gpu_ctx, on_the_line, method[0], device)
            exp, efd = vr.sample_rotate(*on_the_line, method[1])
            compare(got, exp, fd, efd, (shape, "on the line", method[1], device))
    assert (exp != hi.UNDEF).mean() > 0.5


def test_coefficient_flags_untested_instances_and_nan_as_undef(gpu_ctx):
    key = (2, 3, 9, 13, 600, 1)
    case = base(*key)
    every = np.full((4, 3), hi.ALL_DEFINED, np.int32)
    for device in (False, True):
        for method in METHODS:
            # the coefficients under ALL_DEFINED: a stored undef is a value, a NaN computes a NaN
            check(gpu_ctx, key, method, device, fdef_rot=vr.ALL_DEFINED, label="coefficients untested")
            form(gpu_ctx, tested=1)
            check(gpu_ctx, key, method, device, flags=every, label="fields untested, coefficients tested")
            form(gpu_ctx, tested=0)
            check(gpu_ctx, key, method, device, flags=every, fdef_rot=vr.ALL_DEFINED, label="nothing tested")
            form(gpu_ctx, tested=0)
            # NaN as undef, in the fields, the positions and the coefficients
            nan = np.float32(np.nan)
            cn = tuple(np.where(a == hi.UNDEF, nan, a) for a in case)
            got, fd = run(gpu_ctx, cn, method[0], device, undef=nan)
            exp, efd = vr.sample_rotate(*cn, method[1], undef=nan)
            compare(got, exp, fd, efd, ("undef = NaN", method[1], device))
    # no point with defined coefficients: every flag NONE_DEFINED, counted once per pair and level
    fields, x, y, c, s = case
    got, fd = run(gpu_ctx, (fields, x, y, np.full_like(c, hi.UNDEF), s), "bilinear", True, flags=every)
    assert (got == hi.UNDEF).all() and (fd == hi.NONE_DEFINED).all()


def test_equals_sampling_followed_by_rotation_on_the_device(gpu_ctx):
    """hinterp_levels, then vrotate_levels on the (nlev, 1, npos) batches with the flags of the first call: the same bits and
    flags as the one call.  The flags tell the truth here: the planes flagged ALL_DEFINED hold no undef (the second of two
    calls can recognise a hole only by its value, the one call carries it -- tests/vrotate_restate.py, sample_rotate)."""
    import torch

    fields, x, y, c, s = base(2, 5)
    flags = np.random.default_rng(7).choice(MIXED, size=(4, 5)).astype(np.int32)
    flags[0, :3], flags[1, :3] = MIXED, MIXED[::-1]
    honest = fields.copy()
    rng = np.random.default_rng(8)
    for g, k in zip(*np.nonzero(flags == hi.ALL_DEFINED)):
        bad = np.isnan(honest[g, k]) | (honest[g, k] == hi.UNDEF)
        honest[g, k][bad] = rng.normal(280, 10, int(bad.sum())).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    xd, yd, cd, sd = dev(x), dev(y), dev(c), dev(s)
    for given, code in METHODS:
        for f, fl in ((dev(fields), None), (dev(honest), flags)):
            for fdef_rot in (vr.SOME_DEFINED, vr.ALL_DEFINED):
                fused, ffd = gpu_ctx.hinterp_vector_levels(f.view(2, 2, 5, 9, 13), xd, yd, cd, sd, given, fdefined_in=fl, fdef_rot=fdef_rot)
                sampled, sfd = gpu_ctx.hinterp_levels(f, xd, yd, given, fdefined_in=fl)
                two, tfd = gpu_ctx.vrotate_levels(sampled.view(2, 2, 5, 1, 600), cd.view(1, 600), sd.view(1, 600), fdefined_in=sfd, fdef_rot=fdef_rot)
                compare(fused.cpu().numpy().reshape(4, 5, 600), two.cpu().numpy().reshape(4, 5, 600), ffd.reshape(4, 5), tfd.reshape(4, 5),
                        ("fused against two calls", code, fl is not None, fdef_rot))
        assert (fused.cpu().numpy() != hi.UNDEF).mean() >= 0.5


def test_device_arguments_offset_by_one_float_and_out(gpu_ctx):
    import torch

    fields, x, y, c, s = base(1, 5)
    n, npos = fields[0].size, x.size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
    pair = [buf[1 + j * n:1 + (j + 1) * n].view(5, 9, 13) for j in range(2)]  # 4 bytes past the 16-byte grid
    pos = torch.zeros(4 * npos + 5, dtype=torch.float32, device="cuda")
    views = []
    for j, a in enumerate((x, y, c, s)):
        views.append(pos[j * (npos + 1) + 1:j * (npos + 1) + 1 + npos].copy_(torch.from_numpy(a).cuda()))
    sentinel = np.float32(-4242.5)
    obuf = torch.full((2 * 5 * npos + 2,), float(sentinel), dtype=torch.float32, device="cuda")
    for given, code in METHODS:
        out, fd = gpu_ctx.hinterp_vector_levels(pair, *views, given, out=obuf[1:-1].view(2, 5, npos))
        exp, efd = expected(1, 5, 9, 13, 600, 1, code)
        compare(out.cpu().numpy(), exp, fd, efd, ("offset by one float", code))
        assert float(obuf[0]) == sentinel and float(obuf[-1]) == sentinel
    # 2-D positions: a regrid gives (2, nlev) + S
    out, fd = gpu_ctx.hinterp_vector_levels(torch.from_numpy(fields).cuda(), *[torch.from_numpy(a.reshape(20, 30)).cuda() for a in (x, y, c, s)])
    assert tuple(out.shape) == (2, 5, 20, 30) and fd.shape == (2, 5)
    exp, efd = expected(1, 5, 9, 13, 600, 1, hi.BILINEAR)
    compare(out.cpu().numpy().reshape(2, 5, 600), exp, fd, efd, "regrid shape")
    with pytest.raises(ValueError):
        gpu_ctx.hinterp_vector_levels(fields, x, y, c[:-1], s)
    with pytest.raises(ValueError):
        gpu_ctx.hinterp_vector_levels(fields, x, y, c, s, out=np.zeros((2, 5, 599), np.float32))


def test_host_call_in_several_level_chunks(gpu_ctx, mifc_env):
    mifc_env("MIFC_HINTERP_CHUNK_MIB", 1)
    # 4 fields x (100 x 111 cells + 500 points) x 4 bytes = 185 600 bytes per level: five levels per chunk, 12 levels in three
    fields, x, y, c, s = vr.point_case(2, 12, 100, 111, 500, 9)
    flags = np.random.default_rng(9).choice(MIXED, size=(4, 12)).astype(np.int32)
    for method in METHODS:
        got, fd = run(gpu_ctx, (fields, x, y, c, s), method[0], False, flags=flags)
        exp, efd = vr.sample_rotate(fields, x, y, c, s, method[1], flags)
        compare(got, exp, fd, efd, ("level chunks", method[1]))
        form(gpu_ctx, launches=3 * (2 if method[1] == hi.BICUBIC else 1), blocks=2)


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    npairs, nlev, ny, nx, npos = 1, 3, 5, 8, 70
    nf = 2
    fields_h, x_h, y_h, c_h, s_h = base(npairs, nlev, ny, nx, npos, 2)
    res = nlev * npos
    # room of the test's own around the fields and around cosa: an output (longer than a field here) that begins in a field
    # or ends in cosa stays inside it, whatever else the allocator has put nearby
    batch = nlev * ny * nx
    room = torch.zeros(res + nf * batch + res, dtype=torch.float32, device="cuda")
    x = room[res:res + nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(fields_h))
    xp, yp, sp = (torch.from_numpy(a).cuda() for a in (x_h, y_h, s_h))
    croom = torch.zeros(res + npos + res, dtype=torch.float32, device="cuda")
    cp = croom[res:res + npos].copy_(torch.from_numpy(c_h))
    sentinel = -4242.5
    outs = torch.full((nf, nlev, npos), sentinel, dtype=torch.float32, device="cuda")

    def call(nlev_=nlev, npairs_=npairs, npos_=npos, method=1, out_ptrs=None, cos_=0, sin_=0, sync=True):
        tab = (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs is None else out_ptrs))
        fd = np.full(nf * nlev, 7, np.int32)
        rc = lib.mifc_hinterp_vector_levels(c, nx, ny, nlev_, ctypes.addressof(tab), None, npairs_, npos_, xp.data_ptr(), yp.data_ptr(),
                                            cp.data_ptr() if cos_ == 0 else cos_, sp.data_ptr() if sin_ == 0 else sin_, vr.SOME_DEFINED, method,
                                            ctypes.addressof(o), fd.ctypes.data, float(hi.UNDEF), 1)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    null_head = "a null pointer (fields, xpos, ypos, cosa, sina, fres or fdefined_out)"
    refusals = {
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "npairs 0": (dict(npairs_=0), "npairs 0 outside 1..4"),
        "npairs 5": (dict(npairs_=5), "npairs 5 outside 1..4"),
        "npos 0": (dict(npos_=0), "npos < 1"),
        "unknown method": (dict(method=3), "unknown method 3"),
        "null cosa": (dict(cos_=None), null_head),
        "null sina": (dict(sin_=None), null_head),
        "output is sina": (dict(out_ptrs=[outs[0].data_ptr(), sp.data_ptr()]), "fres[1] overlaps sina"),
        "output ends in cosa": (dict(out_ptrs=[cp.data_ptr() - 4 * (res - 1), outs[1].data_ptr()]), "fres[0] overlaps cosa"),
        "output is a field": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
    }
    for what, (kw, tail) in refusals.items():
        rc, err, fd = call(**kw)
        assert rc == 0 and err == "mifc_hinterp_vector_levels: " + tail, (what, err)
        assert (outs == sentinel).all().item() and (fd == 7).all(), what
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, fd = call(sync=False)
    g.close()
    assert rc == 0 and "capture" in err and (fd == 7).all() and (outs == sentinel).all().item()
    rc, err, fd = call()
    assert rc == 1 and err == "" and (fd != 7).all(), err
    exp, efd = expected(npairs, nlev, ny, nx, npos, 2, hi.BILINEAR)
    compare(outs.cpu().numpy(), exp, fd.reshape(nf, nlev), efd, "after the refusals")


def test_section_wind_along_and_across_on_pressure_surfaces(gpu_ctx):
    """The recipe: wind along a line of 65 points rotated to its along- and across-section components while it is sampled,
    pressure sampled beside it, then vinterp_fields of the (12, 1, 65) batches to three surfaces -- bit for bit the
    restatements chained the same way."""
    import torch

    rng = np.random.default_rng(33)
    nlev, ny, nx, npos = 12, 9, 13, 65
    alevel, blevel = vi.hybrid_levels(nlev)
    ps = rng.uniform(700, 1050, (ny, nx)).astype(np.float32)
    p = vi.hybrid_coordinate(ps, alevel, blevel)
    u = hi.sprinkle((10 + 20 * (1 - p / 1000.0) + rng.normal(0, 1, p.shape)).astype(np.float32), rng, 0.02, hi.UNDEF)
    v = hi.sprinkle((-5 + rng.normal(0, 2, p.shape)).astype(np.float32), rng, 0.02, hi.UNDEF)
    t = np.linspace(0, 1, npos)
    x, y = (0.4 + 12.2 * t).astype(np.float32), (7.9 - 7.1 * t * t).astype(np.float32)  # (the last points leave the grid)
    # the section's direction at every point: along = c u + s v, across = -s u + c v -- rule R with (c, -s)
    dx, dy = np.gradient(x.astype(np.float64)), np.gradient(y.astype(np.float64))
    norm = np.hypot(dx, dy)
    c, s = (dx / norm).astype(np.float32), (-dy / norm).astype(np.float32)
    targets = np.array([850, 500, 300], np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for given, code in METHODS:
        wind, wfd = gpu_ctx.hinterp_vector_levels([dev(u), dev(v)], dev(x), dev(y), dev(c), dev(s), given, fdef_rot=vr.ALL_DEFINED)
        psec, pfd = gpu_ctx.hinterp_levels(dev(p), dev(x), dev(y), given)
        assert wind.is_cuda and tuple(wind.shape) == (2, nlev, npos) and wfd.shape == (2, nlev)
        ewind, ewfd = vr.sample_rotate(np.stack([u, v]), x, y, c, s, code, fdef_rot=vr.ALL_DEFINED)
        epsec, epfd = hi.sample(p[None], x, y, code)
        compare(wind.cpu().numpy(), ewind, wfd, ewfd, ("section wind", code))
        on_p, ofd = gpu_ctx.vinterp_fields(wind.view(2, nlev, 1, npos), psec.view(nlev, 1, npos), targets, fdefined_in=wfd, fdef_coord=pfd)
        e_on_p, e_ofd = vi.coord_fields(ewind.reshape(2, nlev, 1, npos), epsec.reshape(nlev, 1, npos), targets, vi.LINEAR, ewfd, epfd[0])
        assert on_p.is_cuda and tuple(on_p.shape) == (2, 3, 1, npos)
        compare(on_p.cpu().numpy(), e_on_p, ofd, e_ofd, ("section wind on pressure surfaces", code))
        assert (e_on_p != hi.UNDEF).mean() > 0.3
