"""Level batches sampled at arbitrary points on the GPU (mifc_hinterp.hip, mifc_hinterp_levels) against the numpy
restatement (tests/hinterp_restate.py): bit for bit (a NaN matches any NaN), flags equal, the three methods, host and device
memory.  No tolerance: every operation of the definition is an IEEE float or double operation rounded on its own, and the
library is built without contraction."""
import ctypes
import functools

import numpy as np
import pytest

import hinterp_restate as hi
import vinterp_restate as vi
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


def run(ctx, fields, x, y, method, device, flags=None, undef=hi.UNDEF, stacked=True, out=None):
    import torch

    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    f = put(fields)
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    res, fd = ctx.hinterp_levels(f, put(x), put(y), method, fdefined_in=flags, undef=undef, out=out)
    return (res.cpu().numpy() if device else res), fd


def check(ctx, fields, x, y, method, device, flags=None, undef=hi.UNDEF, stacked=True, label=None):
    given, code = method
    got, fd = run(ctx, fields, x, y, given, device, flags, undef, stacked)
    exp, efd = expected(fields, x, y, code, flags, undef)
    compare(got, exp, fd, efd, (label, code, "device" if device else "host"))


def expected(fields, x, y, code, flags=None, undef=hi.UNDEF):
    if flags is not None and np.size(flags) == len(fields) != np.size(fields[:, :, 0, 0]):  # one flag per field stands for every level
        flags = np.repeat(np.asarray(flags).reshape(-1, 1), fields.shape[1], axis=1)
    return hi.sample(fields, x, y, code, flags, undef)


@functools.lru_cache(maxsize=None)
def base(nf=3, nlev=5, ny=9, nx=13, npos=600, seed=1):
    fields, x, y = hi.main_case(nf, nlev, ny, nx, npos, seed)
    for a in (fields, x, y):
        a.setflags(write=False)
    return fields, x, y


def form(ctx, **expected_keys):
    """The launch shape of the last call, checked key by key -- unless the run forces a path."""
    got = ctx.last_hinterp_form()
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8])  # a launch takes 4 fields, 2 with the bicubic method
def test_main_case_fields_methods_and_memory(gpu_ctx, nf, device):
    fields, x, y = base(nf)
    flags = np.random.default_rng(nf).choice(MIXED, size=(nf, 5)).astype(np.int32)
    flags[0, :3] = MIXED
    for method in METHODS:
        check(gpu_ctx, fields, x, y, method, device, stacked=(nf != 3), label=("nf", nf))
        check(gpu_ctx, fields, x, y, method, device, flags=flags, stacked=(nf != 3), label=("nf", nf, "mixed flags"))
        passes = 2 if method[1] == hi.BICUBIC else 4
        form(gpu_ctx, method=NAMES[method[1]], nf=min(nf, passes), tested=1, launches=-(-nf // passes), blocks=3)


@pytest.mark.parametrize("npos", [1, 63, 64, 65, 256, 257, 1100])  # one lane, the wave seam, the workgroup seam, several workgroups
def test_points(gpu_ctx, npos):
    fields, x, y = base(2, 3, 9, 13, npos, 3)
    for device in (False, True):
        for method in METHODS:
            check(gpu_ctx, fields, x, y, method, device, label=("npos", npos))
    form(gpu_ctx, blocks=-(-npos // 256))


@pytest.mark.parametrize("nlev", [1, 2, 3, 4, 7])  # every remainder of the unroll
def test_levels(gpu_ctx, nlev):
    fields, x, y = base(3, nlev, 9, 13, 300, 4)
    flags = np.random.default_rng(nlev).choice(MIXED, size=(3, nlev)).astype(np.int32)
    for device in (False, True):
        for method in METHODS:
            check(gpu_ctx, fields, x, y, method, device, flags=flags, label=("nlev", nlev))
    # one workgroup column of 300 points: the levels are cut into chunks of two, the last one shorter when nlev is odd
    form(gpu_ctx, blocks=2, chunk=min(nlev, 2), level_chunks=-(-nlev // 2))


@pytest.mark.parametrize("shape", [(1, 13), (9, 1)], ids=["13x1", "1x9"])
def test_degenerate_grids(gpu_ctx, shape):
    ny, nx = shape
    fields, x, y = base(2, 3, ny, nx, 300, 5)
    on_the_line = np.zeros_like(x)  # and points that are inside: on the one row / column
    for device in (False, True):
        for method in METHODS:
            check(gpu_ctx, fields, x, y, method, device, label=shape)
            check(gpu_ctx, fields, x if ny == 1 else on_the_line, on_the_line if ny == 1 else y, method, device, label=(shape, "on the line"))
    exp, _ = expected(fields, x if ny == 1 else on_the_line, on_the_line if ny == 1 else y, hi.BICUBIC)
    assert (exp != hi.UNDEF).mean() > 0.5


def test_launch_seams(gpu_ctx):
    # few points, many levels: the levels are spread over the device in chunks, the last one shorter
    fields, x, y = base(2, 37, 9, 13, 65, 6)
    for method in METHODS:
        check(gpu_ctx, fields, x, y, method, True, label="65 x 37")
        got = form(gpu_ctx, blocks=1, tested=1)
        if not run_is_forced():
            assert got["level_chunks"] > 1 and got["chunk"] * got["level_chunks"] >= 37 > got["chunk"] * (got["level_chunks"] - 1)
            assert 37 % got["chunk"] != 0  # the last chunk is shorter than the others
    # many points, few levels: several workgroups per chunk, few chunks
    rng = np.random.default_rng(8)
    f = hi.sprinkle(rng.normal(280, 10, (1, 3, 50, 40)).astype(np.float32), rng, 0.03, hi.UNDEF)
    x, y = hi.main_points(50, 40, 70000, 8)
    for method in METHODS:
        check(gpu_ctx, f, x, y, method, True, label="70 000 x 3")
        got = form(gpu_ctx, blocks=274, launches=1)
        if not run_is_forced():
            assert got["level_chunks"] <= 2 and got["chunk"] * got["level_chunks"] >= 3
    # every flag ALL_DEFINED: the instances that test no value
    fields, x, y = base(3, 5)
    every = np.full((3, 5), hi.ALL_DEFINED, np.int32)
    for device in (False, True):
        for method in METHODS:
            check(gpu_ctx, fields, x, y, method, device, flags=every, label="untested")
            form(gpu_ctx, tested=0)
    check(gpu_ctx, fields, x, y, METHODS[1], True, flags=[hi.ALL_DEFINED] * 3, label="one flag per field")
    form(gpu_ctx, tested=0)


def test_forced_levels_per_workgroup(gpu_ctx, mifc_env):
    fields, x, y = base(3, 7, 9, 13, 300, 4)
    for chunk in (1, 3, 7, 50):  # one level per workgroup (the body that is not unrolled), a remainder, one chunk, more than there are
        mifc_env("MIFC_HINTERP_LEVEL_CHUNK", chunk)
        for method in METHODS:
            check(gpu_ctx, fields, x, y, method, True, label=("levels per workgroup", chunk))
            form(gpu_ctx, chunk=min(chunk, 7), level_chunks=-(-7 // min(chunk, 7)))


def test_identity_regrid_on_the_device(gpu_ctx):
    import torch

    fields, _, _ = base(2, 3)
    nf, nlev, ny, nx = fields.shape
    flags = np.array([[hi.ALL_DEFINED, hi.SOME_DEFINED, hi.SOME_DEFINED], [hi.SOME_DEFINED, hi.NONE_DEFINED, hi.ALL_DEFINED]], np.int32)
    yy, xx = torch.meshgrid(torch.arange(ny, dtype=torch.float32, device="cuda"), torch.arange(nx, dtype=torch.float32, device="cuda"), indexing="ij")
    for given, code in METHODS:
        out, fd = gpu_ctx.hinterp_levels(torch.from_numpy(fields[0]).cuda(), xx.contiguous(), yy.contiguous(), given, fdefined_in=flags[0])
        assert out.is_cuda and tuple(out.shape) == (nlev, ny, nx) and fd.shape == (nlev,)
        exp, efd = expected(fields[:1], xx.cpu().numpy(), yy.cpu().numpy(), code, flags[:1])
        compare(out.cpu().numpy(), exp[0], fd, efd[0], ("identity", code))
        assert out.cpu().numpy().tobytes() == fields[0].tobytes()  # the input's bits, holes included
        out, fd = gpu_ctx.hinterp_levels(torch.from_numpy(fields).cuda(), xx.contiguous(), yy.contiguous(), given, fdefined_in=flags)
        assert tuple(out.shape) == fields.shape and out.cpu().numpy().tobytes() == fields.tobytes() and fd.shape == (nf, nlev)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_stored_undef_nan_as_undef_and_no_usable_point(gpu_ctx, device):
    fields, x, y = base(2, 3)
    for method in METHODS:
        # a stored undef under ALL_DEFINED is a value: it is returned, interpolated with, and never counted
        flags = np.array([[hi.ALL_DEFINED] * 3, [hi.SOME_DEFINED, hi.ALL_DEFINED, hi.SOME_DEFINED]], np.int32)
        check(gpu_ctx, fields, x, y, method, device, flags=flags, label="stored undef")
        # NaN as undef, in the fields and in the positions
        nan = np.float32(np.nan)
        fn, xn, yn = (np.where(a == hi.UNDEF, nan, a) for a in (fields, x, y))
        check(gpu_ctx, fn, xn, yn, method, device, undef=nan, label="undef = NaN")
        check(gpu_ctx, fn, xn, yn, method, device, flags=flags, label="NaN values under the usual undef")
        # no usable point at all
        xo = np.where(np.arange(x.size) % 3 == 0, np.float32(-1), np.where(np.arange(x.size) % 3 == 1, np.float32(np.inf), hi.UNDEF)).astype(np.float32)
        every = np.full((2, 3), hi.ALL_DEFINED, np.int32)
        got, fd = run(gpu_ctx, fields, xo, y, method[0], device, flags=every)
        assert (got == hi.UNDEF).all() and (fd == hi.NONE_DEFINED).all()
        exp, efd = expected(fields, xo, y, method[1], every)
        compare(got, exp, fd, efd, "no usable point")


def test_device_batch_and_positions_offset_by_one_float(gpu_ctx):
    import torch

    fields, x, y = base(2, 5)
    n, npos = fields[0].size, x.size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
    batches = [buf[1 + j * n:1 + (j + 1) * n].view(5, 9, 13) for j in range(2)]  # 4 bytes past the 16-byte grid
    pos = torch.zeros(2 * npos + 3, dtype=torch.float32, device="cuda")
    pos[1:1 + npos] = torch.from_numpy(x).cuda()
    pos[2 + npos:2 + 2 * npos] = torch.from_numpy(y).cuda()
    obuf = torch.zeros(2 * 5 * npos + 1, dtype=torch.float32, device="cuda")
    for given, code in METHODS:
        out, fd = gpu_ctx.hinterp_levels(batches, pos[1:1 + npos], pos[2 + npos:2 + 2 * npos], given, out=obuf[1:].view(2, 5, npos))
        exp, efd = expected(fields, x, y, code)
        compare(out.cpu().numpy(), exp, fd, efd, ("offset by one float", code))
        assert float(obuf[0]) == 0.0


def test_host_call_in_several_level_chunks(gpu_ctx, mifc_env):
    mifc_env("MIFC_HINTERP_CHUNK_MIB", 1)
    # 2 fields x (300 x 333 cells + 500 points) x 4 bytes = 803 200 bytes per level: one level per chunk, twelve chunks
    rng = np.random.default_rng(9)
    f = hi.sprinkle(rng.normal(280, 10, (2, 12, 300, 333)).astype(np.float32), rng, 0.03, hi.UNDEF)
    x, y = hi.main_points(300, 333, 500, 9)
    flags = rng.choice(MIXED, size=(2, 12)).astype(np.int32)
    for method in METHODS:
        check(gpu_ctx, f, x, y, method, False, flags=flags, label="level chunks")
        form(gpu_ctx, launches=12, blocks=2, level_chunks=1, chunk=1)
    # 5 fields x (40 x 50 + 500) x 4 = 50 000 bytes per level: 20 levels per chunk, 37 levels in two chunks, the second shorter
    f = hi.sprinkle(rng.normal(280, 10, (5, 37, 50, 40)).astype(np.float32), rng, 0.03, hi.UNDEF)
    x, y = hi.main_points(50, 40, 500, 10)
    for method in METHODS:
        check(gpu_ctx, f, x, y, method, False, label="two level chunks")
        form(gpu_ctx, launches=2 * (3 if method[1] == hi.BICUBIC else 2))


def test_host_level_that_exceeds_the_budget_goes_alone(gpu_ctx, mifc_env):
    mifc_env("MIFC_HINTERP_CHUNK_MIB", 1)
    # one level of both fields is 2 x 600 x 500 x 4 = 2 400 000 bytes, more than the MiB: a chunk is never less than a level
    rng = np.random.default_rng(12)
    f = hi.sprinkle(rng.normal(280, 10, (2, 3, 500, 600)).astype(np.float32), rng, 0.03, hi.UNDEF)
    x, y = hi.main_points(500, 600, 700, 12)
    for method in METHODS:
        check(gpu_ctx, f, x, y, method, False, label="level by level")
        form(gpu_ctx, launches=3, chunk=1)


def test_out_is_honoured_and_nothing_around_it_is_written(gpu_ctx):
    import torch

    fields, x, y = base(2, 5)
    sentinel = np.float32(-4242.5)
    exp, efd = expected(fields, x, y, hi.BICUBIC)
    pool = torch.full((3, 2, 5, 600), float(sentinel), dtype=torch.float32, device="cuda")
    out, fd = gpu_ctx.hinterp_levels(torch.from_numpy(fields).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), "bicubic", out=pool[1])
    assert out.data_ptr() == pool[1].data_ptr()
    got = pool.cpu().numpy()
    compare(got[1], exp, fd, efd, "out on the device")
    assert (got[0] == sentinel).all() and (got[2] == sentinel).all()
    hpool = np.full((3, 5, 600), sentinel, np.float32)
    out, fd = gpu_ctx.hinterp_levels(fields[1], x, y, hi.BICUBIC, out=hpool[1])
    assert out is not None and np.shares_memory(out, hpool[1]) and fd.shape == (5,)
    compare(hpool[1], exp[1], fd, efd[1], "out on the host")
    assert (hpool[0] == sentinel).all() and (hpool[2] == sentinel).all()
    with pytest.raises(ValueError):
        gpu_ctx.hinterp_levels(fields, x, y, out=np.zeros((2, 5, 599), np.float32))
    with pytest.raises(ValueError):
        gpu_ctx.hinterp_levels(fields, x, y[:-1])


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx, npos = 2, 3, 5, 8, 70
    fields_h, x_h, y_h = base(nf, nlev, ny, nx, npos, 2)
    batch, res = nlev * ny * nx, nlev * npos
    # room of the test's own around the fields and around ypos: an output (longer than a field here) that ends in their
    # first float or begins in their last one stays inside it, whatever else the allocator has put nearby
    room = torch.zeros(res + nf * batch + res, dtype=torch.float32, device="cuda")
    x = room[res:res + nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(fields_h))
    xp = torch.from_numpy(x_h).cuda()
    yroom = torch.zeros(res + npos + res, dtype=torch.float32, device="cuda")
    yp = yroom[res:res + npos].copy_(torch.from_numpy(y_h))
    sentinel = -4242.5
    outs = torch.full((nf, nlev, npos), sentinel, dtype=torch.float32, device="cuda")

    def call(nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, npos_=npos, method=1, fields=None, out_ptrs=None, xpos=0, ypos=0, fd_out=True, memkind=1, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        fd = np.full(nf * nlev, 7, np.int32)
        rc = lib.mifc_hinterp_levels(c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_, npos_,
                                     xp.data_ptr() if xpos == 0 else xpos, yp.data_ptr() if ypos == 0 else ypos, method,
                                     None if out_ptrs == "null" else ctypes.addressof(o), fd.ctypes.data if fd_out else None, float(hi.UNDEF), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    null_head = "a null pointer (fields, xpos, ypos, fres or fdefined_out)"
    refusals = {
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "negative nlev": (dict(nlev_=-3), "nlev < 1"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "npos 0": (dict(npos_=0), "npos < 1"),
        "negative npos": (dict(npos_=-1), "npos < 1"),
        "nx 0": (dict(nx_=0), "nx < 1 or ny < 1"),
        "negative ny": (dict(ny_=-2), "nx < 1 or ny < 1"),
        "2^31 cells": (dict(nx_=65536, ny_=32768), "more than 2^31 - 1 cells per level"),
        "unknown method 3": (dict(method=3), "unknown method 3"),
        "negative method": (dict(method=-1), "unknown method -1"),
        "null fields": (dict(fields="null"), null_head),
        "null xpos": (dict(xpos=None), null_head),
        "null ypos": (dict(ypos=None), null_head),
        "null fres": (dict(out_ptrs="null"), null_head),
        "null fdefined_out": (dict(fd_out=False), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or fres[1])"),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None]), "a null pointer (fields[1] or fres[1])"),
        "output is an input": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output ends in an input": (dict(out_ptrs=[x[0].data_ptr() - 4 * (res - 1), outs[1].data_ptr()]), "fres[0] overlaps fields[0]"),
        "output is xpos": (dict(out_ptrs=[outs[0].data_ptr(), xp.data_ptr()]), "fres[1] overlaps xpos"),
        "output ends in ypos": (dict(out_ptrs=[yp.data_ptr() - 4 * (res - 1), outs[1].data_ptr()]), "fres[0] overlaps ypos"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr() + 4 * (res - 1)]), "fres[0] overlaps fres[1]"),
        "bad memkind": (dict(memkind=7), "unknown memkind 7"),
    }
    before = {k: t.clone() for k, t in (("x", x), ("xp", xp), ("yp", yp))}
    for what, (kw, tail) in refusals.items():
        rc, err, fd = call(**kw)
        assert rc == 0 and err == "mifc_hinterp_levels: " + tail, (what, err)
        assert (outs == sentinel).all().item() and (fd == 7).all(), what
    for k, t in (("x", x), ("xp", xp), ("yp", yp)):  # (by bits: ypos holds a NaN)
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
    with pytest.raises(RuntimeError, match="unknown method"):
        gpu_ctx.hinterp_levels(x, xp, yp, "spline")
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, fd = call(sync=False)
    g.close()
    assert rc == 0 and "capture" in err and (fd == 7).all() and (outs == sentinel).all().item()
    # afterwards the same call runs
    rc, err, fd = call()
    assert rc == 1 and err == "" and (fd != 7).all(), err
    exp, efd = expected(fields_h, x_h, y_h, hi.BILINEAR)
    compare(outs.cpu().numpy(), exp, fd.reshape(nf, nlev), efd, "after the refusals")


def test_cross_section_on_pressure_surfaces(gpu_ctx):
    """Two device calls: hinterp_levels of T and of the pressure batch along a line of 65 points, then vinterp_fields of the
    (12, 1, 65) result to three surfaces -- bit for bit the two restatements composed."""
    import torch

    rng = np.random.default_rng(31)
    nlev, ny, nx, npos = 12, 9, 13, 65
    alevel, blevel = vi.hybrid_levels(nlev)
    ps = rng.uniform(700, 1050, (ny, nx)).astype(np.float32)
    p = vi.hybrid_coordinate(ps, alevel, blevel)
    t = hi.sprinkle((220 + 70 * (p / 1000.0) ** 0.19 + rng.normal(0, 0.3, p.shape)).astype(np.float32), rng, 0.02, hi.UNDEF)
    s = np.linspace(0, 1, npos)
    x, y = (0.4 + 12.2 * s).astype(np.float32), (7.9 - 7.1 * s * s).astype(np.float32)  # (the last points leave the grid)
    targets = np.array([850, 500, 300], np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for given, code in METHODS:
        sec, sfd = gpu_ctx.hinterp_levels([dev(t), dev(p)], dev(x), dev(y), given)
        assert sec.is_cuda and tuple(sec.shape) == (2, nlev, npos)
        esec, esfd = expected(np.stack([t, p]), x, y, code)
        compare(sec.cpu().numpy(), esec, sfd, esfd, ("section", code))
        on_p, pfd = gpu_ctx.vinterp_fields(sec[0].view(nlev, 1, npos), sec[1].view(nlev, 1, npos), targets, fdefined_in=sfd[0], fdef_coord=sfd[1])
        e_on_p, e_pfd = vi.coord_fields(esec[:1].reshape(1, nlev, 1, npos), esec[1].reshape(nlev, 1, npos), targets, vi.LINEAR, esfd[:1], esfd[1])
        assert on_p.is_cuda and tuple(on_p.shape) == (3, 1, npos)
        compare(on_p.cpu().numpy(), e_on_p[0], pfd, e_pfd[0], ("section on pressure surfaces", code))
        assert (e_on_p != hi.UNDEF).mean() > 0.3
