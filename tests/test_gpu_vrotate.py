"""Vector pairs of level batches rotated on the GPU (mifc_vrotate.hip, mifc_vrotate_levels) against the numpy restatement
of rule R (tests/vrotate_restate.py): bit for bit (a NaN matches any NaN), flags equal, host and device memory.  No
tolerance: every operation of the rule is an IEEE double operation rounded on its own, the library is built without
contraction."""
import ctypes
import functools

import numpy as np
import pytest

import vrotate_restate as vr
from cases import same_bits
from gpu_util import run_is_forced

pytestmark = pytest.mark.gpu

MIXED = [vr.ALL_DEFINED, vr.SOME_DEFINED, vr.NONE_DEFINED]


def compare(got, exp, gfd, efd, label):
    assert got.shape == exp.shape, (label, got.shape, exp.shape)
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if not same_bits(got, exp, nan_payload=False):
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))


@functools.lru_cache(maxsize=None)
def base(npairs=1, nlev=5, ny=9, nx=13, seed=1):
    fields, c, s = vr.grid_case(npairs, nlev, ny, nx, seed)
    for a in (fields, c, s):
        a.setflags(write=False)
    return fields, c, s


def run(ctx, fields, c, s, device, flags=None, fdef_rot=vr.SOME_DEFINED, undef=vr.UNDEF, stacked=True, out=None):
    import torch

    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    npairs = fields.shape[0] // 2
    f = put(fields.reshape((npairs, 2) + fields.shape[1:]))
    f = f if stacked else [(f[q, 0], f[q, 1]) for q in range(npairs)]
    res, fd = ctx.vrotate_levels(f, put(c), put(s), fdefined_in=flags, fdef_rot=fdef_rot, undef=undef, out=out)
    res = res.cpu().numpy() if device else res
    return res.reshape(fields.shape), fd.reshape(fields.shape[0], -1)


def check(ctx, fields, c, s, device, flags=None, fdef_rot=vr.SOME_DEFINED, undef=vr.UNDEF, stacked=True, label=None):
    got, fd = run(ctx, fields, c, s, device, flags, fdef_rot, undef, stacked)
    exp, efd = vr.rotate(fields, c, s, flags, fdef_rot, undef)
    compare(got, exp, fd, efd, (label, "device" if device else "host"))


def form(ctx, **expected_keys):
    """The launch shape of the last call, checked key by key -- unless the run forces a path."""
    got = ctx.last_vrotate_form()
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


# 13 x 9: a tail inside the last group of four; one cell; the seam of one 256-lane workgroup of four cells; several workgroups
@pytest.mark.parametrize("shape", [(9, 13), (1, 1), (1, 1023), (32, 32), (25, 41), (3, 683)], ids=["13x9", "1x1", "1023", "1024", "1025", "2049"])
def test_grids(gpu_ctx, shape):
    ny, nx = shape
    fields, c, s = base(2, 3, ny, nx, 2)
    for device in (False, True):
        check(gpu_ctx, fields, c, s, device, label=shape)
        cells = ny * nx
        v = 4 if (not device or cells % 4 == 0) else 1  # (a staged band is padded: four cells per lane)
        form(gpu_ctx, v=v, np=2, tested=1, launches=1, blocks=-(-cells // (256 * v)))


def test_off_the_16_byte_grid(gpu_ctx):
    import torch

    # a batch whose pointer is 4 bytes past the 16-byte grid, the level size a multiple of 4
    fields, c, s = base(1, 3, 8, 16, 3)
    n = fields[0].size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
    pair = [buf[1 + j * n:1 + (j + 1) * n].view(3, 8, 16) for j in range(2)]
    obuf = torch.zeros(2 * n + 5, dtype=torch.float32, device="cuda")
    exp, efd = vr.rotate(fields, c, s)
    out, fd = gpu_ctx.vrotate_levels(pair, torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(), out=obuf[4:4 + 2 * n].view(2, 3, 8, 16))
    compare(out.cpu().numpy(), exp, fd, efd, "input offset by one float")
    form(gpu_ctx, v=1, blocks=1)
    # only the output off the grid
    out, fd = gpu_ctx.vrotate_levels(torch.from_numpy(fields).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(),
                                     out=obuf[1:1 + 2 * n].view(2, 3, 8, 16))
    compare(out.cpu().numpy(), exp, fd, efd, "output offset by one float")
    form(gpu_ctx, v=1)
    assert float(obuf[0]) == 0.0 and float(obuf[4 + 2 * n]) == 0.0
    # only a coefficient plane off the grid
    cbuf = torch.zeros(129, dtype=torch.float32, device="cuda")
    cbuf[1:] = torch.from_numpy(c.reshape(-1)).cuda()
    out, fd = gpu_ctx.vrotate_levels(torch.from_numpy(fields).cuda(), cbuf[1:].view(8, 16), torch.from_numpy(s).cuda())
    compare(out.cpu().numpy(), exp, fd, efd, "cosa offset by one float")
    form(gpu_ctx, v=1)
    # aligned pointers, a level size that is no multiple of 4 (every second level starts off the grid)
    fields, c, s = base(1, 3, 7, 9, 3)
    check(gpu_ctx, fields, c, s, True, label="63 cells per level")
    form(gpu_ctx, v=1, blocks=1)
    # and everything on the grid: four cells per lane
    fields, c, s = base(1, 3, 8, 16, 3)
    check(gpu_ctx, fields, c, s, True, label="on the grid")
    form(gpu_ctx, v=4, blocks=1)


@pytest.mark.parametrize("nlev", [1, 2, 3, 7])  # every remainder of the unroll; 7: a last chunk shorter than the others
def test_levels(gpu_ctx, nlev):
    fields, c, s = base(2, nlev, 9, 13, 4)
    flags = np.random.default_rng(nlev).choice(MIXED, size=(4, nlev)).astype(np.int32)
    for device in (False, True):
        check(gpu_ctx, fields, c, s, device, flags=flags, label=("nlev", nlev))
        got = form(gpu_ctx)
        if not run_is_forced():
            assert got["chunk"] * got["level_chunks"] >= nlev > got["chunk"] * (got["level_chunks"] - 1), got
            if nlev == 7:
                assert got["level_chunks"] > 1 and nlev % got["chunk"] != 0, got  # the last chunk is shorter


def test_forced_levels_per_workgroup(gpu_ctx, mifc_env):
    fields, c, s = base(2, 7, 9, 13, 4)
    for chunk in (1, 2, 3, 7, 50):  # the body that is not unrolled, no remainder, a remainder, one chunk, more than there are
        mifc_env("MIFC_HINTERP_LEVEL_CHUNK", chunk)
        check(gpu_ctx, fields, c, s, True, label=("levels per workgroup", chunk))
        form(gpu_ctx, chunk=min(chunk, 7), level_chunks=-(-7 // min(chunk, 7)))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("npairs", [1, 2, 3, 4])
def test_pairs_flags_and_memory(gpu_ctx, npairs, device):
    fields, c, s = base(npairs, 5)
    check(gpu_ctx, fields, c, s, device, stacked=(npairs != 3), label=("npairs", npairs))
    form(gpu_ctx, np=npairs, tested=1, launches=1)
    # mixed flags per component and level
    flags = np.random.default_rng(npairs).choice(MIXED, size=(2 * npairs, 5)).astype(np.int32)
    flags[0, :3], flags[1, :3] = MIXED, MIXED[::-1]
    for fdef_rot in MIXED:
        check(gpu_ctx, fields, c, s, device, flags=flags, fdef_rot=fdef_rot, stacked=(npairs != 3), label=("mixed flags", npairs, fdef_rot))
        form(gpu_ctx, tested=1)
    # one flag per component stands for every level
    per_comp = flags[:, 0].copy()
    got, fd = run(gpu_ctx, fields, c, s, device, flags=per_comp)
    exp, efd = vr.rotate(fields, c, s, np.repeat(per_comp[:, None], 5, axis=1))
    compare(got, exp, fd, efd, "one flag per component")
    # every flag ALL_DEFINED: with the coefficients tested the tested instance, without them the one that tests nothing
    every = np.full((2 * npairs, 5), vr.ALL_DEFINED, np.int32)
    check(gpu_ctx, fields, c, s, device, flags=every, label="only the coefficients are tested")
    form(gpu_ctx, tested=1)
    check(gpu_ctx, fields, c, s, device, flags=every, fdef_rot=vr.ALL_DEFINED, label="untested")
    form(gpu_ctx, tested=0)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nan_as_undef_and_shapes_of_the_python_layer(gpu_ctx, device):
    fields, c, s = base(1, 3)
    nan = np.float32(np.nan)
    fn, cn, sn = (np.where(a == vr.UNDEF, nan, a) for a in (fields, c, s))
    check(gpu_ctx, fn, cn, sn, device, undef=nan, label="undef = NaN")
    check(gpu_ctx, fn, cn, sn, device, label="NaN values under the usual undef")
    # one pair: the leading axis is dropped
    import torch

    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    out, fd = gpu_ctx.vrotate_levels(put(fields), put(c), put(s))
    assert tuple(out.shape) == (2, 3, 9, 13) and fd.shape == (2, 3)
    out, fd = gpu_ctx.vrotate_levels(put(fields.reshape(1, 2, 3, 9, 13)), put(c), put(s))
    assert tuple(out.shape) == (1, 2, 3, 9, 13) and fd.shape == (1, 2, 3)
    with pytest.raises(ValueError):
        gpu_ctx.vrotate_levels(put(fields), put(c[:-1]), put(s))
    with pytest.raises(ValueError):
        gpu_ctx.vrotate_levels(put(fields), put(c), put(s), out=np.zeros((2, 3, 9, 12), np.float32))


def test_the_identity_and_the_quarter_turn_on_the_device(gpu_ctx):
    import torch

    fields, _, _ = base(1, 3, 16, 16, 5)
    one, zero = torch.ones(16, 16, device="cuda"), torch.zeros(16, 16, device="cuda")
    every = np.full((2, 3), vr.ALL_DEFINED, np.int32)
    clean = np.where(np.isnan(fields), np.float32(1.5), fields)
    out, fd = gpu_ctx.vrotate_levels(torch.from_numpy(clean).cuda(), one, zero, fdefined_in=every, fdef_rot=vr.ALL_DEFINED)
    assert out.cpu().numpy().tobytes() == clean.tobytes() and (fd == vr.ALL_DEFINED).all()  # (no zero among the values)
    out, fd = gpu_ctx.vrotate_levels(torch.from_numpy(clean).cuda(), zero, one, fdefined_in=every, fdef_rot=vr.ALL_DEFINED)
    got = out.cpu().numpy()
    assert got[0].tobytes() == (-clean[1]).tobytes() and got[1].tobytes() == clean[0].tobytes()


def test_host_call_in_several_bands(gpu_ctx, mifc_env):
    mifc_env("MIFC_VDERIV_CHUNK_MIB", 1)
    # 2 pairs x 5 levels in and out and the two coefficient planes: 42 planes of 333 floats a row -- 18 rows fit the MiB,
    # 50 rows go in three bands, the last one shorter and no multiple of four cells
    rng = np.random.default_rng(9)
    fields, c, s = vr.grid_case(2, 5, 50, 333, 9)
    flags = rng.choice(MIXED, size=(4, 5)).astype(np.int32)
    check(gpu_ctx, fields, c, s, False, flags=flags, label="bands")
    form(gpu_ctx, v=4, launches=3)
    sentinel = np.float32(-4242.5)
    pool = np.full((3, 2, 2, 5, 50, 333), sentinel, np.float32)
    out, fd = gpu_ctx.vrotate_levels(fields.reshape(2, 2, 5, 50, 333), c, s, fdefined_in=flags, out=pool[1])
    exp, efd = vr.rotate(fields, c, s, flags)
    compare(pool[1].reshape(fields.shape), exp, fd.reshape(4, 5), efd, "bands, out on the host")
    assert np.shares_memory(out, pool[1]) and (pool[0] == sentinel).all() and (pool[2] == sentinel).all()


def test_out_on_the_device_and_nothing_around_it_is_written(gpu_ctx):
    import torch

    fields, c, s = base(1, 5)
    sentinel = np.float32(-4242.5)
    exp, efd = vr.rotate(fields, c, s)
    pool = torch.full((3, 2, 5, 9, 13), float(sentinel), dtype=torch.float32, device="cuda")
    out, fd = gpu_ctx.vrotate_levels(torch.from_numpy(fields).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(s).cuda(), out=pool[1])
    assert out.data_ptr() == pool[1].data_ptr()
    got = pool.cpu().numpy()
    compare(got[1], exp, fd, efd, "out on the device")
    assert (got[0] == sentinel).all() and (got[2] == sentinel).all()


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    npairs, nlev, ny, nx = 2, 3, 5, 8
    nf, cells = 2 * npairs, ny * nx
    fields_h, cos_h, sin_h = base(npairs, nlev, ny, nx, 2)
    batch = nlev * cells
    # room of the test's own around the fields and around cosa: an output that ends in their first float or begins in their
    # last one stays inside it, whatever else the allocator has put nearby
    room = torch.zeros(batch + nf * batch + batch, dtype=torch.float32, device="cuda")
    x = room[batch:batch + nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(fields_h))
    croom = torch.zeros(batch + cells + batch, dtype=torch.float32, device="cuda")
    cosa = croom[batch:batch + cells].copy_(torch.from_numpy(cos_h.reshape(-1)))
    sina = torch.from_numpy(sin_h).cuda()
    sentinel = -4242.5
    outs = torch.full((nf, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")

    def call(nx_=nx, ny_=ny, nlev_=nlev, npairs_=npairs, fields=None, out_ptrs=None, cos_=0, sin_=0, fd_out=True, memkind=1, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        fd = np.full(nf * nlev, 7, np.int32)
        rc = lib.mifc_vrotate_levels(c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, npairs_,
                                     cosa.data_ptr() if cos_ == 0 else cos_, sina.data_ptr() if sin_ == 0 else sin_, vr.SOME_DEFINED,
                                     None if out_ptrs == "null" else ctypes.addressof(o), fd.ctypes.data if fd_out else None, float(vr.UNDEF), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    own = [outs[f].data_ptr() for f in range(nf)]
    null_head = "a null pointer (fields, cosa, sina, fres or fdefined_out)"
    refusals = {
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "negative nlev": (dict(nlev_=-3), "nlev < 1"),
        "npairs 0": (dict(npairs_=0), "npairs 0 outside 1..4"),
        "npairs 5": (dict(npairs_=5), "npairs 5 outside 1..4"),
        "nx 0": (dict(nx_=0), "nx < 1 or ny < 1"),
        "negative ny": (dict(ny_=-2), "nx < 1 or ny < 1"),
        "2^31 cells": (dict(nx_=65536, ny_=32768), "more than 2^31 - 1 cells per level"),
        "null fields": (dict(fields="null"), null_head),
        "null cosa": (dict(cos_=None), null_head),
        "null sina": (dict(sin_=None), null_head),
        "null fres": (dict(out_ptrs="null"), null_head),
        "null fdefined_out": (dict(fd_out=False), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None, x[2].data_ptr(), x[3].data_ptr())), "a null pointer (fields[1] or fres[1])"),
        "null output": (dict(out_ptrs=own[:2] + [None] + own[3:]), "a null pointer (fields[2] or fres[2])"),
        "output is an input": (dict(out_ptrs=[own[0], x[1].data_ptr()] + own[2:]), "fres[1] overlaps fields[1]"),
        "output ends in an input": (dict(out_ptrs=[x[0].data_ptr() - 4 * (batch - 1)] + own[1:]), "fres[0] overlaps fields[0]"),
        "output begins in an input": (dict(out_ptrs=own[:3] + [x[3].data_ptr() + 4 * (batch - 1)]), "fres[3] overlaps fields[3]"),
        "output is sina": (dict(out_ptrs=own[:3] + [sina.data_ptr()]), "fres[3] overlaps sina"),
        "output ends in cosa": (dict(out_ptrs=[cosa.data_ptr() - 4 * (batch - 1)] + own[1:]), "fres[0] overlaps cosa"),
        "output begins in cosa": (dict(out_ptrs=[cosa.data_ptr() + 4 * (cells - 1)] + own[1:]), "fres[0] overlaps cosa"),
        "same output twice": (dict(out_ptrs=[own[0], own[0]] + own[2:]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[own[0], own[0] + 4 * (batch - 1)] + own[2:]), "fres[0] overlaps fres[1]"),
        "bad memkind": (dict(memkind=7), "unknown memkind 7"),
    }
    before = {k: t.clone() for k, t in (("x", x), ("cosa", cosa), ("sina", sina))}
    for what, (kw, tail) in refusals.items():
        rc, err, fd = call(**kw)
        assert rc == 0 and err == "mifc_vrotate_levels: " + tail, (what, err)
        assert (outs == sentinel).all().item() and (fd == 7).all(), what
    for k, t in (("x", x), ("cosa", cosa), ("sina", sina)):  # (by bits: they hold NaNs)
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, fd = call(sync=False)
    g.close()
    assert rc == 0 and err.startswith("mifc_vrotate_levels: ") and "capture" in err and (fd == 7).all() and (outs == sentinel).all().item()
    # afterwards the same call runs
    rc, err, fd = call()
    assert rc == 1 and err == "" and (fd != 7).all(), err
    exp, efd = vr.rotate(fields_h, cos_h, sin_h)
    compare(outs.cpu().numpy(), exp, fd.reshape(nf, nlev), efd, "after the refusals")
