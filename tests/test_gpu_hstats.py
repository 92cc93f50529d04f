"""Horizontal statistics of level batches on the GPU (mifc_hstats.hip, mifc_hstats_levels) against the numpy restatement
(tests/hstats_restate.py): bit for bit (a NaN matches a NaN), host and device memory, both modes, every product mask.  No
tolerance: the order of every addition is part of the definition, every operation is an IEEE double operation rounded on
its own and the library is built without contraction.  The slots of a product group that was not requested must not be
written: the result array starts as NaN and the restatement fills those slots with NaN too."""
import ctypes
import functools

import numpy as np
import pytest

import hstats_restate as hs
import vinterp_restate as vi
from gpu_util import run_is_forced

pytestmark = pytest.mark.gpu

MIXED = [hs.ALL_DEFINED, hs.SOME_DEFINED, hs.NONE_DEFINED]
MASKS = {hs.MOMENTS: ("moments",), hs.EXTREMES: ("extremes",), hs.MOMENTS | hs.EXTREMES: ("moments", "extremes")}


def put(a, device):
    import torch

    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if device else np.ascontiguousarray(a)


def call(ctx, fields, device, stacked=True, minus=None, weight=None, products=hs.MOMENTS | hs.EXTREMES, want_mean=True, **kw):
    """One hstats_levels call on numpy inputs: (stats, mean, flags) as numpy arrays."""
    f = put(fields, device)
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    want_mean = want_mean and bool(products & hs.MOMENTS)
    res = ctx.hstats_levels(f, minus=put(minus, device), weight=put(weight, device), products=MASKS[products] if stacked else products,
                            want_mean=want_mean, **kw)
    stats = res.stats.cpu().numpy() if device else res.stats
    mean = None if not want_mean else (res.mean_batch.cpu().numpy() if device else res.mean_batch)
    return stats, mean, res.mean_flags


def compare(got, exp, label):
    stats, mean, fd = got
    estats, emean, efd = exp
    assert stats.shape == estats.shape, (label, stats.shape, estats.shape)
    if not hs.same_bits64(stats, estats):
        bad = np.argwhere((stats.view(np.uint64) != estats.view(np.uint64)) & ~(np.isnan(stats) & np.isnan(estats)))
        first = tuple(int(b) for b in bad[0])
        raise AssertionError("%s: %d numbers differ; first %s got %r expected %r" % (label, len(bad), first, stats[first], estats[first]))
    if mean is not None:
        assert hs.same_bits64(mean.astype(np.float64), emean.astype(np.float64)), (label, "mean")
        assert np.array_equal(np.asarray(fd), efd), (label, fd, efd)


def check(ctx, fields, device, label=None, stacked=True, minus=None, weight=None, pivot=None, box=None, mode="area",
          products=hs.MOMENTS | hs.EXTREMES, flags=None, flags_minus=None, fdef_weight=hs.SOME_DEFINED, undef=hs.UNDEF):
    got = call(ctx, fields, device, stacked, minus, weight, products, pivot=pivot, box=box, mode=mode, fdefined_in=flags, fdefined_minus=flags_minus,
               fdef_weight=fdef_weight, undef=undef)
    exp = hs.hstats(fields, minus, pivot, weight, box, mode, products, flags, flags_minus, fdef_weight, undef, fill=np.nan)
    compare(got, exp, (label, mode, products, "device" if device else "host"))
    return got


def form(ctx, **expected_keys):
    """The launch shape of the last call, checked key by key -- unless the run forces a path."""
    got = ctx.last_hstats_form()
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


@functools.lru_cache(maxsize=None)
def base(nf=2, nlev=5, ny=9, nx=13, seed=1):
    case = hs.main_case(nf, nlev, ny, nx, seed)
    for a in case[:4]:
        a.setflags(write=False)
    return case


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 2, 4, 5, 8])  # a launch takes 4 fields: one launch, a second one, a partial one
def test_main_case_fields_modes_products_and_memory(gpu_ctx, nf, device):
    fields, _, _, _, _ = base(nf)
    flags = np.random.default_rng(nf).choice(MIXED, size=(nf, 5)).astype(np.int32)
    flags[0, :3] = MIXED
    assert ((fields[0, 0] == hs.UNDEF).any())  # the level flagged ALL_DEFINED stores undef: a value there
    for mode in ("area", "rows"):
        for products in MASKS:
            check(gpu_ctx, fields, device, ("nf", nf), stacked=(nf != 2), mode=mode, products=products)
            check(gpu_ctx, fields, device, ("nf", nf, "mixed flags"), stacked=(nf != 2), mode=mode, products=products, flags=flags)
            form(gpu_ctx, mode=mode, v=1, nf=min(nf, 4), w=0, minus=0, tested=1, products=products, segs=1, blocks=3, launches=-(-nf // 4), bands=1)
    every = np.full((nf, 5), hs.ALL_DEFINED, np.int32)  # the instances that test nothing
    check(gpu_ctx, fields, device, "untested", flags=every, mode="rows")
    form(gpu_ctx, tested=0)


@pytest.mark.parametrize("nx", [1, 3, 4, 5, 255, 256, 257, 260, 1023, 1024, 1027, 4095, 4096, 4097, 4100, 8193])
def test_widths(gpu_ctx, nx):
    """One and several trips, tails, one, two and three segments; 16-byte loads where the rows allow them, dwords else."""
    import torch

    fields, minus, weight, pivot, _ = base(2, 2, 3, nx, seed=nx)
    segs, v = -(-nx // hs.SEGMENT), 4 if nx % 4 == 0 else 1
    for device in (False, True):
        for mode in ("area", "rows"):
            check(gpu_ctx, fields, device, ("nx", nx), mode=mode)
            form(gpu_ctx, v=v, segs=segs, blocks=-(-3 * segs // 4), launches=1)
        check(gpu_ctx, fields, device, ("nx", nx, "everything"), minus=minus, weight=weight, pivot=pivot, mode="rows")
        form(gpu_ctx, v=v, w=1, minus=1)
    if v == 4:  # the same batch off the 16-byte grid: the dword form
        buf = torch.zeros(fields.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
        res = gpu_ctx.hstats_levels(buf[1:].view(fields.shape), mode="rows")
        form(gpu_ctx, v=1, segs=segs)
        exp, _, _ = hs.hstats(fields, mode=hs.ROWS)
        compare((res.stats.cpu().numpy(), None, None), (exp, None, None), ("nx", nx, "dwords"))


def test_misaligned_pointers_give_the_aligned_result(gpu_ctx):
    import torch

    fields, minus, weight, _, _ = base(2, 3, 5, 520, seed=21)
    aligned = call(gpu_ctx, fields, True, minus=minus, weight=weight, mode="rows")
    form(gpu_ctx, v=4, w=1, minus=1)
    compare(aligned, hs.hstats(fields, minus, None, weight, None, hs.ROWS), "aligned")
    n = fields[0].size
    for off in (1, 2, 3):
        for which in ("fields", "minus", "weight"):
            def shifted(a):
                buf = torch.zeros(a.size + off, dtype=torch.float32, device="cuda")
                buf[off:] = torch.from_numpy(a.reshape(-1)).cuda()
                return buf[off:].view(a.shape)

            f = shifted(fields) if which == "fields" else put(fields, True)
            m = shifted(minus) if which == "minus" else put(minus, True)
            w = shifted(weight) if which == "weight" else put(weight, True)
            res = gpu_ctx.hstats_levels([f[0], f[1]], minus=[m[0], m[1]], weight=w, mode="rows", want_mean=True)
            form(gpu_ctx, v=1)
            got = (res.stats.cpu().numpy(), res.mean_batch.cpu().numpy(), res.mean_flags)
            compare(got, aligned, (which, "off by", off))
    assert n % 4 == 0


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_boxes(gpu_ctx, device):
    fields, minus, weight, pivot, _ = base(2, 2, 6, 300, seed=5)
    ny, nx = 6, 300
    for i0 in (0, 1, 3, 4, 255, 256):
        for i1 in (i0 + 1, min(nx, i0 + 6), 259 if i0 < 259 else nx, nx):
            box = (i0, i1, 1, 5)
            for mode in ("area", "rows"):
                stats, _, _ = check(gpu_ctx, fields, device, ("box", box), box=box, mode=mode, weight=weight)
                form(gpu_ctx, segs=1, blocks=1)
                imin = stats[..., hs.IMIN]
                assert ((imin == -1) | ((imin >= nx) & (imin % nx >= i0) & (imin % nx < i1))).all()  # an index of the level, not of the box
    for box in ((0, nx, 2, 3), (7, 8, 0, ny), (299, 300, 5, 6), (0, 1, 0, 1)):  # one row, one column, one cell in two corners
        for mode in ("area", "rows"):
            check(gpu_ctx, fields, device, ("box", box), box=box, mode=mode, minus=minus, pivot=pivot)
    wide = base(1, 2, 3, 8200, seed=6)[0]  # boxes that begin in the second segment and span two
    for box in ((4096, 8200, 0, 3), (4000, 4200, 1, 3), (5000, 8193, 0, 2)):
        stats, _, _ = check(gpu_ctx, wide, device, ("box", box), box=box, mode="rows")
        form(gpu_ctx, segs=(box[1] - 1) // 4096 - box[0] // 4096 + 1)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_weights(gpu_ctx, device):
    fields, _, weight, _, _ = base(2, 3, 7, 260, seed=8)
    w = weight.copy()
    w[2, :] = 0.0  # a row whose W is 0: mean undef, counted in the flag
    w[3, ::3] = -w[3, ::3]  # negatives
    w[4, :] = hs.UNDEF  # a masked row: N == 0
    w[5, 10:20] = 0.0
    for mode in ("area", "rows"):
        for products in MASKS:
            check(gpu_ctx, fields, device, "holes, zeros, negatives", weight=w, mode=mode, products=products)
        form(gpu_ctx, w=1, tested=1)
    _, mean, fd = check(gpu_ctx, fields, device, "rows", weight=w, mode="rows")
    assert (mean[:, :, 2] == hs.UNDEF).all() and (mean[:, :, 4] == hs.UNDEF).all() and (fd == hs.SOME_DEFINED).all()
    # ALL_DEFINED over a stored undef: the undef is a weight like any other
    every = np.full((2, 3), hs.ALL_DEFINED, np.int32)
    dense = np.where(fields == hs.UNDEF, np.float32(1), fields)
    for mode in ("area", "rows"):
        check(gpu_ctx, dense, device, "weight flagged ALL_DEFINED", weight=w, fdef_weight=hs.ALL_DEFINED, flags=every, mode=mode)
        form(gpu_ctx, w=1, tested=0)
        check(gpu_ctx, fields, device, "weight flagged ALL_DEFINED, fields tested", weight=w, fdef_weight=hs.ALL_DEFINED, mode=mode)
    zero = np.zeros_like(w)  # nothing but zero weights: every mean undef
    _, mean, fd = check(gpu_ctx, fields, device, "zero weights", weight=zero, mode="area")
    assert (mean == hs.UNDEF).all() and (fd == hs.NONE_DEFINED).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_minus_and_pivot(gpu_ctx, device):
    for nf in (1, 3, 5):
        fields, minus, weight, pivot, box = base(nf, 4, 9, 13, seed=30 + nf)
        rng = np.random.default_rng(nf)
        flags, flags_minus = (rng.choice(MIXED, size=(nf, 4)).astype(np.int32) for _ in range(2))
        flags[0, :2], flags_minus[0, :2] = [hs.ALL_DEFINED, hs.SOME_DEFINED], [hs.SOME_DEFINED, hs.ALL_DEFINED]
        for mode in ("area", "rows"):
            check(gpu_ctx, fields, device, "minus", minus=minus, mode=mode, flags=flags, flags_minus=flags_minus)
            form(gpu_ctx, minus=1, nf=min(nf, 4), launches=-(-nf // 4))
            check(gpu_ctx, fields, device, "pivot", pivot=pivot, mode=mode, flags=flags)
            check(gpu_ctx, fields, device, "minus, pivot, weight, box", minus=minus, pivot=pivot, weight=weight, box=box, mode=mode, flags=flags,
                  flags_minus=flags_minus, products=hs.MOMENTS)
    # a field against itself: d = 0 everywhere it is defined, RMSE 0, and the second pass about the mean
    fields = base(1, 2, 9, 13, seed=40)[0]
    res = gpu_ctx.hstats_levels(put(fields[0], device), minus=put(fields[0], device))
    form(gpu_ctx, mode="area", nf=1, minus=1, w=0, products=hs.MOMENTS | hs.EXTREMES)
    assert (res.rms() == 0).all() and (res.variance() == 0).all()
    first = gpu_ctx.hstats_levels(put(fields[0], device), products="moments")
    second = gpu_ctx.hstats_levels(put(fields[0], device), pivot=first.mean()[:, 0], products="moments", want_mean=True)
    exp, emean, _ = hs.hstats(fields, pivot=first.mean()[:, 0].reshape(1, 2), products=hs.MOMENTS, fill=np.nan)
    got = second.stats.cpu().numpy() if device else second.stats
    assert hs.same_bits64(got, exp[0]) and second.mean_batch.shape == (2, 1)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_extremes_ties_zeros_infinities_and_an_empty_row(gpu_ctx, device):
    fields, flags = hs.extremes_case()
    nx = fields.shape[-1]
    for mode in ("area", "rows"):
        for products in (hs.EXTREMES, hs.MOMENTS | hs.EXTREMES):
            stats, _, _ = check(gpu_ctx, fields, device, "extremes", flags=flags, mode=mode, products=products)
        form(gpu_ctx, segs=2, v=4)
    assert stats[0, 0, 2, hs.IMIN] == 2 * nx + 3 and stats[0, 1, 1, hs.IMIN] == nx + 17 and np.signbit(stats[0, 1, 1, hs.MIN])
    assert list(stats[0, 2, 0, hs.MIN:]) == [np.inf, -np.inf, -1, -1] and stats[0, 2, 3, hs.MIN] == -np.inf
    odd = np.ascontiguousarray(fields[..., 1:])  # the same specials in other lanes, through the dword form
    for mode in ("area", "rows"):
        check(gpu_ctx, odd, device, "extremes, shifted by one column", flags=flags, mode=mode)
        form(gpu_ctx, v=1)


def test_host_batch_staged_in_several_bands(gpu_ctx, mifc_env):
    import torch

    mifc_env("MIFC_HSTATS_CHUNK_MIB", 1)
    fields, _, weight, pivot, _ = base(3, 6, 64, 1030, seed=50)  # about 5 MiB: 14 rows of the 19 planes fit the MiB
    flags = np.random.default_rng(50).choice(MIXED, size=(3, 6)).astype(np.int32)
    box = (5, 1029, 3, 61)
    for mode in ("area", "rows"):
        host = check(gpu_ctx, fields, False, "bands", weight=weight, pivot=pivot, flags=flags, mode=mode)
        got = form(gpu_ctx, v=1, nf=3, bands=5, launches=5)
        dev = call(gpu_ctx, fields, True, weight=weight, pivot=pivot, fdefined_in=flags, mode=mode)
        form(gpu_ctx, bands=1, launches=1)
        compare(host, dev, "host bands against one device call")
        check(gpu_ctx, fields, False, "bands, box", weight=weight, box=box, mode=mode)
    assert got["bands"] > 1 or run_is_forced()
    four = np.ascontiguousarray(fields[..., :1028])  # the 16-byte form through the staging
    check(gpu_ctx, four, False, "bands, v=4", mode="rows", flags=flags)
    form(gpu_ctx, v=4, bands=5)
    del torch


def test_full_size_level_on_the_device(gpu_ctx):
    fields = hs.wide_fields((1, 3, 720, 1440), 60, frac=0.01)
    weight = hs.wide_weight(720, 1440, 60)
    for mode in ("area", "rows"):
        check(gpu_ctx, fields, True, "720 x 1440", weight=weight, mode=mode)
        form(gpu_ctx, v=4, segs=1, blocks=180, launches=1, bands=1)


def test_zonal_mean_section_on_pressure_surfaces(gpu_ctx):
    """Two device calls: the row-wise mean of T and of the pressure batch, then vinterp_fields of the (nlev, ny, 1) result
    to three surfaces -- bit for bit the two restatements composed."""
    rng = np.random.default_rng(31)
    nlev, ny, nx = 12, 9, 13
    alevel, blevel = vi.hybrid_levels(nlev)
    ps = rng.uniform(700, 1050, (ny, nx)).astype(np.float32)
    p = vi.hybrid_coordinate(ps, alevel, blevel)
    t = hs.sprinkle((220 + 70 * (p / 1000.0) ** 0.19 + rng.normal(0, 0.3, p.shape)).astype(np.float32), rng, 0.02, hs.UNDEF)
    t[:, 4, :] = hs.UNDEF  # a latitude without data: undef in the section
    targets = np.array([850, 500, 300], np.float32)
    res = gpu_ctx.hstats_levels([put(t, True), put(p, True)], mode="rows", products="moments", want_mean=True)
    zonal, zfd = res.mean_batch, res.mean_flags
    form(gpu_ctx, mode="rows", nf=2, products=hs.MOMENTS, tested=1, segs=1, blocks=3, launches=1, bands=1)
    assert zonal.is_cuda and tuple(zonal.shape) == (2, nlev, ny)
    _, emean, efd = hs.hstats(np.stack([t, p]), mode=hs.ROWS, products=hs.MOMENTS)
    compare((res.stats.cpu().numpy(), zonal.cpu().numpy(), zfd), (hs.hstats(np.stack([t, p]), mode=hs.ROWS, products=hs.MOMENTS, fill=np.nan)[0], emean, efd),
            "zonal means")
    on_p, pfd = gpu_ctx.vinterp_fields(zonal[0].view(nlev, ny, 1), zonal[1].view(nlev, ny, 1), targets, fdefined_in=zfd[0], fdef_coord=zfd[1])
    e_on_p, e_pfd = vi.coord_fields(emean[:1].reshape(1, nlev, ny, 1), emean[1].reshape(nlev, ny, 1), targets, vi.LINEAR, efd[:1], efd[1])
    assert on_p.is_cuda and tuple(on_p.shape) == (3, ny, 1)
    got = on_p.cpu().numpy()
    assert hs.same_bits64(got.astype(np.float64), e_on_p[0].astype(np.float64)) and np.array_equal(pfd, e_pfd[0])
    assert (got[:, 4] == hs.UNDEF).all() and (e_on_p != hs.UNDEF).mean() > 0.3


def test_out_is_honoured_and_unrequested_slots_stay(gpu_ctx):
    import torch

    fields = base(2, 5)[0]
    pool = torch.full((3, 2, 5, 1, 8), -4242.5, dtype=torch.float64, device="cuda")
    res = gpu_ctx.hstats_levels(put(fields, True), products="extremes", out=pool[1])
    form(gpu_ctx, mode="area", nf=2, products=hs.EXTREMES, v=1, launches=1)
    got = pool.cpu().numpy()
    exp, _, _ = hs.hstats(fields, products=hs.EXTREMES, fill=-4242.5)
    assert res.stats.data_ptr() == pool[1].data_ptr() and hs.same_bits64(got[1], exp)
    assert (got[0] == -4242.5).all() and (got[2] == -4242.5).all()
    hpool = np.full((3, 5, 9, 8), -4242.5, np.float64)
    res = gpu_ctx.hstats_levels(fields[1], mode="rows", products=hs.MOMENTS, out=hpool[1])
    exp, _, _ = hs.hstats(fields[1:], mode=hs.ROWS, products=hs.MOMENTS, fill=-4242.5)
    assert np.shares_memory(res.stats, hpool[1]) and hs.same_bits64(hpool[1], exp[0]) and (hpool[0] == -4242.5).all() and (hpool[2] == -4242.5).all()
    assert res.n.shape == (5, 9) and np.array_equal(res.n, exp[0, :, :, hs.N])
    with pytest.raises(ValueError):
        gpu_ctx.hstats_levels(fields, out=np.zeros((2, 5, 2, 8)))
    with pytest.raises(ValueError):
        gpu_ctx.hstats_levels(fields, minus=fields[:1])
    with pytest.raises(RuntimeError, match="unknown mode"):
        gpu_ctx.hstats_levels(fields, mode="columns")


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx = 2, 3, 5, 8
    fields_h, minus_h, weight_h, _, _ = base(nf, nlev, ny, nx, seed=2)
    batch, n_stats, n_mean = nlev * ny * nx, nf * nlev * ny * 8, nlev * ny
    # room of the test's own around the fields: an output that ends in their first float or begins in their last one
    # stays inside it, whatever else the allocator has put nearby
    room = torch.zeros(4 * n_stats + nf * batch + 4 * n_stats, dtype=torch.float32, device="cuda")
    x = room[4 * n_stats:4 * n_stats + nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(fields_h))
    yroom = torch.zeros(nf * batch + 4 * n_stats, dtype=torch.float32, device="cuda")  # (and behind the minus batches)
    y = yroom[:nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(minus_h))
    w = torch.from_numpy(weight_h).cuda()
    sentinel = -4242.5
    stats = torch.full((nf, nlev, ny, 8), sentinel, dtype=torch.float64, device="cuda")
    means = torch.full((nf, nlev, ny), sentinel, dtype=torch.float32, device="cuda")

    def run(nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, fields=None, minus=None, weight=0, box=None, mode=1, products=3, stats_ptr=0, mean_ptrs=(),
            fd_mean=True, memkind=1, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        mtab = minus if isinstance(minus, ctypes.Array) else (ctypes.c_void_p * nf)(*[y[j].data_ptr() for j in range(nf)])
        m = (ctypes.c_void_p * nf)(*([means[f].data_ptr() for f in range(nf)] if mean_ptrs == () else mean_ptrs)) if mean_ptrs is not None else None
        bx = None if box is None else np.asarray(box, np.int32)
        fd = np.full(nf * nlev, 7, np.int32)
        rc = lib.mifc_hstats_levels(c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_,
                                    None if minus is None else ctypes.addressof(mtab), None, None, w.data_ptr() if weight == 0 else weight, hs.SOME_DEFINED,
                                    None if bx is None else bx.ctypes.data, mode, products, stats.data_ptr() if stats_ptr == 0 else stats_ptr,
                                    None if m is None else ctypes.addressof(m), fd.ctypes.data if fd_mean else None, float(hs.UNDEF), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    null_head = "a null pointer (fields, stats or fdefined_mean)"
    refusals = {
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "negative nlev": (dict(nlev_=-3), "nlev < 1"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "nx 0": (dict(nx_=0), "nx < 1 or ny < 1"),
        "negative ny": (dict(ny_=-2), "nx < 1 or ny < 1"),
        "2^31 cells": (dict(nx_=65536, ny_=32768), "more than 2^31 - 1 cells per level"),
        "bad memkind": (dict(memkind=7), "unknown memkind 7"),
        "unknown mode": (dict(mode=2), "unknown mode 2"),
        "negative mode": (dict(mode=-1), "unknown mode -1"),
        "no product": (dict(products=0), "products 0: no product or unknown bits"),
        "unknown product bits": (dict(products=5), "products 5: no product or unknown bits"),
        "mean without moments": (dict(products=2), "mean without MIFC_HSTATS_MOMENTS"),
        "null fields": (dict(fields="null"), null_head),
        "null stats": (dict(stats_ptr=None), null_head),
        "null fdefined_mean": (dict(fd_mean=False), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or mean[1])"),
        "null mean": (dict(mean_ptrs=[means[0].data_ptr(), None]), "a null pointer (fields[1] or mean[1])"),
        "minus for one field only": (dict(minus=(ctypes.c_void_p * nf)(y[0].data_ptr(), None)),
                                     "a null pointer (minus[1]): minus is given for every field or for none"),
        "empty box": (dict(box=(3, 3, 0, 5)), "the box {3, 3, 0, 5} is empty or outside the grid"),
        "reversed box": (dict(box=(0, 8, 4, 2)), "the box {0, 8, 4, 2} is empty or outside the grid"),
        "box beyond the columns": (dict(box=(0, 9, 0, 5)), "the box {0, 9, 0, 5} is empty or outside the grid"),
        "box beyond the rows": (dict(box=(0, 8, 0, 6)), "the box {0, 8, 0, 6} is empty or outside the grid"),
        "negative box": (dict(box=(-1, 8, 0, 5)), "the box {-1, 8, 0, 5} is empty or outside the grid"),
        "stats is a field": (dict(stats_ptr=x[1].data_ptr()), "stats[0] overlaps fields[1]"),
        "stats ends in a field": (dict(stats_ptr=x[0].data_ptr() - 8 * n_stats + 4), "stats[0] overlaps fields[0]"),
        "stats is the weight": (dict(stats_ptr=w.data_ptr()), "stats[0] overlaps weight"),
        "stats is a minus batch": (dict(minus=True, stats_ptr=y[1].data_ptr()), "stats[0] overlaps minus[1]"),
        "mean is a field": (dict(mean_ptrs=[means[0].data_ptr(), x[0].data_ptr()]), "mean[1] overlaps fields[0]"),
        "same mean twice": (dict(mean_ptrs=[means[0].data_ptr(), means[0].data_ptr()]), "mean[0] overlaps mean[1]"),
        "mean inside stats": (dict(mean_ptrs=[means[0].data_ptr(), stats.data_ptr() + 16]), "stats[0] overlaps mean[1]"),
    }
    before = {k: t.clone() for k, t in (("x", x), ("y", y), ("w", w))}
    for what, (kw, tail) in refusals.items():
        rc, err, fd = run(**kw)
        assert rc == 0 and err == "mifc_hstats_levels: " + tail, (what, err)
        assert (stats == sentinel).all().item() and (means == sentinel).all().item() and (fd == 7).all(), what
    for k, t in (("x", x), ("y", y), ("w", w)):
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, fd = run(sync=False)
    g.close()
    assert rc == 0 and "capture" in err and (fd == 7).all() and (stats == sentinel).all().item()
    # afterwards the same call runs
    rc, err, fd = run(minus=True)
    assert rc == 1 and err == "", err
    exp = hs.hstats(fields_h, minus_h, None, weight_h, None, hs.ROWS)
    compare((stats.cpu().numpy(), means.cpu().numpy(), fd.reshape(nf, nlev)), exp, "after the refusals")


def test_form_is_empty_before_the_first_call_of_a_thread(gpu_ctx):
    import threading

    seen = []
    t = threading.Thread(target=lambda: seen.append(gpu_ctx._lib.mifc_last_hstats_form()))
    t.start()
    t.join()
    assert seen == [b""]
