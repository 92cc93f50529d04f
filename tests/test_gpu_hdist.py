"""Area histograms and exact percentiles of level batches on the GPU (mifc_hdist.hip, mifc_hdist_*) against the numpy
restatement (tests/hdist_restate.py): counts as integers, percentiles bit for bit (a NaN matches a NaN), host and device
memory.  No tolerance anywhere: a count and an order statistic do not depend on the order of work.  The shapes are the
smallest at which the kernels can go wrong: one lane, one trip of 1024 cells and its tails, several trips, rows on and off
the 16-byte grid, boxes inside one group of four, every digit boundary of the selection."""
import ctypes
import functools

import numpy as np
import pytest

import hdist_restate as hd
from gpu_util import run_is_forced
from mi_fieldcalc_amd import hdist  # (without the feature the file fails here)

pytestmark = pytest.mark.gpu

A, S, N = hd.ALL_DEFINED, hd.SOME_DEFINED, hd.NONE_DEFINED
MIXED = [A, S, N]
U = hd.UNDEF
WIDTHS = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1027, 4096, 4097, 8193]


def put(a, device):
    import torch

    if a is None:
        return None
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if device else np.ascontiguousarray(a)


def back(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def fields_of(f, device, stacked):
    f = put(f, device)
    return f if stacked else [f[j] for j in range(f.shape[0])]


def hist_call(ctx, fields, edges, device, stacked=True, mask=None, **kw):
    return back(hdist.histogram_levels(ctx, fields_of(fields, device, stacked), edges, mask=put(mask, device), **kw))


def hist_check(ctx, fields, edges, device, label=None, stacked=True, mask=None, fdef_mask=S, box=None, mode="area", flags=None, undef=U):
    got = hist_call(ctx, fields, edges, device, stacked, mask, fdef_mask=fdef_mask, box=box, mode=mode, fdefined_in=flags, undef=undef)
    exp = hd.histogram(fields, edges, mask, fdef_mask, box, mode, flags, undef)
    assert got.dtype == np.int32 and got.shape == exp.shape, (label, got.shape, exp.shape)
    if not (got == exp).all():
        bad = np.argwhere(got != exp)
        first = tuple(int(b) for b in bad[0])
        raise AssertionError("%s %s %s: %d counts differ; first %s got %d expected %d" % (label, mode, "device" if device else "host", len(bad), first,
                                                                                          got[first], exp[first]))
    return got


def quant_call(ctx, fields, percentiles, device, stacked=True, mask=None, **kw):
    q, fd = hdist.quantile_levels(ctx, fields_of(fields, device, stacked), percentiles, mask=put(mask, device), **kw)
    return back(q), fd


def quant_check(ctx, fields, percentiles, device, label=None, stacked=True, method="linear", mask=None, fdef_mask=S, box=None, flags=None, undef=U):
    q, fd = quant_call(ctx, fields, percentiles, device, stacked, mask, method=method, fdef_mask=fdef_mask, box=box, fdefined_in=flags, undef=undef)
    with np.errstate(all="ignore"):
        eq, efd = hd.quantiles(fields, percentiles, method, mask, fdef_mask, box, flags, undef)
    where = (label, method, "device" if device else "host")
    assert q.shape == eq.shape and q.dtype == np.float32, (where, q.shape, eq.shape)
    if not hd.same(q, eq):
        bad = np.argwhere((q.view(np.uint32) != eq.view(np.uint32)) & ~(np.isnan(q) & np.isnan(eq)))
        first = tuple(int(b) for b in bad[0])
        raise AssertionError("%s: %d percentiles differ; first %s got %r expected %r" % (where, len(bad), first, q[first], eq[first]))
    assert np.array_equal(np.asarray(fd), efd), (where, fd, efd)
    return q, fd


def form(ctx, **expected_keys):
    """The launch shape of the last call, checked key by key -- unless the run forces a path."""
    got = hdist.last_hdist_form(ctx)
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


@functools.lru_cache(maxsize=None)
def base(nf=2, nlev=2, ny=3, nx=13, seed=1, frac=0.05):
    """Smooth levels around 280 with a little noise and some undefined cells; a mask with holes."""
    rng = np.random.default_rng(seed)
    f = np.stack([np.stack([hd.smooth_level(ny, nx, seed * 100 + g * 10 + k, 280.0 - 3 * k, 10.0 + g) for k in range(nlev)]) for g in range(nf)])
    f = hd.sprinkle(f, rng, frac, U)
    mask = hd.sprinkle(np.ones((ny, nx), np.float32), rng, 0.2, U)
    f.setflags(write=False)
    mask.setflags(write=False)
    return f, mask


EDGES7 = np.array([-np.inf, 268.0, 275.5, 280.0, 284.25, 291.0, 1.0e30], np.float32)


# ------------------------------------------------------------------------------------------------------- histogram
@pytest.mark.parametrize("nx", WIDTHS)
def test_histogram_widths(gpu_ctx, nx):
    """One lane, one trip and its tails, several trips; 16-byte loads where the rows allow them, dwords otherwise."""
    import torch

    fields, mask = base(2, 2, 3, nx, seed=nx)
    v = 4 if nx % 4 == 0 else 1
    for device in (False, True):
        for mode in ("area", "rows"):
            hist_check(gpu_ctx, fields, EDGES7, device, ("nx", nx), mode=mode)
            form(gpu_ctx, entry="hist", mode=mode, v=v, nf=2, nbins=8, mask=0, tested=1, launches=1, bands=1)
        hist_check(gpu_ctx, fields, EDGES7, device, ("nx", nx, "mask"), mask=mask, mode="rows")
        form(gpu_ctx, v=v, mask=1)
    if v == 4:  # the same batch off the 16-byte grid: the dword form
        buf = torch.zeros(fields.size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
        got = hdist.histogram_levels(gpu_ctx, buf[1:].view(fields.shape), EDGES7, mode="rows").cpu().numpy()
        form(gpu_ctx, v=1)
        assert (got == hd.histogram(fields, EDGES7, mode=hd.ROWS)).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 2, 4, 5, 8])
def test_histogram_fields_flags_values_and_mask(gpu_ctx, nf, device):
    fields, mask = base(nf, 3, 5, 70, seed=nf)
    fields = fields.copy()
    fields[0, 0, 1, 2] = np.nan  # under ALL_DEFINED a NaN is a value with a slot of its own; tested, it is a hole
    fields[0, 0, 1, 3] = U       # under ALL_DEFINED a stored undef is a value: it lands in the last bin
    flags = np.random.default_rng(nf).choice(MIXED, size=(nf, 3)).astype(np.int32)
    flags[0] = MIXED
    edges = [np.linspace(265 + g, 295 + g, 9 + 0 * g).astype(np.float32) for g in range(nf)]  # each field its own edges
    for mode in ("area", "rows"):
        got = hist_check(gpu_ctx, fields, edges, device, ("nf", nf), stacked=(nf != 2), flags=flags, mode=mode)
        form(gpu_ctx, nf=nf, nbins=10, tested=1, mask=0)
        assert got[0, 0, :, 10].sum() == 1 and got[0, 0, :, 9].sum() >= 1  # the NaN, the stored undef
        hist_check(gpu_ctx, fields, edges, device, ("nf", nf, "mask"), stacked=(nf != 2), flags=flags, mask=mask, mode=mode)
        form(gpu_ctx, mask=1)
    every = np.full((nf, 3), A, np.int32)
    hist_check(gpu_ctx, fields, edges[0], device, "untested", flags=every, mask=mask, fdef_mask=A)  # one list of edges for all
    form(gpu_ctx, tested=0, mask=0)  # (a mask that is all defined excludes nothing)
    none = hist_check(gpu_ctx, fields, edges, device, "tested mask only", flags=every, mask=mask)
    form(gpu_ctx, tested=1, mask=1)
    assert none.sum() == nf * 3 * int((mask != U).sum())
    nan_undef = np.float32(np.nan)
    hist_check(gpu_ctx, fields, edges, device, "undef is NaN", undef=nan_undef)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_histogram_boxes(gpu_ctx, device):
    ny, nx = 6, 1300
    fields, mask = base(2, 2, ny, nx, seed=5)
    for i0 in (0, 1, 3, 4, 1023, 1024):
        for i1 in (i0 + 1, i0 + 2, min(nx, i0 + 6), 1027 if i0 < 1027 else nx, nx):
            box = (i0, i1, 1 + i0 % 2, ny - (i1 % 2))
            hist_check(gpu_ctx, fields, EDGES7, device, ("box", box), box=box, mode="rows", mask=mask)
    hist_check(gpu_ctx, fields, EDGES7, device, "one cell", box=(1299, 1300, 5, 6))
    odd = np.ascontiguousarray(fields[..., :1297])
    hist_check(gpu_ctx, odd, EDGES7, device, "dwords, box", box=(2, 1295, 0, 6), mode="area")
    form(gpu_ctx, v=1)


@pytest.mark.parametrize("nedges", [1, 2, 63, 64, 65, 1024])
def test_histogram_edge_counts(gpu_ctx, nedges):
    fields, _ = base(2, 2, 7, 260, seed=nedges, frac=0.0)
    inner = np.linspace(262.0, 298.0, nedges).astype(np.float32) if nedges > 1 else np.array([280.0], np.float32)
    assert hd.check_edges(inner) < 0
    ends = inner.copy()
    if nedges >= 2:
        ends[0], ends[-1] = -np.inf, np.inf
    for device in (False, True):
        for e in (inner, ends):
            got = hist_check(gpu_ctx, fields, e, device, ("nedges", nedges), mode="rows")
            form(gpu_ctx, nbins=nedges + 1)
        assert got.shape[-1] == nedges + 2
        if nedges >= 2:
            assert got[..., 0].sum() == 0 and got[..., nedges].sum() == 0  # nothing below -inf, nothing at or above +inf


def test_histogram_values_at_the_edges(gpu_ctx):
    f32 = np.float32
    below = lambda x: np.nextafter(f32(x), f32(-np.inf))  # noqa: E731
    tiny = f32(1.0e-45)  # the smallest subnormal
    edges = np.array([-3.5, -tiny, 0.0, tiny, f32(1.0e-40), 2.0], np.float32)
    vals = np.array([-3.5, below(-3.5), -0.0, 0.0, -tiny, below(-tiny), tiny, f32(5.0e-41), f32(1.0e-40), below(1.0e-40), 2.0, below(2.0), np.inf, -np.inf,
                     3.4028235e38, -3.4028235e38], np.float32)
    level = np.resize(vals, (4, 9)).astype(np.float32)  # every value at least twice, at varying lanes
    fields = np.stack([level, level[::-1]])[None]
    for device in (False, True):
        got = hist_check(gpu_ctx, fields, edges, device, "edge values", flags=np.full((1, 2), A))
        assert (got == hd.histogram_literal(fields, edges, flags=np.full((1, 2), A))).all()
    # an edge -0.0 bins exactly as an edge +0.0 does; -0.0 and +0.0 fall into the same bin
    zeros = np.array([[-0.0, 0.0, -tiny, tiny, -0.0, 0.0]], np.float32)[None, None]
    a = hist_check(gpu_ctx, zeros, np.array([0.0], np.float32), True, "edge +0")
    b = hist_check(gpu_ctx, zeros, np.array([-0.0], np.float32), True, "edge -0")
    assert a.tolist() == b.tolist() == [[[[1, 5, 0]]]]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_histogram_counts_beyond_16_bits_distinct_values_and_a_ramp(gpu_ctx, device):
    const = np.full((1, 1, 300, 300), 281.25, np.float32)  # 90 000 cells in one bin: every wave is of one bin
    got = hist_check(gpu_ctx, const, EDGES7, device, "constant", flags=[[A]])
    assert got[0, 0, 0, 4] == 90000 and got.sum() == 90000
    rows = hist_check(gpu_ctx, const, EDGES7, device, "constant", flags=[[A]], mode="rows")
    assert (rows[0, 0, :, 4] == 300).all()
    distinct = (260.0 + np.random.default_rng(3).permutation(40 * 129).astype(np.float32) * np.float32(0.0078125)).reshape(1, 1, 40, 129)
    assert np.unique(distinct).size == distinct.size
    hist_check(gpu_ctx, distinct, np.linspace(259, 302, 1024).astype(np.float32), device, "distinct")
    ramp = np.broadcast_to(np.linspace(260, 300, 2053).astype(np.float32), (1, 2, 5, 2053)).copy()  # neighbours share bins
    for mode in ("area", "rows"):
        hist_check(gpu_ctx, ramp, np.linspace(262, 298, 17).astype(np.float32), device, "ramp", mode=mode)


def test_histogram_rows_sum_to_the_area_and_host_bands_equal_the_device(gpu_ctx, mifc_env):
    mifc_env("MIFC_HDIST_CHUNK_MIB", 1)
    fields, mask = base(2, 2, 40, 4101, seed=9)  # 16 KiB a row and plane: 12 rows of the 5 planes fit the MiB
    flags = np.array([[A, S], [N, S]], np.int32)
    box = (3, 4099, 2, 39)
    for bx in (None, box):
        host_rows = hist_check(gpu_ctx, fields, EDGES7, False, "bands", mask=mask, flags=flags, box=bx, mode="rows")
        got = form(gpu_ctx, v=1, bands=4, launches=4)
        host_area = hist_check(gpu_ctx, fields, EDGES7, False, "bands", mask=mask, flags=flags, box=bx, mode="area")
        dev_rows = hist_call(gpu_ctx, fields, EDGES7, True, mask=mask, fdefined_in=flags, box=bx, mode="rows")
        form(gpu_ctx, bands=1, launches=1)
        dev_area = hist_call(gpu_ctx, fields, EDGES7, True, mask=mask, fdefined_in=flags, box=bx, mode="area")
        assert (host_rows == dev_rows).all() and (host_area == dev_area).all()
        assert (dev_rows.sum(axis=2, keepdims=True) == dev_area).all()
    assert got["bands"] > 1 or run_is_forced()
    four = np.ascontiguousarray(fields[..., :4100])  # the 16-byte form through the staging
    hist_check(gpu_ctx, four, EDGES7, False, "bands, v=4", mode="rows", flags=flags)
    form(gpu_ctx, v=4, bands=3)  # (no mask: 15 rows of the 4 planes fit)


# ----------------------------------------------------------------------------------------------------- percentiles
PS = [0.0, 50.0, 100.0, 50.0, 2.0, 98.0, 33.3]  # the ends, a repeated one, the colour scale, one that interpolates


@pytest.mark.parametrize("nx", [1, 3, 4, 5, 64, 257, 1027, 4096, 4097])
def test_quantile_widths(gpu_ctx, nx):
    fields, mask = base(2, 2, 3, nx, seed=nx + 1)
    for device in (False, True):
        for method in ("lower", "linear"):
            quant_check(gpu_ctx, fields, PS, device, ("nx", nx), method=method)
            form(gpu_ctx, entry="quant", mode=method, v=4 if nx % 4 == 0 else 1, nf=2, chunks=1)
        quant_check(gpu_ctx, fields, PS, device, ("nx", nx, "mask, box"), mask=mask, box=(0, max(1, nx - 1), 1, 3))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_quantile_small_counts_and_levels_of_different_n(gpu_ctx, device):
    """n = 0, 1, 2, 3 and a full level in one call: levels of one call with different n."""
    level = np.array([[3.5, -1.25, 7.0, 2.0, 9.5, 0.5]], np.float32)
    f = np.stack([np.where(np.arange(6) < n, level, U) for n in (0, 1, 2, 3, 6)]).reshape(1, 5, 1, 6).astype(np.float32)
    for method in ("lower", "linear"):
        q, fd = quant_check(gpu_ctx, f, PS, device, "n = 0..3", method=method)
        assert fd[0].tolist() == [N, A, A, A, A] and (q[0, 0] == U).all() and (q[0, 1] == np.float32(3.5)).all()
        lq, lfd = hd.quantiles_literal(f, PS, method)
        assert hd.same(q, lq) and np.array_equal(fd, lfd)
    q, _ = quant_check(gpu_ctx, f, [50.0], device, "median of two", method="linear")
    assert q[0, 2, 0] == np.float32(1.125) and q[0, 3, 0] == np.float32(3.5)
    flags = np.array([[N, S, A, A, A]], np.int32)  # a NONE_DEFINED level is tested like SOME_DEFINED; ALL_DEFINED counts undef
    q, fd = quant_check(gpu_ctx, f, [100.0], device, "flags", flags=flags)
    assert q[0, 2, 0] == U and fd[0].tolist() == [N, A, A, A, A]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_quantile_ties(gpu_ctx, device):
    rng = np.random.default_rng(4)
    three = rng.choice(np.array([271.5, 280.0, 280.0000305], np.float32), size=(1, 2, 37, 61)).astype(np.float32)
    const = np.full((1, 2, 37, 61), -4.75, np.float32)
    for method in ("lower", "linear"):
        quant_check(gpu_ctx, three, PS, device, "three values", method=method)
        q, _ = quant_check(gpu_ctx, const, PS, device, "constant", method=method, flags=[[A, S]])
        form(gpu_ctx, prefix=32, passes=0)
        assert (q == np.float32(-4.75)).all()
    quant_check(gpu_ctx, np.concatenate([three, const]), PS, device, "both", stacked=False)
    form(gpu_ctx, nf=2)


@pytest.mark.parametrize("bit", range(32))
def test_quantile_two_values_that_first_differ_at_every_bit(gpu_ctx, bit):
    """Whatever the digit width, every digit boundary is crossed by one of these: the median between two values whose keys
    first differ at `bit`, and the extremes."""
    v, lo, hi = hd.two_valued(bit, n=8)
    f = v.reshape(1, 1, 2, 4)
    for device in (False, True):
        q, _ = quant_check(gpu_ctx, f, [50.0, 0.0, 100.0], device, ("bit", bit), method="linear", flags=[[A]])
        got = form(gpu_ctx, prefix=31 - bit, passes=-(-(bit + 1) // 11))
        assert q[0, 0, 1] == lo and q[0, 0, 2] == hi
    assert got["passes"] <= 3
    odd = np.array([hi, lo, hi, lo, hi, lo, hi], np.float32).reshape(1, 1, 1, 7)  # three of the smaller, four of the larger: the median is the larger
    q, _ = quant_check(gpu_ctx, odd, [50.0], True, ("bit", bit, "odd"), method="lower", flags=[[A]])
    assert q.view(np.uint32)[0, 0, 0] == np.array([hi]).view(np.uint32)[0]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_quantile_special_values(gpu_ctx, device):
    tiny = np.float32(1.0e-45)
    vals = np.array([-np.inf, -3.4028235e38, -1.0, -1.0e-40, -tiny, -0.0, 0.0, tiny, 1.0e-40, 1.0, 3.4028235e38, np.inf], np.float32)
    rng = np.random.default_rng(8)
    f = rng.permutation(np.resize(vals, 60)).reshape(1, 1, 5, 12).astype(np.float32)
    ps = np.linspace(0, 100, 16).astype(np.float32)
    for method in ("lower", "linear"):
        q, _ = quant_check(gpu_ctx, f, ps, device, "across the sign", method=method, flags=[[A]])
        form(gpu_ctx, prefix=0, passes=3)
        with np.errstate(all="ignore"):
            lq, _ = hd.quantiles_literal(f, ps, method, flags=[[A]])
        assert hd.same(q, lq)
    zeros = np.array([0.0, -0.0, 0.0, -0.0, -0.0], np.float32).reshape(1, 1, 1, 5)  # -0 < +0: three -0, then two +0
    q, _ = quant_check(gpu_ctx, zeros, [0.0, 50.0, 60.0, 100.0], device, "signed zeros", method="lower")
    assert np.signbit(q[0, 0]).tolist() == [True, True, False, False]
    nans = f.copy()
    nans[0, 0, 0, :3] = [np.nan, -np.nan, np.float32(np.nan)]
    q, fd = quant_check(gpu_ctx, nans, [0.0, 90.0, 96.0, 100.0], device, "NaN above +inf", method="lower", flags=[[A]])
    assert np.isnan(q[0, 0, 2:]).all() and not np.isnan(q[0, 0, :2]).any() and fd[0, 0] == A
    q, _ = quant_check(gpu_ctx, nans, [0.0, 50.0, 100.0], device, "NaN tested away", method="lower")
    assert not np.isnan(q).any()


def test_quantile_eight_fields_sixteen_percentiles_and_blocks_of_levels(gpu_ctx, mifc_env):
    fields, mask = base(8, 3, 9, 130, seed=12)
    ps = np.linspace(0, 100, 16).astype(np.float32)
    flags = np.random.default_rng(12).choice(MIXED, size=(8, 3)).astype(np.int32)
    for device in (False, True):
        for method in ("lower", "linear"):
            one = quant_check(gpu_ctx, fields, ps, device, "8 x 16", method=method, flags=flags, mask=mask)
            form(gpu_ctx, nf=8, chunks=1)
    mifc_env("MIFC_HDIST_CHUNK_MIB", 1)  # 8 fields * 32 prefixes * 8 KiB: one level at a time, on the device too
    for device in (False, True):
        blocks = quant_check(gpu_ctx, fields, ps, device, "8 x 16, blocks", method="linear", flags=flags, mask=mask)
        form(gpu_ctx, chunks=3)
        assert hd.same(blocks[0], one[0]) and np.array_equal(blocks[1], one[1])


def test_quantile_host_chunks_of_levels_equal_the_device(gpu_ctx, mifc_env):
    mifc_env("MIFC_HDIST_CHUNK_MIB", 1)
    fields, mask = base(1, 7, 64, 1030, seed=13)  # 258 KiB a level: three levels and their counters fit the MiB
    host = quant_check(gpu_ctx, fields, [2.0, 50.0, 98.0], False, "chunks", method="lower", mask=mask, box=(1, 1029, 3, 60))
    got = form(gpu_ctx, chunks=3)
    dev = quant_check(gpu_ctx, fields, [2.0, 50.0, 98.0], True, "chunks", method="lower", mask=mask, box=(1, 1029, 3, 60))
    form(gpu_ctx, chunks=1)
    assert hd.same(host[0], dev[0]) and np.array_equal(host[1], dev[1])
    assert got["chunks"] > 1 or run_is_forced()


def test_quantiles_off_the_16_byte_grid_and_counters_without_the_ballot(gpu_ctx, mifc_env):
    import torch

    fields, mask = base(2, 2, 5, 1028, seed=14)
    quant_check(gpu_ctx, fields, PS, True, "aligned", mask=mask)
    form(gpu_ctx, v=4)
    buf = torch.zeros(fields.size + 3, dtype=torch.float32, device="cuda")
    buf[3:] = torch.from_numpy(fields.reshape(-1)).cuda()
    q, fd = hdist.quantile_levels(gpu_ctx, buf[3:].view(fields.shape), PS, mask=put(mask, True))
    form(gpu_ctx, v=1)
    with np.errstate(all="ignore"):
        eq, efd = hd.quantiles(fields, PS, hd.LINEAR, mask)
    assert hd.same(q.cpu().numpy(), eq) and np.array_equal(fd, efd)
    # MIFC_HDIST_AGGREGATE=0: every lane's runs go to the LDS counters one by one -- the same counts and percentiles
    mifc_env("MIFC_HDIST_AGGREGATE", 0)
    const = np.full((1, 1, 300, 300), 281.25, np.float32)
    ramp = np.broadcast_to(np.linspace(260, 300, 2053).astype(np.float32), (1, 2, 5, 2053)).copy()
    for device in (False, True):
        assert hist_check(gpu_ctx, const, EDGES7, device, "constant, plain", flags=[[A]])[0, 0, 0, 4] == 90000
        hist_check(gpu_ctx, ramp, np.linspace(262, 298, 17).astype(np.float32), device, "ramp, plain", mode="rows")
        hist_check(gpu_ctx, fields, EDGES7, device, "plain", mask=mask)
        quant_check(gpu_ctx, fields, PS, device, "plain", mask=mask)
        quant_check(gpu_ctx, const, PS, device, "constant, plain")


def test_quantile_of_a_smooth_level_takes_two_digit_passes(gpu_ctx):
    f = hd.smooth_level(181, 360, 3, span=20.0).reshape(1, 1, 181, 360)  # 260 .. 300: one exponent, two mantissa bits shared
    q, _ = quant_check(gpu_ctx, f, [2.0, 25.0, 50.0, 75.0, 98.0], True, "smooth", flags=[[A]])
    got = form(gpu_ctx, passes=2)
    assert got["prefix"] >= 10 and (np.diff(q[0, 0]) > 0).all()


# -------------------------------------------------------------------------------------------------------- refusals
def test_histogram_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx, ne = 2, 3, 5, 8, 4
    fields_h, mask_h = base(nf, nlev, ny, nx, seed=2)
    batch, n_hist = nlev * ny * nx, nf * nlev * ny * (ne + 2)
    room = torch.zeros(2 * n_hist + nf * batch + 2 * n_hist, dtype=torch.float32, device="cuda")
    x = room[2 * n_hist:2 * n_hist + nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(fields_h))
    m = torch.from_numpy(mask_h).cuda()
    hist = torch.full((nf, nlev, ny, ne + 2), -7, dtype=torch.int32, device="cuda")
    good = np.array([[270, 275, 280, 285]] * nf, np.float32)

    def run(nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, fields=None, edges=good, ne_=ne, mask=0, box=None, mode=1, hist_ptr=0, memkind=1, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        bx = None if box is None else np.asarray(box, np.int32)
        e = None if edges is None else np.ascontiguousarray(edges, np.float32)
        rc = lib.mifc_hdist_histogram_levels(c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_,
                                             None if e is None else e.ctypes.data, ne_, m.data_ptr() if mask == 0 else mask, S,
                                             None if bx is None else bx.ctypes.data, mode, hist.data_ptr() if hist_ptr == 0 else hist_ptr, float(U), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error()

    def edges_with(f, e, value):
        bad = good.copy()
        bad[f, e] = value
        return bad

    refusals = {
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "nx 0": (dict(nx_=0), "nx < 1 or ny < 1"),
        "ny negative": (dict(ny_=-2), "nx < 1 or ny < 1"),
        "memkind": (dict(memkind=5), "unknown memkind 5"),
        "too many cells": (dict(nx_=65536, ny_=32768), "more than 2^31 - 1 cells per level"),
        "empty box": (dict(box=(3, 3, 0, 5)), "the box {3, 3, 0, 5} is empty or outside the grid"),
        "box outside": (dict(box=(0, 9, 0, 5)), "the box {0, 9, 0, 5} is empty or outside the grid"),
        "box rows": (dict(box=(0, 8, 4, 2)), "the box {0, 8, 4, 2} is empty or outside the grid"),
        "mode": (dict(mode=2), "unknown mode 2"),
        "nedges 0": (dict(ne_=0), "nedges 0 outside 1..1024"),
        "nedges 1025": (dict(ne_=1025), "nedges 1025 outside 1..1024"),
        "null fields": (dict(fields="null"), "a null pointer (fields, edges or hist)"),
        "null edges": (dict(edges=None), "a null pointer (fields, edges or hist)"),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1])"),
        "NaN edge": (dict(edges=edges_with(1, 2, np.nan)), "field 1: edge 2 is NaN or not above the edge before it"),
        "equal edges": (dict(edges=edges_with(0, 1, 270)), "field 0: edge 1 is NaN or not above the edge before it"),
        "descending": (dict(edges=edges_with(1, 3, 100)), "field 1: edge 3 is NaN or not above the edge before it"),
        "both zeros": (dict(edges=np.array([[-1, -0.0, 0.0, 1]] * nf, np.float32)), "field 0: edge 2 is NaN or not above the edge before it"),
        "hist inside a field": (dict(hist_ptr=x.data_ptr() + 4 * (batch - 1)), "hist[0] overlaps fields[0]"),
        "hist ends in a field": (dict(hist_ptr=x.data_ptr() - 4 * n_hist + 4), "hist[0] overlaps fields[0]"),
        "hist is the mask": (dict(hist_ptr=m.data_ptr()), "hist[0] overlaps mask"),
    }
    before = {k: t.clone() for k, t in (("x", x), ("m", m))}
    for what, (kw, tail) in refusals.items():
        rc, err = run(**kw)
        assert rc == 0 and err == "mifc_hdist_histogram_levels: " + tail, (what, err)
        assert (hist == -7).all().item(), what
    for k, t in (("x", x), ("m", m)):
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:  # while a graph capture is open (nothing may synchronise inside it)
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err = run(sync=False)
    g.close()
    assert rc == 0 and "capture" in err and (hist == -7).all().item()
    rc, err = run()  # afterwards the same call runs
    assert rc == 1 and err == "", err
    assert (hist.cpu().numpy() == hd.histogram(fields_h, good, mask_h, mode=hd.ROWS)).all()


def test_quantile_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx, nq = 2, 3, 5, 8, 3
    fields_h, mask_h = base(nf, nlev, ny, nx, seed=2)
    batch, n_quant = nlev * ny * nx, nf * nlev * nq
    room = torch.zeros(2 * n_quant + nf * batch + 2 * n_quant, dtype=torch.float32, device="cuda")
    x = room[2 * n_quant:2 * n_quant + nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(fields_h))
    m = torch.from_numpy(mask_h).cuda()
    sentinel = -4242.5
    quant = torch.full((nf, nlev, nq), sentinel, dtype=torch.float32, device="cuda")
    good = np.array([10, 50, 90], np.float32)

    def run(nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, fields=None, ps=good, nq_=nq, method=1, box=None, quant_ptr=0, fd=True, memkind=1, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        bx = None if box is None else np.asarray(box, np.int32)
        p = None if ps is None else np.ascontiguousarray(ps, np.float32)
        flags = np.full(nf * nlev, 7, np.int32)
        rc = lib.mifc_hdist_quantile_levels(c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_,
                                            None if p is None else p.ctypes.data, nq_, method, m.data_ptr(), S, None if bx is None else bx.ctypes.data,
                                            quant.data_ptr() if quant_ptr == 0 else quant_ptr, flags.ctypes.data if fd else None, float(U), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), flags

    null_head = "a null pointer (fields, percentiles, quant or fdefined_q)"
    refusals = {
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "nx 0": (dict(nx_=0), "nx < 1 or ny < 1"),
        "memkind": (dict(memkind=-1), "unknown memkind -1"),
        "too many cells": (dict(nx_=65536, ny_=32768), "more than 2^31 - 1 cells per level"),
        "empty box": (dict(box=(0, 8, 5, 5)), "the box {0, 8, 5, 5} is empty or outside the grid"),
        "method": (dict(method=2), "unknown method 2"),
        "nq 0": (dict(nq_=0), "nq 0 outside 1..16"),
        "nq 17": (dict(nq_=17), "nq 17 outside 1..16"),
        "null fields": (dict(fields="null"), null_head),
        "null percentiles": (dict(ps=None), null_head),
        "null flags": (dict(fd=False), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(None, x[1].data_ptr())), "a null pointer (fields[0])"),
        "NaN p": (dict(ps=[10, np.nan, 90]), "percentile 1 is NaN or outside [0, 100]"),
        "p above": (dict(ps=[10, 50, 100.00001]), "percentile 2 is NaN or outside [0, 100]"),
        "p below": (dict(ps=[-0.5, 50, 90]), "percentile 0 is NaN or outside [0, 100]"),
        "quant inside a field": (dict(quant_ptr=x.data_ptr() + 4 * (nf * batch - 1)), "quant[0] overlaps fields[1]"),
        "quant ends in a field": (dict(quant_ptr=x.data_ptr() - 4 * n_quant + 4), "quant[0] overlaps fields[0]"),
        "quant is the mask": (dict(quant_ptr=m.data_ptr()), "quant[0] overlaps mask"),
    }
    before = {k: t.clone() for k, t in (("x", x), ("m", m))}
    for what, (kw, tail) in refusals.items():
        rc, err, flags = run(**kw)
        assert rc == 0 and err == "mifc_hdist_quantile_levels: " + tail, (what, err)
        assert (quant == sentinel).all().item() and (flags == 7).all(), what
    for k, t in (("x", x), ("m", m)):
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, flags = run(sync=False)
    g.close()
    assert rc == 0 and "capture" in err and (flags == 7).all() and (quant == sentinel).all().item()
    rc, err, flags = run()
    assert rc == 1 and err == "", err
    eq, efd = hd.quantiles(fields_h, good, hd.LINEAR, mask_h)
    assert hd.same(quant.cpu().numpy(), eq) and np.array_equal(flags.reshape(nf, nlev), efd)


def test_form_is_empty_before_the_first_call_of_a_thread(gpu_ctx):
    import threading

    seen = []
    t = threading.Thread(target=lambda: seen.append(gpu_ctx._lib.mifc_last_hdist_form()))
    t.start()
    t.join()
    assert seen == [b""]
