"""Percentiles across ensemble members on the GPU (mifc_quantile.hip, mifc_ensembleQuantiles): bit for bit the numpy
restatement (tests/quantile_restate.py; a NaN matches any NaN), with equal flags, across the sorting-network tiers, the
bisection path and the kernel-argument / device-table split; host and device memory; the refusals; and cross-checks
against extremeValue and meanValue."""
import ctypes

import numpy as np
import pytest

import quantile_restate as qr
from cases import same_bits

pytestmark = pytest.mark.gpu

PS = [0, 2.5, 10, 50, 90, 99.9, 100]
METHODS = {"lower": qr.LOWER, "linear": qr.LINEAR}


def make_members(nmem, nlev, ny, nx, seed, undef=qr.UNDEF, specials=True):
    """Values on a 1/8 grid (many ties), signed zeros, infinities, undef and NaN sprinkled."""
    rng = np.random.default_rng(seed)
    x = (np.round(rng.normal(0, 3, size=(nmem, nlev, ny, nx)) * 8) / 8).astype(np.float32)
    if specials:
        m = rng.random(x.shape)
        x[m < 0.04] = -0.0
        x[(m >= 0.04) & (m < 0.08)] = 0.0
        x[(m >= 0.08) & (m < 0.10)] = np.inf
        x[(m >= 0.10) & (m < 0.12)] = -np.inf
        x[(m >= 0.12) & (m < 0.17)] = undef
        x[(m >= 0.17) & (m < 0.19)] = np.nan
    return x


def mixed_flags(nmem, nlev, seed):
    return np.random.default_rng(seed).choice([qr.ALL_DEFINED, qr.SOME_DEFINED, qr.NONE_DEFINED], size=(nmem, nlev)).astype(np.int32)


def gpu(ctx, x, ps, method, flags=None, undef=qr.UNDEF, device=False, stacked=True):
    import torch

    f = torch.from_numpy(np.ascontiguousarray(x)).cuda() if device else np.ascontiguousarray(x)
    fields = f if stacked else [f[j] for j in range(f.shape[0])]
    out, fd = ctx.ensembleQuantiles(fields, ps, fdefined_in=flags, method=method, undef=undef)
    return (out.cpu().numpy() if device else out), fd


def check(ctx, x, ps, method, flags=None, undef=qr.UNDEF, device=False, stacked=True, label=None):
    got, fd = gpu(ctx, x, ps, method, flags, undef, device, stacked)
    exp, efd = qr.quantiles(x, ps, METHODS[method], flags, undef)
    if not same_bits(got, exp, nan_payload=False):
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))
    assert list(np.atleast_1d(fd)) == efd, label


@pytest.mark.parametrize("nmem", [1, 2, 3, 31, 32, 33, 51, 64, 65, 200])
def test_every_tier_both_methods(gpu_ctx, nmem):
    nlev, ny, nx = 2, 9, 13  # nx not a multiple of 4
    x = make_members(nmem, nlev, ny, nx, 100 + nmem)
    flags = mixed_flags(nmem, nlev, nmem)
    for k, method in enumerate(("lower", "linear")):
        for device in (False, True):
            check(gpu_ctx, x, PS, method, flags, device=device, stacked=(k == 0), label=(nmem, method, device))
    # more percentiles than the kernel arguments hold: the device table with a small ensemble too
    ps = np.linspace(0, 100, 21).astype(np.float32)
    check(gpu_ctx, x, ps, "linear", flags, device=True, label=(nmem, "21 percentiles"))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_levels_one_and_sixteen(gpu_ctx, device):
    for nmem in (51, 70):
        x = make_members(nmem, 16, 21, 37, 16 + nmem)
        flags = mixed_flags(nmem, 16, 3 + nmem)
        for method in ("lower", "linear"):
            check(gpu_ctx, x, [5, 50, 95], method, flags, device=device, label=(nmem, 16, method))
            # one level as 2-D members: one flag back, an int
            got, fd = gpu(gpu_ctx, x[:, 3], [5, 50, 95], method, flags[:, 3], device=device)
            exp, efd = qr.quantiles(x[:, 3], [5, 50, 95], METHODS[method], flags[:, 3])
            assert isinstance(fd, int) and fd == efd[0] and got.shape == (3, 21, 37)
            assert same_bits(got, exp, nan_payload=False)


def test_nan_as_undef_and_cells_without_members(gpu_ctx):
    nan = np.float32(np.nan)
    x = make_members(33, 3, 10, 7, 5, undef=nan)
    x[:, 1, 2:5, :] = nan  # no member counts here unless flagged ALL_DEFINED
    flags = np.full((33, 3), qr.SOME_DEFINED, np.int32)
    flags[4, 0] = qr.ALL_DEFINED
    flags[:, 2] = qr.NONE_DEFINED
    for method in ("lower", "linear"):
        for device in (False, True):
            check(gpu_ctx, x, PS, method, flags, undef=nan, device=device, label=(method, device))
    # every cell without members: undef everywhere, NONE_DEFINED; flags None: SOME_DEFINED members
    x2 = np.full((5, 1, 4, 6), qr.UNDEF, np.float32)
    got, fd = gpu(gpu_ctx, x2, [50], "lower", device=True)
    assert (got == qr.UNDEF).all() and list(fd) == [qr.NONE_DEFINED]


def test_members_off_the_16_byte_grid(gpu_ctx):
    import torch

    nmem, ny, nx = 51, 11, 13
    x = make_members(nmem, 1, ny, nx, 77)[:, 0]
    n = ny * nx
    buf = torch.zeros(nmem * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x.reshape(-1)).cuda()
    members = [buf[1 + j * n:1 + (j + 1) * n].view(ny, nx) for j in range(nmem)]  # 4 bytes past the grid
    flags = mixed_flags(nmem, 1, 9)[:, 0]
    for method in ("lower", "linear"):
        out, fd = gpu_ctx.ensembleQuantiles(members, PS, fdefined_in=flags, method=method)
        exp, efd = qr.quantiles(x, PS, METHODS[method], flags)
        assert same_bits(out.cpu().numpy(), exp, nan_payload=False) and fd == efd[0], method


def test_host_batches_in_several_chunks(gpu_ctx, mifc_env):
    mifc_env("MIFC_QUANTILE_CHUNK_MIB", 1)
    # (nmem, nlev, ny, nx): a level larger than the budget (cell ranges), several levels per chunk, and the bisection path
    for nmem, nlev, ny, nx in ((51, 3, 211, 301), (51, 16, 30, 40), (200, 2, 33, 45)):
        x = make_members(nmem, nlev, ny, nx, nmem + nlev)
        flags = mixed_flags(nmem, nlev, nlev)
        check(gpu_ctx, x, PS, "linear", flags, device=False, label=("chunks", nmem, nlev))
        check(gpu_ctx, x[:, :1], [50], "lower", flags[:, :1], device=False, label=("chunks", nmem, 1))


# The seams of the chunk plan at the smallest shapes that reach them.  The budget is 1 MiB = 1 048 576 bytes, a staged cell
# costs 4 * (nmem + 4 percentiles) bytes: 256 with 60 members (4 096 cells per MiB), 252 with 59 (4 161).
CHUNK_SEAMS = {
    "a level fits exactly": (60, 3, 64, 64, False),        # 4 096 cells: one level per chunk, no cell split
    "one cell over": (60, 2, 17, 241, False),              # 4 097 cells: ranges of 4 096 and 1
    "a short last chunk of levels": (60, 6, 25, 40, False),  # four levels per chunk: 4 + 2
    "ranges off the multiple of 4": (59, 1, 25, 333, False),  # 8 325 cells: 4 161 / 4 161 / 3 (no rounding here)
    "no members": (0, 2, 6, 8, False),                     # no scratch for members; NONE_DEFINED
    "device table, host": (9, 70, 6, 8, False),            # past the 64 levels of the kernel arguments
    "device table, device": (9, 70, 6, 8, True),
}


@pytest.mark.parametrize("case", list(CHUNK_SEAMS))
def test_chunk_seams(gpu_ctx, mifc_env, case):
    mifc_env("MIFC_QUANTILE_CHUNK_MIB", 1)
    nmem, nlev, ny, nx, device = CHUNK_SEAMS[case]
    ps = [10, 37.5, 50, 90]
    x = make_members(nmem, nlev, ny, nx, 7 * nmem + nlev)
    flags = mixed_flags(nmem, nlev, nlev)
    if nmem > 0:
        check(gpu_ctx, x, ps, "linear", flags, device=device, label=case)
        return
    out = np.full((4, nlev, ny, nx), -7.0, np.float32)  # the shape comes from the output
    got, fd = gpu_ctx.ensembleQuantiles([], ps, method="linear", out=out)
    exp, efd = qr.quantiles(x, ps, qr.LINEAR, flags)
    assert same_bits(got, exp) and list(fd) == efd == [qr.NONE_DEFINED] * nlev


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nmem", [51, 70])
def test_output_aliasing_members(gpu_ctx, device, nmem):
    import torch

    x = make_members(nmem, 2, 12, 9, 31 + nmem)
    flags = mixed_flags(nmem, 2, 8)
    for method in ("lower", "linear"):
        exp, efd = qr.quantiles(x, [10, 90], METHODS[method], flags)
        f = torch.from_numpy(x.copy()).cuda() if device else x.copy()
        out, fd = gpu_ctx.ensembleQuantiles(f, [10, 90], fdefined_in=flags, method=method, out=f[3:5])  # outputs = members 3, 4
        got = f.cpu().numpy() if device else f
        assert same_bits(got[3:5], exp, nan_payload=False) and list(fd) == efd, method
        assert same_bits(np.delete(got, [3, 4], axis=0), np.delete(x, [3, 4], axis=0)), "other members untouched"


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nmem, ny, nx, nlev = 5, 6, 7, 2
    x = torch.from_numpy(make_members(nmem, nlev, ny, nx, 1)).cuda()
    sentinel = -4242.5
    outs = torch.full((3, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")

    def call(method=0, nx_=nx, ny_=ny, nlev_=nlev, nmem_=nmem, ps=(10.0, 50.0, 90.0), nq=3, out_ptrs=None, fields=None, fd_out=True, memkind=1,
             sync=True):
        tab = (ctypes.c_void_p * nmem)(*[x[j].data_ptr() for j in range(nmem)]) if fields is None or fields == "null" else fields
        o = (ctypes.c_void_p * 3)(*([outs[q].data_ptr() for q in range(3)] if out_ptrs is None or out_ptrs == "null" else out_ptrs))
        p = np.asarray((0.0,) if ps is None else ps, np.float32)
        fd = np.full(nlev, 7, np.int32)
        rc = lib.mifc_ensembleQuantiles(c, method, nx_, ny_, nlev_, None if fields == "null" else ctypes.addressof(tab), None, nmem_,
                                        None if ps is None else p.ctypes.data, nq, None if out_ptrs == "null" else ctypes.addressof(o),
                                        fd.ctypes.data if fd_out else None, float(qr.UNDEF), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    nan = float("nan")
    shape = "nlev < 1, or a negative nx, ny or nmem"
    null = "a null pointer (percentiles, fres, fdefined_out or fields)"
    cases = {  # what: (the call, the text behind "mifc_ensembleQuantiles: ")
        "unknown method": (dict(method=2), "unknown method 2 (MIFC_QUANTILE_LOWER or MIFC_QUANTILE_LINEAR)"),
        "negative method": (dict(method=-1), "unknown method -1 (MIFC_QUANTILE_LOWER or MIFC_QUANTILE_LINEAR)"),
        "nq < 1": (dict(nq=0), "nq < 1"),
        "NaN percentile": (dict(ps=(10.0, nan, 90.0)), "percentiles[1] is NaN or outside [0, 100]"),
        "percentile < 0": (dict(ps=(-0.5, 50.0, 90.0)), "percentiles[0] is NaN or outside [0, 100]"),
        "percentile > 100": (dict(ps=(10.0, 50.0, 100.5)), "percentiles[2] is NaN or outside [0, 100]"),
        "nlev < 1": (dict(nlev_=0), shape),
        "negative nx": (dict(nx_=-1), shape),
        "negative ny": (dict(ny_=-3), shape),
        "negative nmem": (dict(nmem_=-1), shape),
        "unknown memkind": (dict(memkind=7), "unknown memkind 7"),
        "null fields": (dict(fields="null"), null),
        "null percentiles": (dict(ps=None), null),
        "null fres": (dict(out_ptrs="null"), null),
        "null member": (dict(fields=(ctypes.c_void_p * nmem)(*([x[0].data_ptr()] * (nmem - 1) + [None]))), "a null pointer (fields[4])"),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None, outs[2].data_ptr()]), "a null pointer (fres[1])"),
        "null flags out": (dict(fd_out=False), null),
        "more than 2^31 - 1 cells": (dict(nx_=46341, ny_=46341), "more than 2^31 - 1 cells per level"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[1].data_ptr(), outs[0].data_ptr()]), "two outputs are the same array or overlap"),
    }
    for what, (kw, text) in cases.items():
        rc, err, fd = call(**kw)
        assert rc == 0 and err == "mifc_ensembleQuantiles: " + text, (what, err)
        assert (outs == sentinel).all().item() and (fd == 7).all(), what
    with pytest.raises(RuntimeError, match="mifc_ensembleQuantiles"):
        gpu_ctx.ensembleQuantiles(x, [50], method="median")
    with pytest.raises(RuntimeError, match="outside"):
        gpu_ctx.ensembleQuantiles(x, [101], method="lower")
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, fd = call(sync=False)
    g.close()
    assert rc == 0 and "capture" in err and (outs == sentinel).all().item()
    # afterwards the same call runs
    rc, err, fd = call()
    assert rc == 1 and err == ""


def test_full_level_51_members(gpu_ctx):
    import torch

    nmem, ny, nx = 51, 720, 1440
    x = make_members(nmem, 1, ny, nx, 2024, specials=False)[:, 0]
    x[7, 100:140, 200:260] = qr.UNDEF
    d = torch.from_numpy(x).cuda()
    ps = [10, 25, 50, 75, 90]
    for method in ("lower", "linear"):
        out, fd = gpu_ctx.ensembleQuantiles(d, ps, method=method)
        exp, efd = qr.quantiles(x, ps, METHODS[method])
        assert same_bits(out.cpu().numpy(), exp, nan_payload=False) and fd == efd[0], method


def test_stacked_torch_levels_through_context(gpu_ctx):
    import torch

    nmem, nlev, ny, nx = 20, 4, 17, 23
    x = make_members(nmem, nlev, ny, nx, 4)
    flags = mixed_flags(nmem, nlev, 4)
    out, fd = gpu_ctx.ensembleQuantiles(torch.from_numpy(x).cuda(), [25, 75], fdefined_in=flags, method="linear")
    assert tuple(out.shape) == (2, nlev, ny, nx) and out.is_cuda and fd.dtype == np.int32 and fd.shape == (nlev,)
    exp, efd = qr.quantiles(x, [25, 75], qr.LINEAR, flags)
    assert same_bits(out.cpu().numpy(), exp, nan_payload=False) and list(fd) == efd
    # one flag per member stands for every level
    out, fd = gpu_ctx.ensembleQuantiles(torch.from_numpy(x).cuda(), [25, 75], fdefined_in=flags[:, 0], method="lower")
    exp, efd = qr.quantiles(x, [25, 75], qr.LOWER, np.repeat(flags[:, :1], nlev, axis=1))
    assert same_bits(out.cpu().numpy(), exp, nan_payload=False) and list(fd) == efd


@pytest.mark.parametrize("nmem", [3, 51, 80])
def test_extremes_equal_extremeValue(gpu_ctx, nmem):
    import torch

    x = make_members(nmem, 1, 19, 23, 60 + nmem, specials=False)[:, 0]
    x[x < -4] = -0.0  # signed zeros and infinities, nothing undefined
    x[x > 6] = np.inf
    x[0, 0, :5] = 0.0
    members = [torch.from_numpy(x[j].copy()).cuda() for j in range(nmem)]
    q, fd = gpu_ctx.ensembleQuantiles(members, [0, 100], method="lower")
    q = q.cpu().numpy()
    mx, _ = gpu_ctx.extremeValue(1, members)
    mn, _ = gpu_ctx.extremeValue(2, members)
    assert fd == qr.ALL_DEFINED
    assert np.array_equal(q[0], mn.cpu().numpy()) and np.array_equal(q[1], mx.cpu().numpy())  # as values: -0 == +0


@pytest.mark.parametrize("nmem", [4, 51, 66])
def test_flags_and_undefined_cells_equal_meanValue(gpu_ctx, nmem):
    x = make_members(nmem, 1, 15, 21, 90 + nmem)[:, 0]
    x[:, 3:6, 4:9] = qr.UNDEF  # cells without members
    # SOME / NONE_DEFINED members (an ALL_DEFINED member's stored undef would be a value here, and a sum there)
    for f in (np.where(np.arange(nmem) % 3 == 0, qr.NONE_DEFINED, qr.SOME_DEFINED).astype(np.int32), np.full(nmem, qr.SOME_DEFINED, np.int32)):
        mean, mfd = gpu_ctx.meanValue([x[j] for j in range(nmem)], [int(v) for v in f])
        for method in ("lower", "linear"):
            q, fd = gpu_ctx.ensembleQuantiles(x, [0, 50, 100], fdefined_in=f, method=method)
            assert fd == mfd, method
            for k in range(3):
                assert np.array_equal(q[k] == qr.UNDEF, mean == qr.UNDEF), (method, k)
    x[:, 3:6, 4:9] = 1.0  # only the sprinkled undefined values left
    mean, mfd = gpu_ctx.meanValue([x[j] for j in range(nmem)], [qr.SOME_DEFINED] * nmem)
    q, fd = gpu_ctx.ensembleQuantiles(x, [50], method="lower")
    assert fd == mfd and np.array_equal(q[0] == qr.UNDEF, mean == qr.UNDEF)
