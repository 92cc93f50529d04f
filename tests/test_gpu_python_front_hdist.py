"""The Python front of mifc_hdist_* (mi_fieldcalc_amd.hdist) on the GPU: host arrays against device tensors, where the
results live and what they are, `out=`, one batch against stacked batches and lists, and the library's refusals as
Refused -- every result equal to the numpy restatement (tests/hdist_restate.py), counts as integers and percentiles by
bits."""
import numpy as np
import pytest

import hdist_restate as hd
from gpu_util import run_is_forced
from mi_fieldcalc_amd import hdist  # (without the feature the file fails here)

pytestmark = pytest.mark.gpu

A, S, N = hd.ALL_DEFINED, hd.SOME_DEFINED, hd.NONE_DEFINED
U = hd.UNDEF
EDGES = np.array([270.0, 276.0, 280.0, 283.5, 290.0], np.float32)
PS = [2.0, 50.0, 98.0]


def case(nf=3, nlev=4, ny=7, nx=36, seed=3):
    rng = np.random.default_rng(seed)
    f = np.stack([np.stack([hd.smooth_level(ny, nx, seed + 10 * g + k, 280.0 - 2 * k, 9.0) for k in range(nlev)]) for g in range(nf)])
    f = hd.sprinkle(f, rng, 0.05, U)
    f[1, 2] = U  # a level without a defined cell
    mask = hd.sprinkle(np.ones((ny, nx), np.float32), rng, 0.2, U)
    return f, mask


def form(ctx, **expected_keys):
    got = hdist.last_hdist_form(ctx)
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


def test_histogram_host_arrays_and_device_tensors(gpu_ctx):
    import torch

    f, mask = case()
    box = (1, 35, 1, 6)
    for mode in ("area", "rows"):
        exp = hd.histogram(f, EDGES, mask, S, box, mode)
        host = hdist.histogram_levels(gpu_ctx, f, EDGES, mask=mask, box=box, mode=mode)
        assert isinstance(host, np.ndarray) and host.dtype == np.int32 and (host == exp).all()
        form(gpu_ctx, entry="hist", mode=mode, nf=3, nbins=6, mask=1, tested=1)
        dev = hdist.histogram_levels(gpu_ctx, torch.from_numpy(f).cuda(), EDGES, mask=torch.from_numpy(mask).cuda(), box=box, mode=mode)
        assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.int32 and (dev.cpu().numpy() == exp).all()
        listed = hdist.histogram_levels(gpu_ctx, [torch.from_numpy(f[g]).cuda() for g in range(3)], [EDGES, EDGES + 1, EDGES - 2], mode=mode)
        assert (listed.cpu().numpy() == hd.histogram(f, np.stack([EDGES, EDGES + 1, EDGES - 2]), mode=mode)).all()
    one = hdist.histogram_levels(gpu_ctx, f[0], list(EDGES), fdefined_in=A, mode=hd.ROWS)  # one batch: no leading axis; one flag for all levels
    assert one.shape == (4, 7, 7) and (one == hd.histogram(f[:1], EDGES, mode=hd.ROWS, flags=[[A] * 4])[0]).all()
    form(gpu_ctx, nf=1, tested=0)
    assert one.sum() == 4 * 7 * 36  # nothing is tested: every cell is counted


def test_quantiles_host_arrays_and_device_tensors(gpu_ctx):
    import torch

    f, mask = case()
    for method in ("lower", "linear"):
        eq, efd = hd.quantiles(f, PS, method, mask)
        q, fd = hdist.quantile_levels(gpu_ctx, f, PS, method, mask=mask)
        assert isinstance(q, np.ndarray) and q.dtype == np.float32 and hd.same(q, eq) and isinstance(fd, np.ndarray) and np.array_equal(fd, efd)
        form(gpu_ctx, entry="quant", mode=method, nf=3, mask=1, tested=1, chunks=1)
        dq, dfd = hdist.quantile_levels(gpu_ctx, torch.from_numpy(f).cuda(), PS, method, mask=torch.from_numpy(mask).cuda())
        assert torch.is_tensor(dq) and dq.is_cuda and hd.same(dq.cpu().numpy(), eq) and isinstance(dfd, np.ndarray) and np.array_equal(dfd, efd)
        assert efd[1, 2] == N and (eq[1, 2] == U).all() and (efd == A).sum() == 11
    # quant[f] is a level batch (nlev, 1, nq): the next call takes it as it is
    batch = dq[0].view(4, 1, 3)
    again, _ = hdist.quantile_levels(gpu_ctx, batch, [0.0, 100.0], "lower")
    assert hd.same(again.cpu().numpy(), eq[0][:, [0, 2]])
    # one batch; out= is written and handed back
    pool = torch.full((3, 4, 3), -4242.5, dtype=torch.float32, device="cuda")
    got, fd = hdist.quantile_levels(gpu_ctx, torch.from_numpy(f[2]).cuda(), PS, out=pool[1])
    assert got.data_ptr() == pool[1].data_ptr() and fd.shape == (4,)
    back = pool.cpu().numpy()
    assert hd.same(back[1], hd.quantiles(f[2:], PS)[0][0]) and (back[0] == -4242.5).all() and (back[2] == -4242.5).all()
    hpool = np.full((2, 4, 3), -4242.5, np.float32)
    got, _ = hdist.quantile_levels(gpu_ctx, f[2], PS, out=hpool[0])
    assert np.shares_memory(got, hpool) and hd.same(hpool[0], back[1]) and (hpool[1] == -4242.5).all()


def test_refusals_are_refused_with_the_reason(gpu_ctx):
    import torch

    f, mask = case()
    with pytest.raises(hdist.Refused, match="field 0: edge 2 is NaN or not above the edge before it"):
        hdist.histogram_levels(gpu_ctx, f, [1.0, 2.0, 2.0])
    with pytest.raises(hdist.Refused, match="unknown mode"):
        hdist.histogram_levels(gpu_ctx, f, EDGES, mode="columns")
    with pytest.raises(hdist.Refused, match="the box"):
        hdist.histogram_levels(gpu_ctx, f, EDGES, box=(0, 37, 0, 7))
    with pytest.raises(hdist.Refused, match="unknown method"):
        hdist.quantile_levels(gpu_ctx, f, PS, method="nearest")
    with pytest.raises(hdist.Refused, match="percentile 1 is NaN or outside"):
        hdist.quantile_levels(gpu_ctx, f, [50, 100.5])
    with pytest.raises(RuntimeError, match="nfields 9 outside 1..8"):  # Refused is a RuntimeError too
        hdist.quantile_levels(gpu_ctx, [f[0]] * 9, PS)
    with pytest.raises(ValueError):  # host fields with a device mask
        hdist.histogram_levels(gpu_ctx, f, EDGES, mask=torch.from_numpy(mask).cuda())
    q, fd = hdist.quantile_levels(gpu_ctx, f, PS, mask=mask)  # afterwards the calls run
    assert hd.same(q, hd.quantiles(f, PS, hd.LINEAR, mask)[0])
