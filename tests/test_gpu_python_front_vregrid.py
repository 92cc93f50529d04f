"""mi_fieldcalc_amd.vregrid on the GPU: host arrays against device tensors bit for bit, hybrid_to_hybrid against the
restatement on a target batch built in numpy, and the identity regrid."""
import numpy as np
import pytest

import vinterp_restate as vi
import vregrid_cases as vc
import vregrid_restate as vg
from cases import same_bits
from test_gpu_vregrid import compare

pytestmark = pytest.mark.gpu

U = vg.UNDEF


def front():
    from mi_fieldcalc_amd import vregrid

    return vregrid


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("nx", [13, 16])
def test_host_arrays_and_device_tensors_agree_bit_for_bit(gpu_ctx, nx):
    hyb, fld, lev = (vc.main(kind, 3, 12, 9, nx) for kind in ("hybrid", "field", "levels"))
    for method, from_, outside in (("linear", "first", "undef"), ("log", "last", "clamp")):
        kw = dict(method=method, from_=from_, outside=outside)
        calls = (
            lambda put, seq: front().vregrid_hlevels(gpu_ctx, seq(put(hyb["fields"])), put(hyb["coord"]), hyb["ab"][0], hyb["ab"][1], put(hyb["tcoord"]), **kw),
            lambda put, seq: front().vregrid_fields(gpu_ctx, seq(put(fld["fields"])), put(fld["coord"]), seq(put(fld["tcoord"])), **kw),
            lambda put, seq: front().vregrid_levels(gpu_ctx, put(lev["fields"]), lev["coord"], put(lev["tcoord"]), **kw),
        )
        for call in calls:
            h, hfd = call(np.ascontiguousarray, lambda a: a)
            d, dfd = call(dev, lambda a: [a[j] for j in range(a.shape[0])])  # the device call takes lists of batches and planes
            assert isinstance(h, np.ndarray) and d.is_cuda and h.shape == tuple(d.shape) == (3, 5, 9, nx)
            assert same_bits(h, d.cpu().numpy(), nan_payload=False) and np.array_equal(hfd, dfd)
            assert (h != U).mean() > 0.3
    out = dev(np.zeros((3, 5, 9, nx), np.float32))
    res, _ = front().vregrid_fields(gpu_ctx, dev(fld["fields"]), dev(fld["coord"]), dev(fld["tcoord"]), out=out)
    assert res is out


def other_model(nlev_dst=9):
    """The levels of another model over another orography: ps_dst = ps +- 60 hPa, undefined in places of its own."""
    case = vc.main("hybrid", 4, 12, 9, 16)
    rng = np.random.default_rng(31)
    ps = case["coord"]
    ps_dst = np.where(ps == U, np.float32(950), ps + rng.uniform(-60, 60, ps.shape).astype(np.float32)).astype(np.float32)
    ps_dst = vi.sprinkle(ps_dst, rng, 0.04, U)
    eta = np.linspace(0.05, 1, nlev_dst) ** 1.3
    return case, ps_dst, (1000 * (eta - eta ** 2)).astype(np.float32), (eta ** 2).astype(np.float32)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_hybrid_to_hybrid_against_the_restatement(gpu_ctx, device):
    case, ps_dst, a_dst, b_dst = other_model()
    put = dev if device else np.ascontiguousarray
    tcoord = vg.hybrid_targets(ps_dst, a_dst, b_dst)  # a + b * ps_dst like p_hlevel, undef where ps_dst is
    assert (tcoord[:, ps_dst == U] == U).all() and (tcoord[-1][ps_dst != U] == ps_dst[ps_dst != U]).all()
    for method, outside in (("log", "clamp"), ("linear", "undef")):
        out, fd = front().hybrid_to_hybrid(gpu_ctx, put(case["fields"]), put(case["coord"]), case["ab"][0], case["ab"][1], a_dst, b_dst, put(ps_dst),
                                           method=method, outside=outside)
        exp, efd = vg.hlevels(case["fields"], case["coord"], case["ab"][0], case["ab"][1], tcoord, vc.METHODS[method], vg.FROM_FIRST, vc.OUTSIDE[outside])
        compare(out.cpu().numpy() if device else out, exp, fd, efd, method, U, ("hybrid_to_hybrid", method, outside))
    plain, _ = vg.hlevels(case["fields"], case["coord"], case["ab"][0], case["ab"][1], tcoord, vg.LOG, vg.FROM_FIRST, vg.OUTSIDE_UNDEF)
    exp, _ = vg.hlevels(case["fields"], case["coord"], case["ab"][0], case["ab"][1], tcoord, vg.LOG, vg.FROM_FIRST, vg.OUTSIDE_CLAMP)
    assert ((plain == U) & (exp != U)).mean() > 0.01  # where the new orography is lower, the lowest level's values


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_identity_regrid(gpu_ctx, device):
    """The same levels over the same ps, LINEAR.  Level t's target is the coordinate of level t itself, so FROM_FIRST finds
    the pair (t - 1, t) with weight exactly 1 -- (ct - c_k) / (c_k+1 - c_k) with ct == c_k+1 -- and rule 6 of mifc_vinterp_*
    gives x_k + 1 * (x_k+1 - x_k): the difference and the sum are each rounded, in double, and then to float, so the result
    is x_k+1 or a neighbouring float, not necessarily its bits.  Level 0 has no pair above it: the pair (0, 1), weight 0,
    x_0 + 0 * (...) = x_0 bit for bit."""
    case = vc.main("hybrid", 3, 12, 9, 16)
    put = dev if device else np.ascontiguousarray
    fields, ps = case["fields"], case["coord"]
    out, fd = front().hybrid_to_hybrid(gpu_ctx, put(fields), put(ps), case["ab"][0], case["ab"][1], case["ab"][0], case["ab"][1], None, method="linear",
                                       outside="undef")
    out = out.cpu().numpy() if device else out
    exp, efd = vg.hlevels(fields, ps, case["ab"][0], case["ab"][1], vg.hybrid_targets(ps, *case["ab"]), vg.LINEAR)
    compare(out, exp, fd, efd, "linear", U, "identity")
    ok = (ps != U)[None, None] & np.ones(out.shape, bool)
    ok[:, 0] &= (fields[:, 0] != U) & (fields[:, 1] != U)
    ok[:, 1:] &= (fields[:, 1:] != U) & (fields[:, :-1] != U)
    assert np.array_equal(out != U, ok)  # a result needs both ends of its pair
    assert same_bits(out[:, 0][ok[:, 0]], fields[:, 0][ok[:, 0]], nan_payload=False)
    steps = np.abs(out.view(np.int32)[ok].astype(np.int64) - fields.view(np.int32)[ok].astype(np.int64))
    assert steps.max() <= 1
