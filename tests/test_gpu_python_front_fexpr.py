"""GPU tests of the Python front of mifc_fexpr_levels (mi_fieldcalc_amd.fexpr): numpy arrays and CUDA tensors give the same
bits through evaluate, an expression and its compiled program are the same call, out= is honoured, and a refused call
raises Refused with the library's reason."""
import numpy as np
import pytest

import fexpr_restate as fr
from cases import same_bits
from mi_fieldcalc_amd import fexpr

pytestmark = pytest.mark.gpu


def _inputs(shape=(3, 7, 22)):
    rng = np.random.default_rng(77)
    t, q = fr.fuzz_field(rng, shape), fr.fuzz_field(rng, shape)
    w = fr.fuzz_field(rng, shape[1:])
    p = np.array([1000.0, 850.0, fr.UNDEF], np.float32)
    return t, q, w, p


def test_numpy_and_tensors_give_the_same_bits(gpu_ctx):
    import torch

    t, q, w, p = _inputs()
    expr = "where(t > q, t, q) * w, ifdef(t * (1000 / p) ** 0.2857, -1)"
    prog = fexpr.compile(expr, fields=("t", "q"), planes=("w",), level_scalars=("p",))
    host, hfd = fexpr.evaluate(gpu_ctx, prog, [t, q], [w], [p])
    assert isinstance(host, np.ndarray) and host.shape == (2,) + t.shape and hfd.shape == (2, 3) and hfd.dtype == np.int32
    dt, dq, dw = (torch.from_numpy(x).cuda() for x in (t, q, w))
    device, dfd = fexpr.evaluate(gpu_ctx, prog, [dt, dq], [dw], [p])
    assert torch.is_tensor(device) and device.is_cuda and same_bits(device.cpu().numpy(), host) and np.array_equal(dfd, hfd)
    # the expression itself, by name
    named, nfd = fexpr.evaluate(gpu_ctx, expr, {"t": dt, "q": dq}, planes={"w": dw}, level_scalars={"p": p})
    assert same_bits(named.cpu().numpy(), host) and np.array_equal(nfd, hfd)
    # a stacked batch of fields
    stacked, sfd = fexpr.evaluate(gpu_ctx, prog, torch.stack([dt, dq]), [dw], [p])
    assert same_bits(stacked.cpu().numpy(), host) and np.array_equal(sfd, hfd)
    # the first output against the restatement, bit for bit; the level whose scalar is undefined is -1 in the second
    want, wfd = fr.interpret(prog.code[:, :5], prog.consts, prog.out_regs, [t, q], [w], [p])
    assert same_bits(host[0], want[0], nan_payload=False) and np.array_equal(hfd, wfd) and (host[1, 2] == -1).all()


def test_out_is_honoured_and_one_output_drops_the_axis(gpu_ctx):
    import torch

    t, q, w, p = _inputs()
    prog = fexpr.compile("t - q", fields=("t", "q"))
    res = np.full(t.shape, -7.0, np.float32)
    out, fd = fexpr.evaluate(gpu_ctx, prog, [t, q], out=res)
    assert out is res and fd.shape == (3,) and not (res == -7.0).all()
    dres = torch.full((2,) + t.shape, -7.0, dtype=torch.float32, device="cuda")
    out, fd = fexpr.evaluate(gpu_ctx, prog, [torch.from_numpy(t).cuda(), torch.from_numpy(q).cuda()], out=dres[1])
    assert out.data_ptr() == dres[1].data_ptr() and (dres[0] == -7.0).all().item() and same_bits(dres[1].cpu().numpy(), res)
    with pytest.raises(ValueError, match="out must have shape"):
        fexpr.evaluate(gpu_ctx, prog, [t, q], out=res[:2])
    with pytest.raises(ValueError, match="numpy \\(host\\) or CUDA tensors"):
        fexpr.evaluate(gpu_ctx, prog, [t, torch.from_numpy(q).cuda()])


def test_a_refused_call_raises_refused(gpu_ctx):
    t, q, w, p = _inputs()
    with pytest.raises(fexpr.Refused, match="mifc_fexpr_levels: instruction 0: register 9 is read before anything set it"):
        fexpr.evaluate(gpu_ctx, fexpr.Program.from_code([("add", 3, 0, 9)], out_regs=[3]), t)
    before = t.copy()
    with pytest.raises(fexpr.Refused, match="fres\\[0\\] overlaps fields\\[0\\]"):
        fexpr.evaluate(gpu_ctx, fexpr.compile("t + 1", fields=("t",)), t, out=t)
    assert same_bits(t, before)
    form = fexpr.last_fexpr_form(gpu_ctx)
    assert form == {} or form["family"] == "fexpr"
