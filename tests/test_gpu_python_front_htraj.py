"""The Python front of mifc_htraj_levels (mi_fieldcalc_amd.htraj) on the GPU: host arrays against device tensors, where
the results live and what they are, slices counted from the end, flags given as one value, and the library's refusals as
Refused -- every result equal to the restatement (tests/htraj_restate.py) by bits."""
import numpy as np
import pytest

import htraj_cases as hc
import htraj_restate as ht
from gpu_util import run_is_forced
from mi_fieldcalc_amd import htraj  # (without the feature the file fails here)

pytestmark = pytest.mark.gpu

A, S, N = ht.ALL_DEFINED, ht.SOME_DEFINED, ht.NONE_DEFINED
U = ht.UNDEF


def case():
    c = hc.small(31, nx=11, ny=7, nt=4, nlev=3, npos=300, ntrace=2, holes=0.02)
    return c, ht.run(**c)


def test_results_live_where_the_fields_live(gpu_ctx):
    import torch

    c, (ex, ey, et, efl) = case()
    nt = 4
    host = htraj.trajectories(gpu_ctx, list(c["u"]), list(c["v"]), c["times"], c["xmapr"], c["ymapr"], c["xpos"], c["ypos"], nsub=2, niter=2,
                              trace=[list(c["trace"][0]), list(c["trace"][1])])
    assert sorted(host) == ["flags", "trace", "x", "y"] and isinstance(host["x"], np.ndarray) and host["x"].dtype == np.float32
    assert ht.same(host["x"], ex) and ht.same(host["y"], ey) and ht.same(np.stack(host["trace"]), et) and np.array_equal(host["flags"], efl)
    assert host["flags"].dtype == np.int32 and host["flags"].shape == (3, 4, 3)
    got = htraj.last_htraj_form(gpu_ctx)
    if not run_is_forced():
        assert got == dict(niter=2, nsub=2, ntrace=2, tested=1, blocks=2, level_chunks=3, chunk=1, intervals=3, launches=3, staged=1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    u, v = [dev(c["u"][j]) for j in range(nt)], [dev(c["v"][j]) for j in range(nt)]
    tr = [[dev(c["trace"][f, j]) for j in range(nt)] for f in range(2)]
    res = htraj.trajectories(gpu_ctx, u, v, c["times"], dev(c["xmapr"]), dev(c["ymapr"]), dev(c["xpos"]), dev(c["ypos"]), nsub=2, niter=2, trace=tr)
    assert torch.is_tensor(res["x"]) and res["x"].is_cuda and all(t.is_cuda for t in res["trace"]) and isinstance(res["flags"], np.ndarray)
    assert ht.same(res["x"].cpu().numpy(), ex) and ht.same(res["y"].cpu().numpy(), ey) and np.array_equal(res["flags"], efl)
    assert ht.same(np.stack([t.cpu().numpy() for t in res["trace"]]), et)
    if not run_is_forced():
        assert htraj.last_htraj_form(gpu_ctx)["staged"] == 0
    # slices counted from the end; a backward run; one flag for everything
    back = htraj.trajectories(gpu_ctx, u, v, c["times"], dev(c["xmapr"]), dev(c["ymapr"]), dev(c["xpos"]), dev(c["ypos"]), start=-1, end=1, nsub=2, niter=2,
                              fdefined_in=A, fdef_map=A)
    bx, by, _, bfl = ht.run(**dict(c, j_start=3, j_end=1, trace=None, fdefined_in=np.full((2, 4, 3), A), fdef_map=A))
    assert back["trace"] == [] and ht.same(back["x"].cpu().numpy(), bx) and ht.same(back["y"].cpu().numpy(), by) and np.array_equal(back["flags"], bfl)
    # a slot is a position list for the next call: the run continued from its last slot
    more = htraj.trajectories(gpu_ctx, u, v, c["times"], dev(c["xmapr"]), dev(c["ymapr"]), res["x"][1, 0], res["y"][1, 0], start=1, end=3, nsub=2, niter=2)
    assert ht.same(more["x"][:, 0].cpu().numpy(), ex[1:, 0]) and ht.same(more["y"][:, 0].cpu().numpy(), ey[1:, 0])


def test_refusals_are_refused_with_the_reason(gpu_ctx):
    import torch

    c, exp = case()
    good = (list(c["u"]), list(c["v"]), c["times"], c["xmapr"], c["ymapr"], c["xpos"], c["ypos"])
    with pytest.raises(htraj.Refused, match="nsub outside 1..64"):
        htraj.trajectories(gpu_ctx, *good, nsub=65)
    with pytest.raises(htraj.Refused, match="niter outside 0..8"):
        htraj.trajectories(gpu_ctx, *good, niter=9)
    with pytest.raises(htraj.Refused, match="j_start == j_end"):
        htraj.trajectories(gpu_ctx, *good, start=2, end=-2)
    with pytest.raises(htraj.Refused, match="j_start or j_end outside"):
        htraj.trajectories(gpu_ctx, *good, end=4)
    with pytest.raises(htraj.Refused, match="not strictly increasing"):
        htraj.trajectories(gpu_ctx, good[0], good[1], [0, 2, 1, 3], *good[3:])
    with pytest.raises(RuntimeError, match="undef is a position inside the grid"):  # Refused is a RuntimeError too
        htraj.trajectories(gpu_ctx, *good, undef=3.0)
    with pytest.raises(ValueError):  # host fields with device positions
        htraj.trajectories(gpu_ctx, *good[:5], torch.from_numpy(c["xpos"].copy()).cuda(), torch.from_numpy(c["ypos"].copy()).cuda())
    res = htraj.trajectories(gpu_ctx, *good, nsub=2, niter=2)  # afterwards the calls run
    assert ht.same(res["x"], exp[0]) and ht.same(res["y"], exp[1])
