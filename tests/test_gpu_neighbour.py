"""Neighbourhood statistics on the GPU (mifc_neighbour.hip): bit-identical to the numpy restatement
(tests/neighbour_restate.py) and, where oracle/_ref was built, to the compiled reference through
tests/neighbour_ref_shim.cc."""
import os
import subprocess

import numpy as np
import pytest

import neighbour_cases as nc
import neighbour_restate as nr
from test_neighbour_cpu import GT_UNDEF, gtest_expectations, gtest_runs, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return nc.RefShim(tmp_path_factory.mktemp("nbshim")) if nc.ref_available() else None


def gpu_call(ctx, which, field, consts, compute, out, fdefined=nr.ALL_DEFINED, undef=nc.UNDEF, device=False):
    """-> (status, flag, result as numpy); status as in neighbour_restate."""
    import torch

    fn = ctx.neighbourProbFunctions if which == "prob" else ctx.neighbourFunctions
    f, o = field, out
    if device:
        f = torch.from_numpy(np.ascontiguousarray(field)).cuda()
        o = f if out is field else torch.from_numpy(out.copy()).cuda()
    try:
        res = fn(f, consts, compute, fdefined=fdefined, undef=undef, out=o)
    except RuntimeError as e:
        assert ctx.last_error() and str(e).strip(), "a refusal names its reason"
        status, flag = "refused", fdefined
    else:
        status, flag = ("false", fdefined) if res is None else ("ok", res[1])
    got = o.cpu().numpy() if device else o
    return status, flag, got


def check(ctx, shim, which, field, consts, compute, device, label):
    ny, nx = field.shape
    exp = np.full((ny, nx), nc.SENTINEL, np.float32)
    status, flag = nr.run(which, nx, ny, field, consts, compute, exp, nr.ALL_DEFINED, nc.UNDEF)
    out = np.full((ny, nx), nc.SENTINEL, np.float32)
    gstatus, gflag, got = gpu_call(ctx, which, field, consts, compute, out, device=device)
    pct = which == "functions" and compute == 4
    assert (gstatus, gflag) == (status, flag), label
    assert same(got, exp, percentile=pct), label
    if shim is not None and status != "refused" and nx * ny <= (1 << 22):
        theirs = np.full((ny, nx), nc.SENTINEL, np.float32)
        ok, rflag = shim.run(which, nx, ny, field, consts, compute, theirs, nr.ALL_DEFINED)
        assert ok == (status == "ok") and rflag == flag, label
        assert same(got, theirs, percentile=pct), label


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nx,ny", [(23, 17), (9, 12)])
def test_sweep_bit_identical(gpu_ctx, shim, nx, ny, device):
    for k, (which, compute, consts, specials) in enumerate(nc.sweep(nx, ny)):
        field = nc.make_field(nx, ny, 1000 + k, specials)
        check(gpu_ctx, shim, which, field, consts, compute, device, (which, compute, consts, nx, ny, device))


# (which, compute, constants): ranges 1, 3, 10, 40 on ragged and full-size fields; r = 40 with step 3 needs a
# 71 KiB tile, past the 64 KiB LDS limit, so that walk reads its windows from global memory
BIG = [
    ("prob", 5, [0, 1]), ("prob", 6, [1, 3]), ("prob", 5, [-1, 10]), ("prob", 6, [0, 40]),
    ("functions", 1, [1, 1]), ("functions", 2, [3, 3]), ("functions", 3, [3, 1]), ("functions", 1, [10, 3]),
    ("functions", 5, [0, 3, 1]), ("functions", 6, [1, 10, 5]), ("functions", 4, [50, 1, 1]), ("functions", 4, [90, 3, 3]),
    ("functions", 4, [25, 10, 3]), ("functions", 2, [40, 3]), ("functions", 1, [40, 9]),
]


@pytest.mark.parametrize("nx,ny", [(949, 203), (1441, 150), (1440, 720)])
def test_ragged_and_full_size_windows(gpu_ctx, shim, nx, ny):
    for k, (which, compute, consts) in enumerate(BIG):
        r = consts[0] if (which == "functions" and compute < 4) else consts[1]
        if nx * ny > 500000 and which == "functions" and (compute == 4 or r >= 10) and not (compute == 1 and r == 10):
            continue  # the restatement's cost, not the GPU's: these windows are covered on the two smaller fields
        field = nc.make_field(nx, ny, 77 + k, specials=(True if compute != 4 else "zeros"))
        check(gpu_ctx, shim, which, field, consts, compute, device=(k % 2 == 0), label=(which, compute, consts, nx, ny))


def test_levels_batch_51_members(gpu_ctx):
    import torch

    nlev, ny, nx = 51, 720, 1440
    field = nc.make_field(nx, ny, 5151, nlev=nlev)
    d = torch.from_numpy(field).cuda()
    for which, compute, consts, levels in (("prob", 5, [1, 3], (0, 25, 50)), ("functions", 1, [1, 1], (0, 50)), ("functions", 3, [2, 3], (17,))):
        res = gpu_ctx.neighbour_levels(which, compute, d, consts, fdefined=[nr.ALL_DEFINED] * nlev)
        assert res is not None
        out, flags = res
        assert list(flags) == [nr.SOME_DEFINED] * nlev
        got = out.cpu().numpy()
        for l in levels:
            exp = np.full((ny, nx), nc.UNDEF, np.float32)  # out=None: pre-filled with undef
            assert nr.run(which, nx, ny, field[l], consts, compute, exp, nr.ALL_DEFINED, nc.UNDEF)[0] == "ok"
            assert same(got[l], exp), (which, compute, l)
    # host memory, and a batch with one level not ALL_DEFINED: 0 and nothing written
    small = field[:3, :100, :130].copy()
    out = np.full(small.shape, nc.SENTINEL, np.float32)
    res = gpu_ctx.neighbour_levels("prob", 6, small, [0, 2], fdefined=[0, 0, 0], out=out)
    assert res is not None and list(res[1]) == [nr.SOME_DEFINED] * 3
    for l in range(3):
        exp = np.empty((100, 130), np.float32)
        nr.run("prob", 130, 100, small[l], [0, 2], 6, exp, nr.ALL_DEFINED, nc.UNDEF)
        assert same(out[l], exp)
    out2 = np.full(small.shape, nc.SENTINEL, np.float32)
    assert gpu_ctx.neighbour_levels("prob", 6, small, [0, 2], fdefined=[0, 2, 0], out=out2) is None
    assert (out2 == nc.SENTINEL).all()


def test_gtest_neighbour_known_answers_on_the_gpu(gpu_ctx):
    def run(which, field, consts, compute, out, flag):
        status, f, got = gpu_call(gpu_ctx, which, field.reshape(10, 10), consts, compute, out.reshape(10, 10), flag, GT_UNDEF)
        return status == "ok", f, got.ravel()

    gtest_expectations(gtest_runs(run))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_deviations_are_refused_and_write_nothing(gpu_ctx, device):
    nx, ny = 12, 10
    field = nc.make_field(nx, ny, 3)
    for which, consts, compute in nc.DEVIATIONS:
        out = np.full((ny, nx), nc.SENTINEL, np.float32)
        if consts == "alias":
            f = field.copy()
            status, flag, got = gpu_call(gpu_ctx, which, f, [1, 1], compute, f, device=device)
            assert status == "refused" and same(got, field), (which, consts)
            continue
        status, flag, got = gpu_call(gpu_ctx, which, field, consts, compute, out, device=device)
        assert (status, flag) == ("refused", nr.ALL_DEFINED), (which, consts, compute)
        assert (got == nc.SENTINEL).all(), (which, consts, compute)


def test_beyond_2_pow_24_cells_exact_count(gpu_ctx):
    import torch

    nx = ny = 4400
    rng = np.random.default_rng(24)
    field = (rng.random((ny, nx)) < 0.95).astype(np.float32)
    exp = np.empty((ny, nx), np.float32)
    assert nr.run("prob", nx, ny, field, [0, 2], 5, exp, nr.ALL_DEFINED, nc.UNDEF)[0] == "ok"
    out, flag = gpu_ctx.neighbourProbFunctions(torch.from_numpy(field).cuda(), [0, 2], 5)
    assert flag == nr.SOME_DEFINED and same(out.cpu().numpy(), exp)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_prob_in_place(gpu_ctx, device):
    import torch

    nx, ny = 301, 157
    field = nc.make_field(nx, ny, 11, specials=True)
    for consts, compute in (([0, 3], 5), ([1, 0], 6)):
        exp = field.copy()
        assert nr.run("prob", nx, ny, exp, consts, compute, exp, nr.ALL_DEFINED, nc.UNDEF)[0] == "ok"
        f = field.copy()
        if device:
            f = torch.from_numpy(f).cuda()
        res = gpu_ctx.neighbourProbFunctions(f, consts, compute, out=f)
        assert res is not None
        got = f.cpu().numpy() if device else f
        assert same(got, exp), consts


CXX_CALLER = r"""
#include <mi_fieldcalc/FieldCalculations.h>
#include <cstdio>
#include <string>
#include <vector>
int main()
{
  using namespace miutil;
  const int nx = 10, ny = 10;
  std::vector<float> in(nx * ny, 0.f), out(nx * ny, 61728.f);
  in[25] = in[26] = in[35] = in[36] = 6.f;
  std::vector<float> c;
  c.push_back(5.f);
  c.push_back(2.f);
  ValuesDefined f = ALL_DEFINED;
  const bool ok = fieldcalc::neighbourProbFunctions(nx, ny, in.data(), c, 5, out.data(), f, 123456.f);
  const std::string why = fieldcalc::last_error();
  std::printf("%d %d|%s\n", ok, (int)f, why.c_str());
  for (int k = 0; k < nx * ny; ++k)
    std::printf("%.9g\n", (double)out[k]);
  return 0;
}
"""


def test_cxx_caller_neighbourProbFunctions(gpu_ctx, tmp_path):
    """An unchanged C++ caller of miutil::fieldcalc::neighbourProbFunctions through libmi-fieldcalc.so."""
    src = tmp_path / "nbcaller.cc"
    src.write_text(CXX_CALLER)
    exe = tmp_path / "nbcaller"
    inc = os.path.join(ROOT, "mi-fieldcalc_amd", "include")
    libdir = os.path.join(ROOT, "mi-fieldcalc_amd")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lmi-fieldcalc", "-lmifc",
                    "-Wl,-rpath," + libdir], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=120).stdout.splitlines()
    head, why = lines[0].split("|", 1)
    assert head == "1 %d" % nr.SOME_DEFINED and why == "", lines[0]
    got = np.array([np.float32(float(x)) for x in lines[1:]], np.float32)
    field = np.zeros(100, np.float32)
    field[[25, 26, 35, 36]] = 6
    exp = np.empty(100, np.float32)
    nr.run("prob", 10, 10, field, [5, 2], 5, exp, nr.ALL_DEFINED, GT_UNDEF)
    assert same(got, exp)
