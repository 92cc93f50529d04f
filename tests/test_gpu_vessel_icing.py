"""The iterative vessel-icing models on the GPU (mifc_icing.hip) against the compiled reference, through
tests/icing_ref_shim.cc: the accuracy contract, special inputs, refusals, batches, aliasing, the C++
symbols and the Python drop-in."""
import os
import subprocess

import numpy as np
import pytest

import icing_cases as ic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = [(ic.MODSTALL, 1), (ic.MINCOG, 1), (ic.MINCOG, 2), (ic.MINCOG, 0)]
MODEL_IDS = ["modstall", "mincog-org", "mincog-adj2", "mincog-adj0"]
FULL = (1440, 720)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not ic.ref_available():
        pytest.skip("oracle/_ref/libmifc_ref.so not built (needs the reference sources at build time)")
    return ic.RefShim(tmp_path_factory.mktemp("icref"))


@pytest.fixture(scope="module")
def full_grid(ref):
    """The 1440 x 720 inputs and each model's reference result, computed once per module (7-15 s per call on one
    core; here in row bands on 16 threads)."""
    fields = ic.make_inputs(*FULL, seed=1440, specials=True)
    cache = {}

    def get(model, alt):
        if (model, alt) not in cache:
            cache[(model, alt)] = ref.run_rows(model, fields, alt=alt, fdefined=ic.SOME_DEFINED, **ic.SCALARS)
        return cache[(model, alt)]

    return fields, get


def gpu_run(ctx, model, fields, alt=1, fdefined=ic.SOME_DEFINED, device=False, out=None, **scalars):
    """-> (result or None, flag, output as numpy)"""
    import torch

    s = dict(ic.SCALARS)
    s.update(scalars)
    args = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in fields] if device else list(fields)
    if out is not None and device:
        out = torch.from_numpy(out.copy()).cuda()
    if model == ic.MODSTALL:
        res = ctx.vesselIcingModStall(*args, s["vs"], s["alpha"], s["zmin"], s["zmax"], fdefined=fdefined, undef=ic.UNDEF, out=out)
    else:
        res = ctx.vesselIcingMincog(*args, s["vs"], s["alpha"], s["zmin"], s["zmax"], alt, fdefined=fdefined, undef=ic.UNDEF, out=out)
    if res is None:
        got = None if out is None else (out.cpu().numpy() if device else out)
        return None, fdefined, got
    o, flag = res
    return res, flag, (o.cpu().numpy() if device else o)


def assert_contract(got, gflag, theirs, rflag, label):
    assert gflag == rflag, label
    placed, frac, excess, ndef = ic.contract(got, theirs)
    assert placed, ("undefined cells differ", label)
    assert frac >= 0.999, ("bit-identical fraction %.5f" % frac, label)
    assert excess <= 0, ("beyond 1e-5 |ref| + 5e-5 cm/h by %g" % excess, label)
    return frac, ndef


@pytest.mark.parametrize("model,alt", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("flag", [ic.ALL_DEFINED, ic.SOME_DEFINED], ids=["all", "some"])
@pytest.mark.parametrize("nx,ny", [(1, 1), (129, 40), (484, 71)])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_accuracy_contract(gpu_ctx, ref, model, alt, flag, nx, ny, device):
    fields = ic.make_inputs(nx, ny, 7 * nx + ny + alt, specials=(nx > 1))
    if flag == ic.ALL_DEFINED:
        fields = [np.where(f == ic.UNDEF, np.float32(2.0), f) for f in fields]
    ok, rflag, theirs = ref.run(model, fields, alt=alt, fdefined=flag, **ic.SCALARS)
    res, gflag, got = gpu_run(gpu_ctx, model, fields, alt, flag, device)
    assert ok and res is not None
    assert_contract(got, gflag, theirs, rflag, (model, alt, flag, nx, ny, device))


@pytest.mark.parametrize("model,alt", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_accuracy_contract_full_grid(gpu_ctx, full_grid, model, alt, device):
    fields, get = full_grid
    _, rflag, theirs = get(model, alt)
    res, gflag, got = gpu_run(gpu_ctx, model, fields, alt, ic.SOME_DEFINED, device)
    assert res is not None
    frac, ndef = assert_contract(got, gflag, theirs, rflag, (model, alt, device))
    assert ndef > 700000
    print("\n%s alt %d: %.5f of %d defined cells bit-identical" % ("ModStall" if model == ic.MODSTALL else "MINCOG", alt, frac, ndef))


@pytest.mark.parametrize("model,alt", MODELS, ids=MODEL_IDS)
@pytest.mark.parametrize("zmin,zmax", [(0.0, 0.0), (0.0, 60.0), (1.5, 33.5)], ids=["one-level", "121-levels", "65-levels"])
def test_level_counts(gpu_ctx, ref, model, alt, zmin, zmax):
    """One level, 121 levels (past the 64 level factors that travel in the kernel arguments) and 65."""
    fields = ic.make_inputs(129, 40, 60, specials=True)
    ok, rflag, theirs = ref.run(model, fields, alt=alt, vs=5.0, alpha=0.7, zmin=zmin, zmax=zmax)
    res, gflag, got = gpu_run(gpu_ctx, model, fields, alt, zmin=zmin, zmax=zmax)
    assert ok and res is not None
    assert_contract(got, gflag, theirs, rflag, (model, alt, zmin, zmax))


@pytest.mark.parametrize("vs,alpha", [(0.0, 0.0), (12.0, 3.0), (3.0, 2.0), (5.0, 1.5707964)])
@pytest.mark.parametrize("model,alt", MODELS[:3], ids=MODEL_IDS[:3])
def test_scalars(gpu_ctx, ref, model, alt, vs, alpha):
    """Angles that take each of MINCOG's beta_r branches, a standing ship and a fast one."""
    fields = ic.make_inputs(129, 40, 61, specials=True)
    ok, rflag, theirs = ref.run(model, fields, alt=alt, vs=vs, alpha=alpha, zmin=0.0, zmax=10.0)
    res, gflag, got = gpu_run(gpu_ctx, model, fields, alt, vs=vs, alpha=alpha)
    assert ok and res is not None
    assert_contract(got, gflag, theirs, rflag, (model, alt, vs, alpha))


def test_special_inputs_are_hit(gpu_ctx, ref):
    """The edge cases of icing_cases.add_specials land where the reference puts them: exact zeros for calm wind and
    flat sea, undef for aice exactly 0.4 and below the freezing threshold, a value (not undef) where only Pw is
    undefined, NaN, or 0, and the non-converging shallow-water loop (negative depth)."""
    fields = ic.make_inputs(484, 71, 99, specials=True)
    names = dict(zip(ic.NAMES, fields))
    for model in (ic.MODSTALL, ic.MINCOG):
        ok, rflag, theirs = ref.run(model, fields, **ic.SCALARS)
        _, gflag, got = gpu_run(gpu_ctx, model, fields)
        assert_contract(got, gflag, theirs, rflag, model)
        assert (got[names["aice"] == np.float32(0.4)] == ic.UNDEF).all()
        others_ok = np.ones(got.shape, bool)
        for k, f in enumerate(fields):
            if ic.NAMES[k] != "Pw":
                others_ok &= (f != ic.UNDEF) & ~np.isnan(f)
        pw_bad = others_ok & (names["aice"] < 0.4) & ((names["Pw"] == ic.UNDEF) | np.isnan(names["Pw"]) | (names["Pw"] == 0))
        assert pw_bad.sum() > 100 and (got[pw_bad] != ic.UNDEF).any()
        assert (got[others_ok & (names["depth"] < 0) & (names["aice"] < 0.4)] != ic.UNDEF).any()
        if model == ic.MINCOG:
            calm = others_ok & (names["wave"] == np.float32(0.05)) & (got != ic.UNDEF)
            assert calm.any() and (got[calm] == 0).all()


@pytest.mark.parametrize("model", [ic.MODSTALL, ic.MINCOG])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_write_nothing(gpu_ctx, ref, model, device):
    fields = ic.make_inputs(31, 9, 5)
    for vs, alpha, zmin, zmax in [(-1, 0.7, 0, 10), (5, -0.1, 0, 10), (5, 0.7, -1, 10), (5, 0.7, 3, 2), (5, 0.7, 0, 10.5),
                                  (5, 0.7, float("nan"), 10), (5, 0.7, 0, float("inf"))]:
        sentinel = np.full((9, 31), ic.SENTINEL, np.float32)
        ok, _, _ = ref.run(model, fields, vs, alpha, zmin, zmax)
        assert not ok
        res, _, got = gpu_run(gpu_ctx, model, fields, 1, device=device, out=sentinel, vs=vs, alpha=alpha, zmin=zmin, zmax=zmax)
        assert res is None and (got == ic.SENTINEL).all() and gpu_ctx.last_error() == ""
    sentinel = np.full((9, 31), ic.SENTINEL, np.float32)
    with pytest.raises(RuntimeError, match="do not fit an int"):
        gpu_run(gpu_ctx, model, fields, 1, device=device, out=sentinel, zmin=0.0, zmax=2.0e9)
    assert (sentinel == ic.SENTINEL).all()


@pytest.mark.parametrize("model,alt", [(ic.MODSTALL, 1), (ic.MINCOG, 2)], ids=["modstall", "mincog-adj"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_batch_of_51_members_with_shared_depth(gpu_ctx, model, alt, device):
    import torch

    nlev, nx, ny = 51, 97, 33
    fields = ic.make_inputs(nx, ny, 51, nlev=nlev, specials=True)
    fields[10] = fields[10][0].copy()  # one bathymetry for every member
    flags = np.array([ic.ALL_DEFINED if l % 3 == 0 else ic.SOME_DEFINED for l in range(nlev)], np.int32)
    for l in range(nlev):
        if flags[l] == ic.ALL_DEFINED:
            for f in fields[:10]:
                f[l][f[l] == ic.UNDEF] = np.float32(2.0)
    fields[0][7] = ic.UNDEF  # a member with nothing defined
    flags[7] = ic.SOME_DEFINED
    args = [torch.from_numpy(f).cuda() for f in fields] if device else fields
    name = "modstall" if model == ic.MODSTALL else "mincog"
    out, fl = gpu_ctx.vesselIcing_levels(name, args, alt=alt, fdefined=flags, undef=ic.UNDEF, **ic.SCALARS)
    out = out.cpu().numpy() if device else out
    assert fl[7] == ic.NONE_DEFINED and set(fl.tolist()) >= {ic.SOME_DEFINED}
    for l in range(nlev):
        single = [f[l] if f.ndim == 3 else f for f in fields]
        _, sflag, one = gpu_run(gpu_ctx, model, single, alt, int(flags[l]))
        assert sflag == fl[l] and ic.same_bits(out[l], one), l


def test_batch_refuses_out_over_a_shared_input(gpu_ctx):
    import torch

    fields = [torch.from_numpy(f).cuda() for f in ic.make_inputs(16, 8, 3, nlev=2)]
    big = torch.zeros((2, 8, 16), dtype=torch.float32, device="cuda")
    fields[10] = big[1]  # shared depth inside the output
    with pytest.raises(RuntimeError, match="shared"):
        gpu_ctx.vesselIcing_levels("modstall", fields, out=big, **ic.SCALARS)


@pytest.mark.parametrize("model,alt", [(ic.MODSTALL, 1), (ic.MINCOG, 1)], ids=["modstall", "mincog"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_out_may_alias_airtemp(gpu_ctx, model, alt, device):
    import torch

    fields = ic.make_inputs(129, 40, 12, specials=True)
    _, f0, expect = gpu_run(gpu_ctx, model, fields, alt)
    if device:
        args = [torch.from_numpy(f.copy()).cuda() for f in fields]
        fn = gpu_ctx.vesselIcingModStall if model == ic.MODSTALL else gpu_ctx.vesselIcingMincog
        extra = [] if model == ic.MODSTALL else [alt]
        _, f1 = fn(*args, *[ic.SCALARS[k] for k in ("vs", "alpha", "zmin", "zmax")], *extra, undef=ic.UNDEF, out=args[4])
        got = args[4].cpu().numpy()
    else:
        args = [f.copy() for f in fields]
        fn = gpu_ctx.vesselIcingModStall if model == ic.MODSTALL else gpu_ctx.vesselIcingMincog
        extra = [] if model == ic.MODSTALL else [alt]
        _, f1 = fn(*args, *[ic.SCALARS[k] for k in ("vs", "alpha", "zmin", "zmax")], *extra, undef=ic.UNDEF, out=args[4])
        got = args[4]
    assert f1 == f0 and ic.same_bits(got, expect)


CXX_CALLER = r"""
#include <mi_fieldcalc/FieldCalculations.h>

#include <cstdio>
#include <vector>

using namespace miutil;

int main(int argc, char** argv)
{
  const int nx = 129, ny = 40, n = nx * ny;
  std::vector<float> in(11 * n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(in.data(), sizeof(float), in.size(), f) != in.size())
    return 2;
  std::fclose(f);
  const float* p[11];
  for (int k = 0; k < 11; ++k)
    p[k] = in.data() + k * n;
  std::vector<float> out(2 * n);
  ValuesDefined f1 = SOME_DEFINED, f2 = SOME_DEFINED;
  const bool ok1 = fieldcalc::vesselIcingModStall(nx, ny, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], 5.f, 0.7f, 0.f, 10.f,
                                                  out.data(), f1, 1e35f);
  const bool ok2 = fieldcalc::vesselIcingMincog(nx, ny, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], 5.f, 0.7f, 0.f, 10.f, 2,
                                                out.data() + n, f2, 1e35f);
  FILE* g = std::fopen(argv[2], "wb");
  std::fwrite(out.data(), sizeof(float), out.size(), g);
  std::fclose(g);
  std::printf("%d %d %d %d\n", ok1, ok2, (int)f1, (int)f2);
  return 0;
}
"""


def test_cxx_symbols_compute(gpu_ctx, ref, tmp_path):
    """Both miutil::fieldcalc symbols return true and compute: bit for bit what the Context computes (the same kernel),
    and within the accuracy contract of the reference's values."""
    src = tmp_path / "icing_caller.cc"
    src.write_text(CXX_CALLER)
    exe = tmp_path / "icing_caller"
    inc = os.path.join(ROOT, "mi-fieldcalc_amd", "include")
    libdir = os.path.join(ROOT, "mi-fieldcalc_amd")
    subprocess.run(["g++", "-std=c++11", "-Wall", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lmi-fieldcalc", "-lmifc",
                    "-Wl,-rpath," + libdir], check=True)
    fields = ic.make_inputs(129, 40, 4, specials=True)
    np.concatenate([f.ravel() for f in fields]).astype(np.float32).tofile(str(tmp_path / "in.bin"))
    res = subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, check=True)
    ok1, ok2, f1, f2 = (int(x) for x in res.stdout.split())
    assert ok1 == 1 and ok2 == 1
    out = np.fromfile(str(tmp_path / "out.bin"), np.float32).reshape(2, 40, 129)
    _, g1, c1 = gpu_run(gpu_ctx, ic.MODSTALL, fields)
    _, g2, c2 = gpu_run(gpu_ctx, ic.MINCOG, fields, alt=2)
    assert (f1, f2) == (g1, g2) and ic.same_bits(out[0], c1) and ic.same_bits(out[1], c2)
    _, r1, e1 = ref.run(ic.MODSTALL, fields, **ic.SCALARS)
    _, r2, e2 = ref.run(ic.MINCOG, fields, alt=2, **ic.SCALARS)
    assert_contract(out[0], f1, e1, r1, "ModStall")
    assert_contract(out[1], f2, e2, r2, "MINCOG")


def test_python_drop_in(gpu_ctx):
    import mi_fieldcalc as pyfc

    fields = ic.make_inputs(50, 20, 8, specials=True)
    got = pyfc.vesselIcingModStall(*fields, 5.0, 0.7, 0.0, 10.0, 1e35)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (20, 50)
    expect, _ = gpu_ctx.vesselIcingModStall(*fields, 5.0, 0.7, 0.0, 10.0, undef=1e35)
    assert ic.same_bits(got, expect)
    assert pyfc.vesselIcingModStall(*fields[:10], fields[10][:5], 5.0, 0.7, 0.0, 10.0, 1e35) is None  # shapes differ
    assert pyfc.vesselIcingModStall(*fields, 5.0, 0.7, 3.0, 2.0, 1e35) is None  # the reference's false
