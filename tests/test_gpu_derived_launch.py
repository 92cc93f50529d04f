"""The fused derived batch (mifc_derived.hip) at its launch seams: one to five trips of the grid-stride loop -- every exit of
the two-trip software pipeline and its wrap -- in each instantiation launch_one chooses between, with and without the
per-cell tests (CHECK), with the per-level scalars in the kernel arguments (3 levels) and in device tables (9 levels).

MIFC_DERIVED_BLOCKS = B gives gx = min(ceil(n4 / 256), ceil(B / nlev)) workgroups per level; B = nlev (gx = 1) with
n4 in {255, 256, 257, 512, 513, 769, 1025} walks a level in one to five trips, B = 2 * nlev (gx = 2) with n4 in {513, 1025}
gives workgroup 0 one trip more than workgroup 1.  The fields are 4 x n4 cells.

Every level is compared with the restatement's per-level vectorabs / hleveltemp / hlevelhum / winddir under the bars of
test_gpu_scale._check_derived_batch (bit for bit unless the device power is involved, flags equal); the values also bit for
bit with the same call in its default launch shape; the undefined counts, read through enqueue_counts, exactly with the
number of undefined cells of the restatement's outputs; and mifc_last_pointwise_form says that the instantiation, CHECK,
PIPE and the number of trips are the ones the case is named for."""
import numpy as np
import pytest

import cases
import gpu_util
import launch_cases as lc

pytestmark = pytest.mark.gpu

F = np.float32
ALL, SOME = cases.ALL_DEFINED, cases.SOME_DEFINED
UNDEF = cases.UNDEF
N4 = {1: (255, 256, 257, 512, 513, 769, 1025), 2: (513, 1025)}
NX = 4

# name -> (what mifc_last_pointwise_form reports, the request, MIFC_DERIVED_PIPE)
CONFIGS = {
    "ff+rh+theta": ("ff+rh+theta", dict(temp=("", 3), hum=("", 1), hum2=None, ff=True, dd=False), None),
    "ff+rh+theta+td": ("ff+rh+theta+td", dict(temp=("", 3), hum=("", 1), hum2=("", 9), ff=True, dd=False), None),
    "rh+theta": ("rh+theta", dict(temp=("", 3), hum=("", 1), hum2=None, ff=False, dd=False), None),
    "rh+theta+td": ("rh+theta+td", dict(temp=("", 3), hum=("", 1), hum2=("", 9), ff=False, dd=False), None),
    "ff": ("ff", dict(temp=None, hum=None, hum2=None, ff=True, dd=False), None),
    "generic-thetae-hum-from-theta": ("generic", dict(temp=("", 4), hum=("", 2), hum2=("", 5), ff=True, dd=False), None),
    "generic-dd": ("generic", dict(temp=("celsius", 1), hum=("", 5), hum2=None, ff=False, dd=True), None),
    "ff+rh+theta-unpipelined": ("ff+rh+theta", dict(temp=("", 3), hum=("", 1), hum2=None, ff=True, dd=False), 0),
}
NAMES = ("ff", "temp", "hum", "hum2", "dd")  # the order of enqueue_counts


def make_batch(nlev, n4, gx, mode):
    """u, v, t, q (nlev, n4, 4), ps (n4, 4), a, b, wind flags, thermo flags.  mode "all": every level ALL_DEFINED, nothing
    undefined, and on level 1 a temperature beyond the saturation table at every seam position (humidities and theta-e are
    counted without any input test).  mode "mixed": levels 0, 3, 6 ALL_DEFINED and clean, the others SOME_DEFINED with
    undefined u, t or q at the seam positions of a walk on gx workgroups, and undefined ps (all levels share it)."""
    import mi_fieldcalc_amd.synth as synth

    ny, n = n4, 4 * n4
    u, v = synth.wind(NX, ny, 9100 + n4, nlev=nlev)
    t, q, ps = synth.thermo(NX, ny, 9200 + n4, nlev=nlev)
    a, b = synth.hybrid_levels(nlev)
    cells = np.asarray(lc.flat_cells(lc.seam_cells(n, gx)))
    flat = lambda x: x.reshape(x.shape[0], -1) if x.ndim == 3 else x.reshape(-1)
    if mode == "all":
        fw = ft = np.full(nlev, ALL, np.int32)
        flat(t)[1, cells] = lc.HOT_T
        return u, v, t, q, ps, a, b, fw, ft.copy()
    fw = np.array([ALL if l % 3 == 0 else SOME for l in range(nlev)], np.int32)
    ft = fw.copy()
    for l in range(nlev):
        if l % 3 == 1:
            flat(u)[l, cells[0::2]] = UNDEF
            flat(v)[l, cells[1::2]] = UNDEF
            flat(q)[l, cells[1::3]] = UNDEF
            flat(t)[l, cells[-1]] = lc.HOT_T
        elif l % 3 == 2:
            flat(t)[l, cells[0::2]] = UNDEF
            flat(q)[l, cells[1::2]] = UNDEF
            flat(u)[l, cells[-1]] = np.nan
    flat(ps)[cells[[1, -2]]] = UNDEF
    return u, v, t, q, ps, a, b, fw, ft


_ORACLE = {}


def per_level(oracle, key, name, *args, **kw):
    """One per-level call of the restatement, shared by the configurations that ask for the same output."""
    if key not in _ORACLE:
        with np.errstate(all="ignore"):
            ok, e, f = oracle.call(name, *args, **kw)
        assert ok, key
        _ORACLE[key] = (e, f)
    return _ORACLE[key]


def expected(oracle, req, batch, tag):
    """name -> [(expected field, expected flag, the case for gpu_util.compare)] per level"""
    u, v, t, q, ps, a, b, fw, ft = batch
    nlev, ny, nx = t.shape
    out = {}
    for l in range(nlev):
        al, bl = float(a[l]), float(b[l])
        if req["ff"]:
            e, f = per_level(oracle, (tag, l, "ff"), "vectorabs", nx, ny, u[l], v[l], fdefined=int(fw[l]))
            out.setdefault("ff", []).append((e, f, dict(label="ff l%d %s" % (l, tag), undef=UNDEF, op="vectorabs")))
        if req["dd"]:
            e, f = per_level(oracle, (tag, l, "dd"), "winddir", nx, ny, u[l], v[l], fdefined=int(fw[l]))
            out.setdefault("dd", []).append((e, f, dict(label="dd l%d %s" % (l, tag), undef=UNDEF, op="winddir")))
        if req["temp"]:
            cargs = [t[l], ps, al, bl, req["temp"][0], req["temp"][1]]
            e, f = per_level(oracle, (tag, l, "temp", req["temp"]), "hleveltemp", nx, ny, *cargs, fdefined=int(ft[l]))
            out.setdefault("temp", []).append((e, f, dict(label="temp l%d %s" % (l, tag), undef=UNDEF, op="hleveltemp", args=cargs)))
        for name in ("hum", "hum2"):
            if req[name]:
                cargs = [t[l], q[l], ps, al, bl, req[name][0], req[name][1]]
                e, f = per_level(oracle, (tag, l, "hum", req[name]), "hlevelhum", nx, ny, *cargs, fdefined=int(ft[l]))
                out.setdefault(name, []).append((e, f, dict(label="%s l%d %s" % (name, l, tag), undef=UNDEF, op="hlevelhum", args=cargs)))
    return out


def compare_level(case, got, e):
    if case["op"] == "winddir":
        # the bars of test_gpu_parity.test_winddir_extension: undefined cells in place, 1e-5 relative, one float spacing of 360 across north
        assert np.array_equal(got == UNDEF, e == UNDEF), case["label"]
        m = e != UNDEF
        err = np.abs(got[m].astype(np.float64) - e[m].astype(np.float64))
        wrap = err > 359.0
        assert np.all(360.0 - err[wrap] <= 3.1e-5), case["label"]
        assert np.all(err[~wrap] <= 1e-5 * np.abs(e[m][~wrap].astype(np.float64))), case["label"]
        return
    gpu_util.compare(case, got, e, case["op"] == "vectorabs" or (case["op"] == "hlevelhum" and not gpu_util.uses_device_powf(case)))


def run_enqueue(ctx, req, batch):
    """The asynchronous entry on device tensors: outputs (numpy) and the u64[5 * nlev] counts."""
    import torch

    u, v, t, q, ps, a, b, fw, ft = batch
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (u, v, t, q, ps)]
    nlev = t.shape[0]
    counts = torch.full((5 * nlev,), 12345, dtype=torch.int64, device="cuda")  # the entry zeroes its counters itself
    ctx.use_torch_stream()
    try:
        out = ctx.hlevel_derived_batch(*dev, a, b, fdef_wind=fw, fdef_thermo=ft, enqueue_counts=counts, **req)
        form = ctx.last_pointwise_form()
        torch.cuda.synchronize()
    finally:
        ctx.set_stream(None)
    assert out is not None
    return {k: x.cpu().numpy() for k, x in out.items()}, counts.cpu().numpy().reshape(5, nlev), form


def check_form(form, what, inst, check, pipe, gx, nlev, n4, trips):
    if gpu_util.run_is_forced():  # nothing is asserted about the shape, as in gpu_util.check_form
        return
    want = dict(family="derived", form="vector", inst=inst, check=check, pipe=pipe, grid=gx, nlev=nlev, n=4 * n4, tail=0, partials=0)
    assert {k: form.get(k) for k in want} == want, (what, form)
    assert lc.trips(form["n"] // 4, form["grid"]) == trips, (what, form)


@pytest.mark.parametrize("nlev", [3, 9])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_one_to_five_trips_of_every_instantiation(gpu_ctx, oracle, mifc_env, config, nlev):
    import mi_fieldcalc_amd as fc

    inst, req, pipe = CONFIGS[config]
    seen = set()
    for mode in ("all", "mixed"):
        # the default launch shape first: one trip per lane, host arrays, the synchronous entry
        mifc_env("MIFC_DERIVED_BLOCKS", None)
        mifc_env("MIFC_DERIVED_PIPE", None)
        plain = {}
        for gx in (1, 2):
            for n4 in N4[gx]:
                batch = make_batch(nlev, n4, gx, mode)
                res = gpu_ctx.hlevel_derived_batch(*batch[:7], fdef_wind=batch[7], fdef_thermo=batch[8], **req)
                assert res is not None, (config, n4)
                check_form(gpu_ctx.last_pointwise_form(), (config, n4, "default"), inst, int(mode == "mixed"), 1, -(-n4 // 256), nlev, n4, 1)
                plain[gx, n4] = res
        if pipe is not None:
            mifc_env("MIFC_DERIVED_PIPE", pipe)
        for gx in (1, 2):
            mifc_env("MIFC_DERIVED_BLOCKS", gx * nlev)
            for n4 in N4[gx]:
                n, trips = 4 * n4, lc.trips(n4, gx)
                tag = "derived-%s-nlev%d-n4_%d-gx%d" % (mode, nlev, n4, gx)
                batch = make_batch(nlev, n4, gx, mode)
                got, counts, form = run_enqueue(gpu_ctx, req, batch)
                check_form(form, (config, tag), inst, int(mode == "mixed"), 1 if pipe is None else pipe, gx, nlev, n4, trips)
                seen.add((gx, trips))
                exp = expected(oracle, req, batch, tag)
                assert sorted(got) == sorted(exp) == sorted(plain[gx, n4][0]), tag
                for name, levels in exp.items():
                    row = counts[NAMES.index(name)]
                    for l, (e, f, case) in enumerate(levels):
                        compare_level(case, got[name][l], e)
                        assert int(row[l]) == int(np.count_nonzero(e == UNDEF)), (case["label"], int(row[l]))
                        assert fc.classify(int(row[l]), n) == f == plain[gx, n4][1][name][l], case["label"]
                    assert cases.same_bits(got[name], plain[gx, n4][0][name]), "%s %s: the launch shape changes the result" % (tag, name)
                for k, name in enumerate(NAMES):  # counters of outputs that were not asked for stay zero
                    if name not in exp:
                        assert not counts[k].any(), (tag, name)
    assert seen == {(1, 1), (1, 2), (1, 3), (1, 4), (1, 5), (2, 2), (2, 3)}, seen


@pytest.mark.parametrize("nlev", [3, 9])
def test_original_trio_counts_in_their_own_order(gpu_ctx, oracle, mifc_env, nlev):
    """mifc_hlevel_derived_levels_enqueue keeps its u64[3 * nlev] layout ff | rh | theta (the kernel counts ff | temp | hum)."""
    import torch

    import mi_fieldcalc_amd as fc

    req = CONFIGS["ff+rh+theta"][1]
    for gx, n4 in ((1, 769), (2, 1025)):
        mifc_env("MIFC_DERIVED_BLOCKS", gx * nlev)
        batch = make_batch(nlev, n4, gx, "mixed")
        u, v, t, q, ps, a, b, fw, ft = batch
        tag = "derived-mixed-nlev%d-n4_%d-gx%d" % (nlev, n4, gx)
        exp = expected(oracle, req, batch, tag)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (u, v, t, q, ps)]
        ff, rh, theta = (torch.full_like(dev[0], -7777.0) for _ in range(3))
        counts = torch.full((3 * nlev,), 12345, dtype=torch.int64, device="cuda")
        gpu_ctx.use_torch_stream()
        try:
            assert gpu_ctx.hlevel_derived_levels_enqueue(*dev, a, b, ff, rh, theta, counts, fdef_wind=fw, fdef_thermo=ft)
            form = gpu_ctx.last_pointwise_form()
            torch.cuda.synchronize()
        finally:
            gpu_ctx.set_stream(None)
        check_form(form, tag, "ff+rh+theta", 1, 1, gx, nlev, n4, lc.trips(n4, gx))
        counts = counts.cpu().numpy().reshape(3, nlev)
        for row, (name, out) in enumerate((("ff", ff), ("hum", rh), ("temp", theta))):
            for l, (e, f, case) in enumerate(exp[name]):
                compare_level(case, out[l].cpu().numpy(), e)
                assert int(counts[row, l]) == int(np.count_nonzero(e == UNDEF)) and fc.classify(int(counts[row, l]), 4 * n4) == f, case["label"]
