"""Parcel ascent over level batches on the GPU (mifc_vparcel.hip, mifc_vparcel_hlevels / mifc_vparcel_fields /
mifc_vparcel_levels, through mi_fieldcalc_amd.vparcel) against the numpy restatement (tests/vparcel_restate.py).

Undef cells and flags are exact.  Values: the device's x^kappa is the correctly rounded float or its neighbour, so its pi
is the restatement's or the neighbour's at every point.  The restatement is therefore run once as it is (R0) and once per
member of a family of pi nudges (all down, all up, alternating by level in both phases, two seeded random patterns:
tests/vparcel_cases.py), and a value of a stable cell must lie within
    |got - R0| <= 2 * max_j |R_j - R0| + 2 ulp_float32(R0):
the extreme and the alternating patterns span the response to one-ulp changes of pi, the factor 2 covers mixed patterns
and the last bit of the device's double log / exp.  The bound comes from the restatement alone.  Which cells are stable
(no member changes the undef-ness of an output, the piece that holds LCL, LFC or EL, or whether the adjustment ran at a
level) is a property of the inputs; tests/test_vparcel_cpu.py asserts that at most 2 % of a case's cells are not.
Where the arithmetic is the same -- four cells per lane or one, device or host memory, one band or several, any subset of
the outputs -- results are bit for bit the same."""
import ctypes

import numpy as np
import pytest

import vcumul_restate as vcr
import vinterp_restate as vi
import vparcel_cases as vc
import vparcel_restate as vp
from cases import same_bits

pytestmark = pytest.mark.gpu

U = vp.UNDEF
ALL = vp.OUTPUTS
FORM_NAMES = {"hyb": "hlevels", "fld": "fields", "lev": "levels"}


def front():
    from mi_fieldcalc_amd import vparcel

    return vparcel


def _placer(device, offset=False):
    """Puts a float32 array where the call wants it: a numpy copy (host), a CUDA tensor, or a CUDA tensor that begins one
    float behind the 16-byte grid (offset: the kernel then takes one cell per lane on the same data)."""
    if not device:
        return lambda a: None if a is None else np.array(a, np.float32)
    import torch

    def put(a):
        if a is None:
            return None
        a = np.array(a, np.float32)
        if not offset:
            return torch.from_numpy(a).cuda()
        room = torch.empty(a.size + 5, dtype=torch.float32, device="cuda")
        at = 1 + (-(room.data_ptr() // 4) % 4)  # one float behind a 16-byte boundary
        return room[at:at + a.size].view(a.shape).copy_(torch.from_numpy(a))

    return put


def run(ctx, c, form, device, outputs=ALL, offset=False, **kw):
    put = _placer(device, offset)
    kw = dict(dict(src_level=c["src_level"], from_=c["from"], t_src=put(c["t_src"]), p_src=put(c["p_src"]), outputs=outputs,
                   fdefined_in=c["fdefined_in"]), **kw)
    t, q = put(c["t"]), put(c["q_src"])
    if form == "hyb":
        r = front().vparcel_hlevels(ctx, t, put(c["ps"]), c["al"], c["bl"], q, **kw)
    elif form == "fld":
        r = front().vparcel_fields(ctx, t, put(c["p"]), q, fdef_coord=c["fdef_coord"], **kw)
    else:
        r = front().vparcel_levels(ctx, t, c["plev"], q, **kw)
    return {n: (v.cpu().numpy() if device and n != "flags" else v) for n, v in r.items()}


def same(a, b, label):
    assert sorted(a) == sorted(b), label
    for n in a:
        if n == "flags":
            for m in a[n]:
                assert np.array_equal(a[n][m], b[n][m]), (label, "flags", m)
        else:
            assert same_bits(a[n], b[n], nan_payload=False), (label, n, int((a[n].view(np.uint32) != b[n].view(np.uint32)).sum()))


def against_reference(got, ref, label, ratios=None):
    r0 = ref.r0
    whole = ref.stable.all()
    for n in ALL:
        g, e = got[n], r0[n]
        assert g.shape == e.shape and g.dtype == np.float32, (label, n)
        st = ref.stable if e.ndim == 2 else np.broadcast_to(ref.stable, e.shape)
        gu, eu = g.view(np.uint32) == U.view(np.uint32), e == U
        assert np.array_equal(gu[st], eu[st]), (label, n, "undef cells differ", int((gu != eu)[st].sum()))
        if whole:
            assert np.array_equal(got["flags"][n], r0["flags"][n]), (label, n, got["flags"][n], r0["flags"][n])
        m = st & ~eu
        with np.errstate(all="ignore"):
            err = np.abs(g.astype(np.float64) - e.astype(np.float64))[m]
            bound = ref.bound(n)[m]
        ratio = float((err / bound).max()) if err.size else 0.0
        if ratios is not None:
            ratios[n] = max(ratios.get(n, 0.0), ratio)
        if not (err <= bound).all():
            bad = np.nonzero(~(err <= bound))[0]
            raise AssertionError("%s %s: %d stable values beyond the bound; worst |got - R0| / bound = %.3g (got %r, R0 %r, bound %r)" % (
                label, n, bad.size, ratio, g[m][bad[0]], e[m][bad[0]], bound[bad[0]]))


_RATIOS = {}


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", vc.case_names())
def test_every_case_three_forms_against_the_restatement(gpu_ctx, name, device):
    c = vc.by_name(name)
    v = 4 if (not device or (c["ny"] * c["nx"]) % 4 == 0) else 1  # a staged band always takes four cells per lane
    for form in vc.FORMS:
        got = run(gpu_ctx, c, form, device)
        seen = front().last_vparcel_form(gpu_ctx)
        assert seen == {"v": v, "form": FORM_NAMES[form], "from": c["from"], "src": -1 if c["src_level"] is None else c["src_level"], "outputs": 6,
                        "launches": 1}, (name, form, seen)
        against_reference(got, vc.reference(name, form), (name, form, "device" if device else "host"), _RATIOS)
    print("largest |got - R0| / bound so far:", {n: round(r, 4) for n, r in _RATIOS.items()})


@pytest.mark.parametrize("name", ["n7_9x16_first_planes", "n12_9x16_first_first", "n3_9x16_last_middle", "n7_10x206_last_first", "n4_10x206_first_planes"])
def test_cells_per_lane_and_memory_kind_do_not_change_a_bit(gpu_ctx, name):
    c = vc.by_name(name)
    for form in vc.FORMS:
        four = run(gpu_ctx, c, form, True)
        assert front().last_vparcel_form(gpu_ctx)["v"] == 4
        one = run(gpu_ctx, c, form, True, offset=True)
        assert front().last_vparcel_form(gpu_ctx)["v"] == 1
        same(four, one, (name, form, "v=4 / v=1"))
        host = run(gpu_ctx, c, form, False)
        same(four, host, (name, form, "device / host"))


def test_bands_do_not_change_a_bit(gpu_ctx, mifc_env):
    c = vc.make(7, 41, 651, "last", "first")  # 26 691 cells, 21 planes staged: more than two MiB
    d = vc.make(4, 81, 651, "first", "planes")  # 16 planes and more of 52 731 cells
    for case, form in ((c, "hyb"), (c, "fld"), (d, "lev"), (d, "fld")):
        mifc_env("MIFC_VPARCEL_CHUNK_MIB", None)
        whole = run(gpu_ctx, case, form, False)
        assert front().last_vparcel_form(gpu_ctx)["launches"] == 1
        mifc_env("MIFC_VPARCEL_CHUNK_MIB", 1)
        banded = run(gpu_ctx, case, form, False)
        assert front().last_vparcel_form(gpu_ctx)["launches"] >= 3, front().last_vparcel_form(gpu_ctx)
        same(whole, banded, (case["name"], form, "one band / several"))
        dev = run(gpu_ctx, case, form, True)  # an odd number of cells: one cell per lane on the device
        assert front().last_vparcel_form(gpu_ctx)["v"] == 1
        same(whole, dev, (case["name"], form, "host / device"))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_any_subset_of_the_outputs_equals_all_of_them(gpu_ctx, device):
    for name, form in (("n7_9x16_first_first", "hyb"), ("n12_9x13_last_planes", "fld"), ("n4_9x16_last_middle", "lev")):
        c = vc.by_name(name)
        every = run(gpu_ctx, c, form, device)
        for subset in (("cape",), ("tparcel",), ("pel", "plcl"), ("cin", "plfc", "tparcel"), "plcl"):
            names = (subset,) if isinstance(subset, str) else subset
            got = run(gpu_ctx, c, form, device, outputs=subset)
            assert front().last_vparcel_form(gpu_ctx)["outputs"] == len(names)
            assert sorted(got) == sorted(names + ("flags",)) and sorted(got["flags"]) == sorted(names)
            same(got, {**{n: every[n] for n in names}, "flags": {n: every["flags"][n] for n in names}}, (name, form, subset))


@pytest.mark.parametrize("name", ["n12_9x16_first_first", "n7_9x13_last_planes", "n4_9x16_last_middle"])
def test_levels_form_equals_fields_form_on_the_same_pressures(gpu_ctx, name):
    """The `levels` form takes pi of a level from the host's powf, the `fields` form from the device's tables: within the
    bound of the restatement on these pressures, and bit-equal in every cell when the two pi agree on every level (the
    device's is read back through the dry step of a column that never saturates)."""
    c = vc.by_name(name)
    batch = np.ascontiguousarray(np.broadcast_to(c["plev"][:, None, None], c["t"].shape))
    lev = run(gpu_ctx, c, "lev", True)
    fld = run(gpu_ctx, dict(c, p=batch, fdef_coord=None), "fld", True)
    ref = vc.reference(name, "lev")
    against_reference(lev, ref, (name, "levels"))
    against_reference(fld, ref, (name, "fields on the level pressures"))
    # the device's power through aleveltemp with theta == 1 (tests/test_gpu_seams.py), the host's through libm's powf
    res = gpu_ctx.aleveltemp(np.ones((1, c["nlev"]), np.float32), np.array(c["plev"], np.float32).reshape(1, -1), "kelvin", 2)
    dev_power = np.asarray(res[0] if isinstance(res, tuple) else res, np.float32).ravel()
    powf = ctypes.CDLL("libm.so.6").powf
    powf.restype, powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    host_power = np.array([powf(float(np.float32(x) * vp.P0INV), float(vp.KAPPA)) for x in c["plev"]], np.float32)
    agree = bool((dev_power == host_power).all())
    differ = [n for n in ALL if not same_bits(lev[n], fld[n], nan_payload=False)]
    print(name, "pi agrees on every level:", agree, "outputs that differ between the two forms:", differ)
    if agree:  # (the pi of source planes is the device's in both forms)
        assert not differ, differ


def test_refusals_write_nothing(gpu_ctx):
    import torch

    import mi_fieldcalc_amd._capi as capi

    lib, ctx = capi.lib(), gpu_ctx._ctx
    c = vc.by_name("n4_9x16_first_planes")
    nlev, ny, nx = c["nlev"], c["ny"], c["nx"]
    plane, batch = ny * nx, nlev * ny * nx
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    t, p = dev(c["t"]), dev(c["p"])
    room = torch.zeros(2 * batch + 4 * plane, dtype=torch.float32, device="cuda")  # the planes between two batches of the test's own
    ps, ts, qs, psrc = (room[batch + i * plane:batch + (i + 1) * plane].view(ny, nx).copy_(dev(a)) for i, a in
                        enumerate((c["ps"], c["t_src"], c["q_src"], c["p_src"])))
    sentinel = -4242.5
    outs = torch.full((5, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    tp = torch.full((nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")

    def call(kind, nx_=nx, ny_=ny, nlev_=nlev, t_="own", coord="own", a=None, b=None, lv=None, from_=0, src=-1, t_src="own", q_src="own", p_src="own",
             o=None, tparcel="own", fd_out=True, sync=True):
        own = lambda v, mine: mine if isinstance(v, str) and v == "own" else v  # noqa: E731
        al = np.asarray(c["al"] if a is None or isinstance(a, str) else a, np.float32)
        bl = np.asarray(c["bl"] if b is None or isinstance(b, str) else b, np.float32)
        lev = np.asarray(c["plev"] if lv is None else lv, np.float32)
        fd = np.full(5 + nlev, 7, np.int32)
        op = [outs[i].data_ptr() for i in range(5)] if o is None else o
        tail = [from_, src, own(t_src, ts.data_ptr()), vp.SOME_DEFINED, own(q_src, qs.data_ptr()), vp.SOME_DEFINED, own(p_src, psrc.data_ptr()),
                vp.SOME_DEFINED] + list(op) + [own(tparcel, tp.data_ptr()), fd.ctypes.data if fd_out else None, float(U), 1]
        head = [ctx, nx_, ny_, nlev_, own(t_, t.data_ptr()), None]
        if kind == "hyb":
            rc = lib.mifc_vparcel_hlevels(*head, own(coord, ps.data_ptr()), vp.SOME_DEFINED, None if isinstance(a, str) else al.ctypes.data,
                                          None if isinstance(b, str) else bl.ctypes.data, *tail)
        elif kind == "fld":
            rc = lib.mifc_vparcel_fields(*head, own(coord, p.data_ptr()), None, *tail)
        else:
            rc = lib.mifc_vparcel_levels(*head, own(coord, lev.ctypes.data), *tail)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    o5 = [outs[i].data_ptr() for i in range(5)]
    swap = lambda i, ptr: o5[:i] + [ptr] + o5[i + 1:]  # noqa: E731
    null_head = {"hyb": "a null pointer (t, ps, alevel or blevel)", "fld": "a null pointer (t or p)", "lev": "a null pointer (t or levels)"}
    no_level = "level %d: alevel / blevel are no hybrid level (FieldCalculations.cc:298)"
    every = {
        "nlev < 2": (dict(nlev_=1), "nlev < 2"),
        "negative nx": (dict(nx_=-1), "a negative nx or ny"),
        "negative ny": (dict(ny_=-3), "a negative nx or ny"),
        "unknown from": (dict(from_=2), "unknown from 2"),
        "negative from": (dict(from_=-1), "unknown from -1"),
        "src_level too large": (dict(src=nlev), "src_level %d outside -1..%d" % (nlev, nlev - 1)),
        "src_level -2": (dict(src=-2), "src_level -2 outside -1..%d" % (nlev - 1)),
        "null t": (dict(t_=None), null_head),
        "null coordinate": (dict(coord=None), null_head),
        "null q_src": (dict(q_src=None, src=1), "a null pointer (q_src)"),
        "null t_src with planes": (dict(t_src=None), "a null pointer (t_src, q_src or p_src with src_level -1)"),
        "null p_src with planes": (dict(p_src=None), "a null pointer (t_src, q_src or p_src with src_level -1)"),
        "no output": (dict(o=[None] * 5, tparcel=None), "no output (cape, cin, plcl, plfc, pel and tparcel are all null)"),
        "null fdefined_out": (dict(fd_out=False), "a null pointer (fdefined_out)"),
        "cape is t": (dict(o=swap(0, t.data_ptr())), "cape[0] overlaps fields[0]"),
        "pel ends in t": (dict(o=swap(4, t.data_ptr() - 4 * (plane - 1))), "pel[0] overlaps fields[0]"),
        "tparcel is t": (dict(tparcel=t.data_ptr()), "tparcel[0] overlaps fields[0]"),
        "two outputs are one": (dict(o=swap(1, outs[3].data_ptr())), "cin[0] overlaps plfc[0]"),
        "a plane inside tparcel": (dict(o=swap(2, tp.data_ptr() + 4 * plane)), "plcl[0] overlaps tparcel[0]"),
        "plfc is q_src": (dict(o=swap(3, qs.data_ptr())), "plfc[0] overlaps q_src"),
        "cin ends in t_src": (dict(o=swap(1, ts.data_ptr() - 4 * (plane - 1))), {"hyb": "cin[0] overlaps ps", "fld": "cin[0] overlaps t_src",
                                                                                 "lev": "cin[0] overlaps t_src"}),
        "cape begins in p_src": (dict(o=swap(0, psrc.data_ptr() + 4 * (plane - 1))), "cape[0] overlaps p_src"),
    }
    only = {
        "hyb": {
            "null alevel": (dict(a="null"), null_head),
            "null blevel": (dict(b="null"), null_head),
            "negative alevel": (dict(a=[1.0, -1.0, 2.0, 0.0]), no_level % 1),
            "blevel > 1": (dict(b=[1.0, 0.1, 0.2, 1.5]), no_level % 3),
            "an output is ps": (dict(o=swap(2, ps.data_ptr())), "plcl[0] overlaps ps"),
        },
        "fld": {"tparcel ends in p": (dict(tparcel=p.data_ptr() - 4 * (batch - 1)), "tparcel[0] overlaps coord")},
        "lev": {
            "NaN level": (dict(lv=[900, float("nan"), 500, 300]), "levels[1] is NaN"),
            "zero level": (dict(lv=[0.0, 700, 500, 300]), "levels[0] <= 0"),
            "negative level": (dict(lv=[900, 700, -500, 300]), "levels[2] <= 0"),
        },
    }
    for kind in vc.FORMS:
        before = room.clone(), t.clone(), p.clone()
        for what, (kw, tail) in {**every, **only[kind]}.items():
            rc, err, fd = call(kind, **kw)
            want = "mifc_vparcel_%s: " % FORM_NAMES[kind] + (tail[kind] if isinstance(tail, dict) else tail)
            assert rc == 0 and err == want, (kind, what, err, want)
            assert (outs == sentinel).all().item() and (tp == sentinel).all().item() and (fd == 7).all(), (kind, what)
        bits = lambda x: x.view(torch.int32)  # noqa: E731  (the inputs hold NaNs)
        assert torch.equal(bits(room), bits(before[0])) and torch.equal(bits(t), bits(before[1])) and torch.equal(bits(p), bits(before[2]))
    with pytest.raises(ValueError, match="mifc_vparcel_hlevels: unknown from -1") as info:
        front().vparcel_hlevels(gpu_ctx, t, ps, c["al"], c["bl"], qs, src_level=0, from_="sideways")
    assert isinstance(info.value, RuntimeError)
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        refused = [call(kind, sync=False) for kind in vc.FORMS]
    g.close()
    for rc, err, fd in refused:
        assert rc == 0 and "capture" in err and (fd == 7).all()
    assert (outs == sentinel).all().item() and (tp == sentinel).all().item()
    # afterwards the same calls run, and with a source level t_src and p_src may be absent
    for kind in vc.FORMS:
        rc, err, fd = call(kind)
        assert rc == 1 and err == "" and (fd != 7).all(), (kind, err)
        rc, err, fd = call(kind, src=1, t_src=None, p_src=None, o=swap(1, None))
        assert rc == 1 and err == "" and fd[1] == 7 and (np.delete(fd, 1) != 7).all(), (kind, err, fd)
    got = {n: outs[i].cpu().numpy() for i, n in enumerate(vc.PLANES) if i != 1}
    exp = vp.levels(c["t"], c["plev"], c["q_src"], from_=c["from"], src_level=1)
    for n in got:
        assert np.array_equal(got[n] == U, exp[n] == U), n


def test_empty_grid(gpu_ctx):
    t = np.zeros((3, 0, 5), np.float32)
    r = front().vparcel_levels(gpu_ctx, t, [900, 700, 500], np.zeros((0, 5), np.float32), outputs=ALL)
    assert r["cape"].shape == (0, 5) and r["tparcel"].shape == (3, 0, 5)
    assert all(r["flags"][n] == vp.ALL_DEFINED for n in vc.PLANES) and (r["flags"]["tparcel"] == vp.ALL_DEFINED).all()


def test_height_then_parcel_then_parcel_temperature_on_a_height_surface(gpu_ctx):
    """The chain on device tensors, no host copy in between: vcumul.geopotential_height_hlevels, vparcel_hlevels, then
    mifc_vinterp_fields of tparcel to a height surface -- against the restatements chained the same way (the parcel within
    its bound; the interpolation of the device's own tparcel and height bit for bit)."""
    import torch

    from mi_fieldcalc_amd import vcumul

    c = vc.by_name("n12_9x13_last_first")
    nlev = c["nlev"]
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    ps_h = np.where(c["ps"] == U, np.float32(1000.0), c["ps"])
    t_h = np.where((c["t"] == U) | np.isnan(c["t"]), np.float32(250.0), c["t"])
    t, ps = dev(t_h), dev(ps_h)
    z, zfd = vcumul.geopotential_height_hlevels(gpu_ctx, t, None, ps, c["al"], c["bl"])
    r = front().vparcel_hlevels(gpu_ctx, t, ps, c["al"], c["bl"], dev(c["q_src"]), src_level=c["src_level"], from_="last", outputs=("tparcel", "cape"))
    assert r["tparcel"].is_cuda and z.is_cuda
    targets = np.array([1500.0, 4000.0], np.float32)
    on_z, fd = gpu_ctx.vinterp_fields(r["tparcel"], z, targets, fdefined_in=[list(r["flags"]["tparcel"])], fdef_coord=zfd)
    assert on_z.is_cuda
    # the restatements chained
    cc = dict(c, t=t_h, ps=ps_h)
    ref = vc.Reference(cc, "hyb")
    got = {"tparcel": r["tparcel"].cpu().numpy(), "cape": r["cape"].cpu().numpy()}
    for n in got:
        e = ref.r0[n]
        st = ref.stable if e.ndim == 2 else np.broadcast_to(ref.stable, e.shape)
        assert np.array_equal((got[n] == U)[st], (e == U)[st]), n
        m = st & (e != U)
        assert (np.abs(got[n].astype(np.float64) - e.astype(np.float64))[m] <= ref.bound(n)[m]).all(), n
    exp, efd = vi.coord_fields(got["tparcel"][None], z.cpu().numpy(), targets, vi.LINEAR, np.asarray(r["flags"]["tparcel"])[None], list(zfd))
    assert same_bits(on_z.cpu().numpy(), exp[0], nan_payload=False) and list(fd) == list(efd[0])
    assert (exp[0] != U).any()
    zh, _ = vcr.hlevels(t_h[None], ps_h, c["al"], c["bl"], vcr.LOG, vcr.FROM_LAST, None, vcr.SOME_DEFINED, start=ps_h, scale=[-287.0 / 9.8])
    assert vcr.neighbours(z.cpu().numpy(), zh[0]).all()
