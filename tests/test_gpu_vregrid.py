"""Level batches interpolated to per-cell target surfaces on the GPU (mifc_vregrid.hip, mifc_vregrid_hlevels / _fields /
_levels, through mi_fieldcalc_amd.vregrid) against the numpy restatement (tests/vregrid_restate.py).  LINEAR: bit for bit
(a NaN matches any NaN), flags equal.  LOG: the undefined cells and the flags identical, every other value equal or the
neighbouring float32, and at most 1 % of the compared values differ at all -- tests/test_vregrid_cpu.py holds on these
cases that a double log() an ulp off changes no more than that (the levels are more than 1e-3 apart in ln p, as
tests/test_gpu_vinterp.py argues)."""
import ctypes

import numpy as np
import pytest

import vinterp_restate as vi
import vregrid_cases as vc
import vregrid_restate as vg
from cases import same_bits

pytestmark = pytest.mark.gpu

U = vg.UNDEF
EVERY = [(m, f, o) for m in ("linear", "log") for f in ("first", "last") for o in ("undef", "clamp")]


def front():
    from mi_fieldcalc_amd import vregrid

    return vregrid


def compare(got, exp, gfd, efd, method, undef, label):
    assert got.shape == exp.shape, label
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if method == "linear":
        if not same_bits(got, exp, nan_payload=False):
            bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
            first = tuple(int(b[0]) for b in bad)
            raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))
        return
    isun = np.isnan if np.isnan(undef) else (lambda a: a == np.float32(undef))
    assert np.array_equal(isun(got), isun(exp)), label
    d = ~isun(exp) & ~(np.isnan(got) & np.isnan(exp))
    steps = np.abs(got.view(np.int32)[d].astype(np.int64) - exp.view(np.int32)[d].astype(np.int64))
    assert steps.size == 0 or steps.max() <= 1, (label, int(steps.max()))
    assert steps.size == 0 or (steps != 0).mean() <= 0.01, (label, float((steps != 0).mean()))


def run(ctx, case, method, from_="first", outside="undef", device=True, stacked=True):
    import torch

    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    f = put(case["fields"])
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    kw = dict(method=method, from_=from_, outside=outside, fdefined_in=case.get("flags"), fdef_tcoord=case.get("fdef_t"), undef=case.get("undef", U))
    if case["kind"] == "hybrid":
        out, fd = front().vregrid_hlevels(ctx, f, put(case["coord"]), case["ab"][0], case["ab"][1], put(case["tcoord"]),
                                          fdef_ps=vg.SOME_DEFINED if case.get("fdef_c") is None else case["fdef_c"], **kw)
    elif case["kind"] == "field":
        out, fd = front().vregrid_fields(ctx, f, put(case["coord"]), put(case["tcoord"]), fdef_coord=case.get("fdef_c"), **kw)
    else:
        out, fd = front().vregrid_levels(ctx, f, case["coord"], put(case["tcoord"]), **kw)
    return (out.cpu().numpy() if device else out), fd


def check(ctx, case, method, from_="first", outside="undef", device=True, stacked=True, label=None):
    got, gfd = run(ctx, case, method, from_, outside, device, stacked)
    exp, efd = vc.expected(case, method, from_, outside)
    compare(got, exp, gfd, efd, method, case.get("undef", U), (label, case["kind"], method, from_, outside, "device" if device else "host"))
    return front().last_vregrid_form(ctx)


def check_every(ctx, case, device=True, stacked=True, label=None, methods=("linear", "log")):
    for method, from_, outside in EVERY:
        if method in methods:
            form = check(ctx, case, method, from_, outside, device, stacked, label)
            assert (form["method"], form["from"], form["outside"]) == (method, from_, outside) and form["coord"] == case["kind"], form
    return form


# ------------------------------------------------------------------- coordinate kinds, memory, number of fields
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 3, 8])
@pytest.mark.parametrize("kind", ["hybrid", "field", "levels"])
def test_kinds_memory_and_fields(gpu_ctx, kind, nf, device):
    form = check_every(gpu_ctx, vc.main(kind, nf), device, stacked=(nf != 3), label=("nf", nf))  # nlev 12, ny 9, nx 13
    assert form["v"] == 1 and form["passes"] == 1  # one cell per lane unless the other form is asked for


# ------------------------------------------------------------------------------------- four cells per lane
@pytest.mark.parametrize("shape", [(4, 3, 1100), (12, 9, 16)], ids=["blocks", "nx16"])
def test_vector_form_over_several_workgroups_with_a_tail(gpu_ctx, mifc_env, shape):
    mifc_env("MIFC_VREGRID_V", 4)  # four cells per lane where the batch is on the 16-byte grid
    nlev, ny, nx = shape  # 3300 cells: three workgroups of 1024 and a tail of 228, the last lane's group ends the batch
    for kind in ("hybrid", "field", "levels"):
        form = check_every(gpu_ctx, vc.main(kind, 2, nlev, ny, nx, 3, 7), label=shape)
        assert form["v"] == 4


def test_device_batch_offset_by_one_float_takes_the_scalar_form(gpu_ctx, mifc_env):
    import torch

    mifc_env("MIFC_VREGRID_V", 4)

    case = vc.main("hybrid", 2, 12, 9, 16, 3, 7)
    fields = case["fields"]
    n = fields[0].size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
    batches = [buf[1 + j * n:1 + (j + 1) * n].view(12, 9, 16) for j in range(2)]  # 4 bytes past the 16-byte grid
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for method, from_, outside in (("linear", "first", "clamp"), ("linear", "last", "undef")):
        out, fd = front().vregrid_hlevels(gpu_ctx, batches, dev(case["coord"]), case["ab"][0], case["ab"][1], dev(case["tcoord"]), method, from_, outside)
        assert front().last_vregrid_form(gpu_ctx)["v"] == 1
        aligned, afd = run(gpu_ctx, case, method, from_, outside)
        assert front().last_vregrid_form(gpu_ctx)["v"] == 4
        assert same_bits(out.cpu().numpy(), aligned, nan_payload=False) and np.array_equal(fd, afd)
        exp, efd = vc.expected(case, method, from_, outside)
        compare(aligned, exp, afd, efd, method, U, "offset")


# ------------------------------------------------------------------------------------------------- passes
@pytest.mark.parametrize("nx", [13, 16], ids=["v1", "v4"])
def test_target_counts_across_passes(gpu_ctx, mifc_env, nx):
    if nx == 16:
        mifc_env("MIFC_VREGRID_V", 4)
    tb = check(gpu_ctx, vc.main("field", 2, 5, 3, nx, 1, 3), "linear")["tb"]
    assert 1 <= tb <= 32
    for nt in (tb, tb + 1, 2 * tb + 1):
        case = vc.main("field", 2, 5, 3, nx, nt, 3)
        for method, from_, outside in (("linear", "first", "clamp"), ("log", "last", "clamp"), ("linear", "last", "undef")):
            form = check(gpu_ctx, case, method, from_, outside, label=("nt", nt))
            assert form["tb"] == tb and form["passes"] == -(-nt // tb) and form["v"] == (4 if nx == 16 else 1)
        check(gpu_ctx, case, "linear", "first", "clamp", device=False, label=("nt", nt))


def test_256_targets(gpu_ctx):
    case = vc.main("hybrid", 2, 6, 2, 8, 256, 4)
    form = check(gpu_ctx, case, "linear", "first", "clamp", label="nt 256")
    assert form["passes"] == -(-256 // form["tb"]) and form["v"] == 1
    check(gpu_ctx, case, "log", "last", "undef", device=False, label="nt 256")


# --------------------------------------------------------------------------------------------- level slots
@pytest.mark.parametrize("nlev", [2, 3, 4, 7])
def test_level_slots(gpu_ctx, nlev):
    for kind in ("hybrid", "field"):
        for nx in (13, 16):
            check_every(gpu_ctx, vc.main(kind, 2, nlev, 3, nx, 4, 9), label=("nlev", nlev), methods=("linear",))
    check_every(gpu_ctx, vc.main("field", 1, nlev, 3, 16, 4, 9), label=("nlev", nlev), methods=("log",))


# ----------------------------------------------------------------------------------------------- wave skip
@pytest.mark.parametrize("nx", [128, 130], ids=["v4", "v1"])
def test_wave_interval_decides(gpu_ctx, mifc_env, nx):
    """The skip of a level pair is decided by the wave's own intervals.  (a) Half of the cells of every wave have all their
    targets far outside the source range, the other half inside: the wave's target interval is wide, its pairs are narrow.
    (b) Every cell's column is the same, but the targets step through the pairs with the cell index: at a given pair only
    one cell of a wave brackets (two with V = 4 ... never the wave), and all the others must not be touched."""
    mifc_env("MIFC_VREGRID_V", 4)
    rng = np.random.default_rng(5)
    nlev, ny = 33, 1
    levels = np.linspace(100, 900, nlev).astype(np.float32)
    coord = np.broadcast_to(levels[:, None, None], (nlev, ny, nx)).copy()
    fields = rng.normal(0, 10, (2, nlev, ny, nx)).astype(np.float32)
    i = np.arange(nx)
    far = np.where((i // 32) % 2 == 0, np.float32(1.0e6), np.float32(1.0e-3))
    inside = rng.uniform(100, 900, (3, ny, nx)).astype(np.float32)
    half = np.where(((i // 16) % 2 == 0)[None, None, :], inside, np.broadcast_to(far, (3, ny, nx))).astype(np.float32)
    k = i % (nlev - 1)
    one = (levels[k] + rng.uniform(0.1, 0.9, nx).astype(np.float32) * (levels[k + 1] - levels[k])).astype(np.float32).reshape(1, ny, nx)
    for name, tcoord in (("half outside", half), ("one cell per pair", one)):
        case = dict(kind="field", fields=fields, coord=coord, tcoord=np.ascontiguousarray(tcoord))
        form = check_every(gpu_ctx, case, label=name)
        assert form["v"] == (4 if nx % 4 == 0 else 1)
        check(gpu_ctx, dict(case, kind="levels", coord=levels), "linear", "last", "clamp", label=name)
    exp, _ = vc.expected(dict(kind="field", fields=fields, coord=coord, tcoord=one), "linear")
    assert (exp != U).all()


# ---------------------------------------------------------------------------------------- definition cases
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_non_monotone_coordinates(gpu_ctx, mifc_env, device):
    check_every(gpu_ctx, vc.wavy(), device, label="wavy")
    mifc_env("MIFC_VREGRID_V", 4)
    check_every(gpu_ctx, vc.wavy(), device, label="wavy, four cells per lane where the batch allows")
    check_every(gpu_ctx, vc.main("hybrid", 3, bottom_up=True), device, label="bottom-up")
    check_every(gpu_ctx, vc.heights(), device, label="heights", methods=("linear",))
    check_every(gpu_ctx, vc.heights(2, 7, 9, 16), device, label="heights, four cells per lane")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mixed_flags_over_undef_and_nan(gpu_ctx, device):
    case = vc.flagged()
    check_every(gpu_ctx, case, device, label="flags")
    check_every(gpu_ctx, dict(case, flags=case["flags"][:, 0], fdef_c=[vg.ALL_DEFINED] * 12, fdef_t=[vg.ALL_DEFINED] * 5), device, label="one flag per field")
    rng = np.random.default_rng(8)
    hyb = vc.main("hybrid")
    for fdef_ps in vc.MIXED:
        mixed = dict(hyb, coord=vi.sprinkle(hyb["coord"], rng, 0.05, np.nan), flags=case["flags"], fdef_c=fdef_ps, fdef_t=case["fdef_t"])
        check_every(gpu_ctx, mixed, device, label=("fdef_ps", fdef_ps))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nan_as_undef(gpu_ctx, device):
    for case in (vc.main("hybrid"), vc.main("field"), vc.main("levels"), vc.heights()):
        check_every(gpu_ctx, vc.with_nan_undef(case), device, label="undef = NaN")


# ------------------------------------------------------------------------------- agreement with mifc_vinterp_*
@pytest.mark.parametrize("v", [1, 4])
def test_constant_target_planes_equal_vinterp_on_the_gpu(gpu_ctx, mifc_env, v):
    import torch

    mifc_env("MIFC_VREGRID_V", v)

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    targets = vi.MAIN_TARGETS
    for nx in (13, 16):
        hyb, fld = vc.main("hybrid", 3, 12, 9, nx), vc.main("field", 3, 12, 9, nx)
        tc = dev(np.broadcast_to(targets[:, None, None], (targets.size, 9, nx)))
        a, afd = front().vregrid_hlevels(gpu_ctx, dev(hyb["fields"]), dev(hyb["coord"]), hyb["ab"][0], hyb["ab"][1], tc)
        b, bfd = gpu_ctx.vinterp_hlevels(dev(hyb["fields"]), dev(hyb["coord"]), hyb["ab"][0], hyb["ab"][1], targets)
        assert same_bits(a.cpu().numpy(), b.cpu().numpy(), nan_payload=False) and np.array_equal(afd, bfd)
        a, afd = front().vregrid_fields(gpu_ctx, dev(fld["fields"]), dev(fld["coord"]), tc)
        b, bfd = gpu_ctx.vinterp_fields(dev(fld["fields"]), dev(fld["coord"]), targets)
        assert same_bits(a.cpu().numpy(), b.cpu().numpy(), nan_payload=False) and np.array_equal(afd, bfd)
        assert (b.cpu().numpy() != U).mean() > 0.3


# ---------------------------------------------------------------------------------------------- band staging
def test_host_call_in_several_bands_equals_one_band(gpu_ctx, mifc_env):
    # 36 + 1 + 5 + 15 = 57 planes of 333 floats per row: 13 rows per MiB, so 50 rows go in four bands, the last one short
    hyb, fld = vc.main("hybrid", 3, 12, 50, 333, 5, 9), vc.main("field", 3, 12, 50, 333, 5, 9)
    whole = {}
    for case in (hyb, fld):
        for method, from_, outside in (("linear", "first", "clamp"), ("log", "last", "undef")):
            whole[case["kind"], method] = run(gpu_ctx, case, method, from_, outside, device=False)
            assert front().last_vregrid_form(gpu_ctx)["launches"] == 1
    mifc_env("MIFC_VREGRID_CHUNK_MIB", 1)
    for case in (hyb, fld):
        for method, from_, outside in (("linear", "first", "clamp"), ("log", "last", "undef")):
            out, fd = run(gpu_ctx, case, method, from_, outside, device=False)
            assert front().last_vregrid_form(gpu_ctx)["launches"] == (4 if case["kind"] == "hybrid" else 5)  # (the coordinate batch: 68 planes, 11 rows)
            assert same_bits(out, whole[case["kind"], method][0], nan_payload=False) and np.array_equal(fd, whole[case["kind"], method][1])
    exp, efd = vc.expected(hyb, "linear", "first", "clamp")
    compare(whole["hybrid", "linear"][0], exp, whole["hybrid", "linear"][1], efd, "linear", U, "bands")


def test_form_from_the_environment_changes_no_result(gpu_ctx, mifc_env):
    case = vc.main("field", 2, 12, 9, 16, 7, 3)
    ref, rfd = run(gpu_ctx, case, "linear", "last", "clamp")
    assert front().last_vregrid_form(gpu_ctx)["v"] == 1 and front().last_vregrid_form(gpu_ctx)["passes"] == 1
    for v, tb in ((None, 3), (4, 3), (4, None), (1, 2)):
        mifc_env("MIFC_VREGRID_V", v)
        mifc_env("MIFC_VREGRID_TB", tb)
        out, fd = run(gpu_ctx, case, "linear", "last", "clamp")
        form = front().last_vregrid_form(gpu_ctx)
        assert form["v"] == (4 if v == 4 else 1) and form["tb"] == (tb or 15) and form["passes"] == -(-7 // (tb or 15)), form
        assert same_bits(out, ref, nan_payload=False) and np.array_equal(fd, rfd)


def test_one_batch_drops_the_leading_axis(gpu_ctx):
    case = vc.main("hybrid", 1)
    exp, efd = vc.expected(case, "linear")
    out, fd = front().vregrid_hlevels(gpu_ctx, case["fields"][0], case["coord"], case["ab"][0], case["ab"][1], list(case["tcoord"]))
    assert out.shape == (5, 9, 13) and fd.shape == (5,) and same_bits(out, exp[0], nan_payload=False) and list(fd) == list(efd[0])
    out, fd = front().vregrid_hlevels(gpu_ctx, case["fields"][0], case["coord"], case["ab"][0], case["ab"][1], case["tcoord"][2])
    assert out.shape == (1, 9, 13) and same_bits(out[0], exp[0, 2], nan_payload=False) and list(fd) == [efd[0, 2]]


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx, nt = 2, 4, 3, 8, 3
    hyb, fld = vc.main("hybrid", nf, nlev, ny, nx, nt, 2), vc.main("field", nf, nlev, ny, nx, nt, 2)
    ab = hyb["ab"]
    x = torch.from_numpy(hyb["fields"]).cuda()
    ps, coord, tc = torch.from_numpy(hyb["coord"]).cuda(), torch.from_numpy(fld["coord"]).cuda(), torch.from_numpy(hyb["tcoord"]).cuda()
    levels_h = np.array([100, 200, 400, 800], np.float32)
    sentinel = -4242.5
    outs = torch.full((nf, nt, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    cells = ny * nx

    def call(kind, nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, nt_=nt, method=0, from_=0, outside=0, fields=None, out_ptrs=None, coord_ptr=0, a=None, b=None, tg=True,
             fd_out=True, levels=levels_h, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        al, bl = (np.asarray(own if v in (None, "null") else v, np.float32) for v, own in ((a, ab[0]), (b, ab[1])))
        lv = np.asarray(levels, np.float32)
        fd = np.full(nf * nt, 7, np.int32)
        common = [tc.data_ptr() if tg is True else tg, None, nt_, method, from_, outside, None if isinstance(out_ptrs, str) else ctypes.addressof(o),
                  fd.ctypes.data if fd_out else None, float(U), 1]
        head = [c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_]
        if kind == "hybrid":
            cp = ps.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vregrid_hlevels(*head, cp, vg.SOME_DEFINED, None if isinstance(a, str) else al.ctypes.data, None if isinstance(b, str) else bl.ctypes.data,
                                          *common)
        elif kind == "field":
            cp = coord.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vregrid_fields(*head, cp, None, *common)
        else:
            rc = lib.mifc_vregrid_levels(*head, lv.ctypes.data if coord_ptr == 0 else coord_ptr, *common)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    nan = float("nan")
    heads = {"hybrid": "a null pointer (fields, ps, alevel, blevel, tcoord, fres or fdefined_out)", "field": "a null pointer (fields, coord, tcoord, fres or fdefined_out)",
             "levels": "a null pointer (fields, levels, tcoord, fres or fdefined_out)"}
    no_level = "level %d: alevel / blevel are no hybrid level (FieldCalculations.cc:298)"
    every = {
        "nlev < 2": (dict(nlev_=1), "nlev < 2"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "ntargets 0": (dict(nt_=0), "ntargets 0 outside 1..256"),
        "ntargets 257": (dict(nt_=257), "ntargets 257 outside 1..256"),
        "negative nx": (dict(nx_=-1), "a negative nx or ny"),
        "negative ny": (dict(ny_=-2), "a negative nx or ny"),
        "null fields": (dict(fields="null"), None),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or fres[1])"),
        "null coordinate": (dict(coord_ptr=None), None),
        "null tcoord": (dict(tg=None), None),
        "null fres": (dict(out_ptrs="null"), None),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None]), "a null pointer (fields[1] or fres[1])"),
        "null flags out": (dict(fd_out=False), None),
        "unknown method": (dict(method=2), "unknown method 2 (MIFC_VINTERP_LINEAR or MIFC_VINTERP_LOG)"),
        "unknown from": (dict(from_=2), "unknown from 2 (MIFC_VREGRID_FROM_FIRST or MIFC_VREGRID_FROM_LAST)"),
        "unknown outside": (dict(outside=-1), "unknown outside -1 (MIFC_VREGRID_OUTSIDE_UNDEF or MIFC_VREGRID_OUTSIDE_CLAMP)"),
        "output is an input": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output inside tcoord": (dict(out_ptrs=[tc.data_ptr() + 4 * (nt * cells - 1), outs[1].data_ptr()]), "fres[0] overlaps tcoord"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr() + 4 * (nt * cells - 1)]), "fres[0] overlaps fres[1]"),
    }
    only = {
        "hybrid": {
            "null alevel": (dict(a="null"), None),
            "null blevel": (dict(b="null"), None),
            "negative alevel": (dict(a=[1.0, -1.0, 2.0, 0.0]), no_level % 1),
            "blevel > 1": (dict(b=[0.0, 0.1, 0.2, 1.5]), no_level % 3),
            "output overlaps ps": (dict(out_ptrs=[outs[0].data_ptr(), ps.data_ptr() + 4 * (cells - 1)]), "fres[1] overlaps ps"),
        },
        "field": {"output overlaps coord": (dict(out_ptrs=[coord.data_ptr() + 4 * (nlev * cells - 1), outs[1].data_ptr()]), "fres[0] overlaps coord")},
        "levels": {"NaN level": (dict(levels=[100, nan, 400, 800]), "levels[1] is NaN")},
    }
    before = {k: t.clone() for k, t in (("x", x), ("ps", ps), ("coord", coord), ("tc", tc))}
    for kind in ("hybrid", "field", "levels"):
        for what, (kw, tail) in {**every, **only[kind]}.items():
            rc, err, fd = call(kind, **kw)
            assert rc == 0 and err == "mifc_vregrid_%s: " % {"hybrid": "hlevels", "field": "fields", "levels": "levels"}[kind] + (tail or heads[kind]), (kind, what, err)
            assert (outs == sentinel).all().item() and (fd == 7).all(), (kind, what)
    assert all(torch.equal(t, before[k]) for k, t in (("x", x), ("ps", ps), ("coord", coord), ("tc", tc)))
    with pytest.raises(front().Refused, match="unknown method"):
        front().vregrid_fields(gpu_ctx, x, coord, tc, method="cubic")
    with pytest.raises(front().Refused, match="unknown outside"):
        front().vregrid_levels(gpu_ctx, x, levels_h, tc, outside="nearest")
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        refused = [call(kind, sync=False) for kind in ("hybrid", "field", "levels")]
    g.close()
    for rc, err, fd in refused:
        assert rc == 0 and "capture" in err and (fd == 7).all()
    assert (outs == sentinel).all().item()
    # no cells: the flags, nothing else
    for kind in ("hybrid", "field", "levels"):
        rc, err, fd = call(kind, nx_=0)
        assert rc == 1 and err == "" and (fd == vg.ALL_DEFINED).all() and (outs == sentinel).all().item()
    # afterwards the same calls run
    for kind in ("hybrid", "field", "levels"):
        rc, err, fd = call(kind)
        assert rc == 1 and err == "" and (fd != 7).all()
    assert not (outs == sentinel).any().item()
