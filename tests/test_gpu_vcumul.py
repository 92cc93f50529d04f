"""Running vertical integrals of level batches on the GPU (mifc_vcumul.hip, mifc_vcumul_hlevels / mifc_vcumul_fields /
mifc_vcumul_levels, through mi_fieldcalc_amd.vcumul) against the numpy restatement (tests/vcumul_restate.py).  LINEAR: bit
for bit (a NaN matches any NaN), flags equal -- every operation of the definition is an IEEE float or double operation
rounded on its own, and the library is built without contraction.  LOG: the device's double log() may differ from the
host's in the last bit, so with integrands of one sign (no cancellation: the relative error of S is of order nlev * 2^-52)
a result is the restatement's float or its neighbour; undef cells and flags are exact."""
import ctypes
import functools

import numpy as np
import pytest

import vcumul_restate as vc
import vinterp_restate as vi
import vlayer_restate as vl
from cases import same_bits

pytestmark = pytest.mark.gpu

MIXED = [vc.ALL_DEFINED, vc.SOME_DEFINED, vc.NONE_DEFINED]
KINDS = ("hybrid", "field", "levels")
METHODS = (("linear", vc.LINEAR), (vc.LOG, vc.LOG))  # (what the call is given: a name or a code, what the restatement is)
FROMS = (("first", vc.FROM_FIRST), (vc.FROM_LAST, vc.FROM_LAST))
U = vc.UNDEF


def front():
    from mi_fieldcalc_amd import vcumul

    return vcumul


def compare(got, exp, gfd, efd, method, label):
    assert got.shape == exp.shape, label
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if method == vc.LINEAR:
        if same_bits(got, exp, nan_payload=False):
            return
        ok = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
    else:
        undef = exp.view(np.uint32) == np.float32(U).view(np.uint32)  # exact where the restatement left undef, and nowhere else
        ok = np.where(undef | (got.view(np.uint32) == np.float32(U).view(np.uint32)), got.view(np.uint32) == exp.view(np.uint32), vc.neighbours(got, exp))
    if not ok.all():
        bad = np.nonzero(~ok)
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))


def run(ctx, kind, fields, coord, method, from_, device, ab=None, stacked=True, start=None, base=None, **kw):
    import torch

    # (np.array: a writable copy, the cached cases are read-only)
    put = (lambda a: None if a is None else torch.from_numpy(np.array(a, np.float32)).cuda()) if device else (lambda a: None if a is None else np.ascontiguousarray(a))
    f = put(fields)
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    kw = dict(kw, start=put(start), base=None if base is None else [put(b) for b in base])
    if "fdef_c" in kw:
        kw["fdef_ps" if kind == "hybrid" else "fdef_coord"] = kw.pop("fdef_c")
    if kind == "hybrid":
        res = front().vcumul_hlevels(ctx, f, put(coord), ab[0], ab[1], method, from_, **kw)
    elif kind == "field":
        res = front().vcumul_fields(ctx, f, put(coord), method, from_, **kw)
    else:
        res = front().vcumul_levels(ctx, f, coord, method, from_, **kw)
    return tuple(r.cpu().numpy() if device and not isinstance(r, np.ndarray) else r for r in res)


def expected(kind, fields, coord, method, from_, ab=None, **kw):
    kw = dict(kw)
    flags = kw.pop("fdefined_in", None)
    if flags is not None and np.size(flags) == len(fields):  # one flag per field stands for every level
        flags = np.repeat(np.asarray(flags).reshape(-1, 1), fields.shape[1], axis=1)
    fdef_c = kw.pop("fdef_c", None)
    if kind == "hybrid":
        return vc.hlevels(fields, coord, ab[0], ab[1], method, from_, flags, vc.SOME_DEFINED if fdef_c is None else fdef_c, **kw)
    if kind == "field":
        return vc.coord_fields(fields, coord, method, from_, flags, fdef_c, **kw)
    return vc.levels(fields, coord, method, from_, flags, **kw)


def check(ctx, kind, fields, coord, method, from_, device, label=None, form=None, stacked=True, **kw):
    got = run(ctx, kind, fields, coord, method[0], from_[0], device, stacked=stacked, **kw)
    exp = expected(kind, fields, coord, method[1], from_[1], **kw)
    compare(got[0], exp[0], got[1], exp[1], method[1], (label, kind, method[1], from_[1], "device" if device else "host", sorted(kw)))
    if form is not None:
        seen = front().last_vcumul_form(ctx)
        want = dict(form, method="log" if method[1] else "linear")
        want["from"] = "last" if from_[1] else "first"
        assert {k: seen[k] for k in want} == want, (label, kind, seen, want)


@functools.lru_cache(maxsize=None)
def case(nf=3, nlev=12, ny=9, nx=13, seed=1):
    """The main generator: fields, ps, (alevel, blevel), the pressure of the levels as a coordinate batch, pressure levels
    for the `levels` form, a start plane per walk direction and the base planes."""
    fields, ps, ab, coord, starts, base = vc.cumul_case(nf, nlev, ny, nx, seed)
    levs = vc.main_levels(nlev)
    for a in (fields, ps, ab[0], ab[1], coord, levs, starts, base):
        a.setflags(write=False)
    return fields, ps, ab, coord, levs, starts, base


def options(c, from_, full):
    """The optional arguments of a call on case c: none, or a start on the near side of the walk, base planes (one absent)
    and positive factors."""
    if not full:
        return {}
    nf = len(c[0])
    base = [None if f == 1 else c[6][f] for f in range(nf)]
    return dict(start=c[5][from_[1]], base=base, scale=[0.25 + 1.5 * f for f in range(nf)])


def all_kinds(ctx, c, method, from_, device, full, **kw):
    fields, ps, ab, coord, levs = c[:5]
    kw = dict(kw, **options(c, from_, full))
    check(ctx, "hybrid", fields, ps, method, from_, device, ab=ab, **kw)
    check(ctx, "field", fields, coord, method, from_, device, **kw)
    check(ctx, "levels", fields, levs, method, from_, device, **kw)


def sweep(ctx, c, device, **kw):
    """Both methods, both directions, without and with start / base / scale."""
    for method in METHODS:
        for from_ in FROMS:
            for full in (False, True):
                all_kinds(ctx, c, method, from_, device, full, **kw)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8])  # a launch takes 4 fields
def test_main_case_fields_per_pass_and_memory(gpu_ctx, nf, device):
    launches = (nf + 3) // 4
    sweep(gpu_ctx, case(nf), device, stacked=(nf != 3), label=("nf", nf), form=dict(v=4 if not device else 1, fields=min(nf, 4), launches=launches))


@pytest.mark.parametrize("shape,v", [((2, 9, 13), 1), ((3, 9, 13), 1), ((5, 9, 13), 1), ((12, 5, 1), 1), ((12, 7, 16), 4), ((5, 3, 300), 4)],
                         ids=["nlev2", "nlev3", "nlev5", "nx1", "nx16", "nx300"])
def test_shapes_and_forms(gpu_ctx, shape, v):
    nlev, ny, nx = shape  # nlev 2: the peeled first position and one step; 3 and 5: the remainders of the slot rotation; a device batch
    c = case(3, nlev, ny, nx, 7)  # takes four cells per lane where its levels are a multiple of four cells, a staged band always
    sweep(gpu_ctx, c, True, label=shape, form=dict(v=v, fields=3, launches=1))
    sweep(gpu_ctx, c, False, label=shape, form=dict(v=4, fields=3, launches=1))


def test_vector_form_over_several_workgroups(gpu_ctx):
    c = case(2, 4, 3, 1100)  # 3300 cells, a multiple of 4: four workgroups of 1024 cells, the last one partly empty
    sweep(gpu_ctx, c, True, label="vec4 blocks", form=dict(v=4, fields=2, launches=1))
    c = case(5, 3, 7, 191)  # 1337 cells, one per lane: six workgroups, two launches
    sweep(gpu_ctx, c, True, label="scalar blocks", form=dict(v=1, fields=4, launches=2))


def test_more_levels_than_the_workgroup_counters_hold(gpu_ctx):
    c = case(2, 2049, 1, 8)  # 4 fields x 2049 levels of counters are more than 32 KiB of LDS: the waves add to the global counters
    for from_ in FROMS:
        all_kinds(gpu_ctx, c, METHODS[0], from_, True, True, label="2049 levels", form=dict(v=4, fields=2, launches=1))
    c = case(2, 2048, 1, 5)  # the most that fit, one cell per lane
    all_kinds(gpu_ctx, c, METHODS[1], FROMS[1], True, False, label="2048 levels", form=dict(v=1, fields=2, launches=1))


def test_device_batch_offset_by_one_float(gpu_ctx):
    import torch

    fields, ps, ab, coord, levs, starts, base = case(2, 12, 9, 16)
    n = fields[0].size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1).copy()).cuda()
    batches = [buf[1 + j * n:1 + (j + 1) * n].view(12, 9, 16) for j in range(2)]  # 4 bytes past the 16-byte grid
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    out, fd = front().vcumul_hlevels(gpu_ctx, batches, dev(ps), ab[0], ab[1], "linear", "last", start=dev(starts[1]), base=[dev(base[0]), None], scale=[2.0, -0.5])
    assert front().last_vcumul_form(gpu_ctx)["v"] == 1
    exp, efd = vc.hlevels(fields, ps, ab[0], ab[1], vc.LINEAR, vc.FROM_LAST, start=starts[1], base=[base[0], None], scale=[2.0, -0.5])
    compare(out.cpu().numpy(), exp, fd, efd, vc.LINEAR, "offset inputs")
    obuf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")  # and an output off the grid
    out, fd = front().vcumul_levels(gpu_ctx, dev(fields), levs, out=obuf[1:].view(2, 12, 9, 16))
    assert front().last_vcumul_form(gpu_ctx)["v"] == 1
    exp, efd = vc.levels(fields, levs)
    compare(out.cpu().numpy(), exp, fd, efd, vc.LINEAR, "offset output")
    sbuf = torch.zeros(9 * 16 + 1, dtype=torch.float32, device="cuda")  # and a start plane off the grid
    sbuf[1:] = dev(starts[0]).reshape(-1)
    out, fd = front().vcumul_fields(gpu_ctx, dev(fields), dev(coord), start=sbuf[1:].view(9, 16))
    assert front().last_vcumul_form(gpu_ctx)["v"] == 1
    exp, efd = vc.coord_fields(fields, coord, start=starts[0])
    compare(out.cpu().numpy(), exp, fd, efd, vc.LINEAR, "offset start")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mixed_flags_over_undef_and_nan(gpu_ctx, device):
    c = case(4)
    fields, ps, ab, coord, levs, starts, base = c
    rng = np.random.default_rng(3)
    fields = vc.sprinkle(fields, rng, 0.03, np.nan)
    coord = vc.sprinkle(coord, rng, 0.01, np.nan)
    ps = vc.sprinkle(ps, rng, 0.05, np.nan)
    starts = vc.sprinkle(starts, rng, 0.05, np.nan)
    base = vc.sprinkle(base, rng, 0.05, np.nan)
    flags = rng.choice(MIXED, size=(4, 12)).astype(np.int32)
    fdef_coord = rng.choice(MIXED, size=12).astype(np.int32)
    fdef_base = np.array([vc.ALL_DEFINED, vc.SOME_DEFINED, vc.NONE_DEFINED, vc.ALL_DEFINED], np.int32)
    for method in METHODS:
        for from_ in FROMS:
            opts = dict(start=starts[from_[1]], base=list(base), fdef_base=fdef_base, scale=[1.0, 2.0, 0.5, 3.0], fdefined_in=flags, label="flags")
            for flag in MIXED:
                check(gpu_ctx, "hybrid", fields, ps, method, from_, device, ab=ab, fdef_c=flag, fdef_start=flag, **opts)
            check(gpu_ctx, "field", fields, coord, method, from_, device, fdef_c=fdef_coord, **opts)
            check(gpu_ctx, "field", fields, coord, method, from_, device, fdef_c=[vc.ALL_DEFINED] * 12, fdef_start=vc.ALL_DEFINED, **opts)
            check(gpu_ctx, "levels", fields, levs, method, from_, device, **opts)
            check(gpu_ctx, "levels", fields, levs, method, from_, device, fdefined_in=[vc.ALL_DEFINED] * 4, label="one flag per field")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nan_as_undef(gpu_ctx, device):
    nan = np.float32(np.nan)
    c = case(2)
    c = tuple(np.where(a == U, nan, a) if isinstance(a, np.ndarray) and a.ndim >= 2 else a for a in c)
    sweep(gpu_ctx, c, device, undef=nan, label="undef = NaN")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_holes_at_the_first_and_the_last_walked_level(gpu_ctx, device):
    fields, ps, ab, coord, levs, starts, base = case(2, 5, 7, 16, 3)
    for where in (0, 4):
        x = fields.copy()
        x[0, where, 2:5] = U  # field 0 only, three rows of cells
        x[1, where, 3, 5] = np.nan
        for method in METHODS:
            for from_ in FROMS:
                out, fd = run(gpu_ctx, "field", x, coord, method[0], from_[0], device)
                exp, efd = vc.coord_fields(x, coord, method[1], from_[1])
                compare(out, exp, fd, efd, method[1], ("hole at", where, method[1], from_[1]))
                walked_first = where == (0 if from_[1] == vc.FROM_FIRST else 4)
                assert (out[0, :, 2:5] == U).all() == walked_first and (out[0, where, 2:5] == U).all() and np.isnan(out[1, where, 3, 5]) == False  # noqa: E712
                assert (out[1, :, 3, 5] == U).all() == walked_first and out[1, where, 3, 5] == U


def test_host_call_in_several_bands(gpu_ctx, mifc_env):
    mifc_env("MIFC_VCUMUL_CHUNK_MIB", 1)
    # field form with start and two bases: 2 * 9 + 9 + 1 + 2 + 2 * 9 = 48 planes of 257 floats per row: 21 rows per MiB, so 64
    # rows go in four bands, the last one of one row
    c = case(2, 9, 64, 257, 9)
    for method in METHODS:
        for from_ in FROMS:
            kw = dict(start=c[5][from_[1]], base=list(c[6]), scale=[1.0, 0.5])
            check(gpu_ctx, "field", c[0], c[3], method, from_, False, label="bands", form=dict(v=4, fields=2, launches=4), **kw)
            check(gpu_ctx, "hybrid", c[0], c[1], method, from_, False, ab=c[2], label="bands", form=dict(v=4, fields=2, launches=3), **kw)  # 40 planes: 25 rows
    check(gpu_ctx, "levels", c[0], c[4], METHODS[0], FROMS[1], False, label="bands", form=dict(v=4, fields=2, launches=3))  # 36 planes: 28 rows


def test_host_band_of_one_row_that_exceeds_the_budget(gpu_ctx, mifc_env):
    mifc_env("MIFC_VCUMUL_CHUNK_MIB", 1)
    # 2 * 12 + 1 + 1 + 2 + 2 * 12 = 52 planes of 5100 floats per row are 1060800 bytes, more than the MiB: the band cannot be less
    # than one row, so the three rows go one at a time, each plane of 5100 floats padded to 5120
    c = case(2, 12, 3, 5100, 9)
    for method in METHODS:
        check(gpu_ctx, "hybrid", c[0], c[1], method, FROMS[1], False, ab=c[2], start=c[5][1], base=list(c[6]), label="one-row bands",
              form=dict(v=4, fields=2, launches=3))


def test_last_level_is_the_layer_integral_of_vlayer_on_the_device(gpu_ctx):
    """Strictly ascending coordinate, everything defined, from the first level, no start, base or scale: the last level of
    the running integral and mifc_vlayer_fields' INTEGRAL over the open layer are the same additions in the same order."""
    import torch

    fields, ps, alevel, blevel = vi.main_case(3, 12, 9, 16, 5, frac=0.0)
    coord = vi.hybrid_coordinate(ps, alevel, blevel)
    assert (np.diff(coord, axis=0) > 0).all()
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    for f, co, place in ((fields, coord, "host"), (dev(fields), dev(coord), "device")):
        run_, fd = front().vcumul_fields(gpu_ctx, f, co)
        layer, lfd = gpu_ctx.vlayer_fields(f, co, ["integral"])
        if place == "device":
            run_, layer = run_.cpu().numpy(), layer.cpu().numpy()
        assert run_[:, -1].tobytes() == layer[:, 0].tobytes() and (fd == vc.ALL_DEFINED).all() and (lfd == vc.ALL_DEFINED).all(), place
        exp, _ = vl.coord_fields(fields, coord, [vl.INTEGRAL])
        assert run_[:, -1].tobytes() == exp[:, 0].tobytes()


def test_one_batch_drops_the_leading_axis_and_out_is_honoured(gpu_ctx):
    import torch

    fields, ps, ab, coord, levs, starts, base = case(2)
    exp, efd = vc.hlevels(fields, ps, ab[0], ab[1], base=list(base))
    out, fd = front().vcumul_hlevels(gpu_ctx, fields[0], ps, ab[0], ab[1], base=base[0])
    assert out.shape == (12, 9, 13) and fd.shape == (12,) and same_bits(out, exp[0], nan_payload=False) and list(fd) == list(efd[0])
    o = torch.empty((12, 9, 13), dtype=torch.float32, device="cuda")
    out, fd = front().vcumul_fields(gpu_ctx, torch.from_numpy(fields[1].copy()).cuda(), torch.from_numpy(coord.copy()).cuda(), 0, 1, out=o)
    e1, e1fd = vc.coord_fields(fields[1:], coord, vc.LINEAR, vc.FROM_LAST)
    assert out is o and same_bits(o.cpu().numpy(), e1[0], nan_payload=False) and list(fd) == list(e1fd[0])
    o = np.full((2, 12, 9, 13), -1, np.float32)
    out, fd = front().vcumul_levels(gpu_ctx, [fields[0], fields[1]], levs, scale=-2.0, out=o)
    e2, e2fd = vc.levels(fields, levs, scale=[-2.0, -2.0])
    assert out is o and same_bits(o, e2, nan_payload=False) and fd.shape == (2, 12) and np.array_equal(fd, e2fd)


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx = 2, 4, 3, 8
    fields_h, ps_h, ab, coord_h, levs, starts_h, base_h = case(nf, nlev, ny, nx, 2)
    x = torch.from_numpy(fields_h.copy()).cuda()
    batch, plane = nlev * ny * nx, ny * nx
    # the planes between two batches of the test's own: an output that ends in the first plane begins in the batch in front of them, one
    # that begins in the last plane ends in the batch behind them, whatever else the allocator has put nearby
    room = torch.zeros(2 * batch + 4 * plane, dtype=torch.float32, device="cuda")
    bases = room[batch:batch + 2 * plane].view(2, ny, nx).copy_(torch.from_numpy(base_h.copy()))
    start = room[batch + 2 * plane:batch + 3 * plane].view(ny, nx).copy_(torch.from_numpy(starts_h[0].copy()))
    ps = room[batch + 3 * plane:batch + 4 * plane].view(ny, nx).copy_(torch.from_numpy(ps_h.copy()))
    coord = torch.from_numpy(coord_h.copy()).cuda()
    sentinel = -4242.5
    outs = torch.full((nf, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")

    def call(kind, nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, method=0, from_=0, fields=None, out_ptrs=None, coord_ptr=0, a=None, b=None, lv=None,
             scale=None, fd_out=True, with_start=True, with_base=True, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        bt = (ctypes.c_void_p * nf)(*[bases[f].data_ptr() for f in range(nf)])
        al, bl = (np.asarray(own if v in (None, "null") else v, np.float32) for v, own in ((a, ab[0]), (b, ab[1])))
        lev = np.asarray(levs if lv is None else lv, np.float32)
        sc = None if scale is None else np.asarray(scale, np.float64)
        fd = np.full(nf * nlev, 7, np.int32)
        tail = [method, from_, start.data_ptr() if with_start else None, vc.SOME_DEFINED, ctypes.addressof(bt) if with_base else None, None,
                None if sc is None else sc.ctypes.data, None if out_ptrs == "null" else ctypes.addressof(o), fd.ctypes.data if fd_out else None, float(U), 1]
        head = [c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_]
        if kind == "hybrid":
            cp = ps.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vcumul_hlevels(*head, cp, vc.SOME_DEFINED, None if isinstance(a, str) else al.ctypes.data,
                                         None if isinstance(b, str) else bl.ctypes.data, *tail)
        elif kind == "field":
            cp = coord.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vcumul_fields(*head, cp, None, *tail)
        else:
            rc = lib.mifc_vcumul_levels(*head, lev.ctypes.data if coord_ptr == 0 else coord_ptr, *tail)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    # what: (the arguments, the message behind "<entry name>: "; one per kind where the kinds word it differently)
    null_head = {"hybrid": "a null pointer (fields, ps, alevel or blevel)", "field": "a null pointer (fields or coord)",
                 "levels": "a null pointer (fields or levels)"}
    no_level = "level %d: alevel / blevel are no hybrid level (FieldCalculations.cc:298)"
    every = {
        "nlev < 2": (dict(nlev_=1), "nlev < 2"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "negative nx": (dict(nx_=-1), "a negative nx or ny"),
        "negative ny": (dict(ny_=-2), "a negative nx or ny"),
        "unknown method 2": (dict(method=2), "unknown method 2"),
        "negative method": (dict(method=-1), "unknown method -1"),
        "unknown from 2": (dict(from_=2), "unknown from 2"),
        "negative from": (dict(from_=-1), "unknown from -1"),
        "null fields": (dict(fields="null"), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or fres[1])"),
        "null coordinate": (dict(coord_ptr=None), null_head),
        "null fres": (dict(out_ptrs="null"), "a null pointer (fres or fdefined_out)"),
        "null fdefined_out": (dict(fd_out=False), "a null pointer (fres or fdefined_out)"),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None]), "a null pointer (fields[1] or fres[1])"),
        "NaN scale": (dict(scale=[1.0, np.nan]), "scale[1] is NaN"),
        "output is an input": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output inside an input": (dict(out_ptrs=[x[0].data_ptr() + 4 * (batch - 1), outs[1].data_ptr()]), "fres[0] overlaps fields[0]"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr() + 4 * (batch - 1)]), "fres[0] overlaps fres[1]"),
        "output ends in start": (dict(out_ptrs=[outs[0].data_ptr(), start.data_ptr() - 4 * (batch - 1)]), "fres[1] overlaps start"),  # (the bases too)
        "output ends in a base plane": (dict(out_ptrs=[bases[0].data_ptr() - 4 * (batch - 1), outs[1].data_ptr()]), "fres[0] overlaps base[0]"),
    }
    only = {
        "hybrid": {
            "null alevel": (dict(a="null"), null_head),
            "null blevel": (dict(b="null"), null_head),
            "negative alevel": (dict(a=[1.0, -1.0, 2.0, 0.0]), no_level % 1),
            "blevel > 1": (dict(b=[0.0, 0.1, 0.2, 1.5]), no_level % 3),
            "output overlaps ps": (dict(out_ptrs=[outs[0].data_ptr(), ps.data_ptr() + 4 * (plane - 1)], with_start=False, with_base=False), "fres[1] overlaps ps"),
        },
        "field": {"output overlaps coord": (dict(out_ptrs=[coord.data_ptr() + 4 * (batch - 1), outs[1].data_ptr()]), "fres[0] overlaps coord")},
        "levels": {
            "NaN level": (dict(lv=[100, float("nan"), 300, 400]), "levels[1] is NaN"),
            "LOG with a zero level": (dict(lv=[0.0, 100, 300, 400], method=1), "levels[0] <= 0 with MIFC_VCUMUL_LOG"),
            "LOG with a negative level": (dict(lv=[100, 200, -300, 400], method=1), "levels[2] <= 0 with MIFC_VCUMUL_LOG"),
        },
    }
    for kind, name in (("hybrid", "mifc_vcumul_hlevels: "), ("field", "mifc_vcumul_fields: "), ("levels", "mifc_vcumul_levels: ")):
        before = room.clone(), x.clone(), coord.clone()
        for what, (kw, tail) in {**every, **only[kind]}.items():
            rc, err, fd = call(kind, **kw)
            assert rc == 0 and err == name + (tail[kind] if isinstance(tail, dict) else tail), (kind, what, err)
            assert (outs == sentinel).all().item() and (fd == 7).all(), (kind, what)
        assert torch.equal(room, before[0]) and torch.equal(x, before[1]) and torch.equal(coord, before[2])
    rc, err, fd = call("levels", lv=[0.0, 100, -300, 400])  # LINEAR takes any level that is a number
    assert rc == 1 and err == "" and (fd != 7).all()
    outs.fill_(sentinel)
    with pytest.raises(ValueError, match="mifc_vcumul_hlevels: unknown method -1"):
        front().vcumul_hlevels(gpu_ctx, x, ps, ab[0], ab[1], "spline")
    with pytest.raises(RuntimeError, match="unknown from 7"):
        front().vcumul_levels(gpu_ctx, x, levs, from_=7)
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        refused = [call(kind, sync=False) for kind in KINDS]
    g.close()
    for rc, err, fd in refused:
        assert rc == 0 and "capture" in err and (fd == 7).all()
    assert (outs == sentinel).all().item()
    # afterwards the same calls run
    for kind in KINDS:
        rc, err, fd = call(kind)
        assert rc == 1 and err == "" and (fd != 7).all(), (kind, err)
    exp, efd = vc.levels(fields_h, levs, start=starts_h[0], base=list(base_h))
    compare(outs.cpu().numpy(), exp, fd.reshape(nf, nlev), efd, vc.LINEAR, "after the refusals")


def test_empty_grid(gpu_ctx):
    x = np.zeros((2, 3, 0, 5), np.float32)
    out, fd = front().vcumul_fields(gpu_ctx, x, np.zeros((3, 0, 5), np.float32), "log", "last", start=np.zeros((0, 5), np.float32))
    assert out.shape == (2, 3, 0, 5) and fd.shape == (2, 3) and (fd == vc.ALL_DEFINED).all()
    out, fd = front().vcumul_levels(gpu_ctx, x[0], [100, 200, 300])
    assert out.shape == (3, 0, 5) and fd.shape == (3,) and (fd == vc.ALL_DEFINED).all()


def test_height_of_model_levels_then_height_surfaces_on_the_device(gpu_ctx):
    """The chain the operator exists for, device tensors throughout: an isothermal atmosphere on nine hybrid levels over
    varying ps and zs -> geopotential_height_hlevels, which must be the closed form zs + (Rd T0 / g) ln(ps / c_k) (evaluated
    in float64 from the float32 c_k and rounded to float) exactly or to the neighbouring float -> that height batch, still
    on the device, as the coordinate of Context.vinterp_fields for three height surfaces: bit for bit vinterp_restate on
    the same numbers."""
    import torch

    from mi_fieldcalc_amd._consts import GRAVITY, R_DRY

    rng = np.random.default_rng(31)
    nlev, ny, nx, t0 = 9, 9, 16, 250.0
    alevel, blevel = vc.hybrid_levels(nlev)
    ps = rng.uniform(700, 1050, (ny, nx)).astype(np.float32)
    zs = rng.uniform(0, 2500, (ny, nx)).astype(np.float32)
    c = vc.hybrid_coordinate(ps, alevel, blevel)
    t = np.full((nlev, ny, nx), t0, np.float32)
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    z, zfd = front().geopotential_height_hlevels(gpu_ctx, dev(t), None, dev(ps), alevel, blevel, zs=dev(zs))
    assert z.is_cuda and z.shape == (nlev, ny, nx) and (zfd == vc.ALL_DEFINED).all()
    assert front().last_vcumul_form(gpu_ctx) == {"v": 4, "fields": 1, "method": "log", "from": "last", "launches": 1}
    closed = (zs.astype(np.float64) + (R_DRY * t0 / GRAVITY) * np.log(ps.astype(np.float64) / c.astype(np.float64))).astype(np.float32)
    zh = z.cpu().numpy()
    near = vc.neighbours(zh, closed)
    print("height: exact %d, neighbour %d of %d; range %.1f .. %.1f m" % ((zh == closed).sum(), (near & (zh != closed)).sum(), zh.size, zh.min(), zh.max()))
    assert near.all(), (zh[~near][:4], closed[~near][:4])
    assert (np.diff(zh, axis=0) < 0).all() and (zh[-1] == zs).all()  # top-down: the lowest level is the surface itself (c = ps)
    # a dry atmosphere with moisture given: q = 0 leaves Tv = t
    z2, _ = front().geopotential_height_hlevels(gpu_ctx, dev(t), dev(np.zeros_like(t)), dev(ps), alevel, blevel, zs=dev(zs))
    assert torch.equal(z, z2)
    # the wind on three height surfaces, interpolated in that height batch
    u = rng.normal(5, 12, (nlev, ny, nx)).astype(np.float32)
    targets = np.array([1500, 3000, 5500], np.float32)
    on_z, fd = gpu_ctx.vinterp_fields(dev(u), z, targets, fdef_coord=zfd)
    exp, efd = vi.coord_fields(u[None], zh, targets, vi.LINEAR, fdef_coord=list(zfd))
    assert on_z.is_cuda and same_bits(on_z.cpu().numpy(), exp[0], nan_payload=False) and list(fd) == list(efd[0])
    assert (exp[0][1:] != U).all() and (exp[0][0] == U).any() and (exp[0][0] != U).any()  # 1500 m is below the ground in places
