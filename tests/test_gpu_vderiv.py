"""Vertical derivatives of level batches on the GPU (mifc_vderiv.hip, mifc_vderiv_hlevels / mifc_vderiv_fields /
mifc_vderiv_levels) against the numpy restatement (tests/vderiv_restate.py): bit for bit (a NaN matches any NaN), flags
equal, all three coordinate forms, both methods, host and device memory.  No tolerance: every operation of the definition
is an IEEE float or double operation rounded on its own, and the library is built without contraction."""
import ctypes
import functools

import numpy as np
import pytest

import vderiv_restate as vd
import vinterp_restate as vi
from cases import same_bits

pytestmark = pytest.mark.gpu

MIXED = [vd.ALL_DEFINED, vd.SOME_DEFINED, vd.NONE_DEFINED]
KINDS = ("hybrid", "field", "levels")
METHODS = (("centred", vd.CENTRED), (vd.WEIGHTED, vd.WEIGHTED))  # (what the call is given: a name or a code, what the restatement is)


def compare(got, exp, gfd, efd, label):
    assert got.shape == exp.shape, label
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if not same_bits(got, exp, nan_payload=False):
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))


def run(ctx, kind, fields, coord, method, device, flags=None, fdef_c=None, undef=vd.UNDEF, ab=None, stacked=True, magnitude=None):
    import torch

    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    f = put(fields)
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    if kind == "hybrid":
        res = ctx.vderiv_hlevels(f, put(coord), ab[0], ab[1], method, magnitude, fdefined_in=flags,
                                 fdef_ps=vd.SOME_DEFINED if fdef_c is None else fdef_c, undef=undef)
    elif kind == "field":
        res = ctx.vderiv_fields(f, put(coord), method, magnitude, fdefined_in=flags, fdef_coord=fdef_c, undef=undef)
    else:
        res = ctx.vderiv_levels(f, coord, method, magnitude, fdefined_in=flags, undef=undef)
    return tuple(r.cpu().numpy() if device and not isinstance(r, np.ndarray) else r for r in res)


def expected(kind, fields, coord, method, flags=None, fdef_c=None, undef=vd.UNDEF, ab=None, magnitude=None):
    mag = magnitude is not None
    if flags is not None and np.size(flags) == len(fields):  # one flag per field stands for every level
        flags = np.repeat(np.asarray(flags).reshape(-1, 1), fields.shape[1], axis=1)
    if kind == "hybrid":
        res = vd.hlevels(fields, coord, ab[0], ab[1], method, flags, vd.SOME_DEFINED if fdef_c is None else fdef_c, undef, mag)
    elif kind == "field":
        res = vd.coord_fields(fields, coord, method, flags, fdef_c, undef, mag)
    else:
        res = vd.levels(fields, coord, method, flags, undef, mag)
    return res[2:] if magnitude == "only" else res


def check(ctx, kind, fields, coord, method, device, flags=None, fdef_c=None, undef=vd.UNDEF, ab=None, stacked=True, magnitude=None, label=None):
    given, code = method if isinstance(method, tuple) else (method, method)
    got = run(ctx, kind, fields, coord, given, device, flags, fdef_c, undef, ab, stacked, magnitude)
    exp = expected(kind, fields, coord, code, flags, fdef_c, undef, ab, magnitude)
    assert len(got) == len(exp), label
    for j in range(0, len(exp), 2):
        compare(got[j], exp[j], got[j + 1], exp[j + 1], (label, kind, code, "device" if device else "host", magnitude, "magnitude" if j or magnitude == "only" else "derivative"))


@functools.lru_cache(maxsize=None)
def base(nf=3, nlev=12, ny=9, nx=13, seed=1):
    """The main generator with its extra cells: fields, ps, (alevel, blevel), the pressure of the levels as a coordinate
    batch, and pressure levels for the `levels` form."""
    fields, ps, ab, coord = vd.deriv_case(nf, nlev, ny, nx, seed)
    levs = vd.main_levels(nlev)
    for a in (fields, ps, ab[0], ab[1], coord, levs):
        a.setflags(write=False)
    return fields, ps, ab, coord, levs


def all_kinds(ctx, case, method, device, **kw):
    fields, ps, ab, coord, levs = case
    check(ctx, "hybrid", fields, ps, method, device, ab=ab, **kw)
    check(ctx, "field", fields, coord, method, device, **kw)
    check(ctx, "levels", fields, levs, method, device, **kw)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8])  # a launch takes 4 fields
def test_main_case_fields_methods_and_memory(gpu_ctx, nf, device):
    for method in METHODS:
        all_kinds(gpu_ctx, base(nf), method, device, stacked=(nf != 3), label=("nf", nf))


@pytest.mark.parametrize("shape", [(2, 9, 13), (3, 9, 13), (4, 9, 13), (5, 9, 13), (6, 9, 13), (7, 9, 13), (12, 5, 1), (12, 7, 16), (5, 3, 300)],
                         ids=["nlev2", "nlev3", "nlev4", "nlev5", "nlev6", "nlev7", "nx1", "nx16", "two_blocks"])
def test_shapes(gpu_ctx, shape):
    nlev, ny, nx = shape  # nlev 2: one-sided only, then every remainder of the slot rotation; nx = 16 on the device: four cells per
    case = base(3, nlev, ny, nx, 7)  # lane; 900 cells: more than one workgroup of single cells
    for device in (False, True):
        for method in METHODS:
            all_kinds(gpu_ctx, case, method, device, label=shape)
    all_kinds(gpu_ctx, base(2, nlev, ny, nx, 7), METHODS[1], True, magnitude="also", label=shape)


def test_vector_path_over_several_workgroups(gpu_ctx):
    case = base(2, 4, 3, 1100)  # 3300 cells, a multiple of 4: four blocks of 1024
    for method in METHODS:
        all_kinds(gpu_ctx, case, method, True, magnitude="also", label="vec4 blocks")


def test_device_batch_offset_by_one_float(gpu_ctx):
    import torch

    fields, ps, ab, coord, levs = base(2, 12, 9, 16)
    n = fields[0].size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
    batches = [buf[1 + j * n:1 + (j + 1) * n].view(12, 9, 16) for j in range(2)]  # 4 bytes past the 16-byte grid
    out, fd, mag, mfd = gpu_ctx.vderiv_hlevels(batches, torch.from_numpy(ps).cuda(), ab[0], ab[1], "weighted", "also")
    exp, efd, emag, emfd = vd.hlevels(fields, ps, ab[0], ab[1], vd.WEIGHTED, magnitude=True)
    compare(out.cpu().numpy(), exp, fd, efd, "offset inputs")
    compare(mag.cpu().numpy(), emag, mfd, emfd, "offset inputs, magnitude")
    obuf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")  # and an output off the grid
    out, fd = gpu_ctx.vderiv_levels(torch.from_numpy(fields).cuda(), levs, out=obuf[1:].view(2, 12, 9, 16))
    exp, efd = vd.levels(fields, levs)
    compare(out.cpu().numpy(), exp, fd, efd, "offset output")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bottom_up_non_monotone_and_signed_coordinates(gpu_ctx, device):
    fields, ps, ab, coord, levs = base(3)
    up = (np.ascontiguousarray(ab[0][::-1]), np.ascontiguousarray(ab[1][::-1]))
    rng = np.random.default_rng(11)
    wavy = (coord * rng.uniform(0.5, 1.5, coord.shape)).astype(np.float32)
    wavy[coord == vd.UNDEF] = vd.UNDEF
    # heights: signed, zero (of either sign) among the values, equal neighbours and folded columns (c_k+1 == c_k-1) in plenty
    z = np.round(rng.uniform(-3, 3, coord.shape)).astype(np.float32) * 100
    z[z == 0] = rng.choice(np.array([0.0, -0.0], np.float32), size=int((z == 0).sum()))
    zl = np.array([300, 100, 100, -0.0, 0.0, -200, 100, -200, -200, -200, 50, 1e-3], np.float32)
    for method in METHODS:
        check(gpu_ctx, "hybrid", fields[:, ::-1], ps, method, device, ab=up, label="bottom-up")
        check(gpu_ctx, "field", fields[:, ::-1], coord[::-1], method, device, label="bottom-up")
        check(gpu_ctx, "levels", fields[:, ::-1], levs[::-1], method, device, label="bottom-up")
        check(gpu_ctx, "field", fields, wavy, method, device, label="non-monotone")
        check(gpu_ctx, "field", fields, z, method, device, label="heights")
        check(gpu_ctx, "levels", fields, zl, method, device, label="heights")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mixed_flags_over_undef_and_nan(gpu_ctx, device):
    fields, ps, ab, coord, levs = base(4)
    rng = np.random.default_rng(3)
    fields = vd.sprinkle(fields, rng, 0.03, np.nan)
    coord = vd.sprinkle(coord, rng, 0.01, np.nan)
    ps = vd.sprinkle(ps, rng, 0.05, np.nan)
    flags = rng.choice(MIXED, size=(4, 12)).astype(np.int32)
    fdef_coord = rng.choice(MIXED, size=12).astype(np.int32)
    for method in METHODS:
        for fdef_ps in MIXED:
            check(gpu_ctx, "hybrid", fields, ps, method, device, flags=flags, fdef_c=fdef_ps, ab=ab, magnitude="also", label="flags")
        check(gpu_ctx, "field", fields, coord, method, device, flags=flags, fdef_c=fdef_coord, magnitude="also", label="flags")
        check(gpu_ctx, "field", fields, coord, method, device, flags=flags, fdef_c=[vd.ALL_DEFINED] * 12, label="coordinate ALL_DEFINED")
        check(gpu_ctx, "levels", fields, levs, method, device, flags=flags, magnitude="also", label="flags")
        check(gpu_ctx, "levels", fields, levs, method, device, flags=[vd.ALL_DEFINED] * 4, label="one flag per field")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nan_as_undef(gpu_ctx, device):
    nan = np.float32(np.nan)
    fields, ps, ab, coord, levs = base(2)
    fields, ps, coord = (np.where(a == vd.UNDEF, nan, a) for a in (fields, ps, coord))
    for method in METHODS:
        all_kinds(gpu_ctx, (fields, ps, ab, coord, levs), method, device, undef=nan, magnitude="also", label="undef = NaN")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [2, 4, 8])
def test_magnitude_also_and_only(gpu_ctx, nf, device):
    for method in METHODS:
        for magnitude in ("also", "only"):
            all_kinds(gpu_ctx, base(nf), method, device, magnitude=magnitude, stacked=(nf != 4), label=("nf", nf))


def test_magnitude_only_writes_no_derivative(gpu_ctx):
    """Through the C entry with fres NULL: the magnitudes arrive, a buffer the size of the derivatives that sits between
    them in memory keeps its sentinel, and fdefined_out is not touched."""
    import torch

    fields, ps, ab, coord, levs = base(4, 5, 9, 16)
    nf, nlev, ny, nx = fields.shape
    sentinel = -4242.5
    x = torch.from_numpy(fields).cuda()
    pool = torch.full((2 + nf, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")  # mag 0 | where fres would be | mag 1
    tab = (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
    mags = (ctypes.c_void_p * 2)(pool[0].data_ptr(), pool[nf + 1].data_ptr())
    fd, mfd = np.full(nf * nlev, 7, np.int32), np.full(2 * nlev, 7, np.int32)
    rc = gpu_ctx._lib.mifc_vderiv_fields(gpu_ctx._ctx, nx, ny, nlev, ctypes.addressof(tab), None, nf, torch.from_numpy(coord).cuda().data_ptr(), None,
                                         vd.WEIGHTED, None, fd.ctypes.data, ctypes.addressof(mags), mfd.ctypes.data, float(vd.UNDEF), 1)
    torch.cuda.synchronize()
    assert rc == 1, gpu_ctx.last_error()
    emag, emfd = vd.coord_fields(fields, coord, vd.WEIGHTED, magnitude=True)[2:]
    got = pool.cpu().numpy()
    compare(got[[0, nf + 1]], emag, mfd.reshape(2, nlev), emfd, "magnitude only")
    assert (got[1:nf + 1] == sentinel).all() and (fd == 7).all()


def test_host_call_in_several_bands(gpu_ctx, mifc_env):
    mifc_env("MIFC_VDERIV_CHUNK_MIB", 1)
    # hybrid, derivatives and magnitudes: 2 * 12 + 1 + 2 * 12 + 12 = 61 planes of 333 floats per row: 12 rows per MiB, so 50 rows
    # go in five bands, the last one of two rows
    case = base(2, 12, 50, 333, 9)
    all_kinds(gpu_ctx, case, METHODS[0], False, magnitude="also", label="bands")
    all_kinds(gpu_ctx, case, METHODS[1], False, magnitude="only", label="bands")
    check(gpu_ctx, "field", case[0], case[3], METHODS[1], False, label="bands")
    # the five bands against the one-launch device call itself, bit for bit, flags included
    fields, ps, ab, coord, levs = case
    for kind, c in (("hybrid", ps), ("field", coord), ("levels", levs)):
        host = run(gpu_ctx, kind, fields, c, "weighted", False, ab=ab, magnitude="also")
        dev = run(gpu_ctx, kind, fields, c, "weighted", True, ab=ab, magnitude="also")
        for j in (0, 2):
            compare(host[j], dev[j], host[j + 1], dev[j + 1], ("bands against the device call", kind, j))


def test_host_band_of_one_row_that_exceeds_the_budget(gpu_ctx, mifc_env):
    mifc_env("MIFC_VDERIV_CHUNK_MIB", 1)
    # 61 planes of 4300 floats per row are 1049200 bytes, more than the MiB: the band cannot be less than one row, so the three
    # rows go one at a time, each plane of 4300 floats padded to 4352
    fields, ps, ab, coord, levs = base(2, 12, 3, 4300, 9)
    for method in METHODS:
        check(gpu_ctx, "hybrid", fields, ps, method, False, ab=ab, magnitude="also", label="one-row bands")


def test_one_batch_drops_the_leading_axis_and_out_is_honoured(gpu_ctx):
    import torch

    fields, ps, ab, coord, levs = base(2)
    exp, efd, emag, emfd = vd.hlevels(fields, ps, ab[0], ab[1], vd.CENTRED, magnitude=True)
    out, fd = gpu_ctx.vderiv_hlevels(fields[0], ps, ab[0], ab[1])
    assert out.shape == (12, 9, 13) and fd.shape == (12,) and same_bits(out, exp[0], nan_payload=False) and list(fd) == list(efd[0])
    o = torch.empty((12, 9, 13), dtype=torch.float32, device="cuda")
    out, fd = gpu_ctx.vderiv_fields(torch.from_numpy(fields[1]).cuda(), torch.from_numpy(coord).cuda(), 0, out=o)
    e1, e1fd = vd.coord_fields(fields[1:], coord)
    assert out is o and same_bits(o.cpu().numpy(), e1[0], nan_payload=False) and list(fd) == list(e1fd[0])
    o, m = np.full((2, 12, 9, 13), -1, np.float32), np.full((1, 12, 9, 13), -1, np.float32)
    out, fd, mag, mfd = gpu_ctx.vderiv_hlevels([fields[0], fields[1]], ps, ab[0], ab[1], magnitude="also", out=(o, m))
    assert out is o and mag is m and same_bits(o, exp, nan_payload=False) and same_bits(m, emag, nan_payload=False)
    assert fd.shape == (2, 12) and mfd.shape == (1, 12) and np.array_equal(fd, efd) and np.array_equal(mfd, emfd)
    m = np.full((1, 12, 9, 13), -1, np.float32)
    mag, mfd = gpu_ctx.vderiv_levels(fields, levs, "weighted", "only", out=m)
    assert mag is m and same_bits(m, vd.levels(fields, levs, vd.WEIGHTED, magnitude=True)[2], nan_payload=False)


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx = 2, 4, 3, 8
    fields_h, ps_h, ab, coord_h, levs = base(nf, nlev, ny, nx, 2)
    x = torch.from_numpy(fields_h).cuda()
    batch = nlev * ny * nx
    room = torch.zeros(batch + ny * nx, dtype=torch.float32, device="cuda")  # a batch of the test's own in front of ps: a magnitude that
    ps = room[batch:].view(ny, nx).copy_(torch.from_numpy(ps_h))  # ends in ps begins there, whatever else the allocator has put nearby
    coord = torch.from_numpy(coord_h).cuda()
    sentinel = -4242.5
    outs = torch.full((nf, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    mags = torch.full((1, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")

    def call(kind, nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, method=0, fields=None, out_ptrs=None, mag_ptrs=None, coord_ptr=0, a=None, b=None, lv=None,
             fd_out=True, fd_mag=True, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        m = (ctypes.c_void_p * 1)(*([mags[0].data_ptr()] if mag_ptrs in (None, "null") else mag_ptrs))
        al, bl = (np.asarray(own if v in (None, "null") else v, np.float32) for v, own in ((a, ab[0]), (b, ab[1])))
        lev = np.asarray(levs if lv is None else lv, np.float32)
        fd, mfd = np.full(nf * nlev, 7, np.int32), np.full(nlev, 7, np.int32)
        tail = [method, None if out_ptrs == "null" else ctypes.addressof(o), fd.ctypes.data if fd_out else None,
                None if mag_ptrs == "null" else ctypes.addressof(m), mfd.ctypes.data if fd_mag else None, float(vd.UNDEF), 1]
        head = [c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_]
        if kind == "hybrid":
            cp = ps.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vderiv_hlevels(*head, cp, vd.SOME_DEFINED, None if isinstance(a, str) else al.ctypes.data,
                                         None if isinstance(b, str) else bl.ctypes.data, *tail)
        elif kind == "field":
            cp = coord.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vderiv_fields(*head, cp, None, *tail)
        else:
            rc = lib.mifc_vderiv_levels(*head, lev.ctypes.data if coord_ptr == 0 else coord_ptr, *tail)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd, mfd

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
        "null fields": (dict(fields="null"), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or fres[1])"),
        "null coordinate": (dict(coord_ptr=None), null_head),
        "fres and fmag both null": (dict(out_ptrs="null", mag_ptrs="null"), "fres and fmag are both null: nothing to write"),
        "fmag with an odd nfields": (dict(nf_=1), "fmag with an odd nfields: a magnitude takes the fields 2j and 2j + 1"),
        "fmag without fdefined_mag": (dict(fd_mag=False), "fmag without fdefined_mag"),
        "fres without fdefined_out": (dict(fd_out=False), "fres without fdefined_out"),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None]), "a null pointer (fields[1] or fres[1])"),
        "null magnitude": (dict(mag_ptrs=[None]), "a null pointer (fmag[0])"),
        "output is an input": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output inside an input": (dict(out_ptrs=[x[0].data_ptr() + 4 * (batch - 1), outs[1].data_ptr()]), "fres[0] overlaps fields[0]"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr() + 4 * (batch - 1)]), "fres[0] overlaps fres[1]"),
        "magnitude overlaps a derivative": (dict(mag_ptrs=[outs[1].data_ptr() + 4 * (batch - 1)]), "fres[1] overlaps fmag[0]"),
        "magnitude is an input": (dict(mag_ptrs=[x[0].data_ptr()]), "fmag[0] overlaps fields[0]"),
        "magnitude only, over an input": (dict(out_ptrs="null", mag_ptrs=[x[1].data_ptr() - 4 * (batch - 1)]), "fmag[0] overlaps fields[0]"),
    }
    only = {
        "hybrid": {
            "null alevel": (dict(a="null"), null_head),
            "null blevel": (dict(b="null"), null_head),
            "negative alevel": (dict(a=[1.0, -1.0, 2.0, 0.0]), no_level % 1),
            "negative blevel": (dict(b=[0.0, 0.1, -0.2, 1.0]), no_level % 2),
            "blevel > 1": (dict(b=[0.0, 0.1, 0.2, 1.5]), no_level % 3),
            "alevel = blevel = 0": (dict(a=[1.0, 0.0, 2.0, 0.0], b=[0.0, 0.0, 0.5, 1.0]), no_level % 1),
            "output overlaps ps": (dict(out_ptrs=[outs[0].data_ptr(), ps.data_ptr() + 4 * (ny * nx - 1)]), "fres[1] overlaps ps"),
            "magnitude overlaps ps": (dict(mag_ptrs=[ps.data_ptr() - 4 * (batch - 1)]), "fmag[0] overlaps ps"),
        },
        "field": {
            "output overlaps coord": (dict(out_ptrs=[coord.data_ptr() + 4 * (batch - 1), outs[1].data_ptr()]), "fres[0] overlaps coord"),
            "magnitude overlaps coord": (dict(mag_ptrs=[coord.data_ptr()]), "fmag[0] overlaps coord"),
        },
        "levels": {"NaN level": (dict(lv=[100, float("nan"), 300, 400]), "levels[1] is NaN")},
    }
    for kind, name in (("hybrid", "mifc_vderiv_hlevels: "), ("field", "mifc_vderiv_fields: "), ("levels", "mifc_vderiv_levels: ")):
        before = {k: t.clone() for k, t in (("x", x), ("ps", ps), ("coord", coord))}
        for what, (kw, tail) in {**every, **only[kind]}.items():
            rc, err, fd, mfd = call(kind, **kw)
            assert rc == 0 and err == name + (tail[kind] if isinstance(tail, dict) else tail), (kind, what, err)
            assert (outs == sentinel).all().item() and (mags == sentinel).all().item() and (fd == 7).all() and (mfd == 7).all(), (kind, what)
        assert torch.equal(x, before["x"]) and torch.equal(ps, before["ps"]) and torch.equal(coord, before["coord"])
    with pytest.raises(RuntimeError, match="mifc_vderiv_hlevels"):
        gpu_ctx.vderiv_hlevels(x, ps, ab[0], ab[1], "spline")
    with pytest.raises(RuntimeError, match="odd nfields"):
        gpu_ctx.vderiv_levels(x[:1], levs, magnitude="only")
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        refused = [call(kind, sync=False) for kind in KINDS]
    g.close()
    for rc, err, fd, mfd in refused:
        assert rc == 0 and "capture" in err and (fd == 7).all() and (mfd == 7).all()
    assert (outs == sentinel).all().item() and (mags == sentinel).all().item()
    # afterwards the same calls run
    for kind in KINDS:
        rc, err, fd, mfd = call(kind)
        assert rc == 1 and err == "" and (fd != 7).all() and (mfd != 7).all(), (kind, err)
    exp, efd, emag, emfd = vd.levels(fields_h, levs, magnitude=True)
    compare(outs.cpu().numpy(), exp, fd.reshape(nf, nlev), efd, "after the refusals")
    compare(mags.cpu().numpy(), emag, mfd.reshape(1, nlev), emfd, "after the refusals")


def test_empty_grid_behaves_as_in_vinterp(gpu_ctx):
    x = np.zeros((2, 3, 0, 5), np.float32)
    out, fd, mag, mfd = gpu_ctx.vderiv_fields(x, np.zeros((3, 0, 5), np.float32), magnitude="also")
    assert out.shape == (2, 3, 0, 5) and mag.shape == (1, 3, 0, 5) and (fd == vd.ALL_DEFINED).all() and (mfd == vd.ALL_DEFINED).all()
    out, fd = gpu_ctx.vderiv_levels(x, [100, 200, 300])
    assert out.shape == (2, 3, 0, 5) and fd.shape == (2, 3) and (fd == vd.ALL_DEFINED).all()


def test_static_stability_on_pressure_surfaces_on_the_device(gpu_ctx):
    """Device tensors throughout: theta on hybrid levels -> vinterp_hlevels to eight pressure surfaces -> vderiv_levels
    with the same targets: bit for bit the restatement applied to the restated vinterp output.  Where the lower surfaces
    are below the ground, the lowest one above it carries the one-sided value and the ones below are undef."""
    import torch

    rng = np.random.default_rng(23)
    nlev, ny, nx = 12, 9, 16
    alevel, blevel = vd.hybrid_levels(nlev)
    ps = rng.uniform(700, 1050, (ny, nx)).astype(np.float32)
    p = vd.hybrid_coordinate(ps, alevel, blevel)
    t = (220 + 70 * (p / 1000.0) ** 0.19 + rng.normal(0, 0.3, p.shape)).astype(np.float32)
    theta = (t * (1000.0 / p) ** 0.2857).astype(np.float32)
    targets = np.array([100, 200, 300, 500, 700, 850, 925, 1000], np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    on_p, pfd = gpu_ctx.vinterp_hlevels(dev(theta), dev(ps), alevel, blevel, targets)
    e_on_p, e_pfd = vi.hlevels(theta[None], ps, alevel, blevel, targets, vi.LINEAR)
    assert on_p.is_cuda and list(pfd) == list(e_pfd[0])
    for given, method in METHODS:
        dth, fd = gpu_ctx.vderiv_levels(on_p, targets, given, fdefined_in=pfd)
        exp, efd = vd.levels(e_on_p, targets, method, flags=e_pfd)
        assert dth.is_cuda
        compare(dth.cpu().numpy(), exp[0], fd, efd[0], ("static stability", method))
    got, x = dth.cpu().numpy().reshape(8, -1), e_on_p[0].reshape(8, -1)
    below = x == vd.UNDEF
    seen = 0
    for i in range(ny * nx):
        if below[:, i].any():
            k0 = int(np.argmax(below[:, i]))  # the first surface below the ground
            assert below[k0:, i].all() and k0 >= 2 and (got[k0:, i] == vd.UNDEF).all()
            one_sided = np.float32((np.float64(x[k0 - 1, i]) - np.float64(x[k0 - 2, i])) * (1.0 / (np.float64(targets[k0 - 1]) - np.float64(targets[k0 - 2]))))
            assert got[k0 - 1, i] == one_sided
            seen += 1
    assert seen > 10 and (got[:5] < 0).all()  # theta falls with rising pressure: a stable atmosphere


def test_wind_shear_against_a_height_batch(gpu_ctx):
    """vderiv_fields of (u, v) against a height batch with magnitude="only": the restated shear bit for bit, and not
    negative where it is defined."""
    import torch

    rng = np.random.default_rng(29)
    nlev, ny, nx = 12, 9, 16
    z = (np.cumsum(rng.uniform(50, 900, (nlev, ny, nx)), axis=0)[::-1] + rng.uniform(0, 300, (ny, nx))).astype(np.float32)  # top-down
    z = vd.sprinkle(z, rng, 0.01, vd.UNDEF)
    u = vd.sprinkle(rng.normal(5, 12, (nlev, ny, nx)).astype(np.float32), rng, 0.02, vd.UNDEF)
    v = vd.sprinkle(rng.normal(0, 12, (nlev, ny, nx)).astype(np.float32), rng, 0.02, vd.UNDEF)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for given, method in METHODS:
        shear, sfd = gpu_ctx.vderiv_fields([dev(u), dev(v)], dev(z), given, "only")
        emag, emfd = vd.coord_fields(np.stack([u, v]), z, method, magnitude=True)[2:]
        assert shear.is_cuda and shear.shape == (1, nlev, ny, nx)
        got = shear.cpu().numpy()
        compare(got, emag, sfd, emfd, ("shear", method))
        ok = got != vd.UNDEF
        assert ok.mean() > 0.5 and (got[ok] >= 0).all() and (sfd == vd.SOME_DEFINED).all()
