"""Layer integrals, means and extremes of level batches on the GPU (mifc_vlayer.hip, mifc_vlayer_hlevels /
mifc_vlayer_fields) against the numpy restatement (tests/vlayer_restate.py): bit for bit (a NaN matches any NaN), flags
equal, both coordinate kinds, host and device memory.  No tolerance: every operation of the definition is an IEEE float
or double operation rounded on its own, and the library is built without contraction."""
import ctypes
import functools

import numpy as np
import pytest

import vlayer_restate as vl
from cases import same_bits

pytestmark = pytest.mark.gpu

MIXED = [vl.ALL_DEFINED, vl.SOME_DEFINED, vl.NONE_DEFINED]
ALL = vl.ALL_PRODUCTS
GROUPS = {"all": ALL, "sums": [vl.MEAN, vl.INTEGRAL], "extremes": [vl.COORD_OF_MIN, vl.MAX, vl.MIN, vl.COORD_OF_MAX], "one": [vl.MAX]}


def compare(got, exp, gfd, efd, label):
    assert got.shape == exp.shape, label
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if not same_bits(got, exp, nan_payload=False):
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))


def run(ctx, kind, fields, coord, products, lo, hi, device, flags=None, fdef_c=None, undef=vl.UNDEF, ab=None, stacked=True):
    import torch

    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    f = put(fields)
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    lo, hi = (put(b) if np.ndim(b) else b for b in (lo, hi))
    if kind == "hybrid":
        out, fd = ctx.vlayer_hlevels(f, put(coord), ab[0], ab[1], products, lo, hi, fdefined_in=flags,
                                     fdef_ps=vl.SOME_DEFINED if fdef_c is None else fdef_c, undef=undef)
    else:
        out, fd = ctx.vlayer_fields(f, put(coord), products, lo, hi, fdefined_in=flags, fdef_coord=fdef_c, undef=undef)
    return (out.cpu().numpy() if device else out), fd


def check(ctx, kind, fields, coord, products, lo, hi, device, flags=None, fdef_c=None, undef=vl.UNDEF, ab=None, stacked=True, label=None):
    got, gfd = run(ctx, kind, fields, coord, products, lo, hi, device, flags, fdef_c, undef, ab, stacked)
    if kind == "hybrid":
        exp, efd = vl.hlevels(fields, coord, ab[0], ab[1], products, lo, hi, flags, vl.SOME_DEFINED if fdef_c is None else fdef_c, undef)
    else:
        exp, efd = vl.coord_fields(fields, coord, products, lo, hi, flags, fdef_c, undef)
    compare(got, exp, gfd, efd, (label, kind, lo if not np.ndim(lo) else "lo field", hi if not np.ndim(hi) else "hi field",
                                 "device" if device else "host"))


@functools.lru_cache(maxsize=None)
def base(nf=3, nlev=12, ny=9, nx=13, seed=1):
    """The main generator and the pressure of its levels as a coordinate batch (the field form of the same problem)."""
    fields, ps, alevel, blevel = vl.main_case(nf, nlev, ny, nx, seed)
    coord = vl.hybrid_coordinate(np.where(ps == vl.UNDEF, np.float32(900), ps), alevel, blevel)
    coord[:, ps == vl.UNDEF] = vl.UNDEF
    for a in (fields, ps, alevel, blevel, coord):
        a.setflags(write=False)
    return fields, ps, (alevel, blevel), coord


def both_kinds(ctx, fields, ps, ab, coord, products, lo, hi, device, **kw):
    check(ctx, "hybrid", fields, ps, products, lo, hi, device, ab=ab, **kw)
    check(ctx, "field", fields, coord, products, lo, hi, device, **kw)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8])  # a launch takes 2 fields with all six products, 4 with one group
def test_main_case_fields_layers_and_memory(gpu_ctx, nf, device):
    fields, ps, ab, coord = base(nf)
    for lo, hi in vl.MAIN_LAYERS:
        both_kinds(gpu_ctx, fields, ps, ab, coord, ALL, lo, hi, device, stacked=(nf != 3), label=("nf", nf))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("group", ["sums", "extremes", "one"])
def test_product_groups_alone(gpu_ctx, group, device):
    for nf in (3, 4, 5, 8):
        fields, ps, ab, coord = base(nf)
        for lo, hi in vl.MAIN_LAYERS[:3] if nf == 3 else vl.MAIN_LAYERS[1:2]:
            both_kinds(gpu_ctx, fields, ps, ab, coord, GROUPS[group], lo, hi, device, label=(group, nf))
    fields, ps, ab, coord = base(1)
    for p in ALL:  # each product on its own, by name
        name = [k for k, v in vl.NAMES.items() if v == p]
        both_kinds(gpu_ctx, fields, ps, ab, coord, name, 300, 850, device, label=name)


@pytest.mark.parametrize("shape", [(2, 9, 13), (3, 9, 13), (4, 9, 13), (5, 9, 13), (12, 5, 1), (12, 7, 16), (5, 3, 300)],
                         ids=["nlev2", "nlev3", "nlev4", "nlev5", "nx1", "nx16", "two_blocks"])
def test_shapes(gpu_ctx, shape):
    nlev, ny, nx = shape  # nx = 16 on the device: four cells per lane; 900 cells: more than one workgroup of single cells
    fields, ps, ab, coord = base(3, nlev, ny, nx, 7)
    for device in (False, True):
        for lo, hi in ((-vl.INF, vl.INF), (300, 850)):
            both_kinds(gpu_ctx, fields, ps, ab, coord, ALL, lo, hi, device, label=shape)


def test_vector_path_over_several_workgroups(gpu_ctx):
    fields, ps, ab, coord = base(2, 4, 3, 1100)  # 3300 cells, a multiple of 4: four blocks of 1024
    for lo, hi in ((-vl.INF, vl.INF), (300, 850)):
        both_kinds(gpu_ctx, fields, ps, ab, coord, ALL, lo, hi, True, label="vec4 blocks")


def test_device_batch_offset_by_one_float(gpu_ctx):
    import torch

    fields, ps, ab, coord = base(2, 12, 9, 16)
    n = fields[0].size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
    batches = [buf[1 + j * n:1 + (j + 1) * n].view(12, 9, 16) for j in range(2)]  # 4 bytes past the 16-byte grid
    out, fd = gpu_ctx.vlayer_hlevels(batches, torch.from_numpy(ps).cuda(), ab[0], ab[1], ALL, 300, 850)
    exp, efd = vl.hlevels(fields, ps, ab[0], ab[1], ALL, 300, 850)
    compare(out.cpu().numpy(), exp, fd, efd, "offset")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bottom_up_non_monotone_and_signed_coordinates(gpu_ctx, device):
    fields, ps, ab, coord = base(3)
    up = (np.ascontiguousarray(ab[0][::-1]), np.ascontiguousarray(ab[1][::-1]))
    rng = np.random.default_rng(11)
    wavy = (coord * rng.uniform(0.5, 1.5, coord.shape)).astype(np.float32)  # pairs that overlap: each of them counts
    wavy[coord == vl.UNDEF] = vl.UNDEF
    for lo, hi in vl.MAIN_LAYERS[:3]:
        both_kinds(gpu_ctx, fields[:, ::-1], ps, up, coord[::-1], ALL, lo, hi, device, label="bottom-up")
        check(gpu_ctx, "field", fields, wavy, ALL, lo, hi, device, label="non-monotone")
    # heights: signed, zero (of either sign) among the values and the bounds, equal neighbours
    z = np.round(rng.uniform(-3, 3, coord.shape)).astype(np.float32) * 100
    z[z == 0] = rng.choice(np.array([0.0, -0.0], np.float32), size=int((z == 0).sum()))
    for lo, hi in ((-vl.INF, vl.INF), (-250, 150.5), (-0.0, 300), (-200, 0.0)):
        check(gpu_ctx, "field", fields, z, ALL, lo, hi, device, label="heights")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mixed_flags_over_undef_and_nan(gpu_ctx, device):
    fields, ps, ab, coord = base(3)
    rng = np.random.default_rng(3)
    fields = vl.sprinkle(fields, rng, 0.03, np.nan)
    coord = vl.sprinkle(coord, rng, 0.01, np.nan)
    ps = vl.sprinkle(ps, rng, 0.05, np.nan)
    flags = rng.choice(MIXED, size=(3, 12)).astype(np.int32)
    fdef_coord = rng.choice(MIXED, size=12).astype(np.int32)
    for lo, hi in vl.MAIN_LAYERS[:3]:
        for fdef_ps in MIXED:
            check(gpu_ctx, "hybrid", fields, ps, ALL, lo, hi, device, flags=flags, fdef_c=fdef_ps, ab=ab, label="flags")
        check(gpu_ctx, "field", fields, coord, ALL, lo, hi, device, flags=flags, fdef_c=fdef_coord, label="flags")
        check(gpu_ctx, "field", fields, coord, ALL, lo, hi, device, flags=flags, fdef_c=[vl.ALL_DEFINED] * 12, label="coordinate ALL_DEFINED")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nan_as_undef(gpu_ctx, device):
    nan = np.float32(np.nan)
    fields, ps, ab, coord = base(3)
    fields, ps, coord = (np.where(a == vl.UNDEF, nan, a) for a in (fields, ps, coord))
    for lo, hi in vl.MAIN_LAYERS[:3]:
        both_kinds(gpu_ctx, fields, ps, ab, coord, ALL, lo, hi, device, undef=nan, label="undef = NaN")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_per_cell_bounds(gpu_ctx, device):
    fields, ps, ab, coord = base(3, 12, 9, 16)  # 144 cells: four per lane on the device
    rng = np.random.default_rng(17)
    good = np.where(ps == vl.UNDEF, np.float32(900), ps)
    lo_f = (good - rng.uniform(50, 400, ps.shape)).astype(np.float32)  # the lowest 50 .. 400 hPa
    hi_f = (good - rng.uniform(-20, 40, ps.shape)).astype(np.float32)
    lo_bad = vl.sprinkle(vl.sprinkle(lo_f, rng, 0.05, vl.UNDEF), rng, 0.05, np.nan)
    hi_bad = vl.sprinkle(vl.sprinkle(hi_f, rng, 0.05, vl.UNDEF), rng, 0.05, np.nan)
    cross = rng.random(ps.shape) < 0.1
    hi_bad[cross] = lo_f[cross] - rng.choice(np.array([0, 25], np.float32), size=int(cross.sum()))  # L == H and L > H
    for lo, hi in ((lo_f, vl.INF), (-vl.INF, hi_f), (lo_f, hi_f), (lo_bad, 1200), (100, hi_bad), (lo_bad, hi_bad)):
        both_kinds(gpu_ctx, fields, ps, ab, coord, ALL, lo, hi, device, label="bounds")
    both_kinds(gpu_ctx, fields, ps, ab, coord, GROUPS["sums"], lo_f, lo_f.copy(), device, label="lo == hi")  # undef everywhere


def test_host_call_in_several_bands(gpu_ctx, mifc_env):
    mifc_env("MIFC_VLAYER_CHUNK_MIB", 1)
    # 3 * 12 + 1 + 1 + 3 * 2 = 44 planes of 333 floats per row: 17 rows per MiB, so 50 rows go in three bands, the last one short
    fields, ps, ab, coord = base(3, 12, 50, 333, 9)
    lo_f = (np.where(ps == vl.UNDEF, np.float32(900), ps) - 300).astype(np.float32)
    check(gpu_ctx, "hybrid", fields, ps, GROUPS["sums"], lo_f, vl.INF, False, ab=ab, label="bands")
    check(gpu_ctx, "field", fields, coord, ALL, 300, 850, False, label="bands, two launches each")


def test_one_batch_drops_the_leading_axis(gpu_ctx):
    import torch

    fields, ps, ab, coord = base(1)
    exp, efd = vl.hlevels(fields, ps, ab[0], ab[1], [vl.MEAN, vl.MAX], 300, 850)
    out, fd = gpu_ctx.vlayer_hlevels(fields[0], ps, ab[0], ab[1], ["mean", "max"], 300, 850)
    assert out.shape == (2, 9, 13) and fd.shape == (2,) and same_bits(out, exp[0], nan_payload=False) and list(fd) == list(efd[0])
    o = torch.empty((2, 9, 13), dtype=torch.float32, device="cuda")
    out, fd = gpu_ctx.vlayer_fields(torch.from_numpy(fields[0]).cuda(), torch.from_numpy(coord).cuda(), [vl.MEAN, vl.MAX], 300, 850, out=o)
    assert out is o and same_bits(o.cpu().numpy(), exp[0], nan_payload=False) and list(fd) == list(efd[0])
    o = np.full((1, 2, 9, 13), -1, np.float32)
    out, fd = gpu_ctx.vlayer_fields([fields[0]], coord, [vl.MEAN, vl.MAX], 300, 850, out=o)
    assert out is o and same_bits(o, exp, nan_payload=False) and fd.shape == (1, 2)


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx, npr = 2, 4, 3, 8, 3
    fields_h, ps_h, ab, coord_h = base(nf, nlev, ny, nx, 2)
    x = torch.from_numpy(fields_h).cuda()
    ps, coord = torch.from_numpy(ps_h).cuda(), torch.from_numpy(coord_h).cuda()
    lof, hif = torch.full((ny, nx), 300.0, device="cuda"), torch.full((ny, nx), 850.0, device="cuda")
    sentinel = -4242.5
    outs = torch.full((nf, npr, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    cells = ny * nx

    def call(hybrid, nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, np_=npr, products=(1, 3, 5), lo=300.0, hi=850.0, lo_ptr=None, hi_ptr=None, fields=None,
             out_ptrs=None, coord_ptr=0, a=None, b=None, pr=True, fd_out=True, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        p = np.asarray(products, np.int32)
        al, bl = (np.asarray(own if v in (None, "null") else v, np.float32) for v, own in ((a, ab[0]), (b, ab[1])))
        fd = np.full(nf * npr, 7, np.int32)
        common = [lo, hi, lo_ptr, hi_ptr, p.ctypes.data if pr else None, np_, None if isinstance(out_ptrs, str) else ctypes.addressof(o),
                  fd.ctypes.data if fd_out else None, float(vl.UNDEF), 1]
        head = [c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_]
        if hybrid:
            cp = ps.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vlayer_hlevels(*head, cp, vl.SOME_DEFINED, None if isinstance(a, str) else al.ctypes.data,
                                         None if isinstance(b, str) else bl.ctypes.data, *common)
        else:
            cp = coord.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vlayer_fields(*head, cp, None, *common)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    nan = float("nan")
    # what: (the arguments, the message behind "<entry name>: "; a pair where the two entries word it differently)
    null_head = ("a null pointer (fields, ps, alevel, blevel, products, fres or fdefined_out)", "a null pointer (fields, coord, products, fres or fdefined_out)")
    no_level = "level %d: alevel / blevel are no hybrid level (FieldCalculations.cc:298)"
    no_product = "products[%d] = %d is no MIFC_VLAYER_* product"
    empty = "the layer is empty: not lo < hi"
    both = {
        "nlev < 2": (dict(nlev_=1), "nlev < 2"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "nproducts 0": (dict(np_=0), "nproducts 0 outside 1..6"),
        "nproducts 7": (dict(np_=7), "nproducts 7 outside 1..6"),
        "unknown product 0": (dict(products=(1, 0, 5)), no_product % (1, 0)),
        "unknown product 7": (dict(products=(7, 3, 5)), no_product % (0, 7)),
        "negative product": (dict(products=(1, 3, -2)), no_product % (2, -2)),
        "repeated product": (dict(products=(1, 3, 1)), "product 1 asked for twice"),
        "negative nx": (dict(nx_=-1), "a negative nx or ny"),
        "negative ny": (dict(ny_=-2), "a negative nx or ny"),
        "null fields": (dict(fields="null"), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or fres[1])"),
        "null coordinate": (dict(coord_ptr=None), null_head),
        "null products": (dict(pr=False), null_head),
        "null fres": (dict(out_ptrs="null"), null_head),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None]), "a null pointer (fields[1] or fres[1])"),
        "null flags out": (dict(fd_out=False), null_head),
        "lo == hi": (dict(lo=500.0, hi=500.0), empty),
        "lo > hi": (dict(lo=850.0, hi=300.0), empty),
        "NaN lo": (dict(lo=nan), empty),  # (not NaN < hi: the two scalars are tested against each other first)
        "NaN hi": (dict(hi=nan), empty),
        "NaN scalar lo beside a hi field": (dict(lo=nan, hi_ptr=hif.data_ptr()), "a NaN bound"),
        "NaN scalar hi beside a lo field": (dict(hi=nan, lo_ptr=lof.data_ptr()), "a NaN bound"),
        "output is an input": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output inside an input": (dict(out_ptrs=[x[0].data_ptr() + 4 * (nlev * cells - 1), outs[1].data_ptr()]), "fres[0] overlaps fields[0]"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr() + 4 * (npr * cells - 1)]), "fres[0] overlaps fres[1]"),
        "output overlaps lo_field": (dict(lo_ptr=outs[1].data_ptr() + 4 * (npr * cells - 1)), "fres[1] overlaps lo_field"),
        "output overlaps hi_field": (dict(hi_ptr=outs[0].data_ptr()), "fres[0] overlaps hi_field"),
    }
    hybrid_only = {
        "null alevel": (dict(a="null"), null_head),
        "null blevel": (dict(b="null"), null_head),
        "negative alevel": (dict(a=[1.0, -1.0, 2.0, 0.0]), no_level % 1),
        "negative blevel": (dict(b=[0.0, 0.1, -0.2, 1.0]), no_level % 2),
        "blevel > 1": (dict(b=[0.0, 0.1, 0.2, 1.5]), no_level % 3),
        "alevel = blevel = 0": (dict(a=[1.0, 0.0, 2.0, 0.0], b=[0.0, 0.0, 0.5, 1.0]), no_level % 1),
        "output overlaps ps": (dict(out_ptrs=[outs[0].data_ptr(), ps.data_ptr() + 4 * (cells - 1)]), "fres[1] overlaps ps"),
    }
    field_only = {"output overlaps coord": (dict(out_ptrs=[coord.data_ptr() + 4 * (nlev * cells - 1), outs[1].data_ptr()]), "fres[0] overlaps coord")}
    for hybrid, name, cases in ((True, "mifc_vlayer_hlevels: ", {**both, **hybrid_only}), (False, "mifc_vlayer_fields: ", {**both, **field_only})):
        before = {k: t.clone() for k, t in (("x", x), ("ps", ps), ("coord", coord), ("lo", lof), ("hi", hif))}
        for what, (kw, tail) in cases.items():
            rc, err, fd = call(hybrid, **kw)
            assert rc == 0 and err == name + (tail if isinstance(tail, str) else tail[0 if hybrid else 1]), (what, err)
            assert (outs == sentinel).all().item() and (fd == 7).all(), what
        assert torch.equal(x, before["x"]) and torch.equal(ps, before["ps"]) and torch.equal(coord, before["coord"])
        assert torch.equal(lof, before["lo"]) and torch.equal(hif, before["hi"])
    with pytest.raises(RuntimeError, match="mifc_vlayer_hlevels"):
        gpu_ctx.vlayer_hlevels(x, ps, ab[0], ab[1], ["median"])
    with pytest.raises(RuntimeError, match="twice"):
        gpu_ctx.vlayer_fields(x, coord, ["mean", vl.MEAN])
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        r1 = call(True, sync=False)
        r2 = call(False, sync=False)
    g.close()
    for rc, err, fd in (r1, r2):
        assert rc == 0 and "capture" in err and (fd == 7).all()
    assert (outs == sentinel).all().item()
    # afterwards the same calls run, with scalar bounds and with bound fields
    for hybrid in (True, False):
        rc, err, fd = call(hybrid)
        assert rc == 1 and err == "" and (fd != 7).all()
        rc, err, fd = call(hybrid, lo_ptr=lof.data_ptr(), hi_ptr=hif.data_ptr(), lo=nan, hi=nan)  # the scalars are not in use
        assert rc == 1 and err == "" and (fd != 7).all()


def test_empty_grid_behaves_as_in_vinterp(gpu_ctx):
    x = np.zeros((2, 3, 0, 5), np.float32)
    out, fd = gpu_ctx.vlayer_fields(x, np.zeros((3, 0, 5), np.float32), ALL)
    assert out.shape == (2, 6, 0, 5) and (fd == vl.ALL_DEFINED).all()


def test_precipitable_water_and_the_level_of_maximum_wind_on_the_device(gpu_ctx):
    """Device tensors throughout: q on hybrid levels -> INTEGRAL -> divided by g with the field algebra, bit for bit the
    same division of the restatement's integral; the coordinate of the maximum wind speed is a level's or a bound."""
    import torch

    rng = np.random.default_rng(21)
    nlev, ny, nx = 12, 9, 16
    alevel, blevel = vl.hybrid_levels(nlev)
    eta = np.linspace(0.02, 1, nlev) ** 1.5
    ps = vl.sprinkle(rng.uniform(860, 1050, (ny, nx)).astype(np.float32), rng, 0.03, vl.UNDEF)
    q = (0.012 * eta[:, None, None] ** 3 * rng.uniform(0.5, 1.5, (nlev, ny, nx))).astype(np.float32)
    q = vl.sprinkle(q, rng, 0.01, vl.UNDEF)
    ff = rng.gamma(2.0, 8.0, (nlev, ny, nx)).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    g = 9.80665
    # precipitable water [kg m-2]: the integral of q over p [hPa] * 100 / g
    e_int, e_fd = vl.hlevels(q[None], ps, alevel, blevel, [vl.INTEGRAL])
    integral, fd = gpu_ctx.vlayer_hlevels(dev(q), dev(ps), alevel, blevel, ["integral"])
    assert integral.is_cuda and list(fd) == list(e_fd[0]) and fd[0] == vl.SOME_DEFINED
    pw, pfd = gpu_ctx.fieldOPERconstant(4, integral[0], g / 100.0, fdefined=int(fd[0]))  # 4: divide
    epw, epfd = gpu_ctx.fieldOPERconstant(4, dev(e_int[0, 0]), g / 100.0, fdefined=int(e_fd[0, 0]))
    assert pw.is_cuda and pfd == epfd == vl.SOME_DEFINED
    assert same_bits(pw.cpu().numpy(), epw.cpu().numpy(), nan_payload=False)
    assert (pw.cpu().numpy() != vl.UNDEF).mean() > 0.5
    # the maximum wind between 150 and 500 hPa and where it sits
    out, fd = gpu_ctx.vlayer_hlevels([dev(ff)], dev(ps), alevel, blevel, ["max", "coord_of_max"], 150, 500)
    e_out, e_fd = vl.hlevels(ff[None], ps, alevel, blevel, [vl.MAX, vl.COORD_OF_MAX], 150, 500)
    compare(out.cpu().numpy(), e_out, fd, e_fd, "maximum wind")
    where = out[0, 1].cpu().numpy()
    levels = vl.hybrid_coordinate(ps, alevel, blevel)
    ok = where != vl.UNDEF
    on_level = (levels == where[None]).any(axis=0)
    assert ok.mean() > 0.5 and (on_level | (where == 150) | (where == 500))[ok].all()
