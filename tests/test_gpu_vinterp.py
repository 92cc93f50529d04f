"""Level batches interpolated to constant surfaces on the GPU (mifc_vinterp.hip, mifc_vinterp_hlevels /
mifc_vinterp_fields) against the numpy restatement (tests/vinterp_restate.py).  LINEAR: bit for bit (a NaN matches any
NaN), flags equal.  LOG: the undefined cells and the flags identical, every other value equal or the neighbouring
float32 -- double log() implementations differ by a few ulp of double, i.e. by about 1e-15 in a logarithm of size 7;
the levels here are more than 1e-3 apart in ln p, so the weight is off by less than 1e-10 relative, far below half a
float32 ulp of the result: at most its one rounding can flip."""
import ctypes
import functools

import numpy as np
import pytest

import vinterp_restate as vr
from cases import same_bits

pytestmark = pytest.mark.gpu

METHODS = {"linear": vr.LINEAR, "log": vr.LOG}
MIXED = [vr.ALL_DEFINED, vr.SOME_DEFINED, vr.NONE_DEFINED]


def compare(got, exp, gfd, efd, method, undef, label):
    assert got.shape == exp.shape, label
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if method == "linear":
        if not same_bits(got, exp, nan_payload=False):
            bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
            first = tuple(int(b[0]) for b in bad)
            raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))
        return 0
    isun = (lambda a: np.isnan(a)) if np.isnan(undef) else (lambda a: a == np.float32(undef))
    assert np.array_equal(isun(got), isun(exp)), label
    d = ~isun(exp) & ~(np.isnan(got) & np.isnan(exp))
    gi, ei = got.view(np.int32)[d].astype(np.int64), exp.view(np.int32)[d].astype(np.int64)
    steps = np.abs(gi - ei)  # same sign wherever two neighbouring floats are compared; across zero the difference is huge
    assert steps.size == 0 or steps.max() <= 1, (label, int(steps.max()))
    return int((steps == 1).sum())


def run(ctx, kind, fields, coord, targets, method, device, flags=None, fdef_c=None, undef=vr.UNDEF, ab=None, stacked=True):
    import torch

    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else np.ascontiguousarray
    f = put(fields)
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    if kind == "hybrid":
        out, fd = ctx.vinterp_hlevels(f, put(coord), ab[0], ab[1], targets, method=method, fdefined_in=flags,
                                      fdef_ps=vr.SOME_DEFINED if fdef_c is None else fdef_c, undef=undef)
    else:
        out, fd = ctx.vinterp_fields(f, put(coord), targets, method=method, fdefined_in=flags, fdef_coord=fdef_c, undef=undef)
    return (out.cpu().numpy() if device else out), fd


def check(ctx, kind, fields, coord, targets, method, device, flags=None, fdef_c=None, undef=vr.UNDEF, ab=None, stacked=True, label=None):
    got, gfd = run(ctx, kind, fields, coord, targets, method, device, flags, fdef_c, undef, ab, stacked)
    if flags is not None and np.ndim(flags) == 1:  # one flag per field stands for every level; the restatement takes the table
        flags = np.repeat(np.asarray(flags).reshape(-1, 1), np.shape(fields)[1], axis=1)
    if kind == "hybrid":
        exp, efd = vr.hlevels(fields, coord, ab[0], ab[1], targets, METHODS[method], flags, vr.SOME_DEFINED if fdef_c is None else fdef_c, undef)
    else:
        exp, efd = vr.coord_fields(fields, coord, targets, METHODS[method], flags, fdef_c, undef)
    return compare(got, exp, gfd, efd, method, undef, (label, kind, method, "device" if device else "host"))


@functools.lru_cache(maxsize=None)
def base(nf=3, nlev=12, ny=9, nx=13, seed=1):
    """The main generator and the pressure of its levels as a coordinate batch (the field form of the same problem)."""
    fields, ps, alevel, blevel = vr.main_case(nf, nlev, ny, nx, seed)
    coord = vr.hybrid_coordinate(np.where(ps == vr.UNDEF, np.float32(900), ps), alevel, blevel)
    coord[:, ps == vr.UNDEF] = vr.UNDEF
    for a in (fields, ps, alevel, blevel, coord):
        a.setflags(write=False)
    return fields, ps, (alevel, blevel), coord


def both_kinds(ctx, fields, ps, ab, coord, targets, method, device, **kw):
    n = check(ctx, "hybrid", fields, ps, targets, method, device, ab=ab, **kw)
    return n + check(ctx, "field", fields, coord, targets, method, device, **kw)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("method", ["linear", "log"])
@pytest.mark.parametrize("nf", [1, 3, 8])
def test_main_case_fields_and_memory(gpu_ctx, nf, method, device):
    fields, ps, ab, coord = base(nf)
    both_kinds(gpu_ctx, fields, ps, ab, coord, vr.MAIN_TARGETS, method, device, stacked=(nf != 3), label=("nf", nf))


@pytest.mark.parametrize("nt", [1, 9, 32, 33, 64])
def test_target_counts_across_the_second_pass(gpu_ctx, nt):
    fields, ps, ab, coord = base(3)
    targets = vr.MAIN_TARGETS if nt == 9 else vr.targets_n(nt)
    for method in ("linear", "log"):
        for device in (False, True):
            both_kinds(gpu_ctx, fields, ps, ab, coord, targets, method, device, label=("nt", nt))


@pytest.mark.parametrize("shape", [(2, 9, 13), (12, 5, 1), (12, 7, 16), (5, 3, 300)], ids=["nlev2", "nx1", "nx16", "two_blocks"])
def test_shapes(gpu_ctx, shape):
    nlev, ny, nx = shape  # nx = 16 on the device: four cells per lane; 900 cells: more than one workgroup of single cells
    fields, ps, ab, coord = base(3, nlev, ny, nx, 7)
    for method in ("linear", "log"):
        for device in (False, True):
            both_kinds(gpu_ctx, fields, ps, ab, coord, vr.MAIN_TARGETS, method, device, label=shape)


def test_vector_path_over_several_workgroups(gpu_ctx):
    fields, ps, ab, coord = base(2, 4, 3, 1100)  # 3300 cells, a multiple of 4: four blocks of 1024
    for method in ("linear", "log"):
        both_kinds(gpu_ctx, fields, ps, ab, coord, vr.MAIN_TARGETS, method, True, label="vec4 blocks")


def test_device_batch_offset_by_one_float(gpu_ctx):
    import torch

    fields, ps, ab, coord = base(2, 12, 9, 16)
    n = fields[0].size
    buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(fields.reshape(-1)).cuda()
    batches = [buf[1 + j * n:1 + (j + 1) * n].view(12, 9, 16) for j in range(2)]  # 4 bytes past the 16-byte grid
    out, fd = gpu_ctx.vinterp_hlevels(batches, torch.from_numpy(ps).cuda(), ab[0], ab[1], vr.MAIN_TARGETS)
    exp, efd = vr.hlevels(fields, ps, ab[0], ab[1], vr.MAIN_TARGETS, vr.LINEAR)
    compare(out.cpu().numpy(), exp, fd, efd, "linear", vr.UNDEF, "offset")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bottom_up_and_non_monotone_coordinates(gpu_ctx, device):
    fields, ps, ab, coord = base(3)
    up = (np.ascontiguousarray(ab[0][::-1]), np.ascontiguousarray(ab[1][::-1]))
    rng = np.random.default_rng(11)
    wavy = (coord * rng.uniform(0.5, 1.5, coord.shape)).astype(np.float32)  # pairs that overlap: the first bracket decides
    wavy[coord == vr.UNDEF] = vr.UNDEF
    for method in ("linear", "log"):
        both_kinds(gpu_ctx, fields[:, ::-1], ps, up, coord[::-1], vr.MAIN_TARGETS, method, device, label="bottom-up")
        check(gpu_ctx, "field", fields, wavy, vr.targets_n(9), method, device, label="non-monotone")
    # heights: signed, zero among the values and the targets, equal neighbours (LINEAR only: LOG refuses the targets)
    z = np.round(rng.uniform(-3, 3, coord.shape)).astype(np.float32) * 100
    check(gpu_ctx, "field", fields, z, np.array([-250, -0.0, 0, 100, 300.5], np.float32), "linear", device, label="heights")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_mixed_flags_over_undef_and_nan(gpu_ctx, device):
    fields, ps, ab, coord = base(3)
    rng = np.random.default_rng(3)
    fields = vr.sprinkle(fields, rng, 0.03, np.nan)
    coord = vr.sprinkle(coord, rng, 0.03, np.nan)
    ps = vr.sprinkle(ps, rng, 0.05, np.nan)
    flags = rng.choice(MIXED, size=(3, 12)).astype(np.int32)
    fdef_coord = rng.choice(MIXED, size=12).astype(np.int32)
    for method in ("linear", "log"):
        for fdef_ps in MIXED:
            check(gpu_ctx, "hybrid", fields, ps, vr.MAIN_TARGETS, method, device, flags=flags, fdef_c=fdef_ps, ab=ab, label="flags")
        check(gpu_ctx, "field", fields, coord, vr.MAIN_TARGETS, method, device, flags=flags, fdef_c=fdef_coord, label="flags")
        check(gpu_ctx, "field", fields, coord, vr.MAIN_TARGETS, method, device, flags=flags[:, 0], fdef_c=[vr.ALL_DEFINED] * 12,
              label="one flag per field")


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_nan_as_undef(gpu_ctx, device):
    nan = np.float32(np.nan)
    fields, ps, ab, coord = base(3)
    fields, ps, coord = (np.where(a == vr.UNDEF, nan, a) for a in (fields, ps, coord))
    for method in ("linear", "log"):
        both_kinds(gpu_ctx, fields, ps, ab, coord, vr.MAIN_TARGETS, method, device, undef=nan, label="undef = NaN")


def test_host_call_in_several_bands(gpu_ctx, mifc_env):
    mifc_env("MIFC_VINTERP_CHUNK_MIB", 1)
    # 40 planes of 333 floats per row: 19 rows per MiB, so 50 rows go in three bands, the last one short
    fields, ps, ab, coord = base(3, 12, 50, 333, 9)
    for method in ("linear", "log"):
        check(gpu_ctx, "hybrid", fields, ps, vr.MAIN_TARGETS[:1], method, False, ab=ab, label="bands")
    check(gpu_ctx, "field", fields, coord, vr.targets_n(33), "linear", False, label="bands, two passes")


def test_host_band_without_padding(gpu_ctx, mifc_env):
    mifc_env("MIFC_VINTERP_CHUNK_MIB", 1)
    # 2 + 1 + 1 = 4 planes of 32768 floats per row: two rows fill the MiB exactly and their 65536 floats need no padding, so the
    # planes of the staged band touch; three rows go as a band of two and a band of one
    fields, ps, ab, coord = base(1, 2, 3, 32768, 9)
    check(gpu_ctx, "hybrid", fields, ps, [500], "linear", False, ab=ab, label="unpadded band")


def test_one_batch_drops_the_leading_axis(gpu_ctx):
    import torch

    fields, ps, ab, coord = base(1)
    exp, efd = vr.hlevels(fields, ps, ab[0], ab[1], [850, 500], vr.LINEAR)
    out, fd = gpu_ctx.vinterp_hlevels(fields[0], ps, ab[0], ab[1], [850, 500])
    assert out.shape == (2, 9, 13) and fd.shape == (2,) and same_bits(out, exp[0], nan_payload=False) and list(fd) == list(efd[0])
    o = torch.empty((2, 9, 13), dtype=torch.float32, device="cuda")
    out, fd = gpu_ctx.vinterp_fields(torch.from_numpy(fields[0]).cuda(), torch.from_numpy(coord).cuda(), [850, 500], out=o)
    assert out is o and same_bits(o.cpu().numpy(), exp[0], nan_payload=False) and list(fd) == list(efd[0])


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx, nt = 2, 4, 3, 8, 3
    fields_h, ps_h, ab, coord_h = base(nf, nlev, ny, nx, 2)
    x = torch.from_numpy(fields_h).cuda()
    ps, coord = torch.from_numpy(ps_h).cuda(), torch.from_numpy(coord_h).cuda()
    sentinel = -4242.5
    outs = torch.full((nf, nt, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    cells = ny * nx

    def call(hybrid, nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, nt_=nt, method=0, targets=(850.0, 500.0, 300.0), fields=None, out_ptrs=None, coord_ptr=0,
             a=None, b=None, tg=True, fd_out=True, sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        t = np.asarray(targets, np.float32)
        al, bl = (np.asarray(own if v in (None, "null") else v, np.float32) for v, own in ((a, ab[0]), (b, ab[1])))
        fd = np.full(nf * nt, 7, np.int32)
        common = [t.ctypes.data if tg else None, nt_, method, None if isinstance(out_ptrs, str) else ctypes.addressof(o),
                  fd.ctypes.data if fd_out else None, float(vr.UNDEF), 1]
        head = [c, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_]
        if hybrid:
            cp = ps.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vinterp_hlevels(*head, cp, vr.SOME_DEFINED, None if isinstance(a, str) else al.ctypes.data,
                                          None if isinstance(b, str) else bl.ctypes.data, *common)
        else:
            cp = coord.data_ptr() if coord_ptr == 0 else coord_ptr
            rc = lib.mifc_vinterp_fields(*head, cp, None, *common)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    nan = float("nan")
    # what: (the arguments, the message behind "<entry name>: "; a pair where the two entries word it differently)
    null_head = ("a null pointer (fields, ps, alevel, blevel, targets, fres or fdefined_out)", "a null pointer (fields, coord, targets, fres or fdefined_out)")
    no_level = "level %d: alevel / blevel are no hybrid level (FieldCalculations.cc:298)"
    both = {
        "nlev < 2": (dict(nlev_=1), "nlev < 2"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "ntargets 0": (dict(nt_=0), "ntargets 0 outside 1..64"),
        "ntargets 65": (dict(nt_=65), "ntargets 65 outside 1..64"),
        "negative nx": (dict(nx_=-1), "a negative nx or ny"),
        "negative ny": (dict(ny_=-2), "a negative nx or ny"),
        "null fields": (dict(fields="null"), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or fres[1])"),
        "null coordinate": (dict(coord_ptr=None), null_head),
        "null targets": (dict(tg=False), null_head),
        "null fres": (dict(out_ptrs="null"), null_head),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None]), "a null pointer (fields[1] or fres[1])"),
        "null flags out": (dict(fd_out=False), null_head),
        "unknown method": (dict(method=2), "unknown method 2 (MIFC_VINTERP_LINEAR or MIFC_VINTERP_LOG)"),
        "negative method": (dict(method=-1), "unknown method -1 (MIFC_VINTERP_LINEAR or MIFC_VINTERP_LOG)"),
        "NaN target": (dict(targets=(850.0, nan, 300.0)), "targets[1] is NaN"),
        "LOG with a zero target": (dict(method=1, targets=(850.0, 0.0, 300.0)), "MIFC_VINTERP_LOG with targets[1] <= 0"),
        "LOG with a negative target": (dict(method=1, targets=(-850.0, 500.0, 300.0)), "MIFC_VINTERP_LOG with targets[0] <= 0"),
        "output is an input": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output inside an input": (dict(out_ptrs=[x[0].data_ptr() + 4 * (nlev * cells - 1), outs[1].data_ptr()]), "fres[0] overlaps fields[0]"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr() + 4 * (nt * cells - 1)]), "fres[0] overlaps fres[1]"),
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
    for hybrid, name, cases in ((True, "mifc_vinterp_hlevels: ", {**both, **hybrid_only}), (False, "mifc_vinterp_fields: ", {**both, **field_only})):
        before = {k: t.clone() for k, t in (("x", x), ("ps", ps), ("coord", coord))}
        for what, (kw, tail) in cases.items():
            rc, err, fd = call(hybrid, **kw)
            assert rc == 0 and err == name + (tail if isinstance(tail, str) else tail[0 if hybrid else 1]), (what, err)
            assert (outs == sentinel).all().item() and (fd == 7).all(), what
        assert torch.equal(x, before["x"]) and torch.equal(ps, before["ps"]) and torch.equal(coord, before["coord"])
    with pytest.raises(RuntimeError, match="mifc_vinterp_hlevels"):
        gpu_ctx.vinterp_hlevels(x, ps, ab[0], ab[1], [500], method="cubic")
    with pytest.raises(RuntimeError, match="NaN"):
        gpu_ctx.vinterp_fields(x, coord, [nan])
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
    # afterwards the same calls run
    for hybrid in (True, False):
        rc, err, fd = call(hybrid)
        assert rc == 1 and err == "" and (fd != 7).all()


def test_kindex_from_a_hybrid_batch_on_the_device(gpu_ctx):
    """Device tensors throughout: t and rh on hybrid levels -> 500 / 700 / 850 hPa -> kIndex, bit for bit what kIndex gives
    on the restatement's interpolated fields."""
    import torch

    rng = np.random.default_rng(21)
    nlev, ny, nx = 12, 9, 13
    alevel, blevel = vr.hybrid_levels(nlev)
    eta = np.linspace(0.02, 1, nlev) ** 1.5
    ps = vr.sprinkle(rng.uniform(860, 1050, (ny, nx)).astype(np.float32), rng, 0.03, vr.UNDEF)
    t = (215 + 75 * eta[:, None, None] + rng.normal(0, 2, (nlev, ny, nx))).astype(np.float32)
    rh = rng.uniform(5, 100, (nlev, ny, nx)).astype(np.float32)
    t, rh = vr.sprinkle(t, rng, 0.03, vr.UNDEF), vr.sprinkle(rh, rng, 0.03, vr.UNDEF)
    targets = [500.0, 700.0, 850.0]
    (et, erh), efd = vr.hlevels(np.stack([t, rh]), ps, alevel, blevel, targets, vr.LINEAR)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    out, fd = gpu_ctx.vinterp_hlevels([dev(t), dev(rh)], dev(ps), alevel, blevel, targets)
    assert out.is_cuda and np.array_equal(fd, efd)
    assert (fd == vr.SOME_DEFINED).all()
    k, kfd = gpu_ctx.kIndex(out[0, 0], out[0, 1], out[1, 1], out[0, 2], out[1, 2], 500, 700, 850, 1, fdefined=vr.SOME_DEFINED)
    ek, ekfd = gpu_ctx.kIndex(dev(et[0]), dev(et[1]), dev(erh[1]), dev(et[2]), dev(erh[2]), 500, 700, 850, 1, fdefined=vr.SOME_DEFINED)
    assert k.is_cuda and kfd == ekfd == vr.SOME_DEFINED
    assert same_bits(k.cpu().numpy(), ek.cpu().numpy(), nan_payload=False)
    assert ((k.cpu().numpy() != vr.UNDEF).mean()) > 0.5
