"""Ertel potential vorticity of level batches on the GPU (mifc_pvort.hip, mifc_pvort_hlevels / mifc_pvort_fields /
mifc_pvort_levels, through mi_fieldcalc_amd.pvort) against the numpy restatement (tests/pvort_restate.py): bit for bit (a
NaN matches any NaN), flags equal.  Every operation of the definition is an IEEE float or double operation rounded on its
own, and the library is built without contraction: there is no tolerance anywhere."""
import functools

import numpy as np
import pytest

import pvort_restate as pv
import vinterp_restate as vi
from cases import same_bits

pytestmark = pytest.mark.gpu

KINDS = ("hybrid", "field", "levels")
METHODS = (("centred", pv.CENTRED), (pv.WEIGHTED, pv.WEIGHTED))  # (what the call is given: a name or a code, what the restatement is)
A, S_, N = pv.ALL_DEFINED, pv.SOME_DEFINED, pv.NONE_DEFINED
U = pv.UNDEF
LANES_X, TY = 32, 8  # the tile is 32 * v columns by 8 rows; asserted against mifc_last_pvort_form in every comparison


def front():
    from mi_fieldcalc_amd import pvort

    return pvort


def compare(got, exp, gfd, efd, label):
    assert got.shape == exp.shape, label
    if not same_bits(got, exp, nan_payload=False):
        ok = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
        bad = np.nonzero(~ok)
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)


def guarded(a, pad):
    """The array on the device as a view into a larger tensor whose surroundings are NaN."""
    import torch

    a = np.ascontiguousarray(a, np.float32)
    big = torch.full((a.size + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
    view = big[pad:pad + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a.copy()))
    return view


def run(ctx, kind, c, method, device, fcor=True, pad=64, form=None, **kw):
    """One call on the case c (pv_restate.pv_case); device: the inputs are guarded views (pad floats in front: 64 keeps the
    16-byte grid, 65 leaves it) and the output a view into a sentinel-filled tensor, which must be intact around it."""
    import torch

    put = (lambda a: guarded(a, pad)) if device else (lambda a: np.ascontiguousarray(a, np.float32))
    u, v, th, xm, ym = (put(c[k]) for k in ("u", "v", "th", "xmapr", "ymapr"))
    f = put(c["fcoriolis"]) if fcor else None
    sentinel, room = -4242.5, None
    if device:
        n = c["u"].size
        room = torch.full((n + 2 * pad,), sentinel, dtype=torch.float32, device="cuda")
        kw["out"] = room[pad:pad + n].view(c["u"].shape)
    if "fdef_c" in kw:
        kw["fdef_ps" if kind == "hybrid" else "fdef_coord"] = kw.pop("fdef_c")
    if kind == "hybrid":
        out, fd = front().pvort_hlevels(ctx, u, v, th, put(c["ps"]), c["alevel"], c["blevel"], xm, ym, f, method, **kw)
    elif kind == "field":
        out, fd = front().pvort_fields(ctx, u, v, th, put(c["p"]), xm, ym, f, method, **kw)
    else:
        kw.pop("fdef_c", None)
        out, fd = front().pvort_levels(ctx, u, v, th, c["levels"], xm, ym, f, method, **kw)
    if device:
        assert out is kw["out"] and (room[:pad] == sentinel).all().item() and (room[pad + n:] == sentinel).all().item(), "the sentinel around the output"
        out = out.cpu().numpy()
    nx = c["u"].shape[2]
    got = front().last_pvort_form(ctx)
    v4 = 4 if nx % 4 == 0 and (not device or pad % 4 == 0) else 1
    want = {"v": v4, "kind": kind, "method": "weighted" if method in ("weighted", pv.WEIGHTED) else "centred", "tile": "%dx%d" % (LANES_X * v4, TY),
            "launches": 1, "bands": 1}
    want.update(form or {})
    assert got == want, (got, want)
    return out, fd


def expected(kind, c, method, fcor=True, **kw):
    kw = dict(kw)
    flags = kw.pop("fdefined_in", None)
    fdef_c = kw.pop("fdef_c", None)
    f = c["fcoriolis"] if fcor else None
    if kind == "hybrid":
        return pv.hlevels(c["u"], c["v"], c["th"], c["ps"], c["alevel"], c["blevel"], c["xmapr"], c["ymapr"], f, method, flags=flags,
                          fdef_ps=S_ if fdef_c is None else fdef_c, **kw)
    if kind == "field":
        return pv.coord_fields(c["u"], c["v"], c["th"], c["p"], c["xmapr"], c["ymapr"], f, method, flags=flags, fdef_coord=fdef_c, **kw)
    return pv.levels(c["u"], c["v"], c["th"], c["levels"], c["xmapr"], c["ymapr"], f, method, flags=flags, **kw)


@functools.lru_cache(maxsize=None)
def case(nlev, ny, nx, seed=3, frac=0.02):
    return pv.pv_case(nlev, ny, nx, seed, frac=frac)


@pytest.mark.parametrize("kind", KINDS)
def test_main_case(gpu_ctx, kind):
    c = case(13, 9, 12)
    for given, method in METHODS:
        for fcor in (True, False):
            exp, efd = expected(kind, c, method, fcor, scale=-9.8e4)
            assert (exp == U).any() and (exp != U).sum() > exp.size // 2 and (efd == S_).any()
            for device in (False, True):
                got, fd = run(gpu_ctx, kind, c, given, device, fcor, scale=-9.8e4)
                compare(got, exp, fd, efd, (kind, method, fcor, device))


def test_tile_seams(gpu_ctx):
    """nx and ny around the tile, for the 16-byte form (tile 128 x 8) and the dword form (32 x 8); the kinds, the methods,
    nlev 2..5 (the remainders of the slot rotation) and the optional f taken in turn."""
    n = 0
    for v4 in (1, 4):
        tx = LANES_X * v4
        nxs = [3, 4, 5, tx - 1, tx, tx + 1, 2 * tx + 3] + ([tx - 4, tx + 4, 2 * tx + 4] if v4 == 4 else [])
        for nx in nxs:
            for ny in (3, 4, TY, TY + 1, TY + 2, 2 * TY + 1, 2 * TY + 3):
                nlev, kind, (given, method), fcor = 2 + n % 4, KINDS[n % 3], METHODS[(n // 3) % 2], n % 5 != 0
                # (pad 65: a device batch off the 16-byte grid, one cell per lane whatever nx is)
                pad = 65 if v4 == 1 else 64
                c = case(nlev, ny, nx, seed=100 + n, frac=0.0 if n % 2 else 0.03)
                exp, efd = expected(kind, c, method, fcor)
                got, fd = run(gpu_ctx, kind, c, given, True, fcor, pad=pad)
                compare(got, exp, fd, efd, (nx, ny, nlev, kind, method, fcor))
                n += 1
    assert n == 17 * 7


@pytest.mark.parametrize("nlev", [2, 3, 4, 5, 6, 7])
def test_slot_rotation(gpu_ctx, nlev):
    for kind in KINDS:
        for given, method in METHODS:
            c = case(nlev, 5, 8, seed=nlev)
            exp, efd = expected(kind, c, method)
            for device in (True, False):
                got, fd = run(gpu_ctx, kind, c, given, device)
                compare(got, exp, fd, efd, (nlev, kind, method, device))


def test_many_levels(gpu_ctx):
    """The level counters do not share LDS with the number of levels (one word per tile buffer): no limit on nlev follows.
    A 3 x 3 and a 4 x 5 grid with 300 levels, holes on many of them."""
    for ny, nx in ((3, 3), (5, 4)):
        c = case(300, ny, nx, seed=nx, frac=0.05)
        for kind, (given, method) in zip(KINDS, (METHODS[0], METHODS[1], METHODS[1])):
            exp, efd = expected(kind, c, method)
            assert len(set(efd.tolist())) >= 2
            got, fd = run(gpu_ctx, kind, c, given, True)
            compare(got, exp, fd, efd, (ny, nx, kind))


@pytest.mark.parametrize("v4", [1, 4])
def test_holes_at_tile_edges_in_the_ring_and_at_the_end_levels(gpu_ctx, v4):
    tx = LANES_X * v4
    nlev, ny, nx = 6, 2 * TY + 3, 2 * tx + (4 if v4 == 4 else 3)
    base = pv.pv_case(nlev, ny, nx, seed=7, frac=0.0)
    for j, name in enumerate(("u", "v", "th")):
        c = {k: a.copy() for k, a in base.items()}
        a = c[name]
        a[np.isnan(a)] = 1
        for k, bad in ((0, U), (1, np.nan), (nlev - 2, U), (nlev - 1, np.nan)):
            a[k, 3, tx - 1] = a[k, 5, tx] = bad  # the last column of a tile, the first of the next
            a[k, TY, 9] = a[k, TY + 1, 11] = bad  # the last row of a tile (rows 1 .. TY), the first of the next
            a[k, TY, tx - 1] = a[k, TY + 1, tx] = bad  # the tiles' corners
            a[k, 0, 20] = a[k, ny - 1, 22] = a[k, 12, 0] = a[k, 13, nx - 1] = bad  # the ring: neighbours of row 1 / column 1 ...
            a[k, 0, 0] = a[k, ny - 1, nx - 1] = a[k, 0, nx - 1] = a[k, ny - 1, 0] = bad  # ... the corners are nobody's
            a[k, 1, 30] = a[k, 6, 1] = a[k, ny - 2, 5] = a[k, 10, nx - 2] = bad  # row 1 / column 1 reach the ring
        c["ps"][4, tx] = c["ps"][TY, 3] = U
        c["p"][:, 4, tx] = c["p"][:, TY, 3] = U
        for kind in KINDS:
            for given, method in METHODS:
                exp, efd = expected(kind, c, method)
                ends = [0, 1, nlev - 2, nlev - 1]
                assert (exp[ends, 0, 30] == U).all() and (exp[ends, 6, 0] == U).all() and (efd[ends] == S_).all()  # row 1 / column 1 reach the ring
                got, fd = run(gpu_ctx, kind, c, given, True, pad=64 if v4 == 4 else 65)
                compare(got, exp, fd, efd, (name, kind, method))
    # the corners alone change nothing
    c = {k: a.copy() for k, a in base.items()}
    for a in (c["u"], c["v"], c["th"]):
        a[np.isnan(a)] = 1
    exp0, efd0 = expected("field", c, pv.WEIGHTED)
    for a in (c["u"], c["v"], c["th"], c["p"]):
        a[:, ::ny - 1, ::nx - 1] = U
    got, fd = run(gpu_ctx, "field", c, "weighted", True, pad=64 if v4 == 4 else 65)
    compare(got, exp0, fd, efd0, "corners")
    assert (efd0 == A).all()


def test_mixed_flags_all_defined_over_nan_and_nan_as_undef(gpu_ctx):
    c = case(7, 10, 36, seed=9, frac=0.04)
    rng = np.random.default_rng(5)
    flags = rng.choice([A, S_, N], (3, 7))
    flags[0, 0] = flags[2, 0] = A  # the generator's NaN cells lie on level 0: values there
    fdef_c = list(rng.choice([A, S_], 7))
    for kind in KINDS:
        for given, method in METHODS:
            kw = dict(fdefined_in=flags)
            if kind != "levels":
                kw["fdef_c"] = A if kind == "hybrid" else fdef_c
            exp, efd = expected(kind, c, method, **kw)
            assert np.isnan(exp).any() and (exp == U).any()
            for device in (True, False):
                got, fd = run(gpu_ctx, kind, c, given, device, **kw)
                compare(got, exp, fd, efd, (kind, method, device))
    # NaN is the undefined value
    nan = float("nan")
    cn = {k: (np.where(a == U, np.float32(nan), a) if k in ("u", "v", "th", "ps", "p") else a) for k, a in c.items()}
    for kind in KINDS:
        exp, efd = expected(kind, cn, pv.WEIGHTED, undef=nan)
        assert np.isnan(exp).any() and not (exp == U).any() and (efd == S_).any()
        got, fd = run(gpu_ctx, kind, cn, "weighted", True, undef=nan)
        compare(got, exp, fd, efd, (kind, "nan"))


def test_host_bands(gpu_ctx, mifc_env):
    """MIFC_PVORT_CHUNK_MIB=1: 24 planes of 128 columns stage 85 rows, 83 of them owned: 250 rows are four bands, the last of
    one row; 12 planes of 10924 columns stage three rows, one owned.  Holes on the rows at the band boundaries; the same bits
    as the one-band device call."""
    mifc_env("MIFC_PVORT_CHUNK_MIB", 1)
    # (the planes of a call: 4 nlev, the coordinate's, xmapr, ymapr and f; the rows of 1 MiB less two are owned)
    wide = ((5, 250, 128), (82, 83, 84, 165, 166, 167, 248, 249), (("hybrid", METHODS[1], True, 4), ("levels", METHODS[0], False, 3), ("field", METHODS[0], True, 4)))
    thin = ((2, 4, 10924), (0, 1, 2, 3), (("hybrid", METHODS[0], True, 4),))
    for (nlev, ny, nx), rows, calls in (wide, thin):
        c = {k: a.copy() for k, a in pv.pv_case(nlev, ny, nx, seed=13, frac=0.001).items()}
        rng = np.random.default_rng(3)
        for r in rows:
            for a in (c["u"], c["v"], c["th"]):
                a[rng.integers(0, nlev), r, rng.integers(0, nx, 5)] = U
        for kind, (given, method), fcor, bands in calls:
            exp, efd = expected(kind, c, method, fcor)
            got, fd = run(gpu_ctx, kind, c, given, False, fcor, form={"launches": bands, "bands": bands})
            compare(got, exp, fd, efd, (nx, kind, "bands"))
            dev, dfd = run(gpu_ctx, kind, c, given, True, fcor)
            compare(dev, got, dfd, fd, (nx, kind, "device"))
            assert (efd == S_).all()
    mifc_env("MIFC_PVORT_CHUNK_MIB", None)
    got, fd = run(gpu_ctx, kind, c, given, False, fcor)  # the default: one band
    compare(got, exp, fd, efd, "one band")


def bands_of(nlev, ny, nx, coord_planes, n_map, mib=1):
    """The bands of a host call from the rule of the level-batch driver with a halo of one row, restated: the rows that fit
    the budget (each plane padded to 64 floats, one row at least), three staged at least and ny at most, two of the staged
    rows are neighbours unless one band holds every row."""
    planes, budget = 4 * nlev + coord_planes + n_map, mib << 20
    rows = max(1, min(ny, budget // (planes * nx * 4)))
    while rows > 1 and planes * (-(-rows * nx // 64) * 64) * 4 > budget:
        rows -= 1
    staged = min(ny, max(3, rows))
    own = ny if staged >= ny else staged - 2
    return -(-ny // own)


@pytest.mark.parametrize("ny,nx,kind,fcor", [(3, 10924, "hybrid", True), (5, 10924, "hybrid", True), (5, 10926, "field", False), (6, 5464, "levels", True)],
                         ids=["ny3", "ny5_one_row_owned", "ny5_dword_form", "ny6_two_rows_owned"])
def test_host_bands_of_few_rows(gpu_ctx, mifc_env, ny, nx, kind, fcor):
    """MIFC_PVORT_CHUNK_MIB=1, 12 or 11 planes: a row of 10924 floats in 12 planes is half a MiB, fewer than three rows fit, so
    three are staged and one is owned.  ny = 5: five bands; rows 0 and 4 are owned by bands that compute row 1 and row 3 for them
    and do not count them, rows 1 and 3 by bands of their own.  ny = 3: the three staged rows are all there are, so one band
    holds every row whatever the budget (the rule above; there is no way to own one row of three).  nx = 10926: no multiple
    of four, one cell per lane with a halo.  ny = 6 of 5464: four staged, two owned, three bands.  Holes on every row; the
    host call against the restatement and against the one-launch device call, bit for bit, flags included."""
    mifc_env("MIFC_PVORT_CHUNK_MIB", 1)
    nlev = 2
    bands = bands_of(nlev, ny, nx, {"hybrid": 1, "field": nlev, "levels": 0}[kind], 3 if fcor else 2)
    assert bands == {3: 1, 5: 5, 6: 3}[ny]
    c = {k: a.copy() for k, a in pv.pv_case(nlev, ny, nx, seed=17, frac=0.001).items()}
    rng = np.random.default_rng(4)
    for r in range(ny):
        for a in (c["u"], c["v"], c["th"]):
            a[rng.integers(0, nlev), r, rng.integers(0, nx, 5)] = U
    for given, method in METHODS:
        exp, efd = expected(kind, c, method, fcor)
        got, fd = run(gpu_ctx, kind, c, given, False, fcor, form={"launches": bands, "bands": bands})
        compare(got, exp, fd, efd, (ny, nx, kind, method, "bands"))
        dev, dfd = run(gpu_ctx, kind, c, given, True, fcor, pad=64 if nx % 4 == 0 else 65)
        compare(dev, got, dfd, fd, (ny, nx, kind, method, "device"))
        assert (efd == S_).all()


def test_identity_a_absvort_on_the_device(gpu_ctx):
    import torch

    rng = np.random.default_rng(17)
    nlev, ny, nx = 5, 11, 132
    u, v = (rng.normal(0, 1, (nlev, ny, nx)).astype(np.float32) for _ in range(2))
    xm, ym, f = (rng.normal(0, 1, (ny, nx)).astype(np.float32) for _ in range(3))
    levs = (128.0 * np.arange(1, nlev + 1)).astype(np.float32)
    th = np.broadcast_to(levs.reshape(-1, 1, 1), (nlev, ny, nx)).copy()
    dev = lambda a: torch.from_numpy(a.copy()).cuda()  # noqa: E731
    du, dv, dxm, dym, df = dev(u), dev(v), dev(xm), dev(ym), dev(f)
    for given, method in METHODS:
        out, fd = front().pvort_levels(gpu_ctx, du, dv, dev(th), levs, dxm, dym, df, given)
        for k in range(nlev):
            e, flag = gpu_ctx.absvort(du[k], dv[k], dxm, dym, df)
            assert torch.equal(out[k], e) and flag == fd[k] == A, (method, k)  # the whole field, ring included


def test_identity_b_vderiv_on_the_device(gpu_ctx):
    import torch

    c = case(9, 10, 36, seed=21, frac=0.0)
    th = c["th"].copy()
    th[np.isnan(th)] = 300
    th[4, 3, 5] = th[0, 6, 30] = U  # holes at centres: their neighbours differ from vderiv, everything else is it
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    zero, one, ones = dev(np.zeros((10, 36))), dev(np.ones((10, 36))), dev(np.ones((9, 10, 36)))
    yc, xc = torch.arange(10).clamp(1, 8).cuda(), torch.arange(36).clamp(1, 34).cuda()
    near = np.zeros(th.shape, bool)
    for k, y, x in ((4, 3, 5), (0, 6, 30)):
        near[k, y - 1:y + 2, x] = near[k, y, x - 1:x + 2] = True
    keep = torch.from_numpy(~near[:, np.clip(np.arange(10), 1, 8)][:, :, np.clip(np.arange(36), 1, 34)]).cuda()
    for given, method in METHODS:
        for kind in KINDS:
            if kind == "hybrid":
                out, _ = front().pvort_hlevels(gpu_ctx, ones, ones, dev(th), dev(c["ps"]), c["alevel"], c["blevel"], zero, zero, one, given)
                e, _ = gpu_ctx.vderiv_hlevels(dev(th), dev(c["ps"]), c["alevel"], c["blevel"], given)
            elif kind == "field":
                out, _ = front().pvort_fields(gpu_ctx, ones, ones, dev(th), dev(c["p"]), zero, zero, one, given)
                e, _ = gpu_ctx.vderiv_fields(dev(th), dev(c["p"]), given)
            else:
                out, _ = front().pvort_levels(gpu_ctx, ones, ones, dev(th), c["levels"], zero, zero, one, given)
                e, _ = gpu_ctx.vderiv_levels(dev(th), c["levels"], given)
            want = e[:, yc][:, :, xc]
            assert torch.equal(out[keep], want[keep]) and (out[~keep] == float(U)).sum().item() >= 8, (kind, method)


def test_refusals_write_nothing(gpu_ctx):
    import torch

    lib, ctx = gpu_ctx._lib, gpu_ctx._ctx
    nlev, ny, nx = 4, 3, 8
    c = pv.pv_case(nlev, ny, nx, seed=2)
    batch, plane = nlev * ny * nx, ny * nx
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    # the planes between two batches of the test's own, as in test_gpu_vcumul.py
    room = torch.zeros(2 * batch + 4 * plane, dtype=torch.float32, device="cuda")
    xm = room[batch:batch + plane].view(ny, nx).copy_(dev(c["xmapr"]))
    ym = room[batch + plane:batch + 2 * plane].view(ny, nx).copy_(dev(c["ymapr"]))
    fc = room[batch + 2 * plane:batch + 3 * plane].view(ny, nx).copy_(dev(c["fcoriolis"]))
    ps = room[batch + 3 * plane:batch + 4 * plane].view(ny, nx).copy_(dev(c["ps"]))
    # u, v and th one behind the other between two spare batches, so that what lies next to them is the test's own too
    uvt = torch.zeros(5 * batch, dtype=torch.float32, device="cuda")
    u, v, th = (uvt[(1 + j) * batch:(2 + j) * batch].view(nlev, ny, nx).copy_(dev(c[k])) for j, k in enumerate(("u", "v", "th")))
    p = dev(c["p"])
    sentinel = -4242.5
    out = torch.full((nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731

    def call(kind, nx_=nx, ny_=ny, nlev_=nlev, method=0, scale=1.0, u_=u, v_=v, th_=th, coord=0, a=None, b=None, lv=None, xm_=xm, ym_=ym, fc_=fc, out_=out,
             fd_out=True, sync=True):
        al, bl = (np.asarray(own if x in (None, "null") else x, np.float32) for x, own in ((a, c["alevel"]), (b, c["blevel"])))
        lev = np.asarray(c["levels"] if lv is None else lv, np.float32)
        fd = np.full(nlev, 7, np.int32)
        head = [ctx, nx_, ny_, nlev_, ptr(u_), ptr(v_), ptr(th_), None]
        tail = [ptr(xm_), ptr(ym_), ptr(fc_), method, scale, ptr(out_), fd.ctypes.data if fd_out else None, float(U), 1]
        if kind == "hybrid":
            rc = lib.mifc_pvort_hlevels(*head, ptr(ps) if coord == 0 else coord, S_, None if isinstance(a, str) else al.ctypes.data,
                                        None if isinstance(b, str) else bl.ctypes.data, *tail)
        elif kind == "field":
            rc = lib.mifc_pvort_fields(*head, ptr(p) if coord == 0 else coord, None, *tail)
        else:
            rc = lib.mifc_pvort_levels(*head, lev.ctypes.data if coord == 0 else coord, *tail)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    null_head = {"hybrid": "a null pointer (u, v, th, ps, alevel or blevel)", "field": "a null pointer (u, v, th or p)", "levels": "a null pointer (u, v, th or levels)"}
    no_level = "level %d: alevel / blevel are no hybrid level (FieldCalculations.cc:298)"
    small = "nx < 3 or ny < 3: a centred difference needs both neighbours"
    every = {
        "nlev < 2": (dict(nlev_=1), "nlev < 2"),
        "negative nx": (dict(nx_=-1), "a negative nx or ny"),
        "negative ny": (dict(ny_=-2), "a negative nx or ny"),
        "nx < 3": (dict(nx_=2), small),
        "ny < 3": (dict(ny_=1), small),
        "unknown method 2": (dict(method=2), "unknown method 2"),
        "negative method": (dict(method=-1), "unknown method -1"),
        "NaN scale": (dict(scale=float("nan")), "scale is NaN"),
        "null u": (dict(u_=None), null_head),
        "null v": (dict(v_=None), null_head),
        "null th": (dict(th_=None), null_head),
        "null coordinate": (dict(coord=None), null_head),
        "null xmapr": (dict(xm_=None), "a null pointer (xmapr or ymapr)"),
        "null ymapr": (dict(ym_=None), "a null pointer (xmapr or ymapr)"),
        "null fpv": (dict(out_=None), "a null pointer (fpv or fdefined_out)"),
        "null fdefined_out": (dict(fd_out=False), "a null pointer (fpv or fdefined_out)"),
        "output is u": (dict(out_=u), "fpv[0] overlaps fields[0]"),
        "output inside v": (dict(out_=v.data_ptr() + 4 * (batch - 1)), "fpv[0] overlaps fields[1]"),
        "output begins in th": (dict(out_=th.data_ptr() + 4 * (batch - 1)), "fpv[0] overlaps fields[2]"),
        "output ends in u": (dict(out_=u.data_ptr() - 4 * (batch - 1)), "fpv[0] overlaps fields[0]"),
        "output ends in xmapr": (dict(out_=xm.data_ptr() - 4 * (batch - 1)), "fpv[0] overlaps xmapr"),
        "output ends in ymapr": (dict(out_=ym.data_ptr() - 4 * (batch - 1), fc_=None, xm_=fc), "fpv[0] overlaps ymapr"),  # (the plane in front is no input here)
        "output begins in fcoriolis": (dict(out_=fc.data_ptr() + 4 * (plane - 1)), "fpv[0] overlaps fcoriolis"),
    }
    only = {
        "hybrid": {
            "null alevel": (dict(a="null"), null_head),
            "null blevel": (dict(b="null"), null_head),
            "negative alevel": (dict(a=[1.0, -1.0, 2.0, 0.0]), no_level % 1),
            "blevel > 1": (dict(b=[0.0, 0.1, 0.2, 1.5]), no_level % 3),
            "output overlaps ps": (dict(out_=ps.data_ptr() + 4 * (plane - 1)), "fpv[0] overlaps ps"),
        },
        "field": {"output overlaps p": (dict(out_=p.data_ptr() + 4 * (batch - 1)), "fpv[0] overlaps coord")},
        "levels": {"NaN level": (dict(lv=[100, float("nan"), 300, 400]), "levels[1] is NaN")},
    }
    skip = {"hybrid": ("output begins in fcoriolis",), "field": (), "levels": ()}  # (ps lies behind fcoriolis and is named first)
    for kind in KINDS:
        name = {"hybrid": "mifc_pvort_hlevels: ", "field": "mifc_pvort_fields: ", "levels": "mifc_pvort_levels: "}[kind]
        before = room.clone(), uvt.clone(), p.clone()
        for what, (kw, tail) in {**every, **only[kind]}.items():
            if what in skip[kind]:
                continue
            rc, err, fd = call(kind, **kw)
            assert rc == 0 and err == name + (tail[kind] if isinstance(tail, dict) else tail), (kind, what, err)
            assert (out == sentinel).all().item() and (fd == 7).all(), (kind, what)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip((room, uvt, p), before))  # (bits: the case holds NaN)
    with pytest.raises(ValueError, match="mifc_pvort_hlevels: unknown method -1"):
        front().pvort_hlevels(gpu_ctx, u, v, th, ps, c["alevel"], c["blevel"], xm, ym, fc, "spline")
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        refused = [call(kind, sync=False) for kind in KINDS]
    g.close()
    for rc, err, fd in refused:
        assert rc == 0 and "capture" in err and (fd == 7).all()
    assert (out == sentinel).all().item()
    # afterwards the same calls run
    for kind in KINDS:
        rc, err, fd = call(kind)
        assert rc == 1 and err == "" and (fd != 7).all(), (kind, err)
        exp, efd = expected(kind, c, pv.CENTRED)
        compare(out.cpu().numpy(), exp, fd, efd, ("after the refusals", kind))


def test_empty_grid(gpu_ctx):
    z3, z2 = np.zeros((3, 0, 5), np.float32), np.zeros((0, 5), np.float32)
    out, fd = front().pvort_fields(gpu_ctx, z3, z3, z3, z3, z2, z2, z2, "weighted")
    assert out.shape == (3, 0, 5) and fd.shape == (3,) and (fd == A).all()
    z3, z2 = np.zeros((3, 2, 0), np.float32), np.zeros((2, 0), np.float32)
    out, fd = front().pvort_levels(gpu_ctx, z3, z3, z3, [100, 200, 300], z2, z2)
    assert out.shape == (3, 2, 0) and (fd == A).all()


def test_pv_on_model_levels_then_the_dynamic_tropopause_on_the_device(gpu_ctx):
    """The chain the entry exists for, device tensors throughout: potential_vorticity_hlevels (theta by the fused derived
    batch, PV in PVU), then the pressure of the 2 PVU surface by Context.vinterp_fields with PV as the coordinate batch:
    against the two restatements chained (theta taken from the derived batch itself, which has its own tests)."""
    import torch

    rng = np.random.default_rng(41)
    nlev, ny, nx = 15, 9, 16
    alevel, blevel = pv.hybrid_levels(nlev)
    ps = rng.uniform(950, 1040, (ny, nx)).astype(np.float32)
    p = pv.hybrid_coordinate(ps, alevel, blevel)
    t = np.maximum(216.65, 288.15 * (p.astype(np.float64) / 1013.25) ** (1 / 5.2559)).astype(np.float32)  # ICAO, isothermal above
    t += rng.normal(0, 0.2, t.shape).astype(np.float32)
    u, v = (rng.normal(0, 3, (nlev, ny, nx)).astype(np.float32) for _ in range(2))
    xm = np.full((ny, nx), 0.5 / 25000.0, np.float32)  # a 25 km grid
    f = rng.uniform(0.9e-4, 1.3e-4, (ny, nx)).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
    du, dv, dt, dps, dxm, df, dp = dev(u), dev(v), dev(t), dev(ps), dev(xm), dev(f), dev(p)
    pvu, flags = front().potential_vorticity_hlevels(gpu_ctx, du, dv, dt, dps, alevel, blevel, dxm, dxm, df)
    assert pvu.is_cuda and pvu.shape == (nlev, ny, nx) and (flags == A).all()
    assert front().last_pvort_form(gpu_ctx) == {"v": 4, "kind": "hybrid", "method": "weighted", "tile": "128x8", "launches": 1, "bands": 1}
    got = gpu_ctx.hlevel_derived_batch(None, None, dt, None, dps, alevel, blevel, temp=("", 3), ff=False)
    th = got[0]["temp"].cpu().numpy()
    exp, efd = pv.hlevels(u, v, th, ps, alevel, blevel, xm, xm, f, pv.WEIGHTED, scale=-9.8e4)
    compare(pvu.cpu().numpy(), exp, flags, efd, "PVU")
    print("PVU: lowest level %.2f .. %.2f, top level %.1f .. %.1f" % (exp[-1].min(), exp[-1].max(), exp[0].min(), exp[0].max()))
    assert 0.05 < np.median(exp[-3]) < 1.5 and np.median(exp[1]) > 4  # a troposphere and a stratosphere
    p_trop, fd = gpu_ctx.vinterp_fields(dp, pvu, [2.0], fdef_coord=flags)
    e, efd = vi.coord_fields(p[None], exp, np.array([2.0], np.float32), vi.LINEAR, fdef_coord=list(flags))
    assert p_trop.is_cuda and same_bits(p_trop.cpu().numpy(), e[0], nan_payload=False) and list(fd) == list(efd[0])
    found = e[0][0][e[0][0] != U]
    assert found.size > ny * nx // 2 and 100 < np.median(found) < 400  # the tropopause, in hPa
