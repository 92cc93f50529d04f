"""Device tensors and host arrays take the same road through the Python front's call helpers: every level-batch and
batched method is called on the same tiny inputs once as numpy arrays and once as CUDA tensors, and the two answers
agree bit for bit; a given `out` comes back as the same object; an allocated one has the documented shape and lives where
the inputs live.  What the C entries are handed is pinned, for host arrays, by tests/test_python_front_cpu.py; this file
is the part of that a stub library cannot see.  The width 7 is not a multiple of 4, so the kernels' scalar forms run too.
The two fused derived batches refuse a grid whose nx * ny is no multiple of 4 (they walk the cells in fours), so they get
the first four rows of the same fields: 4 x 7."""
import numpy as np
import pytest

import icing_cases as ic
from cases import same_bits

pytestmark = pytest.mark.gpu

NLEV, NY, NX, NPOS, NT = 3, 5, 7, 5, 2
BATCH = (NLEV, NY, NX)
DNY = 4  # rows of the grid of the derived batches
DBATCH = (NLEV, DNY, NX)


def _inputs():
    import mi_fieldcalc_amd as fc
    import mi_fieldcalc_amd.synth as synth

    xm, ym, fcor = synth.grid_maps(NX, NY)
    u, v = synth.wind(NX, NY, 11, nlev=NLEV)
    u2, v2 = synth.wind(NX, NY, 12, nlev=NLEV)
    t, q, ps = synth.thermo(NX, NY, 13, nlev=NLEV)
    al, bl = synth.hybrid_levels(NLEV)
    pairs = np.stack([np.stack([u, v]), np.stack([u2, v2])]).astype(np.float32)
    pairs[0, 0, 1] = synth.sprinkle_undef(pairs[0, 0, 1], 7, 0.15)  # a few undefined values (and a NaN) in one level
    angle = synth.uniform((NY, NX), 14, 0.0, 6.28)
    pangle = synth.uniform((NPOS,), 15, 0.0, 6.28)
    d = {
        "P": pairs, "F2": pairs[0].copy(), "MEM": pairs.reshape((4,) + BATCH).copy(), "T": t, "Q": q, "PS": ps,
        "COORD": (al[:, None, None] + bl[:, None, None] * ps[None]).astype(np.float32), "XM": xm, "YM": ym, "FCOR": fcor,
        "COSA": np.cos(angle), "SINA": np.sin(angle), "COSP": np.cos(pangle), "SINP": np.sin(pangle),
        "XP": synth.uniform((NPOS,), 16, 0.0, NX - 1.0), "YP": synth.uniform((NPOS,), 17, 0.0, NY - 1.0),
        "LO": synth.uniform((NY, NX), 18, 100.0, 300.0), "ICE": np.stack(ic.make_inputs(NX, NY, 19, nlev=NLEV)),
    }
    d.update(DU=d["P"][0, 0][:, :DNY], DV=d["P"][0, 1][:, :DNY], DT=t[:, :DNY], DQ=q[:, :DNY], DPS=ps[:DNY])
    d = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in d.items()}
    return d, dict(AL=al, BL=bl, TG=[300.0, 450.0], LV=[850.0, 700.0, 500.0], UNDEF=fc.UNDEF)


# name -> (call(ctx, a, k, o), [(shape, dtype) of each output that may be given]).  a: the fields, placed; k: the host-side
# arguments; o: the outputs, given or None.  The shapes are the documented ones, and the order is that of the results.
# neighbour_levels takes a batch without undefined values (MEM[2]): like the reference it answers None to anything else.
F32, F64 = "float32", "float64"
METHODS = {
    "vinterp_hlevels": (lambda c, a, k, o: c.vinterp_hlevels(a["F2"], a["PS"], k["AL"], k["BL"], k["TG"], out=o[0]), [((2, NT, NY, NX), F32)]),
    "vinterp_fields": (lambda c, a, k, o: c.vinterp_fields(a["F2"][0], a["COORD"], k["TG"], method="log", out=o[0]), [((NT, NY, NX), F32)]),
    "vlayer_hlevels": (lambda c, a, k, o: c.vlayer_hlevels(a["F2"], a["PS"], k["AL"], k["BL"], ["integral", "max"], 150.0, 600.0, out=o[0]),
                       [((2, 2, NY, NX), F32)]),
    "vlayer_fields": (lambda c, a, k, o: c.vlayer_fields([a["F2"][0], a["F2"][1]], a["COORD"], "mean", lo=a["LO"], out=o[0]), [((2, 1, NY, NX), F32)]),
    "vderiv_hlevels": (lambda c, a, k, o: c.vderiv_hlevels(a["F2"], a["PS"], k["AL"], k["BL"], out=o[0]), [((2,) + BATCH, F32)]),
    "vderiv_fields_only": (lambda c, a, k, o: c.vderiv_fields(a["F2"], a["COORD"], method="weighted", magnitude="only", out=o[0]), [((1,) + BATCH, F32)]),
    "vderiv_levels_also": (lambda c, a, k, o: c.vderiv_levels(a["F2"], k["LV"], magnitude="also", out=None if o[0] is None else (o[0], o[1])),
                           [((2,) + BATCH, F32), ((1,) + BATCH, F32)]),
    "hinterp_levels": (lambda c, a, k, o: c.hinterp_levels(a["F2"], a["XP"], a["YP"], method="bicubic", out=o[0]), [((2, NLEV, NPOS), F32)]),
    "hinterp_vector_levels": (lambda c, a, k, o: c.hinterp_vector_levels(a["P"], a["XP"], a["YP"], a["COSP"], a["SINP"], out=o[0]),
                              [((2, 2, NLEV, NPOS), F32)]),
    "vrotate_levels": (lambda c, a, k, o: c.vrotate_levels(a["P"], a["COSA"], a["SINA"], out=o[0]), [((2, 2) + BATCH, F32)]),
    "vrotate_levels_one": (lambda c, a, k, o: c.vrotate_levels([a["P"][0, 0], a["P"][0, 1]], a["COSA"], a["SINA"], out=o[0]), [((2,) + BATCH, F32)]),
    "hstats_levels": (lambda c, a, k, o: c.hstats_levels(a["F2"], mode="rows", weight=a["COSA"], pivot=2.0, want_mean=True, out=o[0]),
                      [((2, NLEV, NY, 8), F64)]),
    "ensembleQuantiles": (lambda c, a, k, o: c.ensembleQuantiles(a["MEM"], [25.0, 75.0], out=o[0]), [((2,) + BATCH, F32)]),
    "ensembleStatistics": (lambda c, a, k, o: c.ensembleStatistics(a["MEM"], ["mean", "max", ("probability", 1, [0.0])], out=None if o[0] is None else o),
                           [(BATCH, F32)] * 3),
    "neighbour_levels": (lambda c, a, k, o: c.neighbour_levels("functions", 1, a["MEM"][2], [1, 1], out=o[0]), [(BATCH, F32)]),
    "vesselIcing_levels": (lambda c, a, k, o: c.vesselIcing_levels("modstall", [a["ICE"][j] for j in range(11)], out=o[0], **ic.SCALARS), [(BATCH, F32)]),
    "vortdiv_levels": (lambda c, a, k, o: c.vortdiv_levels(a["F2"][0], a["F2"][1], a["XM"], a["YM"], rvort=o[0], diverg=o[1]), [(BATCH, F32)] * 2),
    "stencil_levels": (lambda c, a, k, o: c.stencil_levels("vortdiv", a["F2"][0], a["F2"][1], a["XM"], a["YM"], out0=o[0], out1=o[1]), [(BATCH, F32)] * 2),
    "stencil_levels_ex": (lambda c, a, k, o: c.stencil_levels_ex("advection", a["T"], a["F2"][0], a["F2"][1], a["XM"], a["YM"], scalar=6.0, out0=o[0]),
                          [(BATCH, F32)]),
    "hlevel_derived_levels": (lambda c, a, k, o: c.hlevel_derived_levels(a["DU"], a["DV"], a["DT"], a["DQ"], a["DPS"], k["AL"], k["BL"],
                                                                         out=None if o[0] is None else dict(zip(("ff", "rh", "theta"), o))), [(DBATCH, F32)] * 3),
    "hlevel_derived_batch": (lambda c, a, k, o: c.hlevel_derived_batch(a["DU"], a["DV"], a["DT"], a["DQ"], a["DPS"], k["AL"], k["BL"], temp=("", 3), hum=("", 1),
                                                                       dd=True, out=None if o[0] is None else dict(zip(("ff", "temp", "hum", "dd"), o))),
                             [(DBATCH, F32)] * 4),
}


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def _leaves(x):
    """The arrays, tensors and flags of a result, in order."""
    if x is None:
        return []
    if type(x).__name__ == "HstatsResult":
        return [x.stats, x.mean_batch, x.mean_flags] + [np.asarray(x.pivot)]
    if isinstance(x, (tuple, list)):
        return [leaf for y in x for leaf in _leaves(y)]
    if isinstance(x, dict):
        return [leaf for key in sorted(x) for leaf in _leaves(x[key])]
    return [x]


def _host(x):
    return x.cpu().numpy() if _is_tensor(x) else np.asarray(x)


def _same(a, b, what):
    a, b = _host(a), _host(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == np.float32:
        assert same_bits(a, b), what
    elif a.dtype == np.float64:
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), what
    else:
        assert np.array_equal(a, b), what


@pytest.fixture(scope="module")
def placed():
    import torch

    d, k = _inputs()
    for a in d.values():
        a.setflags(write=False)
    return d, {name: torch.from_numpy(a.copy()).cuda() for name, a in d.items()}, k


@pytest.mark.parametrize("name", sorted(METHODS))
def test_host_and_device_take_the_same_road(gpu_ctx, placed, name):
    import torch

    host, dev, k = placed
    call, outs = METHODS[name]
    nothing = [None] * len(outs)
    on_host, on_dev = call(gpu_ctx, host, k, nothing), call(gpu_ctx, dev, k, nothing)
    assert on_host is not None and on_dev is not None
    lh, ld = _leaves(on_host), _leaves(on_dev)
    assert len(lh) == len(ld)
    for i, (h, g) in enumerate(zip(lh, ld)):
        _same(h, g, (name, "host against device", i))
    # allocated outputs: the documented shapes, where the inputs live (flags and pivots are host arrays everywhere)
    where = [i for i, x in enumerate(ld) if _is_tensor(x)]
    assert [tuple(ld[i].shape) for i in where][: len(outs)] == [shape for shape, _ in outs], name
    assert all(ld[i].is_cuda for i in where) and all(isinstance(lh[i], np.ndarray) for i in where), name
    # given outputs come back as the same objects, and hold the same answer
    for fields, tensors in ((host, False), (dev, True)):
        if tensors:
            given = [torch.full(shape, -1.0, dtype=getattr(torch, dtype), device="cuda") for shape, dtype in outs]
        else:
            given = [np.full(shape, -1.0, dtype) for shape, dtype in outs]
        leaves = _leaves(call(gpu_ctx, fields, k, given))
        for j, g in enumerate(given):
            assert any(x is g for x in leaves), (name, "device" if tensors else "host", "output %d is another object" % j)
        for i, (h, g) in enumerate(zip(lh, leaves)):
            _same(h, g, (name, "given outputs", "device" if tensors else "host", i))


def test_prepared_enqueue_calls_repeat_the_direct_ones(gpu_ctx, placed):
    """prepare() around two vortdiv_levels_enqueue calls; the PreparedCalls launched twice leaves what the direct calls left."""
    import torch

    _, dev, _ = placed
    u, v, u2, v2 = dev["P"][0, 0], dev["P"][0, 1], dev["P"][1, 0], dev["P"][1, 1]
    maps = (dev["XM"], dev["YM"])

    def enqueue(outs, counts):
        assert gpu_ctx.vortdiv_levels_enqueue(u, v, *maps, outs[0], outs[1], n_undefined=counts[0])
        assert gpu_ctx.vortdiv_levels_enqueue(u2, v2, *maps, outs[2], None, fdefined=[0, 2, 0], n_undefined=counts[1])

    def fresh():
        return [torch.full(BATCH, -1.0, device="cuda") for _ in range(3)], [torch.full((NLEV,), -1, dtype=torch.int64, device="cuda") for _ in range(2)]

    direct, direct_counts = fresh()
    enqueue(direct, direct_counts)
    torch.cuda.synchronize()
    again, counts = fresh()
    prepared = gpu_ctx.prepare(lambda: enqueue(again, counts))
    assert len(prepared) == 2
    for _ in range(2):
        for t in again + counts:
            t.fill_(-1)
        assert prepared.launch()
        torch.cuda.synchronize()
        for i, (d, a) in enumerate(zip(direct + direct_counts, again + counts)):
            _same(d, a, ("prepared", i))
