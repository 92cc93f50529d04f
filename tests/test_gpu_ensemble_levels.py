"""The ensemble reductions over a level batch in one pass (mifc_ensemble_levels.hip, mifc_ensemble_levels): for every
level and product bit for bit the oracle's single-field function on that level's slices (a NaN matches any NaN), with
equal flags -- across the kernel-argument / device-table split, the 16-byte and the scalar form, host and device memory,
chunked host staging, every product alone and all fifteen together; the refusals; and the single-field GPU entries."""
import ctypes

import numpy as np
import pytest

from cases import same_bits
from cpulib import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF

pytestmark = pytest.mark.gpu


def make_members(nmem, nlev, ny, nx, seed, undef=UNDEF, specials=True):
    """As in test_gpu_ensemble_quantiles.py: values on a 1/8 grid (many ties), signed zeros, infinities, undef and NaN."""
    rng = np.random.default_rng(seed)
    x = (np.round(rng.normal(0, 3, size=(nmem, nlev, ny, nx)) * 8) / 8).astype(np.float32)
    if specials:
        m = rng.random(x.shape)
        x[m < 0.04] = -0.0
        x[(m >= 0.04) & (m < 0.08)] = 0.0
        x[(m >= 0.08) & (m < 0.10)] = np.inf
        x[(m >= 0.10) & (m < 0.12)] = -np.inf
        x[(m >= 0.12) & (m < 0.17)] = undef
        x[(m >= 0.17) & (m < 0.19)] = np.nan
    return x


def mixed_flags(nmem, nlev, seed):
    return np.random.default_rng(seed).choice([ALL_DEFINED, SOME_DEFINED, NONE_DEFINED], size=(nmem, nlev)).astype(np.int32)


EXTREME = {"max": 1, "min": 2, "argmax": 3, "argmin": 4}
# all fifteen: one of each statistic with an input flag or none, and eight probabilities over the six computes
FULL = ["sum", "mean", "stddev", "max", "min", "argmax", "argmin", ("probability", 1, [0.5]), ("probability", 2, [-0.25]),
        ("probability", 3, [-1.0, 2.0]), ("probability", 4, [1.0]), ("probability", 5, [0.0]), ("probability", 6, [-3.0, 0.125]),
        ("probability", 1, [-2.0, 7.0]), ("probability", 5, [np.inf])]


def with_flags(products, nlev, seed):
    """Gives every sum / extreme product of the list its own per-level input flags."""
    rng = np.random.default_rng(seed)
    out = []
    for p in products:
        name = p if isinstance(p, str) else p[0]
        if name == "sum" or name in EXTREME:
            out.append((name, rng.choice([ALL_DEFINED, SOME_DEFINED, NONE_DEFINED], size=nlev).astype(np.int32)))
        else:
            out.append(p)
    return out


def expected(cpu, x, flags, product, undef=UNDEF):
    """One product on every level through the single-field function of the CPU checker -> (out[nlev][ny][nx], flags[nlev])."""
    nmem, nlev, ny, nx = x.shape
    name = product if isinstance(product, str) else product[0]
    out, fds = np.empty((nlev, ny, nx), np.float32), []
    for l in range(nlev):
        fields = [x[j, l] for j in range(nmem)]
        fin = [int(flags[j, l]) for j in range(nmem)]
        if name == "mean":
            ok, e, fd = cpu.call("meanValue", nx, ny, fields, fin, undef=undef)
        elif name == "stddev":
            ok, e, fd = cpu.call("stddevValue", nx, ny, fields, fin, undef=undef)
        elif name == "sum":
            ok, e, fd = cpu.call("sumFields", nx, ny, fields, fdefined=int(product[1][l]), undef=undef)
        elif name in EXTREME:
            ok, e, fd = cpu.call("extremeValue", nx, ny, EXTREME[name], fields, fdefined=int(product[1][l]), undef=undef)
        else:
            ok, e, fd = cpu.call("probability", nx, ny, product[1], fields, fin, product[2], undef=undef)
        assert ok, (name, l)
        out[l] = e
        fds.append(fd)
    return out, fds


def run(ctx, x, flags, products, undef=UNDEF, device=False, stacked=True):
    import torch

    f = torch.from_numpy(np.ascontiguousarray(x)).cuda() if device else np.ascontiguousarray(x)
    fields = f if stacked else [f[j] for j in range(f.shape[0])]
    res = ctx.ensembleStatistics(fields, products, fdefined_in=flags, undef=undef)
    return [((o.cpu().numpy() if device else o), fd) for o, fd in res]


def check(ctx, cpu, x, flags, products, undef=UNDEF, device=False, stacked=True, label=None):
    res = run(ctx, x, flags, products, undef, device, stacked)
    assert len(res) == len(products)
    for (got, fd), p in zip(res, products):
        exp, efd = expected(cpu, x, flags, p, undef)
        what = (label, p if isinstance(p, str) else p[0], p[1] if not isinstance(p, str) and p[0] == "probability" else None)
        if not same_bits(got, exp, nan_payload=False):
            bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
            first = tuple(int(b[0]) for b in bad)
            raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (what, len(bad[0]), first, got[first], exp[first]))
        assert list(np.atleast_1d(fd)) == efd, what


@pytest.mark.parametrize("nmem", [1, 2, 7, 8, 9, 51, 64, 65, 200])
def test_members_and_levels_all_fifteen(gpu_ctx, oracle, nmem):
    """Both sides of 64 members (kernel arguments / device table) and of 64 levels, host and device, stacked and listed."""
    for k, (nlev, ny, nx) in enumerate(((1, 12, 20), (2, 9, 16), (16, 6, 12), (137, 3, 8))):
        x = make_members(nmem, nlev, ny, nx, 1000 + 10 * nmem + nlev)
        flags = mixed_flags(nmem, nlev, nmem + nlev)
        products = with_flags(FULL, nlev, nmem * 7 + nlev)
        check(gpu_ctx, oracle, x, flags, products, device=(k + nmem) % 2 == 0, stacked=k % 2 == 0, label=(nmem, nlev))
    # the other memory kind once more on the 16-level batch
    check(gpu_ctx, oracle, x[:, :16], flags[:, :16], with_flags(FULL, 16, 5), device=(3 + nmem) % 2 != 0, label=(nmem, 16, "other memory"))


def test_every_single_product_and_shuffled_subsets(gpu_ctx, oracle):
    nmem, nlev, ny, nx = 9, 3, 10, 12
    x = make_members(nmem, nlev, ny, nx, 42)
    flags = mixed_flags(nmem, nlev, 43)
    full = with_flags(FULL, nlev, 44)
    for k, p in enumerate(full):
        check(gpu_ctx, oracle, x, flags, [p], device=k % 2 == 0, label=("single", k))
    rng = np.random.default_rng(45)
    for size in (2, 3, 5, 7, 11, 15):
        idx = rng.permutation(len(full))[:size]
        check(gpu_ctx, oracle, x, flags, [full[i] for i in idx], device=size % 2 == 1, label=("subset", tuple(int(i) for i in idx)))
    # 2-D members: one flag per product back, an int
    res = gpu_ctx.ensembleStatistics(x[:, 1], ["mean", ("max", ALL_DEFINED)], fdefined_in=flags[:, 1])
    for (got, fd), p in zip(res, ["mean", ("max", [ALL_DEFINED])]):
        exp, efd = expected(oracle, x[:, 1:2], flags[:, 1:2], p)
        assert isinstance(fd, int) and fd == efd[0] and got.shape == (ny, nx) and same_bits(got, exp[0], nan_payload=False)


def test_reference_itself(gpu_ctx, ref):
    nmem, nlev, ny, nx = 51, 4, 11, 16
    x = make_members(nmem, nlev, ny, nx, 7)
    check(gpu_ctx, ref, x, mixed_flags(nmem, nlev, 8), with_flags(FULL, nlev, 9), device=True, label="ref")


@pytest.mark.parametrize("nmem", [7, 51, 70])
def test_scalar_form(gpu_ctx, oracle, nmem):
    """nx * ny not a multiple of 4, and members 4 bytes off the 16-byte grid."""
    import torch

    nlev, ny, nx = 3, 11, 13
    x = make_members(nmem, nlev, ny, nx, 77 + nmem)
    flags = mixed_flags(nmem, nlev, 9)
    products = with_flags(FULL, nlev, 10)
    for device in (False, True):
        check(gpu_ctx, oracle, x, flags, products, device=device, label=("ragged", nmem, device))
    ny, nx = 8, 12
    x = make_members(nmem, nlev, ny, nx, 78 + nmem)
    n = nlev * ny * nx
    buf = torch.zeros(nmem * n + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(x.reshape(-1)).cuda()
    members = [buf[1 + j * n:1 + (j + 1) * n].view(nlev, ny, nx) for j in range(nmem)]  # 4 bytes past the grid
    res = gpu_ctx.ensembleStatistics(members, products, fdefined_in=flags)
    for (got, fd), p in zip(res, products):
        exp, efd = expected(oracle, x, flags, p)
        assert same_bits(got.cpu().numpy(), exp, nan_payload=False) and list(fd) == efd, p


def test_nan_as_undef_and_a_level_where_no_member_counts(gpu_ctx, oracle):
    nan = np.float32(np.nan)
    nmem, nlev = 33, 4
    x = make_members(nmem, nlev, 10, 8, 5, undef=nan)
    x[:, 1, 2:5, :] = nan
    flags = np.full((nmem, nlev), SOME_DEFINED, np.int32)
    flags[4, 0] = ALL_DEFINED
    flags[:, 2] = NONE_DEFINED  # probability: nfields_defined == 0 on this level
    x[:, 3] = nan               # mean / stddev: no defined value on this one
    for device in (False, True):
        check(gpu_ctx, oracle, x, flags, with_flags(FULL, nlev, 6), undef=nan, device=device, label=("nan undef", device))
    x = make_members(nmem, nlev, 10, 8, 6)
    x[:, 3] = UNDEF
    check(gpu_ctx, oracle, x, flags, with_flags(FULL, nlev, 7), device=True, label="undef level")


def test_no_members(gpu_ctx, oracle):
    import torch

    nlev, ny, nx = 2, 5, 8
    x = np.empty((0, nlev, ny, nx), np.float32)
    flags = np.empty((0, nlev), np.int32)
    products = ["mean", "stddev", ("sum", np.array([SOME_DEFINED, ALL_DEFINED], np.int32)), ("probability", 1, [0.0])]
    for device in (False, True):
        out = torch.full((4, nlev, ny, nx), -7.0, device="cuda") if device else np.full((4, nlev, ny, nx), -7.0, np.float32)
        res = gpu_ctx.ensembleStatistics([], products, out=out)
        for (got, fd), p in zip(res, products):
            exp, efd = expected(oracle, x, flags, p)
            got = got.cpu().numpy() if device else got
            assert same_bits(got, exp) and list(fd) == efd, (p, device)
    with pytest.raises(RuntimeError, match="without members"):
        gpu_ctx.ensembleStatistics([], ["max"], out=np.zeros((1, ny, nx), np.float32))


def test_host_batches_in_several_chunks(gpu_ctx, oracle, mifc_env):
    mifc_env("MIFC_ENSEMBLE_CHUNK_MIB", 1)
    seven = ["mean", "stddev", "max", "min", ("probability", 1, [0.5]), ("probability", 1, [2.0]), ("probability", 4, [-1.0])]
    # a level larger than the budget (cell ranges, the last one ragged), several levels per chunk, more levels than 64
    for nmem, nlev, ny, nx, products in ((51, 3, 211, 301, seven), (51, 16, 30, 40, FULL), (9, 70, 30, 40, FULL), (70, 5, 33, 45, seven)):
        x = make_members(nmem, nlev, ny, nx, nmem + nlev)
        check(gpu_ctx, oracle, x, mixed_flags(nmem, nlev, nlev), with_flags(products, nlev, nmem), device=False, label=("chunks", nmem, nlev))


# The seams of the chunk plan at the smallest shapes that reach them.  The budget is 1 MiB = 1 048 576 bytes, a staged cell
# costs 4 * (nmem + 4 products) bytes: 256 with 60 members (4 096 cells per MiB), 252 with 59 (4 161).
CHUNK_SEAMS = {
    "a level fits exactly": (60, 3, 64, 64, False),        # 4 096 cells: one level per chunk, no cell split
    "one cell over": (60, 2, 17, 241, False),              # 4 097 cells: ranges of 4 096 and 1
    "a short last chunk of levels": (60, 6, 25, 40, False),  # four levels per chunk: 4 + 2
    "ranges cut at a multiple of 4": (59, 1, 25, 333, False),  # 8 325 cells: 4 161 rounded to 4 160 / 4 160 / 5
    "no members": (0, 2, 6, 8, False),                     # no scratch for members; the flags of `mean`
    "device table, host": (9, 70, 6, 8, False),            # past the 64 levels of the kernel arguments
    "device table, device": (9, 70, 6, 8, True),
}


@pytest.mark.parametrize("case", list(CHUNK_SEAMS))
def test_chunk_seams(gpu_ctx, oracle, mifc_env, case):
    mifc_env("MIFC_ENSEMBLE_CHUNK_MIB", 1)
    nmem, nlev, ny, nx, device = CHUNK_SEAMS[case]
    four = ["mean", "stddev", "max", ("probability", 1, [0.5])]
    x = make_members(nmem, nlev, ny, nx, 7 * nmem + nlev)
    flags = mixed_flags(nmem, nlev, nlev)
    if nmem > 0:
        check(gpu_ctx, oracle, x, flags, with_flags(four, nlev, nmem), device=device, label=case)
        return
    four = ["mean", "stddev", ("sum", np.full(nlev, SOME_DEFINED, np.int32)), ("probability", 1, [0.5])]  # (no extreme without members)
    res = gpu_ctx.ensembleStatistics([], four, out=np.full((4, nlev, ny, nx), -7.0, np.float32))  # the shape comes from the output
    for (got, fd), p in zip(res, four):
        exp, efd = expected(oracle, x, flags, p)
        assert same_bits(got, exp) and list(fd) == efd, p


def test_big_level_counts_through_partials(gpu_ctx, oracle):
    """2 048 workgroups per level and more: the undefined counts go through the per-workgroup table."""
    nmem, nlev, ny, nx = 3, 2, 1100, 2048
    x = make_members(nmem, nlev, ny, nx, 3, specials=False)
    x[:, 0, 100:300, 500:900] = UNDEF
    x[1, 1, 700:, :] = UNDEF
    flags = np.full((nmem, nlev), SOME_DEFINED, np.int32)
    flags[2, 1] = NONE_DEFINED
    products = ["mean", ("sum", np.array([SOME_DEFINED, SOME_DEFINED], np.int32)), ("min", np.array([SOME_DEFINED, ALL_DEFINED], np.int32)),
                ("probability", 2, [0.0])]
    check(gpu_ctx, oracle, x, flags, products, device=True, label="big level")


def test_refusals_write_nothing(gpu_ctx):
    import torch

    import mi_fieldcalc_amd._capi as capi

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nmem, ny, nx, nlev = 5, 6, 8, 2
    x = torch.from_numpy(make_members(nmem, nlev, ny, nx, 1)).cuda()
    sentinel = -4242.5
    outs = torch.full((16, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    fds = np.full((16, nlev), 7, np.int32)

    def product(k, stat, compute=0, limits=(0.0,), out=True, fd=True):
        return dict(stat=stat, compute=compute, limits=limits, out=outs[k].data_ptr() if out is True else out,
                    fd=fds[k].ctypes.data if fd else None)

    def call(products, nx_=nx, ny_=ny, nlev_=nlev, nmem_=nmem, fields=None, nproducts=None, null_products=False, memkind=1, sync=True):
        tab = (ctypes.c_void_p * nmem)(*[x[j].data_ptr() for j in range(nmem)]) if fields is None or fields == "null" else fields
        arr = (capi.EnsProduct * max(len(products), 1))()
        for k, p in enumerate(products):
            arr[k].stat, arr[k].compute, arr[k].nlimits = p["stat"], p["compute"], len(p["limits"])
            for i, v in enumerate(p["limits"][:2]):
                arr[k].limits[i] = v
            arr[k].out, arr[k].fdefined = p["out"], p["fd"]
        rc = lib.mifc_ensemble_levels(c, nx_, ny_, nlev_, None if fields == "null" else ctypes.addressof(tab), None, nmem_,
                                      None if null_products else ctypes.addressof(arr), len(products) if nproducts is None else nproducts,
                                      float(UNDEF), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error()

    SUM, MEAN, STD, EXT, PROB = 0, 1, 2, 3, 4
    mean = [product(0, MEAN)]
    held, shape, null = ": the list holds this statistic already", "nlev < 1, or a negative nx, ny or nmem", "a null pointer (products or fields)"
    between = ": PROBABILITY between two limits with one limit (the reference returns false)"
    cases = {  # what: (the call, the text behind "mifc_ensemble_levels: ")
        "nproducts < 1": (dict(products=mean, nproducts=0), "nproducts < 1"),
        "sixteen products": (dict(products=[product(k, PROB, 1) for k in range(16)]), "more than 15 products"),
        "nine probabilities": (dict(products=[product(k, PROB, 1 + k % 6, (0.0, 1.0)) for k in range(9)]), "more than 8 PROBABILITY products"),
        "two means": (dict(products=[product(0, MEAN), product(1, MEAN)]), "products[1]" + held),
        "two sums": (dict(products=[product(0, SUM), product(1, STD), product(2, SUM)]), "products[2]" + held),
        "two max": (dict(products=[product(0, EXT, 1), product(1, EXT, 1)]), "products[1]" + held),
        "unknown stat": (dict(products=[product(0, 5)]), "products[0]: unknown stat 5"),
        "negative stat": (dict(products=[product(0, -1)]), "products[0]: unknown stat -1"),
        "extreme compute 0": (dict(products=[product(0, EXT, 0)]), "products[0]: EXTREME compute 0 outside 1..4"),
        "extreme compute 5": (dict(products=[product(0, EXT, 5)]), "products[0]: EXTREME compute 5 outside 1..4"),
        "probability compute 0": (dict(products=[product(0, PROB, 0)]), "products[0]: PROBABILITY compute 0 outside 1..6"),
        "probability compute 7": (dict(products=[product(0, PROB, 7)]), "products[0]: PROBABILITY compute 7 outside 1..6"),
        "probability nlimits 0": (dict(products=[product(0, PROB, 1, ())]), "products[0]: PROBABILITY nlimits 0 outside 1..2"),
        "probability nlimits 3": (dict(products=[product(0, PROB, 1, (0.0, 1.0, 2.0))]), "products[0]: PROBABILITY nlimits 3 outside 1..2"),
        "between with one limit (3)": (dict(products=[product(0, PROB, 3)]), "products[0]" + between),
        "between with one limit (6)": (dict(products=[product(0, MEAN), product(1, PROB, 6)]), "products[1]" + between),
        "extreme without members": (dict(products=[product(0, EXT, 2)], nmem_=0), "products[0]: EXTREME without members (the reference returns false)"),
        "nlev < 1": (dict(products=mean, nlev_=0), shape),
        "negative nx": (dict(products=mean, nx_=-1), shape),
        "negative ny": (dict(products=mean, ny_=-3), shape),
        "negative nmem": (dict(products=mean, nmem_=-1), shape),
        "unknown memkind": (dict(products=mean, memkind=7), "unknown memkind 7"),
        "null products": (dict(products=mean, null_products=True), null),
        "null fields": (dict(products=mean, fields="null"), null),
        "null member": (dict(products=mean, fields=(ctypes.c_void_p * nmem)(*([x[0].data_ptr()] * (nmem - 1) + [None]))), "a null pointer (fields[4])"),
        "null output": (dict(products=[product(0, MEAN), product(1, STD, out=None)]), "a null pointer (products[1].out or .fdefined)"),
        "null flags": (dict(products=[product(0, MEAN), product(1, STD, fd=False)]), "a null pointer (products[1].out or .fdefined)"),
        "more than 2^31 - 1 cells": (dict(products=mean, nx_=46341, ny_=46341), "more than 2^31 - 1 cells per level"),
        "same output twice": (dict(products=[product(0, MEAN), product(0, STD)]), "two outputs are the same array or overlap"),
        "outputs overlap": (dict(products=[product(0, MEAN), product(1, STD, out=outs[0].data_ptr() + 4 * ny * nx)]),
                            "two outputs are the same array or overlap"),
        "output is a member": (dict(products=[product(0, MEAN), product(1, STD, out=x[3].data_ptr())]), "products[1].out overlaps fields[3]"),
        "output overlaps a member": (dict(products=[product(0, MEAN, out=x[1].data_ptr() + 16)]), "products[0].out overlaps fields[1]"),
    }
    before = x.clone()

    def untouched():  # the members hold NaN, so their bits are compared
        return (outs == sentinel).all().item() and (fds == 7).all() and torch.equal(x.view(torch.int32), before.view(torch.int32))

    for what, (kw, text) in cases.items():
        rc, err = call(**kw)
        assert rc == 0 and err == "mifc_ensemble_levels: " + text, (what, rc, err)
        assert untouched(), what
    with pytest.raises(ValueError):
        gpu_ctx.ensembleStatistics(x, ["median"])
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err = call(mean, sync=False)
    g.close()
    assert rc == 0 and "capture" in err and untouched()
    # afterwards the same call runs
    rc, err = call(mean)
    assert rc == 1 and err == "" and not (outs[0] == sentinel).any().item() and (fds[0] != 7).all() and (outs[1:] == sentinel).all().item()


@pytest.mark.parametrize("nmem", [4, 51, 66])
def test_equal_to_the_single_field_entries(gpu_ctx, nmem):
    nlev, ny, nx = 3, 15, 20
    x = make_members(nmem, nlev, ny, nx, 90 + nmem)
    flags = mixed_flags(nmem, nlev, 91)
    products = with_flags(FULL, nlev, 92)
    res = gpu_ctx.ensembleStatistics(x, products, fdefined_in=flags)
    for (got, fd), p in zip(res, products):
        name = p if isinstance(p, str) else p[0]
        for l in range(nlev):
            fields, fin = [x[j, l] for j in range(nmem)], [int(v) for v in flags[:, l]]
            if name == "mean":
                e, f = gpu_ctx.meanValue(fields, fin)
            elif name == "stddev":
                e, f = gpu_ctx.stddevValue(fields, fin)
            elif name == "sum":
                e, f = gpu_ctx.sumFields(fields, fdefined=int(p[1][l]))
            elif name in EXTREME:
                e, f = gpu_ctx.extremeValue(EXTREME[name], fields, fdefined=int(p[1][l]))
            else:
                e, f = gpu_ctx.probability(p[1], fields, fin, p[2])
            assert same_bits(got[l], e, nan_payload=False) and fd[l] == f, (name, l)
