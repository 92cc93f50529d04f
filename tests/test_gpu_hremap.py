"""Level batches regridded by a weight table on the GPU (mifc_hremap.hip, mifc_hremap_levels) against the numpy restatement
(tests/hremap_restate.py): bit for bit (a NaN matches any NaN), flags equal, both modes, host and device memory.  No
tolerance: every operation of the definition is an IEEE double operation rounded on its own, and the library is built
without contraction.  Every table reaches the GPU through a plan, which validates it: no test feeds the kernel an index
the plan did not check."""
import ctypes
import functools

import numpy as np
import pytest

import hremap_restate as hr
from cases import same_bits
from gpu_util import run_is_forced

pytestmark = pytest.mark.gpu

MIXED = [hr.ALL_DEFINED, hr.SOME_DEFINED, hr.NONE_DEFINED]
MODES = (("strict", hr.STRICT, 0.0), (hr.RENORM, hr.RENORM, 0.0), ("renorm", hr.RENORM, 0.5), ("renorm", hr.RENORM, 1.0))  # (given, the restatement's, min_frac)


def hremap():
    from mi_fieldcalc_amd import hremap as module

    return module


def compare(got, exp, gfd, efd, label):
    assert got.shape == exp.shape, (label, got.shape, exp.shape)
    assert np.array_equal(np.asarray(gfd), np.asarray(efd)), (label, gfd, efd)
    if not same_bits(got, exp, nan_payload=False):
        bad = np.nonzero((got.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(got) & np.isnan(exp)))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, got[first], exp[first]))


def run(ctx, plan, fields, mode, min_frac, device, flags=None, undef=hr.UNDEF, stacked=True, out=None, dst_shape=None):
    import torch

    put = (lambda a: torch.from_numpy(np.array(a, order="C")).cuda()) if device else np.ascontiguousarray
    f = put(fields)
    f = f if stacked else [f[j] for j in range(f.shape[0])]
    res, fd = hremap().hremap_levels(ctx, plan, f, mode, min_frac, fdefined_in=flags, undef=undef, out=out, dst_shape=dst_shape)
    return (res.cpu().numpy() if device else res), fd


def check(ctx, plan, table, fields, mode, device, flags=None, undef=hr.UNDEF, stacked=True, label=None):
    given, code, min_frac = mode
    got, fd = run(ctx, plan, fields, given, min_frac, device, flags, undef, stacked)
    exp, efd = expected(table, fields, code, min_frac, flags, undef)
    compare(got, exp, fd, efd, (label, code, min_frac, "device" if device else "host"))


def expected(table, fields, code, min_frac=0.0, flags=None, undef=hr.UNDEF):
    if flags is not None and np.size(flags) == len(fields) != np.size(fields[:, :, 0, 0]):  # one flag per field stands for every level
        flags = np.repeat(np.asarray(flags).reshape(-1, 1), fields.shape[1], axis=1)
    return hr.remap(fields, *table, code, min_frac, flags, undef)


@functools.lru_cache(maxsize=None)
def base(nf=3, nlev=5, ny=9, nx=13, ndst=600, seed=1):
    fields, table = hr.main_case(nf, nlev, ny, nx, ndst, seed)
    for a in (fields,) + table:
        a.setflags(write=False)
    return fields, table


def form(ctx, **expected_keys):
    """The launch shape of the last call, checked key by key -- unless the run forces a path."""
    got = hremap().last_hremap_form(ctx)
    if not run_is_forced():
        for key, value in expected_keys.items():
            assert got.get(key) == value, (key, value, got)
    return got


def make_plan(ctx, table, nsrc, device=False):
    import torch

    t = [torch.from_numpy(np.array(a)).cuda() for a in table] if device else [np.array(a) for a in table]
    return hremap().Plan(ctx, *t, nsrc=nsrc)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 8])  # an untested launch takes 4 fields, a tested one 2
def test_main_case_fields_modes_and_memory(gpu_ctx, nf, device):
    fields, table = base(nf)
    flags = np.random.default_rng(nf).choice(MIXED, size=(nf, 5)).astype(np.int32)
    flags[0, :3] = MIXED
    every = np.full((nf, 5), hr.ALL_DEFINED, np.int32)
    with make_plan(gpu_ctx, table, 117, device) as plan:
        for mode in MODES:
            check(gpu_ctx, plan, table, fields, mode, device, stacked=(nf != 3), label=("nf", nf))
            form(gpu_ctx, mode="strict" if mode[1] == hr.STRICT else "renorm", nf=min(nf, 2), tested=1, launches=-(-nf // 2), blocks=3, width=17)
            check(gpu_ctx, plan, table, fields, mode, device, flags=flags, stacked=(nf != 3), label=("nf", nf, "mixed flags"))
            check(gpu_ctx, plan, table, fields, mode, device, flags=every, stacked=(nf != 3), label=("nf", nf, "untested"))
            form(gpu_ctx, nf=min(nf, 4), tested=0, launches=-(-nf // 4), blocks=3)


@pytest.mark.parametrize("ndst", [1, 63, 64, 65, 256, 257, 1100])  # one lane, the slice seam, the workgroup seam, several workgroups
def test_destinations(gpu_ctx, ndst):
    fields, table = base(2, 3, 9, 13, ndst, 3)
    with make_plan(gpu_ctx, table, 117) as plan:
        assert plan.info() == {"nnz": int(table[0][-1]), "max_row": int(np.diff(table[0]).max()), "empty_rows": int((np.diff(table[0]) == 0).sum())}
        for device in (False, True):
            for mode in MODES:
                check(gpu_ctx, plan, table, fields, mode, device, label=("ndst", ndst))
        form(gpu_ctx, blocks=-(-ndst // 256))


@pytest.mark.parametrize("nlev", [1, 2, 3, 4, 7, 8, 13])  # every remainder of the register blocks of four and of eight levels
def test_levels(gpu_ctx, mifc_env, nlev):
    fields, table = base(3, nlev, 12, 16, 300, 4)
    flags = np.random.default_rng(nlev).choice(MIXED, size=(3, nlev)).astype(np.int32)
    every = np.full((3, nlev), hr.ALL_DEFINED, np.int32)
    with make_plan(gpu_ctx, table, 192) as plan:
        for mode in MODES:
            check(gpu_ctx, plan, table, fields, mode, True, flags=flags, label=("nlev", nlev))
        # five slices, two workgroups per level chunk: so few destinations are spread over the device level by level
        form(gpu_ctx, blocks=2, chunk=1, level_chunks=nlev)
        # all levels in one workgroup: register blocks of eight (one field; two untested), of four, and the remainders
        mifc_env("MIFC_HREMAP_LEVEL_CHUNK", 16)
        for nf in (1, 2, 3):
            for device in (False, True):
                for mode in MODES:
                    check(gpu_ctx, plan, table, fields[:nf], mode, device, flags=flags[:nf], label=("nlev", nlev, "nf", nf))
                    form(gpu_ctx, blocks=2, chunk=nlev, level_chunks=1, nf=min(nf, 2), tested=1)
                    check(gpu_ctx, plan, table, fields[:nf], mode, device, flags=every[:nf], label=("nlev", nlev, "nf", nf, "untested"))
                    form(gpu_ctx, blocks=2, chunk=nlev, level_chunks=1, nf=nf, tested=0)


def pattern_table(name, nsrc, seed):
    rng = np.random.default_rng(seed)
    if name == "all empty":
        lengths = np.zeros(70, np.int64)
    elif name == "lengths 0..63 in one slice":
        lengths = np.arange(64)
    elif name == "one row of 300 among short ones":
        lengths = np.full(130, 2)
        lengths[70] = 300
    elif name == "a last partial slice":
        lengths = rng.integers(1, 6, 64 + 5)
    else:
        lengths = rng.integers(1, 8, 100)
    rowptr, col, w = hr.table_from_lengths(lengths, nsrc, seed)
    if name == "columns 0 and nsrc - 1":
        col[::2], col[1::2] = 0, nsrc - 1
    elif name == "repeated and descending columns":
        for d in range(lengths.size):
            n = rowptr[d + 1] - rowptr[d]
            col[rowptr[d]:rowptr[d + 1]] = (np.arange(n, 0, -1) // 2 + d) % nsrc
    return (rowptr, col, w), int(lengths.max()), -(-lengths.size // 256)


PATTERNS = ["all empty", "lengths 0..63 in one slice", "one row of 300 among short ones", "a last partial slice", "columns 0 and nsrc - 1",
            "repeated and descending columns"]


@pytest.mark.parametrize("name", PATTERNS)
def test_row_length_patterns(gpu_ctx, name):
    fields = hr.main_fields(2, 3, 9, 13, seed=11)
    table, width, blocks = pattern_table(name, 117, len(name))
    flags = np.array([[hr.ALL_DEFINED, hr.SOME_DEFINED, hr.NONE_DEFINED], [hr.SOME_DEFINED, hr.ALL_DEFINED, hr.SOME_DEFINED]], np.int32)
    with make_plan(gpu_ctx, table, 117, device=True) as plan:
        assert plan.info()["max_row"] == width
        for device in (False, True):
            for mode in MODES:
                check(gpu_ctx, plan, table, fields, mode, device, label=name)
                form(gpu_ctx, width=width, blocks=blocks, tested=1)
                check(gpu_ctx, plan, table, fields, mode, device, flags=flags, label=(name, "mixed flags"))
                check(gpu_ctx, plan, table, fields, mode, device, flags=[hr.ALL_DEFINED] * 2, label=(name, "untested"))
                form(gpu_ctx, width=width, tested=0)
    if name == "all empty":
        with make_plan(gpu_ctx, table, 117) as plan:
            got, fd = run(gpu_ctx, plan, fields, "strict", 0.0, True, flags=[hr.ALL_DEFINED] * 2)
        assert (got == hr.UNDEF).all() and (fd == hr.NONE_DEFINED).all()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_holes_values_weights_and_undef(gpu_ctx, device):
    fields, _ = base(2, 3)
    fields = fields.copy()
    table = hr.table_from_lengths(hr.main_lengths(300, 5), 117, 5, negative=True)  # negative weights: Wdef may cancel
    quarter = hr.table_from_lengths(np.full(200, 4), 117, 6)
    quarter[2][:] = 0.25  # four weights of 0.25: min_frac 0.5 lies exactly on the threshold of two holes
    stored = np.array([[hr.ALL_DEFINED] * 3, [hr.SOME_DEFINED, hr.ALL_DEFINED, hr.SOME_DEFINED]], np.int32)
    for tab in (table, quarter):
        with make_plan(gpu_ctx, tab, 117) as plan:
            for mode in MODES:
                check(gpu_ctx, plan, tab, fields, mode, device, label="holes")
                # a stored undef under ALL_DEFINED is a value: it is summed, and never counted
                check(gpu_ctx, plan, tab, fields, mode, device, flags=stored, label="stored undef")
                # NaN and infinity among the values, tested and as values
                special = fields.copy()
                special[0, 0, 2, 3], special[0, 1, 4, 5], special[1, 1, 0, 0], special[1, 2, 8, 12] = np.nan, np.inf, -np.inf, np.nan
                check(gpu_ctx, plan, tab, special, mode, device, label="NaN and infinity")
                check(gpu_ctx, plan, tab, special, mode, device, flags=stored, label="NaN and infinity as values")
                # a non-default undef: NaN, and a plain number
                nan = np.float32(np.nan)
                check(gpu_ctx, plan, tab, np.where(fields == hr.UNDEF, nan, fields), mode, device, undef=nan, label="undef = NaN")
                check(gpu_ctx, plan, tab, np.where(fields == hr.UNDEF, np.float32(-999), fields), mode, device, undef=np.float32(-999), label="undef = -999")
    exp, _ = expected(quarter, fields, hr.RENORM, 0.5)
    strict, _ = expected(quarter, fields, hr.STRICT)
    assert ((exp != hr.UNDEF) & (strict == hr.UNDEF)).sum() > 20 and ((exp == hr.UNDEF).sum() > 0)  # both sides of the threshold occur


def test_one_result_for_all_launch_shapes(gpu_ctx, mifc_env):
    fields, table = base(3, 7, 9, 13, 300, 4)
    flags = np.random.default_rng(7).choice(MIXED, size=(3, 7)).astype(np.int32)
    with make_plan(gpu_ctx, table, 117) as plan:
        for chunk in (1, 2, 3, 5, 6, 7, 50):  # one level per workgroup, remainders, a block and a remainder, one chunk, more than there are
            mifc_env("MIFC_HREMAP_LEVEL_CHUNK", chunk)
            for mode in MODES[:2]:
                check(gpu_ctx, plan, table, fields, mode, True, flags=flags, label=("levels per workgroup", chunk))
                form(gpu_ctx, chunk=min(chunk, 7), level_chunks=-(-7 // min(chunk, 7)))
        mifc_env("MIFC_HREMAP_LEVEL_CHUNK", None)
        # few destinations, many levels: one level per workgroup spreads them over the device
        deep = hr.main_fields(2, 37, 9, 13, seed=6)
        check(gpu_ctx, plan, table, deep, MODES[0], True, label="300 x 37")
        form(gpu_ctx, blocks=2, tested=1, chunk=1, level_chunks=37)
    # many destinations: one register block per workgroup -- eight levels of one field, four of three --, the last chunk shorter
    rng = np.random.default_rng(8)
    table = hr.table_from_lengths(rng.integers(0, 4, 530000), 192, 8)
    f = hr.main_fields(3, 9, 12, 16, seed=8)
    every = np.full((3, 9), hr.ALL_DEFINED, np.int32)
    with make_plan(gpu_ctx, table, 192) as plan:
        check(gpu_ctx, plan, table, f[:1], MODES[1], True, label="530 000 x 9, one field")
        form(gpu_ctx, blocks=2071, chunk=8, level_chunks=2, launches=1)
        check(gpu_ctx, plan, table, f, MODES[0], True, flags=every, label="530 000 x 9, three fields untested")
        form(gpu_ctx, blocks=2071, chunk=4, level_chunks=3, launches=1)


def test_host_call_in_several_level_chunks_equals_one_device_call(gpu_ctx, mifc_env):
    mifc_env("MIFC_HREMAP_CHUNK_MIB", 1)
    # 2 fields x (300 x 333 cells + 500 destinations) x 4 bytes = 803 200 bytes per level: one level per chunk, five chunks
    rng = np.random.default_rng(9)
    f = hr.sprinkle(rng.normal(280, 10, (2, 5, 300, 333)).astype(np.float32), rng, 0.03, hr.UNDEF)
    table = hr.table_from_lengths(rng.integers(0, 9, 500), 300 * 333, 9)
    flags = rng.choice(MIXED, size=(2, 5)).astype(np.int32)
    with make_plan(gpu_ctx, table, 300 * 333) as plan:
        for mode in MODES[:2]:
            host, hfd = run(gpu_ctx, plan, f, mode[0], mode[2], False, flags=flags)
            form(gpu_ctx, launches=5, blocks=2, level_chunks=1, chunk=1)
            dev, dfd = run(gpu_ctx, plan, f, mode[0], mode[2], True, flags=flags)
            form(gpu_ctx, launches=1, chunk=1, level_chunks=5)
            compare(host, dev, hfd, dfd, "host in chunks against one device call")
            exp, efd = expected(table, f, mode[1], mode[2], flags)
            compare(dev, exp, dfd, efd, "level chunks")
    # 5 fields x (40 x 50 + 500) x 4 = 50 000 bytes per level: 20 levels per chunk, 37 levels in two chunks, the second shorter
    f = hr.sprinkle(rng.normal(280, 10, (5, 37, 50, 40)).astype(np.float32), rng, 0.03, hr.UNDEF)
    table = hr.table_from_lengths(rng.integers(0, 9, 500), 2000, 10)
    with make_plan(gpu_ctx, table, 2000) as plan:
        check(gpu_ctx, plan, table, f, MODES[1], False, label="two level chunks")
        form(gpu_ctx, launches=2 * 3)


def test_out_offsets_and_listed_fields(gpu_ctx):
    import torch

    fields, table = base(2, 5)
    n, ndst = fields[0].size, 600
    exp, efd = expected(table, fields, hr.STRICT)
    with make_plan(gpu_ctx, table, 117) as plan:
        # pointers 4 bytes past the 16-byte grid, listed fields, out= given
        buf = torch.zeros(2 * n + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(np.array(fields).reshape(-1)).cuda()
        batches = [buf[1 + j * n:1 + (j + 1) * n].view(5, 9, 13) for j in range(2)]
        obuf = torch.zeros(2 * 5 * ndst + 1, dtype=torch.float32, device="cuda")
        out, fd = hremap().hremap_levels(gpu_ctx, plan, batches, out=obuf[1:].view(2, 5, ndst))
        compare(out.cpu().numpy(), exp, fd, efd, "offset by one float")
        assert float(obuf[0]) == 0.0 and out.data_ptr() == obuf.data_ptr() + 4
        # nothing around the output is written; dst_shape
        sentinel = np.float32(-4242.5)
        pool = torch.full((3, 2, 5, 20, 30), float(sentinel), dtype=torch.float32, device="cuda")
        out, fd = hremap().hremap_levels(gpu_ctx, plan, torch.from_numpy(np.array(fields)).cuda(), out=pool[1], dst_shape=(20, 30))
        got = pool.cpu().numpy()
        compare(got[1].reshape(2, 5, 600), exp, fd, efd, "out on the device")
        assert tuple(out.shape) == (2, 5, 20, 30) and (got[0] == sentinel).all() and (got[2] == sentinel).all()
        hpool = np.full((3, 5, 600), sentinel, np.float32)
        out, fd = hremap().hremap_levels(gpu_ctx, plan, fields[1], out=hpool[1])
        assert np.shares_memory(out, hpool[1]) and fd.shape == (5,)
        compare(hpool[1], exp[1], fd, efd[1], "out on the host")
        assert (hpool[0] == sentinel).all() and (hpool[2] == sentinel).all()


def test_conservative_coarsening_composes_with_hstats(gpu_ctx):
    import torch

    rng = np.random.default_rng(21)
    x = rng.integers(-40, 40, (5, 12, 16)).astype(np.float32)  # (sums of four such values times 0.25 are exact)
    table = hremap().conservative_weights_regular(np.arange(17), np.arange(13), np.arange(0, 17, 2), np.arange(0, 13, 2))
    every = np.full(5, hr.ALL_DEFINED, np.int32)
    with make_plan(gpu_ctx, table, 192) as plan:
        out, fd = hremap().hremap_levels(gpu_ctx, plan, torch.from_numpy(x).cuda(), fdefined_in=every, dst_shape=(6, 8))
        assert out.is_cuda and tuple(out.shape) == (5, 6, 8) and (fd == hr.ALL_DEFINED).all()
        exp, efd = expected(table, x[None], hr.STRICT, flags=every[None])
        compare(out.cpu().numpy().reshape(1, 5, 48), exp, fd[None], efd, "2 x 2 coarsening")
        means = (x.reshape(5, 6, 2, 8, 2).astype(np.float64).sum(axis=(2, 4)) / 4).astype(np.float32)
        assert out.cpu().numpy().tobytes() == means.tobytes() == exp.reshape(5, 6, 8).tobytes()  # the block means of the restatement
        stats = gpu_ctx.hstats_levels(out, fdefined_in=fd)  # the result is a level batch as it is
        # conservation: the area mean is kept -- exactly: the sums of these integers and quarters are exact in double, and S1 / 48 = (sum / 4) / 48 is
        # the same correctly rounded quotient as sum / 192
        assert stats.mean().reshape(5).tobytes() == (x.reshape(5, -1).astype(np.float64).sum(axis=1) / 192.0).tobytes()


def test_a_plan_is_reused_and_owns_its_copy(gpu_ctx):
    import torch

    _, table = base(2, 3)
    rowptr, col, w = (np.array(a) for a in table)
    plan = hremap().Plan(gpu_ctx, rowptr, col, w, nsrc=117)
    d_table = [torch.from_numpy(np.array(a)).cuda() for a in table]
    dplan = hremap().Plan(gpu_ctx, *d_table, nsrc=117)
    rowptr[:], col[:], w[:] = 0, 116, 7.0  # the caller's arrays are overwritten after creation
    for t in d_table:
        t.zero_()
    torch.cuda.synchronize()
    for seed in (31, 32, 33):  # three calls with different fields
        fields = hr.main_fields(2, 3, 9, 13, seed=seed)
        for p in (plan, dplan):
            check(gpu_ctx, p, table, fields, MODES[1], True, label=("reused", seed))
            check(gpu_ctx, p, table, fields, MODES[0], False, label=("reused", seed))
    plan.close()
    dplan.close()


def test_plan_refusals(gpu_ctx):
    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    gpu_ctx.set_stream(None)

    def create(nsrc=5, ndst=2, rowptr=(0, 1, 2), col=(0, 4), w=(0.5, 0.5), memkind=0, null=None):
        r, cc, s = np.array(rowptr, np.int32), np.array(col, np.int32), np.array(w, np.float32)
        ptrs = [None if null == k else a.ctypes.data for k, a in enumerate((r, cc, s))]
        handle = lib.mifc_hremap_plan_create(c, nsrc, ndst, *ptrs, memkind)
        return handle, gpu_ctx.last_error()

    refusals = {
        "nsrc 0": (dict(nsrc=0), "nsrc < 1 or ndst < 1"),
        "ndst -1": (dict(ndst=-1), "nsrc < 1 or ndst < 1"),
        "rowptr[0]": (dict(rowptr=(1, 1, 2)), "rowptr[0] != 0"),
        "decreasing": (dict(rowptr=(0, 2, 1)), "rowptr decreases at row 1"),
        "negative nnz": (dict(rowptr=(0, -1, -1)), "nnz = rowptr[ndst] is negative"),
        "col nsrc": (dict(col=(0, 5)), "col[1] = 5 outside [0, nsrc)"),
        "col -1": (dict(col=(-1, 4)), "col[0] = -1 outside [0, nsrc)"),
        "NaN weight": (dict(w=(0.5, np.nan)), "w[1] is NaN or infinite"),
        "infinite weight": (dict(w=(np.inf, 0.5)), "w[0] is NaN or infinite"),
        "null rowptr": (dict(null=0), "a null pointer (rowptr, col or w)"),
        "null col": (dict(null=1), "a null pointer (rowptr, col or w)"),
        "null w": (dict(null=2), "a null pointer (rowptr, col or w)"),
        "bad memkind": (dict(memkind=7), "unknown memkind 7"),
    }
    for what, (kw, tail) in refusals.items():
        handle, err = create(**kw)
        assert not handle and err == "mifc_hremap_plan_create: " + tail, (what, err)
    handle, err = create()
    assert handle and err == ""
    nnz, longest, empty = ctypes.c_longlong(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.mifc_hremap_plan_info(handle, ctypes.addressof(nnz), ctypes.addressof(longest), ctypes.addressof(empty)) == 1
    assert (nnz.value, longest.value, empty.value) == (2, 1, 0)
    assert lib.mifc_hremap_plan_info(handle, None, None, None) == 1 and lib.mifc_hremap_plan_info(None, None, None, None) == 0
    lib.mifc_hremap_plan_destroy(handle)
    lib.mifc_hremap_plan_destroy(None)
    handle, err = create(rowptr=(0, 0, 0), col=(0,), w=(0.0,))  # nnz == 0 is legal
    assert handle and err == ""
    lib.mifc_hremap_plan_destroy(handle)
    with pytest.raises(hremap().Refused, match="rowptr decreases at row 1"):
        hremap().Plan(gpu_ctx, [0, 3, 2], [0, 1, 2], [1, 1, 1], nsrc=5)


def test_entry_refusals_write_nothing(gpu_ctx):
    import torch

    import mi_fieldcalc_amd as fc

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nf, nlev, ny, nx, ndst = 2, 3, 5, 8, 70
    fields_h, table = base(nf, nlev, ny, nx, ndst, 2)
    batch, res = nlev * ny * nx, nlev * ndst
    # room of the test's own around the fields: an output (longer than a field here) that ends in their first float or
    # begins in their last one stays inside it, whatever else the allocator has put nearby
    room = torch.zeros(res + nf * batch + res, dtype=torch.float32, device="cuda")
    x = room[res:res + nf * batch].view(nf, nlev, ny, nx).copy_(torch.from_numpy(np.array(fields_h)))
    sentinel = -4242.5
    outs = torch.full((nf, nlev, ndst), sentinel, dtype=torch.float32, device="cuda")
    plan = make_plan(gpu_ctx, table, ny * nx)
    other = fc.Context(0)
    foreign = hremap().Plan(other, *[np.array(a) for a in table], nsrc=ny * nx)
    gpu_ctx.use_torch_stream()

    def call(nx_=nx, ny_=ny, nlev_=nlev, nf_=nf, mode=0, min_frac=0.0, fields=None, out_ptrs=None, fd_out=True, memkind=1, handle="own", sync=True):
        tab = fields if isinstance(fields, ctypes.Array) else (ctypes.c_void_p * nf)(*[x[j].data_ptr() for j in range(nf)])
        o = (ctypes.c_void_p * nf)(*([outs[f].data_ptr() for f in range(nf)] if out_ptrs in (None, "null") else out_ptrs))
        fd = np.full(nf * nlev, 7, np.int32)
        h = {"own": plan.handle, "foreign": foreign.handle, "null": None}[handle]
        rc = lib.mifc_hremap_levels(c, h, nx_, ny_, nlev_, None if isinstance(fields, str) else ctypes.addressof(tab), None, nf_, mode, min_frac,
                                    None if out_ptrs == "null" else ctypes.addressof(o), fd.ctypes.data if fd_out else None, float(hr.UNDEF), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    null_head = "a null pointer (fields, fres or fdefined_out)"
    not_nsrc = "nx * ny is not the plan's nsrc 40"
    refusals = {
        "null plan": (dict(handle="null"), "a null plan"),
        "a plan of another context": (dict(handle="foreign"), "the plan belongs to another context"),
        "nx * ny": (dict(nx_=7), not_nsrc),
        "nx 0": (dict(nx_=0), not_nsrc),
        "negative nx and ny": (dict(nx_=-8, ny_=-5), not_nsrc),
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "negative nlev": (dict(nlev_=-3), "nlev < 1"),
        "nfields 0": (dict(nf_=0), "nfields 0 outside 1..8"),
        "nfields 9": (dict(nf_=9), "nfields 9 outside 1..8"),
        "unknown mode 2": (dict(mode=2), "unknown mode 2"),
        "negative mode": (dict(mode=-1), "unknown mode -1"),
        "min_frac NaN": (dict(mode=1, min_frac=float("nan")), "min_frac is NaN or outside [0, 1]"),
        "min_frac above 1": (dict(mode=1, min_frac=1.5), "min_frac is NaN or outside [0, 1]"),
        "min_frac below 0 under STRICT": (dict(mode=0, min_frac=-0.25), "min_frac is NaN or outside [0, 1]"),
        "null fields": (dict(fields="null"), null_head),
        "null fres": (dict(out_ptrs="null"), null_head),
        "null fdefined_out": (dict(fd_out=False), null_head),
        "null field": (dict(fields=(ctypes.c_void_p * nf)(x[0].data_ptr(), None)), "a null pointer (fields[1] or fres[1])"),
        "null output": (dict(out_ptrs=[outs[0].data_ptr(), None]), "a null pointer (fields[1] or fres[1])"),
        "output is an input": (dict(out_ptrs=[outs[0].data_ptr(), x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output ends in an input": (dict(out_ptrs=[x[0].data_ptr() - 4 * (res - 1), outs[1].data_ptr()]), "fres[0] overlaps fields[0]"),
        "same output twice": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr()]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[outs[0].data_ptr(), outs[0].data_ptr() + 4 * (res - 1)]), "fres[0] overlaps fres[1]"),
        "bad memkind": (dict(memkind=7), "unknown memkind 7"),
    }
    before = x.clone()
    for what, (kw, tail) in refusals.items():
        rc, err, fd = call(**kw)
        assert rc == 0 and err == "mifc_hremap_levels: " + tail, (what, err)
        assert (outs == sentinel).all().item() and (fd == 7).all(), what
    assert torch.equal(x.view(torch.int32), before.view(torch.int32))
    with pytest.raises(hremap().Refused, match="unknown mode"):
        hremap().hremap_levels(gpu_ctx, plan, x, "bilinear")
    # while a graph capture is open (nothing may synchronise inside it): the entry and the plan
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rowptr, col, w = (np.array(a) for a in table)
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, fd = call(sync=False)
        handle = lib.mifc_hremap_plan_create(c, ny * nx, ndst, rowptr.ctypes.data, col.ctypes.data, w.ctypes.data, 0)
        plan_err = gpu_ctx.last_error()
    g.close()
    assert rc == 0 and "capture" in err and (fd == 7).all() and (outs == sentinel).all().item()
    assert not handle and plan_err == "mifc_hremap_plan_create: not available while a mifc_graph capture is open"
    # afterwards the same call runs
    rc, err, fd = call()
    assert rc == 1 and err == "" and (fd != 7).all(), err
    exp, efd = expected(table, fields_h, hr.STRICT)
    compare(outs.cpu().numpy(), exp, fd.reshape(nf, nlev), efd, "after the refusals")
    foreign.close()
    other.close()
    plan.close()
