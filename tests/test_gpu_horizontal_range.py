"""The horizontal families (mifc_hinterp_levels, mifc_hinterp_vector_levels, mifc_hremap_levels, mifc_hstats_levels) at the
ends of the float range on the GPU: every case of tests/horizontal_range_cases.py through the library, bit for bit against
its numpy restatement (a NaN matching any NaN), flags equal; for hstats all eight slots, the mean and its flags.  What the
cases hold and why they would show a flush to zero, a float intermediate, a multiplication by zero in the place of a
select or a result taken for a hole after the fact is asserted on the CPU in tests/test_horizontal_range_cpu.py.

Per case: device memory on the 16-byte grid, device memory one float past it (not a bit may change), host memory; then
host memory staged in several bands (hstats) or level chunks (hinterp and hremap on a case widened along y) with the
family's MIFC_*_CHUNK_MIB at 1.  The inputs are unchanged after each call, the floats around a device output are intact, and
the launch shape of every call is read back, so that the instances the cases are for are known to have run."""
import numpy as np
import pytest

import hinterp_restate as hi
import horizontal_range_cases as hc
import hstats_restate as hs
import vrotate_restate as vr
from gpu_util import run_is_forced
from test_gpu_pvort import guarded

pytestmark = pytest.mark.gpu

A, S = hc.ALL_DEFINED, hc.SOME_DEFINED
SENTINEL = -4242.5
PAD = {"aligned": 64, "offset": 65}  # floats in front of a device array: 64 keeps the 16-byte grid, 65 leaves it
GROUPS = [(family, klass) for family in hc.FAMILIES for klass in hc.CLASSES]
PRODUCTS = {hs.MOMENTS: ("moments",), hs.EXTREMES: ("extremes",), hs.MOMENTS | hs.EXTREMES: ("moments", "extremes")}


def hremap():
    from mi_fieldcalc_amd import hremap as module

    return module


def same32(a, b):
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def compare(case, got, exp, label):
    """got, exp: (out, flags), or (stats, mean, flags) for hstats."""
    assert np.array_equal(np.asarray(got[-1]).reshape(exp[-1].shape), exp[-1]), (label, "flags", got[-1], exp[-1])
    if case["family"] == "hstats":
        stats, mean = got[0], got[1]
        assert stats.shape == exp[0].shape, (label, stats.shape)
        if not hs.same_bits64(stats, exp[0]):
            bad = np.argwhere((stats.view(np.uint64) != exp[0].view(np.uint64)) & ~(np.isnan(stats) & np.isnan(exp[0])))
            first = tuple(int(b) for b in bad[0])
            raise AssertionError("%s: %d numbers differ; first %s got %r expected %r" % (label, len(bad), first, stats[first], exp[0][first]))
        if mean is not None:
            assert mean.shape == exp[1].shape and same32(mean, exp[1]), (label, "mean")
        return
    out = got[0].reshape(exp[0].shape)
    if not same32(out, exp[0]):
        bad = np.nonzero((out.view(np.uint32) != exp[0].view(np.uint32)) & ~(np.isnan(out) & np.isnan(exp[0])))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r expected %r" % (label, len(bad[0]), first, out[first], exp[0][first]))


def check_form(seen, want, label):
    if not run_is_forced():
        assert {k: seen.get(k) for k in want} == want, (label, seen, want)


def call(ctx, case, where, plan=None, form=None, forms=None):
    """One call on the case with its arrays in host memory (where = "host") or on the device as guarded views ("aligned",
    "offset"), a float output a view into a sentinel-filled tensor.  Asserts that no input has changed, that the sentinel
    around the output is intact and the launch shape (form: keys to add or, with None, to leave out; forms: a
    list that receives the launch shape as read back).  Returns the
    result as numpy arrays: (out, flags), or (stats, mean, flags)."""
    import torch

    device = where != "host"
    kept = []

    def put(a):
        if a is None:
            return None
        p = guarded(a, PAD[where]) if device else np.array(a, np.float32)
        kept.append((p, a))
        return p

    family, undef, flags = case["family"], case["undef"], case["flags"]
    nf, nlev, ny, nx = case["fields"].shape
    f = put(case["fields"])
    tested = int((flags != A).any())
    room = None

    def out_view(shape):
        nonlocal room
        if not device:
            return None
        n, pad = int(np.prod(shape)), PAD[where]
        room = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float32, device="cuda")
        return room[pad:pad + n].view(shape)

    if family in ("hinterp", "hvector"):
        per = 2 if case["method"] == "bicubic" else 4
        npos = case["x"].size
        want = dict(method=case["method"], nf=min(nf, per), tested=tested, launches=-(-nf // per), blocks=-(-npos // 256))
        if family == "hinterp":
            out, fd = ctx.hinterp_levels(f, put(case["x"]), put(case["y"]), case["method"], fdefined_in=flags, undef=undef, out=out_view((nf, nlev, npos)))
        else:
            pairs = f.reshape((nf // 2, 2, nlev, ny, nx))
            out, fd = ctx.hinterp_vector_levels(pairs, put(case["x"]), put(case["y"]), put(case["cosa"]), put(case["sina"]), case["method"],
                                                fdefined_in=flags, fdef_rot=case["fdef_rot"], undef=undef, out=out_view((nf // 2, 2, nlev, npos)))
        seen = ctx.last_hinterp_form()
        res = (out,)
    elif family == "hremap":
        ndst = case["table"][0].size - 1
        per = 2 if tested else 4
        mode = case["mode"] if tested else None  # (both modes are one rule where nothing is tested)
        want = dict(mode=mode, nf=min(nf, per), tested=tested, launches=-(-nf // per), blocks=-(-ndst // 256))
        out, fd = hremap().hremap_levels(ctx, plan, f, case["mode"], case["min_frac"], fdefined_in=flags, undef=undef, out=out_view((nf, nlev, ndst)))
        seen = hremap().last_hremap_form(ctx)
        res = (out,)
    else:
        moments = bool(case["products"] & hs.MOMENTS)
        weighted, minus = case["weight"] is not None, case["minus"] is not None
        i0, i1 = (case["box"][0], case["box"][1]) if case["box"] else (0, nx)
        tested = int(tested or (minus and (case["flags_minus"] != A).any()) or (weighted and case["fdef_weight"] != A))
        v = 4 if nx % 4 == 0 and (not device or PAD[where] % 4 == 0) else 1
        want = dict(mode=case["mode"], v=v, nf=min(nf, 4), w=int(weighted), minus=int(minus), tested=tested, products=case["products"],
                    segs=(i1 - 1) // hs.SEGMENT - i0 // hs.SEGMENT + 1, launches=-(-nf // 4), bands=1)
        r = ctx.hstats_levels(f, minus=put(case["minus"]), pivot=case["pivot"], weight=put(case["weight"]), box=case["box"], mode=case["mode"],
                              products=PRODUCTS[case["products"]], want_mean=moments, fdefined_in=flags, fdefined_minus=case["flags_minus"],
                              fdef_weight=case["fdef_weight"], undef=undef)
        seen = ctx.last_hstats_form()
        stats, mean, fd = r.stats, (r.mean_batch if moments else None), (r.mean_flags if moments else np.zeros((nf, nlev), np.int32))
        if device:
            stats, mean = stats.cpu().numpy(), (None if mean is None else mean.cpu().numpy())
        res = (stats, mean)
    want.update(form or {})
    want = {k: v for k, v in want.items() if v is not None}
    check_form(seen, want, (case["label"], where))
    if forms is not None:
        forms.append(seen)
    if device:
        torch.cuda.synchronize()
        if room is not None:
            pad = PAD[where]
            assert out.data_ptr() == room[pad:].data_ptr(), (case["label"], where)
            assert (room[:pad] == SENTINEL).all().item() and (room[room.numel() - pad:] == SENTINEL).all().item(), (case["label"], where, "the sentinel")
            res = (out.cpu().numpy(),)
    for p, a in kept:
        now = p.cpu().numpy() if device else p
        assert np.array_equal(now.view(np.uint32), np.ascontiguousarray(a, np.float32).view(np.uint32)), (case["label"], where, "an input has changed")
    return res + (np.asarray(fd),)


def check(ctx, case, where, plan=None, form=None, exp=None):
    exp = hc.expected(case) if exp is None else exp
    got = call(ctx, case, where, plan, form)
    compare(case, got, exp, (case["label"], where))
    return got


def with_plan(ctx, case):
    import contextlib

    if case["family"] != "hremap":
        return contextlib.nullcontext()
    ny, nx = case["fields"].shape[2:]
    return hremap().Plan(ctx, *[np.array(a) for a in case["table"]], nsrc=ny * nx)


@pytest.mark.parametrize("family,klass", GROUPS)
def test_range_cases_in_device_and_host_memory(gpu_ctx, family, klass):
    for case in hc.cases(family, klass):
        with with_plan(gpu_ctx, case) as plan:
            on_grid = check(gpu_ctx, case, "aligned", plan)
            off_grid = check(gpu_ctx, case, "offset", plan)
            compare(case, off_grid, on_grid[:-1] + (np.asarray(on_grid[-1]).reshape(hc.expected(case)[-1].shape),), (case["label"], "off the grid"))
            check(gpu_ctx, case, "host", plan)


def test_every_instance_the_cases_are_for_has_run(gpu_ctx):
    """Read back from the launch shapes of every case: tested and untested launches of every method and mode, 1 .. 4
    fields per launch, a second launch of a call, 16-byte and dword rows, weighted and minus."""
    if run_is_forced():
        return
    seen = {family: [] for family in hc.FAMILIES}
    for family, klass in GROUPS:
        for case in hc.cases(family, klass):
            with with_plan(gpu_ctx, case) as plan:
                call(gpu_ctx, case, "aligned", plan, forms=seen[family])
                if family == "hstats":
                    call(gpu_ctx, case, "offset", plan, forms=seen[family])
    hinterp = seen["hinterp"] + seen["hvector"]
    for method in hi.METHODS:
        assert {s["tested"] for s in hinterp if s["method"] == method} == {0, 1}, method
    assert {s["nf"] for s in seen["hinterp"]} == {1, 2, 3, 4} and {s["nf"] for s in seen["hvector"]} == {2, 4}
    assert any(s["launches"] == 2 for s in seen["hinterp"]) and any(s["launches"] == 2 for s in seen["hvector"])
    # hremap: a tested launch takes two fields, an untested one four
    assert {(s["nf"], s["tested"]) for s in seen["hremap"]} == {(1, 1), (2, 1), (1, 0), (2, 0), (3, 0), (4, 0)}
    assert {(s["mode"], s["tested"]) for s in seen["hremap"]} >= {("strict", 1), ("renorm", 1), ("strict", 0), ("renorm", 0)}
    assert any(s["launches"] == 2 for s in seen["hremap"])
    assert {(s["v"], s["tested"]) for s in seen["hstats"]} == {(4, 0), (4, 1), (1, 0), (1, 1)}
    assert {(s["w"], s["minus"]) for s in seen["hstats"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {s["nf"] for s in seen["hstats"]} == {1, 2, 3, 4} and {s["mode"] for s in seen["hstats"]} == {"area", "rows"}


@pytest.mark.parametrize("klass", hc.CLASSES)
def test_hremap_register_blocks_of_levels(gpu_ctx, mifc_env, klass):
    """All levels of a call in one workgroup: the register blocks of eight and of four levels and each remainder (7 = 4 + 3,
    13 = 8 + 4 + 1 or 3 x 4 + 1), which the few destinations of these cases do not reach by themselves."""
    mifc_env("MIFC_HREMAP_LEVEL_CHUNK", 16)
    for case in hc.cases("hremap", klass):
        nlev = case["fields"].shape[1]
        with with_plan(gpu_ctx, case) as plan:
            check(gpu_ctx, case, "aligned", plan, form=dict(chunk=nlev, level_chunks=1))
            check(gpu_ctx, case, "host", plan, form=dict(chunk=nlev, level_chunks=1))


@pytest.mark.parametrize("klass", hc.CLASSES)
def test_hinterp_levels_per_workgroup(gpu_ctx, mifc_env, klass):
    """By themselves the cases walk two levels per workgroup, the last chunk of seven one: the unrolled pair and the
    remainder (asserted).  Here one level per workgroup, and all of them."""
    for case in hc.cases("hinterp", klass) + hc.cases("hvector", klass):
        nlev = case["fields"].shape[1]
        mifc_env("MIFC_HINTERP_LEVEL_CHUNK", None)
        check(gpu_ctx, case, "aligned", form=dict(chunk=min(nlev, 2), level_chunks=-(-nlev // 2)) if case["x"].size > 256 else None)
        for chunk in (1, 16):
            mifc_env("MIFC_HINTERP_LEVEL_CHUNK", chunk)
            check(gpu_ctx, case, "offset", form=dict(chunk=min(chunk, nlev), level_chunks=-(-nlev // min(chunk, nlev))))


def chunk_variable(family):
    return "MIFC_%s_CHUNK_MIB" % ("HREMAP" if family == "hremap" else "HINTERP")


@pytest.mark.parametrize("family,klass", [g for g in GROUPS if g[0] != "hstats"])
def test_host_call_in_several_level_chunks(gpu_ctx, mifc_env, family, klass):
    """Every case of two levels or more, repeated along y until 1.25 MiB / nlev of fields make a level: a call that
    honours a budget of one MiB then stages fewer levels than there are at a time, and each chunk is launched on its own,
    which the launch count shows.  A case of one level cannot be cut: a chunk is never less than a level."""
    n = 0
    for case in hc.cases(family, klass):
        nf, nlev, ny, nx = case["fields"].shape
        if nlev < 2:
            continue
        wide = hc.widened(case, -(-int(1.25 * 2 ** 20) // (nlev * nf * ny * nx * 4)))
        assert wide["fields"][:, 0].nbytes * nlev > 2 ** 20 and wide["fields"][:, 0].nbytes < 2 ** 20, wide["label"]
        exp = hc.restate(wide)
        tested = (wide["flags"] != A).any()
        per_chunk = -(-nf // (2 if (family == "hremap" and tested) or wide.get("method") == "bicubic" else 4))
        with with_plan(gpu_ctx, wide) as plan:
            mifc_env(chunk_variable(family), 1)
            check(gpu_ctx, wide, "host", plan, form=dict(launches=None), exp=exp)
            seen = hremap().last_hremap_form(gpu_ctx) if family == "hremap" else gpu_ctx.last_hinterp_form()
            if not run_is_forced():
                assert seen["launches"] >= 2 * per_chunk and seen["launches"] % per_chunk == 0, (wide["label"], seen)
            mifc_env(chunk_variable(family), None)
            check(gpu_ctx, wide, "aligned", plan, exp=exp)  # and the chunks against the one device call itself
        n += 1
    assert n >= 1, (family, klass)


@pytest.mark.parametrize("klass", hc.CLASSES)
def test_hstats_host_call_in_several_bands(gpu_ctx, mifc_env, klass):
    """A band of rows of every level of every field at a time: every case of 4100 columns, repeated along y where it is
    smaller than the MiB, takes two bands or more, and the partial sums of all bands combine to the bits of the
    restatement.  The cases of 13 x 9 cells are left out: the smallest budget is one MiB, and enough of their rows to
    exceed it would be 3000 rows of one short segment each."""
    mifc_env("MIFC_HSTATS_CHUNK_MIB", 1)
    n = 0
    for case in hc.cases("hstats", klass):
        if case["fields"].shape[2:] != hc.WIDE:
            continue
        planes = case["fields"].shape[0] * (2 if case["minus"] is not None else 1)
        times = -(-int(1.25 * 2 ** 20) // (planes * case["fields"][0].nbytes))
        wide = case if times == 1 else hc.widened(case, times)
        exp = hc.expected(case) if times == 1 else hc.restate(wide)
        check(gpu_ctx, wide, "host", form=dict(bands=None, launches=None), exp=exp)
        if not run_is_forced():
            assert gpu_ctx.last_hstats_form()["bands"] >= 2, (wide["label"], gpu_ctx.last_hstats_form())
        n += 1
    assert n >= 2, klass


def test_hinterp_vector_is_hinterp_then_vrotate(gpu_ctx):
    """mifc_hinterp_vector_levels against mifc_hinterp_levels followed by mifc_vrotate_levels with the flags of the first
    call, on the device.  The one call carries the holes of the sampling, the second of two calls recognises them by value:
    they differ exactly where a sampled component is a VALUE that is NaN or equal to undef (stored under ALL_DEFINED, or
    computed: inf - inf, a midpoint that rounds to 1e35f) while the first call's flag of that component says that the level
    has holes (include/mifc.h).  Those points are left out, everything else is bit for bit."""
    import torch

    excluded = 0
    for klass in hc.CLASSES:
        for case in hc.cases("hvector", klass):
            nf, nlev, ny, nx = case["fields"].shape
            npos = case["x"].size
            one, fd_one = call(gpu_ctx, case, "aligned")
            one, fd_one = one.reshape(nf, nlev, npos), fd_one.reshape(nf, nlev)
            put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
            first, fd1 = gpu_ctx.hinterp_levels(put(case["fields"]), put(case["x"]), put(case["y"]), case["method"], fdefined_in=case["flags"])
            pairs = first.reshape(nf // 2, 2, nlev, 1, npos)
            two, fd_two = gpu_ctx.vrotate_levels(pairs, put(case["cosa"].reshape(1, npos)), put(case["sina"].reshape(1, npos)), fdefined_in=fd1.reshape(nf, nlev),
                                                 fdef_rot=case["fdef_rot"])
            two, fd_two = two.cpu().numpy().reshape(nf, nlev, npos), np.asarray(fd_two).reshape(nf, nlev)
            # the sampled values that the second call takes for holes, from the restatement's branches
            br = np.zeros((nf, nlev, npos), np.int64)
            sampled, sfd = hi.sample(case["fields"], case["x"], case["y"], case["method"], case["flags"], branches=br)
            assert same32(first.cpu().numpy(), sampled) and np.array_equal(np.asarray(fd1).reshape(nf, nlev), sfd)
            value = ~np.isin(br, vr.SAMPLING_HOLES) & (np.isnan(sampled) | (sampled == hc.UNDEF)) & (sfd != A)[:, :, None]
            apart = value[0::2] | value[1::2]  # per pair
            apart = np.repeat(apart, 2, axis=0)
            excluded += int(apart.sum())
            same = (one.view(np.uint32) == two.view(np.uint32)) | (np.isnan(one) & np.isnan(two))
            assert same[~apart].all(), (case["label"], int((~same & ~apart).sum()))
            quiet = ~apart.any(axis=2)
            assert np.array_equal(fd_one[quiet], fd_two[quiet]), case["label"]
    assert excluded > 0


def test_hstats_box_is_the_data_with_everything_outside_overwritten(gpu_ctx):
    n = 0
    for klass in hc.CLASSES:
        for case in hc.cases("hstats", klass):
            if case["box"] is None:
                continue
            twin = hc.outside_overwritten(case)
            for where in ("aligned", "offset"):
                got = call(gpu_ctx, case, where)
                other = call(gpu_ctx, twin, where)
                compare(case, other, got[:-1] + (np.asarray(got[-1]),), (case["label"], where, "outside overwritten by inf"))
            n += 1
    assert n >= 3


def test_hremap_strict_and_renorm_give_equal_bits_where_no_entry_is_bad(gpu_ctx):
    n = 0
    for klass in hc.CLASSES:
        for case in hc.cases("hremap", klass):
            if "clean" in case["label"]:
                continue
            with with_plan(gpu_ctx, case) as plan:
                strict, _ = call(gpu_ctx, dict(case, mode="strict", min_frac=0.0), "aligned", plan)
                renorm, _ = call(gpu_ctx, dict(case, mode="renorm", min_frac=0.5), "aligned", plan)
            same = (strict.view(np.uint32) == renorm.view(np.uint32)) | (np.isnan(strict) & np.isnan(renorm))
            assert same[:, :, :64].all() and same[case["flags"] == A].all(), case["label"]  # slice 0 has no bad entry; ALL_DEFINED levels have none
            n += int(not same.all())
    assert n >= 5  # and they do differ where an entry is bad
