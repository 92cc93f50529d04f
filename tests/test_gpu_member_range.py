"""The entries that walk ensemble members (the five single-field reductions, mifc_ensemble_levels, mifc_ensembleQuantiles) at
the ends of the float range on the GPU: every case of tests/member_range_cases.py through the library, bit for bit against
its numpy restatement (a NaN matching any NaN), flags equal.  What the cases hold, that the restatement of the reductions
is the CPU checker bit for bit, and which mistakes -- double accumulators, a contracted Welford update, a reciprocal for a
division, fmax for a comparison, flushed subnormals, a hole taken by magnitude, LINEAR in float or as a lerp, a bisection
short of a bit -- the cases tell from the definition is asserted on the CPU in tests/test_member_range_cpu.py.

Per case: device memory on the 16-byte grid, device memory one float past it (not a bit may change), host memory; then host
memory staged in several chunks (cell ranges with a ragged last one, and level chunks) with MIFC_ENSEMBLE_CHUNK_MIB and
MIFC_QUANTILE_CHUNK_MIB at 1.  The inputs are unchanged after each call, the floats around a device output are intact, and the
launch shape of every call is read back (mifc_last_ensemble_form), so that the instances the cases are for are known to
have run."""
import numpy as np
import pytest

import ensemble_restate as er
import member_range_cases as mc
from gpu_util import run_is_forced
from test_gpu_pvort import guarded

pytestmark = pytest.mark.gpu

SENTINEL = -4242.5
PAD = {"aligned": 64, "offset": 65}  # floats in front of a device array: 64 keeps the 16-byte grid, 65 leaves it
GROUPS = [(family, klass) for family in mc.FAMILIES for klass in mc.CLASSES]
EXTREME = er.EXTREME


def same32(a, b):
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def compare(got, exp, label):
    """got, exp: (out, flags)."""
    out, fd = np.asarray(got[0]), np.asarray(got[1])
    assert out.shape == exp[0].shape, (label, out.shape, exp[0].shape)
    if not same32(out, exp[0]):
        bad = np.nonzero((out.view(np.uint32) != exp[0].view(np.uint32)) & ~(np.isnan(out) & np.isnan(exp[0])))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError("%s: %d values differ; first %s got %r (0x%08x) expected %r (0x%08x)" % (
            label, len(bad[0]), first, out[first], out.view(np.uint32)[first], exp[0][first], exp[0].view(np.uint32)[first]))
    assert np.array_equal(fd.reshape(np.shape(exp[1])), exp[1]), (label, "flags", fd, exp[1])


def check_form(seen, want, label):
    if not run_is_forced():
        assert {k: seen.get(k) for k in want} == want, (label, seen, want)


def unchanged(kept, device, label):
    for p, a in kept:
        now = p.cpu().numpy() if device else p
        assert np.array_equal(now.view(np.uint32), np.ascontiguousarray(a, np.float32).view(np.uint32)), (label, "an input has changed")


class Room:
    """Device outputs as views into one sentinel-filled tensor, `pad` floats on either side of them."""

    def __init__(self, shape, pad):
        import torch

        self.pad, self.n = pad, int(np.prod(shape))
        self.room = torch.full((self.n + 2 * pad,), SENTINEL, dtype=torch.float32, device="cuda")
        self.view = self.room[pad:pad + self.n].view(shape)

    def intact(self):
        return (self.room[:self.pad] == SENTINEL).all().item() and (self.room[self.pad + self.n:] == SENTINEL).all().item()


def level_form(case, where, **more):
    """What mifc_last_ensemble_form must say about a levels or quantiles call on the whole case in one chunk."""
    nmem, nlev, ny, nx = case["members"].shape
    want = dict(case["form"], lev_chunk=nlev, cell_chunk=ny * nx)
    if where == "offset" and case["family"] == "levels":
        want.update(c=1, welford=1, flagged=1, np=8)  # off the 16-byte grid: the one scalar instance
    want.update(more)
    return want


def call_levels(ctx, case, where, form=None, forms=None, products=None):
    """mifc_ensemble_levels or mifc_ensembleQuantiles on the case: host memory (where = "host") or guarded device views.
    -> [(out, flags)] per product, or (out, flags) for the quantiles, as numpy arrays."""
    import torch

    device = where != "host"
    label = (case["label"], where)
    x = guarded(case["members"], PAD[where]) if device else np.array(case["members"], np.float32)
    nmem, nlev, ny, nx = case["members"].shape
    if case["family"] == "quantiles":
        nq = len(case["percentiles"])
        room = Room((nq, nlev, ny, nx), PAD[where]) if device else None
        out, fd = ctx.ensembleQuantiles(x, case["percentiles"], fdefined_in=case["flags"], method=case["method"], undef=case["undef"],
                                        out=room.view if device else None)
        res = (out.cpu().numpy() if device else out, np.asarray(fd))
    else:
        products = case["products"] if products is None else products
        room = Room((len(products), nlev, ny, nx), PAD[where]) if device else None
        got = ctx.ensembleStatistics(x, products, fdefined_in=case["flags"], undef=case["undef"], out=room.view if device else None)
        res = [((o.cpu().numpy() if device else o), np.asarray(fd)) for o, fd in got]
    seen = ctx.last_ensemble_form()
    if form is not None:
        check_form(seen, form, label)
    if forms is not None:
        forms.append(seen)
    if device:
        torch.cuda.synchronize()
        assert room.intact(), label + ("the sentinel",)
    unchanged([(x, case["members"])], device, label)
    return res


def call_single(ctx, case, where, level, forms=None, only=None):
    """The five single-field entries on one level of the case, product by product -> [(out, flag)] as numpy; the members are
    put where `where` says once and must be unchanged after the last product."""
    import torch

    device = where != "host"
    label = (case["label"], where, level)
    x = case["members"][:, level]
    nmem, ny, nx = x.shape
    cells = ny * nx
    if device:
        # every member on (or one float past) the 16-byte grid: rows of a tensor whose pitch is a multiple of four floats
        pad, pitch = PAD[where], (cells + 3) // 4 * 4 + 64
        big = torch.full((nmem * pitch + 2 * pad,), float("nan"), dtype=torch.float32, device="cuda")
        fields = [big[pad + j * pitch:pad + j * pitch + cells].view(ny, nx) for j in range(nmem)]
        for j in range(nmem):
            fields[j].copy_(torch.from_numpy(np.ascontiguousarray(x[j])))
    else:
        fields = [np.array(x[j], np.float32) for j in range(nmem)]
    fin = [int(v) for v in case["flags"][:, level]]
    undef = case["undef"]
    want = dict(entry="single", c=4 if where != "offset" else 1, inline=int(nmem <= 64), lev_chunk=1, cell_chunk=cells, partials=0)
    want["tail"] = int(want["c"] == 4 and cells % 4 != 0)
    want["launches"] = 1 + want["tail"]
    res = []
    for p in case["products"]:
        name = er.name_of(p)
        if only is not None and name not in only:
            continue
        room = Room((ny, nx), PAD[where]) if device else None
        out = room.view if device else None
        if name == "sum":
            r = ctx.sumFields(fields, fdefined=int(p[1][level]), undef=undef, out=out)
        elif name == "mean":
            r = ctx.meanValue(fields, fin, undef=undef, out=out)
        elif name == "stddev":
            r = ctx.stddevValue(fields, fin, undef=undef, out=out)
        elif name in EXTREME:
            r = ctx.extremeValue(EXTREME[name], fields, fdefined=int(p[1][level]), undef=undef, out=out)
        else:
            r = ctx.probability(p[1], fields, fin, p[2], undef=undef, out=out)
        assert r is not None, label + (name,)
        seen = ctx.last_ensemble_form()
        check_form(seen, want, label + (name,))
        if forms is not None:
            forms.append((name, seen))
        if device:
            torch.cuda.synchronize()
            assert room.intact(), label + (name, "the sentinel")
        res.append((r[0].cpu().numpy() if device else r[0], r[1]))
    unchanged(list(zip(fields, x)), device, label)
    return res


def run_case(ctx, case, where, form=True):
    """The case in one placement against expected(case) -> the results, level-shaped for every family."""
    exp = mc.expected(case)
    label = (case["label"], where)
    if case["family"] == "quantiles":
        got = call_levels(ctx, case, where, form=level_form(case, where) if form else None)
        compare(got, exp, label)
        return [got]
    if case["family"] == "levels":
        got = call_levels(ctx, case, where, form=level_form(case, where) if form else None)
        assert len(got) == len(exp)
        for g, e, p in zip(got, exp, case["products"]):
            compare(g, e, label + (er.name_of(p), p[1:] if er.name_of(p) == "probability" else None))
        return got
    nlev = case["members"].shape[1]
    per_level = [call_single(ctx, case, where, l) for l in range(nlev)]
    got = []
    for k, (p, e) in enumerate(zip(case["products"], exp)):
        out = np.stack([per_level[l][k][0] for l in range(nlev)])
        fd = np.array([per_level[l][k][1] for l in range(nlev)], np.int32)
        compare((out, fd), e, label + (er.name_of(p), p[1:] if er.name_of(p) == "probability" else None))
        got.append((out, fd))
    return got


@pytest.mark.parametrize("family,klass", GROUPS)
def test_range_cases_in_device_and_host_memory(gpu_ctx, family, klass):
    for case in mc.cases(family, klass):
        on_grid = run_case(gpu_ctx, case, "aligned")
        off_grid = run_case(gpu_ctx, case, "offset")
        for k, (a, b) in enumerate(zip(on_grid, off_grid)):
            compare(b, a, (case["label"], "off the grid", k))
        run_case(gpu_ctx, case, "host")


@pytest.mark.parametrize("klass", mc.CLASSES)
def test_single_entries_equal_the_levels_entry(gpu_ctx, klass):
    """The single-field cases through mifc_ensemble_levels as well: the seven fixed slots and the first eight probabilities."""
    for case in mc.cases("single", klass):
        fixed = [k for k, p in enumerate(case["products"]) if er.name_of(p) != "probability"]
        prob = [k for k, p in enumerate(case["products"]) if er.name_of(p) == "probability"][:8]
        pick = fixed + prob
        got = call_levels(gpu_ctx, dict(case, family="levels"), "aligned", products=[case["products"][k] for k in pick])
        nlev = case["members"].shape[1]
        singles = [call_single(gpu_ctx, case, "aligned", l) for l in range(nlev)]
        for g, k in zip(got, pick):
            one = (np.stack([singles[l][k][0] for l in range(nlev)]), np.array([singles[l][k][1] for l in range(nlev)], np.int32))
            compare(g, one, (case["label"], "levels against single", er.name_of(case["products"][k])))
            compare(g, mc.expected(case)[k], (case["label"], "levels", er.name_of(case["products"][k])))


def test_every_instance_the_cases_are_for_has_run(gpu_ctx):
    """Read back from the launch shapes: all eleven 16-byte instantiations of mifc_ensemble_levels and the scalar one, every
    sorting tier and the bisection with both methods, the 16-byte launch, the launch with a scalar tail and the scalar launch
    of each single-field operator, kernel arguments and device table for all three entries."""
    if run_is_forced():
        return
    levels, quantiles, single = [], [], []
    for klass in mc.CLASSES:
        for case in mc.cases("levels", klass):
            call_levels(gpu_ctx, case, "aligned", forms=levels)
        for case in mc.cases("quantiles", klass):
            seen = []
            call_levels(gpu_ctx, case, "aligned", forms=seen)
            quantiles += [(case["method"], s) for s in seen]
    for case in mc.cases("single", "huge"):
        for where in ("aligned", "offset"):
            call_single(gpu_ctx, case, where, 0, forms=single, only=("sum", "mean", "stddev", "max", "probability"))
    assert all(s["entry"] == "levels" for s in levels) and all(s["entry"] == "quantiles" for _, s in quantiles) and all(s["entry"] == "single" for _, s in single)
    instances = {(s["c"], s["welford"], s["flagged"], s["np"]) for s in levels}
    assert instances == {(4, w, f, n) for w in (0, 1) for f in (0, 1) for n in (0, 3, 8)} - {(4, 1, 0, 3)} | {(1, 1, 1, 8)}, sorted(instances)
    assert len(instances) == 12
    assert {(s["tier"], method) for method, s in quantiles} == {(t, m) for t in (8, 16, 32, 64, 0) for m in ("lower", "linear")}
    operator = {"sum": "sum", "mean": "mean", "stddev": "stddev", "max": "extreme", "probability": "probability"}
    assert {(operator[name], s["c"], s["tail"]) for name, s in single} == {(o, c, t) for o in operator.values() for c, t in ((4, 0), (4, 1), (1, 0))}
    assert {s["inline"] for s in levels} == {0, 1} and {s["inline"] for _, s in quantiles} == {0, 1} and {s["inline"] for _, s in single} == {0, 1}


# ------------------------------------------------------------------------------------------------ chunked host staging
# The budget is 1 MiB = 1 048 576 bytes; a staged cell costs 4 * (members + outputs) bytes.  The cases have 7 members, 3
# levels and 12 x 20 cells: with the fifteen products 88 bytes a cell, 11 915 cells a chunk; with the nine percentiles 64
# bytes, 16 384 cells.  Repeated along y: `ranges` makes one level larger than the budget (cell ranges, the last one
# ragged: 14 400 = 11 912 + 2 488 cells, the range cut at a multiple of 4, and 16 800 = 16 384 + 416), `levels` makes two
# levels too large for it (one level a chunk).  (times along y, cells per chunk, launches of the call)
CHUNKS = {"levels": dict(var="MIFC_ENSEMBLE_CHUNK_MIB", ranges=(60, 11912, 6), levels=(25, 6000, 3)),
          "quantiles": dict(var="MIFC_QUANTILE_CHUNK_MIB", ranges=(70, 16384, 6), levels=(35, 8400, 3))}


@pytest.mark.parametrize("family", ["levels", "quantiles"])
@pytest.mark.parametrize("klass", mc.CLASSES)
def test_host_batches_in_several_chunks(gpu_ctx, mifc_env, klass, family):
    plan = CHUNKS[family]
    base = [c for c in mc.cases(family, klass) if c["members"].shape == (7, 3, 12, 20)]
    base = base[-1] if family == "levels" else [c for c in base if c["method"] == "linear"][0]  # all fifteen products; LINEAR
    assert family == "quantiles" or len(base["products"]) == 15
    for what in ("ranges", "levels"):
        times, cell_chunk, launches = plan[what]
        wide = mc.widened(base, times)
        exp = mc.restate(wide)
        whole = call_levels(gpu_ctx, wide, "aligned")  # device memory: one call, one chunk
        mifc_env(plan["var"], 1)
        form = dict(launches=launches, lev_chunk=1, cell_chunk=cell_chunk)
        staged = call_levels(gpu_ctx, wide, "host", form=form)
        mifc_env(plan["var"], None)
        if not run_is_forced():
            assert gpu_ctx.last_ensemble_form()["launches"] >= 2
        if family == "quantiles":
            whole, staged, exp = [whole], [staged], [exp]
        for k, (w, s, e) in enumerate(zip(whole, staged, exp)):
            compare(s, e, (wide["label"], what, "staged", k))
            compare(s, w, (wide["label"], what, "staged against the device call", k))


# ------------------------------------------------------------------------------------------------ quantile relations
def relation_cases(klass):
    return [c for c in mc.cases("quantiles", klass) if c["members"].shape[0] in (9, 33, 70) and c["members"].shape[1] == 3 and not np.isnan(c["undef"])]


@pytest.mark.parametrize("klass", mc.CLASSES)
def test_quantiles_do_not_depend_on_the_member_order(gpu_ctx, klass):
    for case in relation_cases(klass):
        order = np.random.default_rng(len(case["label"])).permutation(case["members"].shape[0])
        shuffled = dict(case, members=np.ascontiguousarray(case["members"][order]), flags=np.ascontiguousarray(case["flags"][order]))
        got = call_levels(gpu_ctx, shuffled, "aligned")
        compare(got, mc.expected(case), (case["label"], "shuffled"))


@pytest.mark.parametrize("klass", mc.CLASSES)
def test_percentiles_0_and_100_are_the_extremes(gpu_ctx, klass):
    """On level 1, where every member is ALL_DEFINED and so every value counts, against mifc_extremeValue with its flag
    ALL_DEFINED.  The cells are picked by what the two restatements branch on: no NaN among the values (the total order
    puts it last, extremeValue keeps or skips it), no stored undef (extremeValue takes the next member whatever it is),
    and no zero extreme (-0 sorts below +0, extremeValue keeps the first of the two)."""
    for case in relation_cases(klass):
        if case["method"] != "lower":
            continue
        x = case["members"][:, 1]
        level = dict(case, members=np.ascontiguousarray(x[:, None]), flags=np.ascontiguousarray(case["flags"][:, 1:2]), percentiles=np.array([0.0, 100.0], np.float32))
        for method in ("lower", "linear"):
            (out, _) = call_levels(gpu_ctx, dict(level, method=method), "aligned")
            fields = [np.array(f, np.float32) for f in x]
            with np.errstate(invalid="ignore"):
                mask = ~np.isnan(x).any(axis=0) & ~(x == case["undef"]).any(axis=0) & (x.min(axis=0) != 0) & (x.max(axis=0) != 0)
            assert mask.mean() > 0.5, (case["label"], float(mask.mean()))
            for q, compute in ((0, 2), (1, 1)):
                ext, _ = gpu_ctx.extremeValue(compute, fields, fdefined=mc.ALL_DEFINED, undef=case["undef"])
                assert same32(out[q, 0][mask], ext[mask]), (case["label"], method, compute)


@pytest.mark.parametrize("klass", mc.CLASSES)
def test_an_output_that_is_a_member_gives_the_same_bits(gpu_ctx, klass):
    import torch

    for case in relation_cases(klass):
        x = torch.from_numpy(np.ascontiguousarray(case["members"])).cuda()
        ps = case["percentiles"][[2, 5, 8]]
        separate, fd = gpu_ctx.ensembleQuantiles(x, ps, fdefined_in=case["flags"], method=case["method"], undef=case["undef"])
        separate = separate.cpu().numpy()
        out, fd2 = gpu_ctx.ensembleQuantiles(x, ps, fdefined_in=case["flags"], method=case["method"], undef=case["undef"], out=x[2:5])  # members 2, 3, 4
        torch.cuda.synchronize()
        assert out.data_ptr() == x[2].data_ptr()
        compare((out.cpu().numpy(), fd2), (separate, np.asarray(fd)), (case["label"], "in place"))
        k = [2, 5, 8]
        compare((separate, fd), (mc.expected(case)[0][k], mc.expected(case)[1]), (case["label"], "three percentiles"))
