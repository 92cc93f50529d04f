"""The host-memory level pipeline (csrc/mifc_hostpipe.hip) and its two callers (run_stencil in mifc_capi_stencil.hip,
derived_sync in mifc_capi_derived.hip) at their chunk and buffer seams.

MIFC_HOST_PIPE_MIN_KIB=1 lets batches of a few thousand cells in, MIFC_HOST_CHUNK_LEVELS sets the levels per chunk, and
every case asserts through mifc_last_host_chunks that it was piped in the chunks it is named for (or, for the requests
the pipeline does not carry, that it was staged whole).  Inputs are host arrays.  The references: the restatement called
level by level (stencil values bit for bit, flags equal; derived outputs under the bars of test_gpu_derived_launch), and
the same call with MIFC_HOST_PIPELINE=0, bit for bit including flags.

Both callers re-base per-level state by the first level of a chunk: flags, counters, hybrid coefficients.  So that one
taken from the wrong level shows, the levels of every batch cycle through four kinds,
    ALL_DEFINED, clean data                      -> ALL_DEFINED
    SOME_DEFINED, about 2 % undefined            -> SOME_DEFINED
    SOME_DEFINED, clean data                     -> ALL_DEFINED
    SOME_DEFINED, every cell undefined           -> NONE_DEFINED
neighbouring levels never share an expected flag, the hybrid coefficients differ on every level, and the wind and the
thermodynamic fields of the derived batch run through the cycle two levels apart.  A counter or a coefficient from the
wrong level shows in every chunking.  An input flag read from the wrong level shows only where the flag of a level that
is ALL_DEFINED is read for a level with undefined cells (those are then computed untested); a cycle of four against chunks
of two levels never does that.  So the stencil operators also run in chunks of one, three and five levels
(test_chunk_counts, test_copy_threads_and_slices), and both derived entries in chunks of one and three levels: with three,
the first level of the second chunk has no defined wind and reads the wind flag of level 0, its last level has no defined
temperature and reads the thermodynamic flag of level 2, both ALL_DEFINED."""
import threading

import numpy as np
import pytest

import cases
import gpu_util
from test_gpu_derived_launch import compare_level
from test_gpu_derived_launch import expected as derived_expected

pytestmark = pytest.mark.gpu

ALL, NONE, SOME = cases.ALL_DEFINED, cases.NONE_DEFINED, cases.SOME_DEFINED
UNDEF = cases.UNDEF
SENTINEL = np.float32(-7777.0)
KINDS = ("all", "some", "clean", "none")
KIND_FLAG_OUT = dict(all=ALL, some=SOME, clean=ALL, none=NONE)
HOURS = 3.0

# name -> (the restatement's operator, first input, second input, Coriolis field, compute)
STENCIL_OPS = {
    "relvort": ("relvort", "u", "v", False, None), "absvort": ("absvort", "u", "v", True, None),
    "divergence": ("divergence", "u", "v", False, None), "vortdiv": (None, "u", "v", False, None),
    "gradient1": ("gradient", "z", None, False, 1), "gradient2": ("gradient", "z", None, False, 2),
    "gradient3": ("gradient", "z", None, False, 3), "gradient4": ("gradient", "z", None, False, 4),
    "plevelgwind_xcomp": ("plevelgwind_xcomp", "z", None, True, None), "plevelgwind_ycomp": ("plevelgwind_ycomp", "z", None, True, None),
    "plevelgvort": ("plevelgvort", "z", None, True, None), "ilevelgwind": ("ilevelgwind", "z", None, True, None),
    "jacobian": ("jacobian", "z", "u", False, None),
}
# what the tests call: the operators of mifc_stencil_levels, advection through mifc_stencil_levels_ex and the three requests
# of mifc_vortdiv_levels
CALLS = sorted(STENCIL_OPS) + ["advection", "vortdiv_levels:rvort+diverg", "vortdiv_levels:rvort", "vortdiv_levels:diverg"]
# advection reads three level fields: run_stencil stages it whole (the pipeline is not offered a third input)
STAGED_WHOLE = ("advection",)


def level_pattern(fields, seed, undef, offset=0):
    """Walks the levels of the (nlev, ny, nx) fields through KINDS, in place; returns the input flags."""
    import mi_fieldcalc_amd.synth as synth

    nlev = fields[0].shape[0]
    flags = np.full(nlev, SOME, np.int32)
    for l in range(nlev):
        kind = KINDS[(l + offset) % 4]
        if kind == "all":
            flags[l] = ALL
        for k, f in enumerate(fields):
            if kind == "some":
                f[l] = synth.sprinkle_undef(f[l], seed + 31 * l + k, 0.02, undef=undef)
            elif kind == "none":
                f[l] = undef
    return flags


def flags_out(nlev, offset=0):
    return np.array([KIND_FLAG_OUT[KINDS[(l + offset) % 4]] for l in range(nlev)], np.int32)


_INPUTS = {}


def stencil_inputs(nx, ny, nlev, nan_undef=False):
    key = (nx, ny, nlev, nan_undef)
    if key not in _INPUTS:
        import mi_fieldcalc_amd.synth as synth

        xm, ym, fcor = synth.grid_maps(nx, ny)
        u, v = synth.wind(nx, ny, 4100 + nx + nlev, nlev=nlev)
        z = np.stack([synth.scalar_field(nx, ny, 4200 + 7 * nlev + l, base=5500.0 - 40.0 * l) for l in range(nlev)])
        undef = np.float32(np.nan) if nan_undef else UNDEF
        flags = level_pattern([u, v, z], 4300 + nx, undef)
        for a in (u, v, z, xm, ym, fcor, flags):
            a.setflags(write=False)
        _INPUTS[key] = dict(key=key, nx=nx, ny=ny, nlev=nlev, u=u, v=v, z=z, xm=xm, ym=ym, fcor=fcor, flags=flags, undef=undef)
    return _INPUTS[key]


_EXPECTED = {}


def stencil_expected(oracle, inp, call):
    """(out0, out1 or None, flags) of the restatement's per-level calls, computed once per batch and operator."""
    name = "vortdiv" if call.startswith("vortdiv_levels") else call
    key = (inp["key"], name)
    if key in _EXPECTED:
        return _EXPECTED[key]
    nx, ny, nlev, xm, ym, fcor, undef = (inp[k] for k in ("nx", "ny", "nlev", "xm", "ym", "fcor", "undef"))
    e0 = np.empty((nlev, ny, nx), np.float32)
    e1 = np.empty_like(e0) if name in ("vortdiv", "ilevelgwind") else None
    fo = np.empty(nlev, np.int32)
    for l in range(nlev):
        fl = int(inp["flags"][l])
        if name == "vortdiv":
            ok, e0[l], fo[l] = oracle.call("relvort", nx, ny, inp["u"][l], inp["v"][l], xm, ym, fdefined=fl, undef=undef)
            ok2, e1[l], f2 = oracle.call("divergence", nx, ny, inp["u"][l], inp["v"][l], xm, ym, fdefined=fl, undef=undef)
            assert ok and ok2 and f2 == fo[l]
        elif name == "advection":
            ok, e0[l], fo[l] = oracle.call("advection", nx, ny, inp["z"][l], inp["u"][l], inp["v"][l], xm, ym, HOURS, fdefined=fl, undef=undef)
            assert ok
        else:
            cpu_op, f0, f1, use_fc, compute = STENCIL_OPS[name]
            args = [inp[f0][l]] + ([inp[f1][l]] if f1 else []) + [xm, ym] + ([fcor] if use_fc else []) + ([compute] if compute else [])
            ok, e, fo[l] = oracle.call(cpu_op, nx, ny, *args, fdefined=fl, undef=undef)
            assert ok
            if e1 is None:
                e0[l] = e
            else:
                e0[l], e1[l] = e
    _EXPECTED[key] = (e0, e1, fo)
    return _EXPECTED[key]


def stencil_run(ctx, inp, call):
    """The call on host arrays, outputs prefilled with the sentinel: (out0 or None, out1 or None, flags).  (An output that is
    not asked for never reaches the library: the wrappers pass no array for it.)"""
    shape = (inp["nlev"], inp["ny"], inp["nx"])
    o0, o1 = np.full(shape, SENTINEL, np.float32), np.full(shape, SENTINEL, np.float32)
    kw = dict(fdefined=inp["flags"], undef=inp["undef"])
    if call.startswith("vortdiv_levels"):
        want = tuple(call.split(":")[1].split("+"))
        res = ctx.vortdiv_levels(inp["u"], inp["v"], inp["xm"], inp["ym"], rvort=o0 if "rvort" in want else None,
                                 diverg=o1 if "diverg" in want else None, want=want, **kw)
        assert res is not None, call
        (r0, r1), fo = res
        assert (r0 is o0 or r0 is None) and (r1 is o1 or r1 is None)
        return r0, r1, fo
    if call == "advection":
        res = ctx.stencil_levels_ex("advection", inp["z"], inp["u"], inp["v"], xmapr=inp["xm"], ymapr=inp["ym"], scalar=HOURS, out0=o0, **kw)
        assert res is not None, call
        return res[0], None, res[1]
    _, f0, f1, use_fc, _ = STENCIL_OPS[call]
    two = call in ("vortdiv", "ilevelgwind")
    res = ctx.stencil_levels(call, inp[f0], inp[f1] if f1 else None, inp["xm"], inp["ym"], inp["fcor"] if use_fc else None, out0=o0,
                             out1=o1 if two else None, **kw)
    assert res is not None, call
    (r0, r1), fo = res
    assert r0 is o0 and (r1 is o1 if two else r1 is None)
    return r0, r1, fo


def check_chunks(ctx, nlev, L, what):
    """The call went through the pipeline in ceil(nlev / L) chunks of L levels (L = 0: it was staged whole)."""
    if gpu_util.run_is_forced():
        return
    got = ctx.last_host_chunks()
    if L == 0:
        assert got[0] == 0, (what, got)
    else:
        L = min(L, nlev)
        assert got == (-(-nlev // L), L), (what, got)


def check_stencil(ctx, oracle, inp, call, L):
    """One piped call against the per-level restatement; returns what it gave for the staged-whole comparison."""
    got = stencil_run(ctx, inp, call)
    check_chunks(ctx, inp["nlev"], 0 if call in STAGED_WHOLE else L, call)
    r0, r1, fo = got
    e0, e1, fo_e = stencil_expected(oracle, inp, call)
    for l in range(inp["nlev"]):
        if r0 is not None:
            assert cases.same_bits(r0[l], e0[l], nan_payload=False), (call, inp["key"], L, "out0, level %d" % l)
        if r1 is not None:
            assert cases.same_bits(r1[l], e1[l], nan_payload=False), (call, inp["key"], L, "out1, level %d" % l)
    assert np.array_equal(fo, fo_e), (call, inp["key"], L, fo, fo_e)
    return got


def same_as(got, whole, what):
    for k in (0, 1):
        assert (got[k] is None) == (whole[k] is None), what
        if got[k] is not None:
            assert cases.same_bits(got[k], whole[k], nan_payload=False), (what, "out%d differs from the batch staged whole" % k)
    assert np.array_equal(got[2], whole[2]), (what, got[2], whole[2])


def piped_and_whole(ctx, oracle, mifc_env, todo):
    """todo: (inputs, call, L).  Every case piped and checked against the restatement, then every case staged whole
    (MIFC_HOST_PIPELINE=0) and compared with its piped result bit for bit."""
    piped = []
    for inp, call, L in todo:
        mifc_env("MIFC_HOST_CHUNK_LEVELS", L)
        piped.append(check_stencil(ctx, oracle, inp, call, L))
    mifc_env("MIFC_HOST_PIPELINE", "0")
    for (inp, call, L), got in zip(todo, piped):
        whole = stencil_run(ctx, inp, call)
        check_chunks(ctx, inp["nlev"], 0, call)
        same_as(got, whole, (call, inp["key"], L))
    mifc_env("MIFC_HOST_PIPELINE", None)


def test_the_level_pattern_gives_the_flags_it_is_named_for(oracle):
    """The four kinds of levels give ALL, SOME, ALL and NONE_DEFINED in turn for the fused pair.  gradient compute 1 and
    ilevelgwind count fewer cells than they classify against, so a level without a defined cell is SOME_DEFINED there;
    neighbouring levels still never share a flag."""
    inp = stencil_inputs(260, 9, 9)
    assert list(inp["flags"][:4]) == [ALL, SOME, SOME, SOME]
    assert np.array_equal(stencil_expected(oracle, inp, "vortdiv")[2], flags_out(9))
    for call in ("vortdiv", "ilevelgwind", "gradient1"):
        assert np.all(np.diff(stencil_expected(oracle, inp, call)[2]) != 0), call


# ------------------------------------------------------------------ 1. every operator streams
@pytest.mark.parametrize("call", CALLS)
def test_every_operator_streams(gpu_ctx, oracle, mifc_env, call):
    """Five levels in chunks of 2, 2 and 1 on a grid of whole column groups and on a width off the 4-grid: one and two inputs,
    the Coriolis field, two outputs from one input, the swapped single output of the fused pair, and plevelgwind_xcomp, whose
    flag does not come from the counters.  Advection is pinned as staged whole."""
    import mi_fieldcalc_amd as fc

    assert set(STENCIL_OPS) == set(fc.Context.OPS)
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    piped_and_whole(gpu_ctx, oracle, mifc_env, [(stencil_inputs(nx, ny, 5), call, 2) for nx, ny in ((64, 12), (949, 7))])


@pytest.mark.parametrize("call", ["vortdiv_levels:rvort+diverg", "vortdiv_levels:diverg", "gradient1", "ilevelgwind", "jacobian"])
def test_every_operator_streams_with_nan_as_undef(gpu_ctx, oracle, mifc_env, call):
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    piped_and_whole(gpu_ctx, oracle, mifc_env, [(stencil_inputs(64, 12, 5, nan_undef=True), call, 2)])


def test_an_operator_that_never_pipes_reports_no_chunks(gpu_ctx, mifc_env):
    """The two-stage operators of mifc_stencil_levels_ex stage their batch whole: the report of the piped call before them
    does not stay."""
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    mifc_env("MIFC_HOST_CHUNK_LEVELS", 2)
    inp = stencil_inputs(64, 12, 5)
    stencil_run(gpu_ctx, inp, "relvort")
    check_chunks(gpu_ctx, 5, 2, "relvort")
    res = gpu_ctx.stencil_levels_ex("thermalFrontParameter", inp["z"], xmapr=inp["xm"], ymapr=inp["ym"], fdefined=inp["flags"])
    assert res is not None
    check_chunks(gpu_ctx, 5, 0, "thermalFrontParameter")


# ------------------------------------------------------------------ 2. chunk counts
CHUNKINGS = [(1, 1), (2, 1), (3, 1), (2, 2), (3, 2), (4, 2), (5, 2), (6, 3), (7, 3), (9, 2)]


@pytest.mark.parametrize("call", ["vortdiv_levels:rvort+diverg", "gradient1", "ilevelgwind"])
def test_chunk_counts(gpu_ctx, oracle, mifc_env, call):
    """1, 2, 3, 1, 2, 2, 3, 2, 3 and 5 chunks: the re-use of the double buffers (from the third chunk on) not entered, entered
    once and more often, ragged and exact last chunks, either parity holding the last chunk, one level per chunk."""
    assert [-(-n // L) for n, L in CHUNKINGS] == [1, 2, 3, 1, 2, 2, 3, 2, 3, 5]
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    piped_and_whole(gpu_ctx, oracle, mifc_env, [(stencil_inputs(260, 9, nlev), call, L) for nlev, L in CHUNKINGS])


# ------------------------------------------------------------------ 3. derived requests
_DERIVED = {}


def derived_inputs(nx, ny, nlev):
    """u, v, t, q, ps, a, b, wind flags, thermo flags (the batch of test_gpu_derived_launch.expected): the wind fields walk
    through KINDS from "all", t and q two kinds ahead, so that the two flag arrays differ on a level of every chunk of two;
    the surface pressure is clean, the hybrid coefficients differ on every level."""
    key = (nx, ny, nlev)
    if key not in _DERIVED:
        import mi_fieldcalc_amd.synth as synth

        u, v = synth.wind(nx, ny, 5100 + nx + nlev, nlev=nlev)
        t, q, ps = synth.thermo(nx, ny, 5200 + nx + nlev, nlev=nlev)
        a, b = synth.hybrid_levels(nlev)
        a = (a + 7.0 * np.arange(nlev)).astype(np.float32)  # (the ramp of a is symmetric about the middle level)
        assert len(set(a)) == nlev and len(set(b)) == nlev
        fw = level_pattern([u, v], 5300, UNDEF, offset=0)
        ft = level_pattern([t, q], 5400, UNDEF, offset=2)
        for l0 in range(0, nlev, 2):
            assert np.any(fw[l0:l0 + 2] != ft[l0:l0 + 2])
        for x in (u, v, t, q, ps, a, b, fw, ft):
            x.setflags(write=False)
        _DERIVED[key] = (u, v, t, q, ps, a, b, fw, ft)
    return _DERIVED[key]


BATCH_REQUESTS = {
    "ff": dict(ff=True, temp=None, hum=None, hum2=None, dd=False),
    "temp": dict(ff=False, temp=("", 3), hum=None, hum2=None, dd=False),
    "hum": dict(ff=False, temp=None, hum=("", 1), hum2=None, dd=False),
    "ff+dd": dict(ff=True, temp=None, hum=None, hum2=None, dd=True),
    "temp+hum+hum2": dict(ff=False, temp=("", 3), hum=("", 1), hum2=("", 9), dd=False),
    "ff+temp+hum+hum2": dict(ff=True, temp=("", 3), hum=("", 1), hum2=("", 9), dd=False),
    "ff+temp+hum+hum2+dd": dict(ff=True, temp=("", 3), hum=("", 1), hum2=("", 9), dd=True),  # five outputs: staged whole
}
NAMES = ("ff", "temp", "hum", "hum2", "dd")


def batch_run(ctx, batch, req, alevel=None):
    """mifc_hlevel_derived_batch with only the inputs the request reads, all five outputs prefilled with the sentinel."""
    u, v, t, q, ps, a, b, fw, ft = batch
    wind = req["ff"] or req["dd"]
    thermo = bool(req["temp"] or req["hum"] or req["hum2"])
    humid = bool(req["hum"] or req["hum2"])
    out = {k: np.full(fw.shape + ps.shape, SENTINEL, np.float32) for k in NAMES}
    res = ctx.hlevel_derived_batch(u if wind else None, v if wind else None, t if thermo else None, q if humid else None, ps if thermo else None,
                                   (a if alevel is None else alevel) if thermo else None, b if thermo else None,
                                   fdef_wind=fw, fdef_thermo=ft, out=out, **req)
    return res, out


def batch_check(res, out, exp, req, what):
    assert res is not None, what
    got, flags = res
    asked = [k for k in NAMES if req[k]]
    assert sorted(got) == sorted(exp) == sorted(asked), what
    for name in NAMES:
        if name not in asked:
            assert np.all(out[name] == SENTINEL), (what, name, "an output that was not asked for was written")
            continue
        assert got[name] is out[name]
        for l, (e, f, case) in enumerate(exp[name]):
            compare_level(case, got[name][l], e)
            assert flags[name][l] == f, (what, case["label"], flags[name][l], f)


# (levels, levels per chunk): chunks of two as the common case; of one and three, so that a chunk's flags are not those of
# the batch's first levels (see the module's docstring)
DERIVED_CHUNKINGS = [(3, 2), (8, 2), (9, 2), (8, 1), (9, 1), (8, 3), (9, 3)]


@pytest.mark.parametrize("nlev,L", DERIVED_CHUNKINGS)
@pytest.mark.parametrize("request_name", sorted(BATCH_REQUESTS))
def test_derived_batch_requests(gpu_ctx, oracle, mifc_env, request_name, nlev, L):
    """Every packing of the pipeline's input slots (u v | t | t h | u v t h) and output slots; up to 8 levels an unpiped call
    carries its per-level scalars in the kernel arguments, which a chunk must not do (its levels are not the first ones):
    the hybrid coefficients differ on every level.  Five outputs are more than the pipeline carries."""
    req = BATCH_REQUESTS[request_name]
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    mifc_env("MIFC_HOST_CHUNK_LEVELS", L)
    for nx, ny in ((64, 12), (260, 9)):
        batch = derived_inputs(nx, ny, nlev)
        what = (request_name, nx, ny, nlev, L)
        exp = derived_expected(oracle, req, batch, "hostpipe-%dx%dx%d" % (nx, ny, nlev))
        res, out = batch_run(gpu_ctx, batch, req)
        check_chunks(gpu_ctx, nlev, 0 if len(exp) == 5 else L, what)
        batch_check(res, out, exp, req, what)
        mifc_env("MIFC_HOST_PIPELINE", "0")
        res0, out0 = batch_run(gpu_ctx, batch, req)
        check_chunks(gpu_ctx, nlev, 0, what)
        mifc_env("MIFC_HOST_PIPELINE", None)
        assert res0 is not None
        for name in res[0]:
            assert cases.same_bits(res[0][name], res0[0][name], nan_payload=False), (what, name, "differs from the batch staged whole")
            assert np.array_equal(res[1][name], res0[1][name]), (what, name)


TRIO = dict(ff=True, temp=("", 3), hum=("", 1), hum2=None, dd=False)  # what mifc_hlevel_derived_levels computes: ff, theta, rh
TRIO_NAMES = dict(ff="ff", theta="temp", rh="hum")


def trio_run(ctx, batch, want, alevel=None):
    u, v, t, q, ps, a, b, fw, ft = batch
    out = {k: np.full(t.shape, SENTINEL, np.float32) for k in want}
    res = ctx.hlevel_derived_levels(u, v, t, q, ps, a if alevel is None else alevel, b, fdef_wind=fw, fdef_thermo=ft, want=want, out=out)
    return res, out


@pytest.mark.parametrize("nlev,L", DERIVED_CHUNKINGS)
@pytest.mark.parametrize("want", [("ff", "rh", "theta"), ("theta",), ("ff",), ("rh",)])
def test_derived_levels_requests(gpu_ctx, oracle, mifc_env, want, nlev, L):
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    mifc_env("MIFC_HOST_CHUNK_LEVELS", L)
    for nx, ny in ((64, 12), (260, 9)):
        batch = derived_inputs(nx, ny, nlev)
        what = (want, nx, ny, nlev, L)
        exp = derived_expected(oracle, TRIO, batch, "hostpipe-%dx%dx%d" % (nx, ny, nlev))
        res, out = trio_run(gpu_ctx, batch, want)
        check_chunks(gpu_ctx, nlev, L, what)
        assert res is not None and sorted(res[0]) == sorted(want), what
        for name in want:
            assert res[0][name] is out[name]
            for l, (e, f, case) in enumerate(exp[TRIO_NAMES[name]]):
                compare_level(case, res[0][name][l], e)
                assert res[1][name][l] == f, (what, case["label"], res[1][name][l], f)
        mifc_env("MIFC_HOST_PIPELINE", "0")
        res0, _ = trio_run(gpu_ctx, batch, want)
        check_chunks(gpu_ctx, nlev, 0, what)
        mifc_env("MIFC_HOST_PIPELINE", None)
        for name in want:
            assert cases.same_bits(res[0][name], res0[0][name], nan_payload=False), (what, name, "differs from the batch staged whole")
            assert np.array_equal(res[1][name], res0[1][name]), (what, name)


@pytest.mark.parametrize("bad_level", [0, 4])
def test_a_bad_hybrid_level_refuses_the_piped_call_and_leaves_the_outputs(gpu_ctx, oracle, mifc_env, bad_level):
    """bad_hlevel (a < 0) on a level of the first or of the last chunk: the call returns false before anything is written,
    and the corrected call then succeeds on the same context."""
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    mifc_env("MIFC_HOST_CHUNK_LEVELS", 2)
    nx, ny, nlev = 64, 12, 5
    batch = derived_inputs(nx, ny, nlev)
    a_bad = batch[5].copy()
    a_bad[bad_level] = -a_bad[bad_level]
    req = BATCH_REQUESTS["ff+temp+hum+hum2"]
    res, out = batch_run(gpu_ctx, batch, req, alevel=a_bad)
    assert res is None
    check_chunks(gpu_ctx, nlev, 0, "refused")
    for name in NAMES:
        assert np.all(out[name] == SENTINEL), name
    res, out = trio_run(gpu_ctx, batch, ("ff", "rh", "theta"), alevel=a_bad)
    assert res is None
    for name in out:
        assert np.all(out[name] == SENTINEL), name
    exp = derived_expected(oracle, req, batch, "hostpipe-%dx%dx%d" % (nx, ny, nlev))
    res, out = batch_run(gpu_ctx, batch, req)
    check_chunks(gpu_ctx, nlev, 2, "corrected")
    batch_check(res, out, exp, req, "corrected")


# ------------------------------------------------------------------ 4. one context, changing layouts
def _changing_layouts(ctx, oracle, mifc_env):
    first = stencil_inputs(64, 12, 9)
    second = stencil_inputs(260, 9, 3)
    batch = derived_inputs(64, 12, 8)
    req = BATCH_REQUESTS["ff+temp+hum+hum2"]
    mifc_env("MIFC_HOST_CHUNK_LEVELS", 2)
    got1 = check_stencil(ctx, oracle, first, "vortdiv_levels:rvort+diverg", 2)  # 2 + 2 slots of two levels
    mifc_env("MIFC_HOST_CHUNK_LEVELS", 1)
    check_stencil(ctx, oracle, second, "gradient1", 1)  # 1 + 2 slots of one (larger) level
    mifc_env("MIFC_HOST_CHUNK_LEVELS", 2)
    res, out = batch_run(ctx, batch, req)  # 4 + 4 slots
    check_chunks(ctx, 8, 2, "derived batch")
    batch_check(res, out, derived_expected(oracle, req, batch, "hostpipe-64x12x8"), req, "derived batch between two stencil calls")
    got4 = check_stencil(ctx, oracle, first, "vortdiv_levels:rvort+diverg", 2)  # the first layout again, in buffers that have grown
    same_as(got4, got1, "the first call repeated")
    return first, second


def test_one_context_through_changing_staging_layouts(oracle, mifc_env):
    """The staging buffers grow and are cut up differently from call to call; a context of its own, so that they start
    empty.  Then the same with the map fields held on the device (mifc_hold_field)."""
    import mi_fieldcalc_amd as fc

    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    with fc.Context(0) as ctx:
        first, second = _changing_layouts(ctx, oracle, mifc_env)
        held = [first["xm"], first["ym"], second["xm"], second["ym"]]
        for a in held:
            ctx.hold_field(a)
        try:
            _changing_layouts(ctx, oracle, mifc_env)
        finally:
            for a in held:
                ctx.release_field(a)
        _changing_layouts(ctx, oracle, mifc_env)


# ------------------------------------------------------------------ 5. two contexts, two threads
def test_two_contexts_pipe_on_two_threads(oracle, mifc_env):
    """Each thread streams another operator and shape through its own context (own pipeline, own copy threads), five calls
    each; mifc_last_host_chunks is the calling thread's."""
    import mi_fieldcalc_amd as fc

    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    mifc_env("MIFC_HOST_CHUNK_LEVELS", 2)
    work = [(stencil_inputs(64, 12, 9), "vortdiv_levels:rvort+diverg"), (stencil_inputs(260, 9, 5), "ilevelgwind")]
    for inp, call in work:
        stencil_expected(oracle, inp, call)  # computed here, shared, left unchanged
    errors = []

    def worker(inp, call):
        try:
            with fc.Context(0) as ctx:
                for it in range(5):
                    check_stencil(ctx, oracle, inp, call, 2)
        except BaseException as e:  # noqa: BLE001 - reported below
            errors.append((call, repr(e)))

    threads = [threading.Thread(target=worker, args=w) for w in work]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# ------------------------------------------------------------------ 6. copy threads and slices
@pytest.mark.parametrize("copy_threads", [1, 3])
def test_copy_threads_and_slices(oracle, mifc_env, copy_threads):
    """1440 x 92 x 11 in chunks of 5 levels: 2.65 MB per field and chunk, so every copy of the pool is one full 2 MiB slice
    and a remainder.  The pool is sized when a context creates its pipeline: a context of its own, created after
    MIFC_HOST_THREADS is set.  Nothing reports the size of the pool, so this covers the slicing under both settings, not that
    the pool has that many threads.  Levels 0, 4, 5, 9 and 10 against the restatement, every level against the batch staged
    whole."""
    import mi_fieldcalc_amd as fc

    nx, ny, nlev, L = 1440, 92, 11, 5
    assert L * nx * ny * 4 > (2 << 20)
    mifc_env("MIFC_HOST_THREADS", copy_threads)
    mifc_env("MIFC_HOST_PIPE_MIN_KIB", 1)
    mifc_env("MIFC_HOST_CHUNK_LEVELS", L)
    inp = stencil_inputs(nx, ny, nlev)
    call = "vortdiv_levels:rvort+diverg"
    with fc.Context(0) as ctx:
        rv, dv, fo = stencil_run(ctx, inp, call)
        check_chunks(ctx, nlev, L, call)
        for l in (0, 4, 5, 9, 10):
            fl = int(inp["flags"][l])
            ok, e, f = oracle.call("relvort", nx, ny, inp["u"][l], inp["v"][l], inp["xm"], inp["ym"], fdefined=fl)
            assert ok and f == fo[l] and cases.same_bits(rv[l], e, nan_payload=False), l
            ok, e, f = oracle.call("divergence", nx, ny, inp["u"][l], inp["v"][l], inp["xm"], inp["ym"], fdefined=fl)
            assert ok and f == fo[l] and cases.same_bits(dv[l], e, nan_payload=False), l
        assert np.array_equal(fo, flags_out(nlev))
        mifc_env("MIFC_HOST_PIPELINE", "0")
        whole = stencil_run(ctx, inp, call)
        check_chunks(ctx, nlev, 0, call)
        same_as((rv, dv, fo), whole, call)
