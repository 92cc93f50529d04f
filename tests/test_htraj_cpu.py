"""CPU checks of mifc_htraj_levels: the restatement (tests/htraj_restate.py, the oracle of the GPU tests) pinned to the
text of include/mifc.h by hand-computed particles, each named mistake shown to change the cases aimed at it, the
composition property of rule 5, the conditions on the seeded cases, the rules header
(mi-fieldcalc_amd/csrc/mifc_htraj_rules.h) compiled with the host compiler -- through a shim and, under the address and
undefined-behaviour sanitizers, as a stand-alone program -- and held to the restatement bit for bit, that the entries are
declared, bound and configured where the others are, the front's marshalling against a recording stub library, and the
compiler's resource remarks for the kernel."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hinterp_restate as hi
import htraj_cases as hc
import htraj_restate as ht
import test_python_front_cpu as front
from mi_fieldcalc_amd import htraj as htraj_module  # (without the feature the file fails here)
from test_python_front_cpu import _data, _stub_context

U = ht.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
A, S, N = ht.ALL_DEFINED, ht.SOME_DEFINED, ht.NONE_DEFINED
# the host tables of the entry for the recording stub: positions after the context
front.SPEC.setdefault("mifc_htraj_levels", [(4, "ptr", front._at(3)), (5, "ptr", front._at(3)), (18, "ptr", lambda a: a[20] * a[3]), (23, "ptr", front._at(20))])


# -------------------------------------------------------------------------------- hand-computed particles: the header's text
def test_uniform_wind_moves_exactly_h_u_m_per_substep():
    # m = 2^-10, u = 1 m/s, v = -0.5 m/s, 1024 s: one cell in x, half a cell back in y, whatever nsub and niter
    for nsub in (1, 4, 64):
        for niter in (0, 1, 8):
            c = hc.uniform(vval=-0.5, xpos=(3.0, 0.25, 1.0), ypos=(1.0, 3.0, 0.25), nsub=nsub, niter=niter)
            x, y, tr, fl = ht.run(**c)
            assert x[:, 0, 0].tolist() == [3.0, 4.0] and y[:, 0, 0].tolist() == [1.0, 0.5]  # exactly onto the last column
            assert x[:, 0, 1].tolist() == [0.25, 1.25] and y[:, 0, 1].tolist() == [3.0, 2.5]
            assert x[0, 0, 2] == 1.0 and x[1, 0, 2] == U and y[1, 0, 2] == U  # y = 0.25 - 0.5 leaves the grid
            assert fl.tolist() == [[[A], [S]]] and tr.shape == (0, 2, 1, 3)
    # backward: tau = -1024 s
    c = hc.uniform(vval=-0.5, xpos=(3.0,), ypos=(1.0,), j_start=1, j_end=0, nsub=2, niter=2)
    x, y, _, _ = ht.run(**c)
    assert x[:, 0, 0].tolist() == [3.0, 2.0] and y[:, 0, 0].tolist() == [1.0, 1.5]


def test_two_substep_petterssen_step_by_hand():
    # one row; u_A = i m/s at column i, u_B = u_A + 1, m = 2^-10, tau = 1024 s, nsub = 2 (h = 512, hh = 256), niter = 1, x0 = 1:
    # s = 0: g0 = u_A(1) m = 1 / 1024, x* = 1.5; w = 0.5: uu = 1.5 + 0.5 * (2.5 - 1.5) = 2, x* = 1 + 256 * 3 / 1024 = 1.75
    # s = 1: w = 0.5: uu = 1.75 + 0.5 = 2.25, x* = 1.75 + 512 * 2.25 / 1024 = 2.875; w = 1: uu = u_B(2.875) = 3.875,
    #        x* = 1.75 + 256 * (2.25 + 3.875) / 1024 = 3.28125
    ramp = np.arange(5, dtype=np.float32).reshape(1, 1, 1, 5)
    c = hc.uniform(nx=5, ny=1, xpos=(1.0,), ypos=(0.0,), nsub=2, niter=1, u=np.concatenate([ramp, ramp + 1]), v=np.zeros((2, 1, 1, 5), np.float32))
    x, y, _, fl = ht.run(**c)
    assert x[:, 0, 0].tolist() == [1.0, 3.28125] and y[:, 0, 0].tolist() == [0.0, 0.0] and fl.tolist() == [[[A], [A]]]
    x, _, _, _ = ht.run(**dict(c, niter=0))  # Euler: 1 -> 1.5 -> 1.5 + 512 * (1.5 + 0.5) / 1024 = 2.5
    assert x[:, 0, 0].tolist() == [1.0, 2.5]
    x, _, _, _ = ht.run(**dict(c, nsub=1, niter=1))  # h = 1024: x* = 2, then 1 + 512 * (1 + u_B(2)) / 1024 = 3
    assert x[:, 0, 0].tolist() == [1.0, 3.0]
    # the trace is sampled at the float position of the slot, from the slice of the slot
    t = np.concatenate([10 * ramp, 100 * ramp])[None]
    _, _, tr, fl = ht.run(**dict(c, trace=t))
    assert tr[0, :, 0, 0].tolist() == [10.0, 328.125] and fl.tolist() == [[[A], [A]], [[A], [A]]]


def test_trace_is_hinterp_at_the_slot():
    args, (x, y, tr, fl) = ht.seeded(ht.SEEDS[0], 3, 3)
    for f in range(tr.shape[0]):
        for n in range(x.shape[0]):
            exp, _ = hi.sample(args["trace"][f, n][None], x[n, 0], y[n, 0], hi.BILINEAR, undef=U)  # slot n is slice n: j_start = 0, forward
            assert ht.same(tr[f, n, 0], exp[0, 0])


# ------------------------------------------------------------------------------------------- each mistake is visible
def test_each_mistake_changes_the_cases_aimed_at_it():
    cases = hc.cases()
    aimed = {
        "state kept in double across slices": cases["irregular times"],
        "no select at w == 1": cases["a huge wind in slice A at w == 1"],  # (u_A + 1 * (u_B - u_A) is 0 there, not u_B)
        "slice B not needed at w == 0": dict(cases["holes in slice B only"], nsub=1, niter=0),
        "end of interval not tested": cases["exactly onto the last column, niter=0"],
        "trace from the double position": cases["ntrace = 4 with trace holes"],
        "predictor reused as g0": cases["niter = 8"],
    }
    for name, c in aimed.items():
        right, wrong = ht.run(**c), ht.run(mistakes=(name,), **c)
        assert not all(ht.same(r, w) for r, w in zip(right, wrong)), name
    assert set(aimed) == set(ht.MISTAKES)


# ----------------------------------------------------------------------- rule 5: a run composes from its intervals
def test_composition_of_runs_on_the_restatement():
    args, (x, y, tr, fl) = ht.seeded(ht.SEEDS[1], 3, 3)
    first = ht.run(**dict(args, j_end=1))
    assert ht.same(first[0], x[:2]) and ht.same(first[1], y[:2]) and ht.same(first[2], tr[:, :2]) and np.array_equal(first[3], fl[:, :2])
    rest = ht.run(**dict(args, xpos=x[1, 0], ypos=y[1, 0], j_start=1, j_end=3))
    assert ht.same(rest[0], x[1:]) and ht.same(rest[1], y[1:]) and ht.same(rest[2], tr[:, 1:]) and np.array_equal(rest[3], fl[:, 1:])
    # a backward run over the same slices is another trajectory, its slots in the order of the run
    back = ht.run(**dict(args, j_start=3, j_end=0))
    assert ht.same(back[0][0], np.where(np.isnan(args["xpos"]), U, args["xpos"])[None]) and not ht.same(back[0][3], x[0])


@pytest.mark.parametrize("seed", ht.SEEDS)
@pytest.mark.parametrize("nsub,niter", ht.SCHEMES)
def test_seeded_cases_keep_half_and_lose_some_in_every_interval(seed, nsub, niter):
    args, (x, y, tr, fl) = ht.seeded(seed, nsub, niter)
    npos = args["xpos"].size
    alive = (x[:, 0] != U).sum(axis=1)
    assert npos == 600 and alive[0] == npos and alive[-1] >= npos // 2, alive
    assert (-np.diff(alive) >= 0.02 * npos).all(), alive
    assert ((x == U) == (y == U)).all() and (fl[0, 1:] == S).all() and fl[0, 0, 0] == A


# ------------------------------------------------------------------------ the rules header through the host compiler
def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    return cxx


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("htraj") / "libhtraj_rules_shim.so")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I", CSRC, "-I", os.path.join(ROOT, "tests"),
                    os.path.join(ROOT, "tests", "htraj_rules_shim.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    p, i, f, d = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    lib.mifc_test_htraj_run.restype = None
    lib.mifc_test_htraj_run.argtypes = [i, i, i, i, p, p, p, p, p, p, i, i, p, p, i, i, i, i, p, p, i, p, p, p, p, f]
    lib.mifc_test_htraj_check.restype = ctypes.c_char_p
    lib.mifc_test_htraj_check.argtypes = [i] * 10 + [p, f]
    lib.mifc_test_htraj_plan.restype = None
    lib.mifc_test_htraj_plan.argtypes = [i, i, p]
    lib.mifc_test_htraj_levels_per_chunk.argtypes = [ctypes.c_ulonglong] * 3 + [i, i, i]
    lib.mifc_test_htraj_level_chunk.argtypes = [i, i]
    lib.mifc_test_htraj_value.argtypes = [p, i, i, d, d, i, f, p]
    return lib


def header_run(shim, u, v, times, xmapr, ymapr, xpos, ypos, j_start, j_end, nsub, niter, trace=None, fdefined_in=None, fdef_map=S, fdef_trace=None, undef=U):
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    nt, nlev, ny, nx = u.shape
    tr_in = None if trace is None else np.ascontiguousarray(trace, np.float32)
    ntrace = 0 if tr_in is None else tr_in.shape[0]
    times = np.ascontiguousarray(times, np.float64)
    xm, ym = np.ascontiguousarray(xmapr, np.float32), np.ascontiguousarray(ymapr, np.float32)
    xp, yp = np.ascontiguousarray(xpos, np.float32), np.ascontiguousarray(ypos, np.float32)
    fin = None if fdefined_in is None else np.ascontiguousarray(np.asarray(fdefined_in).reshape(2, nt, nlev), np.int32)
    ftr = None if fdef_trace is None else np.ascontiguousarray(np.asarray(fdef_trace).reshape(ntrace, nt, nlev), np.int32)
    nslots = abs(j_end - j_start) + 1
    x = np.full((nslots, nlev, xp.size), -77.0, np.float32)
    y, tr = x.copy(), np.full((ntrace, nslots, nlev, xp.size), -77.0, np.float32)
    fl = np.full((1 + ntrace, nslots, nlev), -1, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    shim.mifc_test_htraj_run(nx, ny, nlev, nt, ptr(u), ptr(v), ptr(fin), ptr(times), ptr(xm), ptr(ym), int(fdef_map), xp.size, ptr(xp), ptr(yp), j_start, j_end,
                             nsub, niter, ptr(tr_in), ptr(ftr), ntrace, ptr(x), ptr(y), ptr(tr), ptr(fl), float(np.float32(undef)))
    return x, y, tr, fl


def assert_same_run(got, exp, label):
    for name, g, e in zip(("x", "y", "trace", "flags"), got, exp):
        assert ht.same(g, e), (label, name, np.argwhere(g.view(np.uint32 if g.dtype == np.float32 else np.int32) != e.view(np.uint32 if e.dtype == np.float32 else np.int32))[:4].tolist())


@pytest.mark.parametrize("seed", ht.SEEDS)
@pytest.mark.parametrize("nsub,niter", ht.SCHEMES)
def test_header_against_the_restatement_on_the_seeded_cases(shim, seed, nsub, niter):
    args, exp = ht.seeded(seed, nsub, niter)
    assert_same_run(header_run(shim, **args), exp, (seed, nsub, niter))


@pytest.mark.parametrize("name", hc.NAMES)
def test_header_against_the_restatement_on_the_seam_cases(shim, name):
    assert_same_run(header_run(shim, **hc.cases()[name]), hc.expected(name), name)


def test_seam_cases_reach_their_seams():
    exp = {name: hc.expected(name) for name in hc.NAMES}
    x = exp["starts on nodes and edges"][0]
    assert (x[0, 0] == hc.cases()["starts on nodes and edges"]["xpos"]).all() and np.signbit(x[0, 0, 5])  # every start usable, -0.0 kept
    x = exp["unusable starts"][0]
    assert (x[:, 0, :10] == U).all() and x[0, 0, 10] == 3 and (x[:, 0, 11] == U).all()
    for niter in (0, 2):
        x = exp["exactly onto the last column, niter=%d" % niter][0]
        assert x[1, 0].tolist() == [4.0, float(U), 3.5]
        y = exp["exactly onto the last row, niter=%d" % niter][1]
        assert y[1, 0].tolist() == [3.0, float(U), 1.5]
    assert exp["exactly onto column 0, backward in the index"][0][1, 0].tolist() == [0.0, float(U), float(U)]
    assert exp["a huge wind in slice A at w == 1"][0][:, 0, 0].tolist() == [1.0, 2.0]
    assert exp["predictor leaves the grid, one substep"][0][1, 0, 0] == U and exp["predictor stays inside, four substeps"][0][1, 0, 0] != U
    tested, untested = exp["holes in slice B only"][0], exp["holes in slice B under ALL_DEFINED"][0]
    assert (tested[1] == U).sum() > 0 and not ht.same(tested, untested)
    assert not ht.same(exp["holes in the map planes"][0], exp["holes in the map planes under ALL_DEFINED"][0])
    assert not ht.same(exp["a stored undef is a hole"][0], exp["a stored undef under ALL_DEFINED is a value"][0])
    for name in ("nx == 1", "ny == 1", "nx == 1 and ny == 1", "npos == 1"):
        x = exp[name][0]
        assert (x[-1] != U).any(), name  # some particle survives on the degenerate grid
    assert (exp["nx == 1"][0][-1] == U).any() and (exp["ny == 1"][0][-1] == U).any()
    tr, fl = exp["ntrace = 4 with trace holes"][2:]
    x = exp["ntrace = 4 with trace holes"][0]
    assert ((tr[0] == U) & (x != U)).any() and ((tr[2, :, 1] == U)).all() and (fl[3, :, 1] == N).all()  # a trace hole under a live particle
    assert np.isnan(exp["ntrace = 4, some trace planes ALL_DEFINED"][2][3]).any()  # the NaN of an ALL_DEFINED trace plane is a value
    x, y, tr, fl = exp["undef = NaN"]
    assert np.isnan(x[:, 0, 3]).all() and np.isnan(x[-1]).sum() > 1 and (np.isnan(tr) & ~np.isnan(x)[None]).any()


REFUSALS = [
    (dict(nt=1, j_end=0), "nt < 2"), (dict(nlev=0), "nlev < 1"), (dict(npos=0), "npos < 1"), (dict(nx=0), "nx < 1 or ny < 1"), (dict(ny=0), "nx < 1 or ny < 1"),
    (dict(nx=(1 << 24) + 1, ny=1), "nx or ny above 2^24"), (dict(ny=(1 << 24) + 1, nx=1), "nx or ny above 2^24"),
    (dict(nx=1 << 24, ny=128), "more than 2^31 - 1 cells per level"), (dict(j_start=-1), "j_start or j_end outside 0..nt-1"),
    (dict(j_end=4), "j_start or j_end outside 0..nt-1"), (dict(j_start=2, j_end=2), "j_start == j_end"), (dict(nsub=0), "nsub outside 1..64"),
    (dict(nsub=65), "nsub outside 1..64"), (dict(niter=-1), "niter outside 0..8"), (dict(niter=9), "niter outside 0..8"), (dict(ntrace=-1), "ntrace outside 0..4"),
    (dict(ntrace=5), "ntrace outside 0..4"), (dict(times=None), "a null pointer (times)"),
    (dict(times=[0.0, np.inf, 2.0, 3.0]), "a time of the used slices is not finite"), (dict(times=[0.0, 1.0, np.nan, 3.0]), "a time of the used slices is not finite"),
    (dict(times=[0.0, 1.0, 1.0, 3.0]), "the times of the used slices are not strictly increasing"),
    (dict(times=[3.0, 2.0, 1.0, 0.0], j_start=3, j_end=0), "the times of the used slices are not strictly increasing"),
    (dict(undef=0.0), "undef is a position inside the grid"), (dict(undef=5.0), "undef is a position inside the grid"),  # max(nx, ny) - 1 = 5
]
ACCEPTED = [dict(), dict(undef=np.nan), dict(undef=-0.5), dict(undef=5.0000005), dict(undef=-np.inf), dict(nx=1 << 24, ny=127), dict(nx=1, ny=1, undef=0.5),
            dict(times=[np.nan, 1.0, 2.0, np.inf], j_start=1, j_end=2), dict(times=[5.0, 1.0, 2.0, 0.0], j_start=2, j_end=1), dict(nsub=64, niter=8, ntrace=4),
            dict(nsub=1, niter=0, ntrace=0)]


def test_header_argument_check_gives_every_refusal(shim):
    base = dict(nx=6, ny=5, nlev=2, nt=4, npos=3, j_start=0, j_end=3, nsub=4, niter=2, ntrace=1, times=[0.0, 1.0, 2.0, 3.0], undef=U)
    order = ("nx", "ny", "nlev", "nt", "npos", "j_start", "j_end", "nsub", "niter", "ntrace")

    def both(kw):
        a = dict(base, **kw)
        t = None if a["times"] is None else np.array(a["times"], np.float64)
        got = shim.mifc_test_htraj_check(*[a[k] for k in order], None if t is None else t.ctypes.data, float(np.float32(a["undef"])))
        got = None if got is None else got.decode()
        assert got == ht.check_args(**a), (kw, got)
        return got

    for kw, reason in REFUSALS:
        assert both(kw) == reason, kw
    for kw in ACCEPTED:
        assert both(kw) is None, kw
    assert len({r for _, r in REFUSALS}) == 15


def test_header_plans(shim):
    out = (ctypes.c_int * 16)()
    for j0, j1 in ((0, 3), (3, 0), (2, 1), (1, 2), (0, 9)):
        shim.mifc_test_htraj_plan(j0, j1, out)
        d = 1 if j1 > j0 else -1
        n = abs(j1 - j0) + 1
        assert (out[0], out[1], out[2]) == (d, n, n - 1) and [out[3 + k] for k in range(n)] == list(range(j0, j1 + d, d))
    per_level = (2 * 3 * 1000 + 3 * 3 * 10) * 4  # two slice buffers of u, v and one trace field, three slots of x, y and the trace
    assert shim.mifc_test_htraj_levels_per_chunk(1 << 20, 1000, 10, 3, 1, 50) == (1 << 20) // per_level == 43
    assert shim.mifc_test_htraj_levels_per_chunk(1 << 20, 1000, 10, 3, 1, 7) == 7 and shim.mifc_test_htraj_levels_per_chunk(100, 1000, 10, 3, 1, 7) == 1
    assert [shim.mifc_test_htraj_level_chunk(n, f) for n, f in ((137, 0), (137, 50), (7, 50), (65535, 0), (65536, 0), (200000, 3))] == [1, 50, 7, 1, 2, 4]


def test_header_plane_value_against_the_restatement(shim):
    rng = np.random.default_rng(5)
    plane = ht.sprinkle(rng.normal(0, 5, (4, 6)).astype(np.float32), rng, 0.15, U)
    value = ctypes.c_double()
    xs = np.concatenate([rng.uniform(0, 5, 300), np.arange(6.0), [5.0, -0.0, 2.5]])
    ys = np.concatenate([rng.uniform(0, 3, 300), rng.integers(0, 4, 6).astype(float), [3.0, -0.0, 3.0]])
    for xd, yd in zip(xs, ys):
        for all_defined in (False, True):
            ok = shim.mifc_test_htraj_value(plane.ctypes.data, 6, 4, xd, yd, int(all_defined), float(U), ctypes.addressof(value))
            exp = ht.plane_value(plane, float(xd), float(yd), all_defined, U)
            assert bool(ok) == (exp is not None) and (exp is None or value.value == exp), (xd, yd, all_defined)


def test_rules_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "htraj_rules_asan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "host", "htraj_rules_main.cc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)  # (the environment as it is: the runtimes are linked in)
    assert run.returncode == 0 and " checks, 0 failures" in run.stdout, run.stdout + run.stderr


# ------------------------------------------------------------------------------- declared, bound and configured
def test_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    whole = open(os.path.join(ROOT, "include", "mifc.h")).read()
    header = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    for name in ("mifc_htraj_levels", "mifc_last_htraj_form"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    sig = capi.SIGNATURES["mifc_htraj_levels"]
    assert sig[0] == "i" and len(sig[1]) == 28 and sig[1][-2:] == ["f", "i"] and sig[1][:5] == ["ctx", "i", "i", "i", "i"] and capi.SIGNATURES["mifc_last_htraj_form"] == ("s", [])
    declared = re.search(r"int mifc_htraj_levels\((.*?)\);", header, flags=re.S).group(1)
    assert len(declared.split(",")) == 28 and "mifc_abi_version" in header
    assert header.index("mifc_last_hdist_form(void)") < header.index("mifc_htraj_levels(") < header.index("mifc_neighbourProbFunctions(")
    for rule in ("1. Start.", "2. Sampling a plane", "3. Index velocity", "4. Interval.", "5. Slot.", "6. Lost.", "7. Trace.", "8. Flags."):
        assert rule in whole, rule
    for var in ("MIFC_HTRAJ_CHUNK_MIB", "MIFC_HTRAJ_LEVEL_CHUNK"):
        readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if '"%s"' % var in open(p, errors="replace").read()]
        assert readers == ["mifc_env.hip"], (var, readers)
    host = open(os.path.join(CSRC, "mifc_capi_htraj.hip")).read()
    assert "getenv" not in host and re.search(r"htraj_chunk_mib > 0 \? mifc::env\(\)\.htraj_chunk_mib : 256", host)
    for shared in ("Staging", "htraj_check", "htraj_plan", "htraj_levels_per_chunk", "htraj_level_chunk", "overlaps", "mifc_classify"):
        assert shared in host, shared
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_htraj.hip") == 1 and makefile.count("mifc_capi_htraj.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    assert makefile.count("mifc_htraj_rules.h") == 1  # HDRS
    rules = open(os.path.join(CSRC, "mifc_htraj_rules.h")).read()
    assert "hip" not in re.sub(r"//.*", "", rules).lower()  # HIP-free: the host compiler builds it
    kernel = open(os.path.join(CSRC, "mifc_htraj.hip")).read()
    assert '#include "mifc_htraj_rules.h"' in kernel and '#include "mifc_htraj_rules.h"' in host
    for rule in ("htraj_usable", "htraj_interval", "htraj_trace", "htraj_level_chunk"):
        assert rule in kernel, rule
    assert "### 4.26" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert htraj_module.MAX_NSUB == 64 and htraj_module.MAX_NITER == 8 and htraj_module.MAX_TRACE == 4


# ------------------------------------------------------------------------------- the front against a recording stub
def test_front_marshals_the_entry_in_header_order():
    d = _data()
    ctx, lib = _stub_context(d)
    fin = np.array([[[A, S, S], [S, S, A]], [[S, S, S], [A, A, A]]])
    res = htraj_module.trajectories(ctx, [d["B"], d["V"]], [d["T"], d["Q"]], [0, 3600], d["XM"], d["YM"], d["XP"], d["YP"], start=-1, end=0, nsub=3, niter=1,
                                    trace=[[d["F2"][0], d["F2"][1]], [d["COORD"], d["MINUS1"]]], fdefined_in=fin, fdef_map=A, fdef_trace=A, undef=-5.0)
    name, a = lib.calls[-1]
    assert name == "mifc_htraj_levels" and a[:4] == [5, 4, 3, 2] and a[4] == [["B", 0], ["V", 0]] and a[5] == [["T", 0], ["Q", 0]]
    assert a[6]["values"] == fin.ravel().tolist() and a[6]["numpy"] == "int32" and a[7]["values"] == [0.0, 3600.0] and a[7]["numpy"] == "float64"
    assert a[8:14] == [["XM", 0], ["YM", 0], A, 7, ["XP", 0], ["YP", 0]] and a[14:18] == [1, 0, 3, 1]
    assert a[18] == [["F2", 0], ["F2", 4 * 60], ["COORD", 0], ["MINUS1", 0]] and a[19]["values"] == [A] * 12 and a[20] == 2
    assert a[21] == "<other>" and a[22] == "<other>" and a[23] == ["<other>", "<other>"] and a[24]["shape"] == [3, 2, 3] and a[24]["numpy"] == "int32"
    assert a[25] == -5.0 and a[26] == 0 and len(a) == 27
    assert sorted(res) == ["flags", "trace", "x", "y"] and res["x"].shape == res["y"].shape == (2, 3, 7) and [t.shape for t in res["trace"]] == [(2, 3, 7)] * 2
    assert res["x"].dtype == np.float32 and res["flags"].shape == (3, 2, 3)
    res = htraj_module.trajectories(ctx, [d["B"], d["V"], d["T"]], [d["T"], d["Q"], d["B"]], [0, 1, 2], d["XM"], d["YM"], d["XP"], d["YP"])
    name, a = lib.calls[-1]
    assert a[3] == 3 and a[6] is None and a[10] == S and a[14:18] == [0, 2, 4, 2] and a[18] is None and a[19] is None and a[20] == 0 and a[23] is None
    assert a[24]["shape"] == [1, 3, 3] and a[25] == float(U) and res["trace"] == [] and res["x"].shape == (3, 3, 7)


def test_front_refusals_that_need_no_library():
    d = _data()
    ctx, lib = _stub_context(d)
    n = len(lib.calls)
    good = ([d["B"], d["V"]], [d["T"], d["Q"]], [0, 3600], d["XM"], d["YM"], d["XP"], d["YP"])
    with pytest.raises(ValueError, match="v must hold one"):
        htraj_module.trajectories(ctx, good[0], [d["T"]], *good[2:])
    with pytest.raises(ValueError, match="every batch of u"):
        htraj_module.trajectories(ctx, [d["B"], d["XM"]], *good[1:])
    with pytest.raises(ValueError, match="times must hold"):
        htraj_module.trajectories(ctx, good[0], good[1], [0, 1, 2], *good[3:])
    with pytest.raises(ValueError, match="xmapr and ymapr"):
        htraj_module.trajectories(ctx, good[0], good[1], good[2], d["B"], *good[4:])
    with pytest.raises(ValueError, match="xpos and ypos"):
        htraj_module.trajectories(ctx, *good[:6], d["XM"])
    with pytest.raises(ValueError, match="trace must hold 0..4"):
        htraj_module.trajectories(ctx, *good, trace=[good[0]] * 5)
    with pytest.raises(ValueError, match="a trace field must hold one"):
        htraj_module.trajectories(ctx, *good, trace=[[d["B"]]])
    with pytest.raises(ValueError, match="fdefined_in must hold"):
        htraj_module.trajectories(ctx, *good, fdefined_in=[A, S, A])
    assert len(lib.calls) == n  # nothing reached the library
    ctx, lib = _stub_context(d, rc=0)  # a refusal of the library comes back as Refused, a ValueError and a RuntimeError
    with pytest.raises(htraj_module.Refused) as e:
        htraj_module.trajectories(ctx, *good, nsub=65)
    assert isinstance(e.value, ValueError) and isinstance(e.value, RuntimeError) and lib.calls[-1][1][16] == 65


# ------------------------------------------------------------------------------------------- no scratch, no spills
def test_no_kernel_instance_uses_scratch_or_spills(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if not hipcc:
        pytest.skip("hipcc is not installed")
    flags = re.search(r"^HIPFLAGS := (.*)$", open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read(), flags=re.M).group(1).replace("$(ARCH)", "gfx950")
    run = subprocess.run([hipcc] + flags.split() + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mifc_htraj.hip"), "-o",
                                                    str(tmp_path / "mifc_htraj.o")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    kernels = re.findall(r"Function Name: (\S*htraj_kernel\S*)", run.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", run.stderr)]
    sgpr = [int(x) for x in re.findall(r"SGPRs Spill: (\d+)", run.stderr)]
    vgpr = [int(x) for x in re.findall(r"VGPRs Spill: (\d+)", run.stderr)]
    assert len(set(kernels)) == 4 and len(scratch) == len(sgpr) == len(vgpr) == 4, (kernels, scratch, sgpr, vgpr)  # TESTED x (ntrace > 0)
    assert scratch == [0] * 4 and sgpr == [0] * 4 and vgpr == [0] * 4, (kernels, scratch, sgpr, vgpr)
