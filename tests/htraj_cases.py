"""The seam cases of mifc_htraj_levels: small calls, each aimed at one edge of the definition (include/mifc.h) -- the
arguments of htraj_restate.run() as dicts, by name.  tests/test_htraj_cpu.py runs them through the rules header compiled
by the host compiler, tests/test_gpu_htraj.py through the library; both compare with the restatement for equality.
Out-of-grid and NaN positions are ordinary inputs with a defined result, undef."""
import functools

import numpy as np

import htraj_restate as ht

A, S, N = ht.ALL_DEFINED, ht.SOME_DEFINED, ht.NONE_DEFINED
U = ht.UNDEF
M = np.float32(2.0 ** -10)  # an exact map ratio: 1 m/s for 1024 s is one grid cell


def small(seed=0, nx=6, ny=5, nt=3, nlev=1, npos=40, ntrace=1, holes=0.0, undef=U, speed=3.0):
    """A random small call: winds uniform in +-speed m/s, map ratios 1e-4 * U(0.9, 1.1), slices 3000 s apart."""
    rng = np.random.default_rng(1000 + seed)
    u = rng.uniform(-speed, speed, (nt, nlev, ny, nx)).astype(np.float32)
    v = rng.uniform(-speed, speed, (nt, nlev, ny, nx)).astype(np.float32)
    if holes:
        u = ht.sprinkle(u, rng, holes, undef)
    xm = (1.0e-4 * rng.uniform(0.9, 1.1, (ny, nx))).astype(np.float32)
    ym = (1.0e-4 * rng.uniform(0.9, 1.1, (ny, nx))).astype(np.float32)
    trace = np.stack([(rng.normal(0, 10, (nt, nlev, ny, nx)) + 280 - 5 * f).astype(np.float32) for f in range(ntrace)]) if ntrace else None
    xpos = rng.uniform(0, max(nx - 1, 0), npos).astype(np.float32)
    ypos = rng.uniform(0, max(ny - 1, 0), npos).astype(np.float32)
    return dict(u=u, v=v, times=3000.0 * np.arange(nt), xmapr=xm, ymapr=ym, xpos=xpos, ypos=ypos, j_start=0, j_end=nt - 1, nsub=2, niter=2,
                trace=trace, fdefined_in=None, fdef_map=S, fdef_trace=None, undef=undef)


def uniform(nx=5, ny=4, nt=2, uval=1.0, vval=0.0, tau=1024.0, xpos=(1.0,), ypos=(1.0,), **kw):
    """A uniform wind on the uniform exact map M: a particle moves exactly h * u * M per substep."""
    c = dict(u=np.full((nt, 1, ny, nx), uval, np.float32), v=np.full((nt, 1, ny, nx), vval, np.float32), times=tau * np.arange(nt),
             xmapr=np.full((ny, nx), M, np.float32), ymapr=np.full((ny, nx), M, np.float32), xpos=np.array(xpos, np.float32),
             ypos=np.array(ypos, np.float32), j_start=0, j_end=nt - 1, nsub=1, niter=0, trace=None, fdefined_in=None, fdef_map=S, fdef_trace=None,
             undef=U)
    c.update(kw)
    return c


def _build():
    cases = {}

    # starts on nodes, on the last column or row, at -0.0
    c = small(1)
    c["xpos"] = np.array([0, 1, 2, 5, 5, -0.0, 1.5, 5, 0, 2.25], np.float32)
    c["ypos"] = np.array([0, 1, 4, 4, 1.5, -0.0, 4, 0, 4, 3.0], np.float32)
    cases["starts on nodes and edges"] = c
    # a start that is undef, NaN or outside the grid
    c = small(2)
    c["xpos"] = np.array([U, 1, np.nan, 2, -0.5, 5.0000005, 2, 2, np.inf, -np.inf, 3, 1.0e30], np.float32)
    c["ypos"] = np.array([1, U, 2, np.nan, 2, 2, -1.0e-30, 4.0000005, 2, 2, 1.25, 2], np.float32)
    cases["unusable starts"] = c
    # a wind that carries a particle exactly onto nx - 1, and one ulp beyond (Euler and Petterssen)
    beyond = np.nextafter(np.float32(3), np.float32(4))
    for niter in (0, 2):
        cases["exactly onto the last column, niter=%d" % niter] = uniform(xpos=(3.0, beyond, 2.5), ypos=(1.0, 1.0, 3.0), niter=niter)
        cases["exactly onto the last row, niter=%d" % niter] = uniform(uval=0.0, vval=1.0, xpos=(1.0, 1.0, 4.0), ypos=(2.0, np.nextafter(np.float32(2), np.float32(3)), 0.5), niter=niter)
    cases["exactly onto column 0, backward in the index"] = uniform(uval=-1.0, xpos=(1.0, np.nextafter(np.float32(1), np.float32(0)), 0.0), ypos=(0.0, 0.0, 0.0), niter=1)
    # a predictor that leaves the grid while the corrector would not: the wind turns back in the last cell
    turn = uniform(nx=5, uval=0.0, xpos=(3.25, 3.0, 3.5), ypos=(1.0, 2.0, 0.0), niter=2)
    turn["u"][..., 3] = 2.0
    turn["u"][..., 4] = -2.0
    cases["predictor leaves the grid, one substep"] = turn
    cases["predictor stays inside, four substeps"] = dict(turn, nsub=4)
    # slice A is not read at w == 1: the corrector lands on the node of a huge u_A and takes u_B = 1 there, x = 1 + 512 * 2 / 1024
    huge = uniform(xpos=(1.0,), ypos=(1.0,), niter=1)
    huge["u"][0, 0, :, 2] = 1.0e30
    cases["a huge wind in slice A at w == 1"] = huge
    # a hole in slice B only; a hole in a map plane; both under ALL_DEFINED too
    c = small(3, npos=60)
    c["u"][1, 0, 2, 2:4] = U
    c["v"][2, 0, 1, 1] = np.nan
    cases["holes in slice B only"] = c
    cases["holes in slice B under ALL_DEFINED"] = dict(c, fdefined_in=np.full((2, 3, 1), A))
    mixed = np.full((2, 3, 1), S)
    mixed[0, 1, 0] = A
    cases["mixed flags per slice"] = dict(c, fdefined_in=mixed)
    c = small(4, npos=60, undef=-1.0e-4)  # (under ALL_DEFINED the stored undef is a map ratio of -1e-4: the particle moves on)
    c["xmapr"][2, 3] = -1.0e-4
    c["ymapr"][0, 0] = -1.0e-4
    cases["holes in the map planes"] = c
    cases["holes in the map planes under ALL_DEFINED"] = dict(c, fdef_map=A)
    # inf and NaN winds under ALL_DEFINED
    c = small(5, npos=60)
    c["u"][0, 0, 1, 1], c["u"][1, 0, 3, 4], c["v"][1, 0, 2, 2], c["v"][2, 0, 0, 5] = np.inf, -np.inf, np.nan, np.inf
    cases["inf and NaN winds under ALL_DEFINED"] = dict(c, fdefined_in=np.full((2, 3, 1), A))
    cases["inf and NaN winds tested"] = c
    # a stored undef under ALL_DEFINED is a value: with undef = -2 it is a wind of -2 m/s
    c = small(6, npos=60, undef=-2.0)
    c["u"][:, 0, 1:3, 2:4] = -2.0
    c["trace"][0, :, 0, 3, 1] = -2.0
    cases["a stored undef is a hole"] = c
    cases["a stored undef under ALL_DEFINED is a value"] = dict(c, fdefined_in=np.full((2, 3, 1), A), fdef_trace=np.full((1, 3, 1), A))
    # nx == 1 and ny == 1: a component that is not zero leaves the grid at once
    c = small(7, nx=1, ny=7, npos=30)
    c["u"][:, :, :4, :] = 0.0
    cases["nx == 1"] = c
    c = small(8, nx=9, ny=1, npos=30)
    c["v"][:, :, :, 3:] = np.float32(-0.0)
    cases["ny == 1"] = c
    cases["nx == 1 and ny == 1"] = uniform(nx=1, ny=1, uval=0.0, vval=-0.0, xpos=(0.0, -0.0, 0.5), ypos=(0.0, 0.0, 0.0), niter=2)
    cases["npos == 1"] = small(9, npos=1)
    # a backward run, over all slices and over some
    c = small(10, nt=4, nlev=2, npos=50, holes=0.02)
    cases["backward"] = dict(c, j_start=3, j_end=0)
    cases["backward over the middle slices"] = dict(c, j_start=2, j_end=1)
    cases["forward over the last slices"] = dict(c, j_start=2, j_end=3)
    # the ends of nsub and niter
    c = small(11, npos=50, holes=0.02)
    cases["nsub = 64"] = dict(c, nsub=64, niter=1)
    cases["niter = 0"] = dict(c, nsub=3, niter=0)
    cases["niter = 8"] = dict(c, nsub=1, niter=8)
    # ntrace 0, 1 and 4; a trace hole under a live particle; trace flags per slice
    cases["ntrace = 0"] = small(12, ntrace=0)
    c = small(13, ntrace=4, nlev=2, npos=50)
    c["trace"][0, 1, 0, 1:3, 1:4] = U
    c["trace"][2, :, 1, :, :] = U
    c["trace"][3, 2, 0, 2, 2] = np.nan
    cases["ntrace = 4 with trace holes"] = c
    ftr = np.full((4, 3, 2), S)
    ftr[0, 1, 0] = ftr[3, 2, 0] = ftr[2, 0, 1] = A
    cases["ntrace = 4, some trace planes ALL_DEFINED"] = dict(c, fdef_trace=ftr)
    # undef = NaN
    c = small(14, npos=60, undef=np.nan)
    c["u"][1, 0, 2, 2] = np.nan
    c["trace"][0, 0, 0, 1, 1] = np.nan
    c["xpos"][3] = np.nan
    cases["undef = NaN"] = c
    # nothing tested at all
    c = small(15, npos=60)
    cases["every flag ALL_DEFINED"] = dict(c, fdefined_in=np.full((2, 3, 1), A), fdef_map=A, fdef_trace=np.full((1, 3, 1), A))
    # irregular times
    c = small(16, nt=4, npos=50)
    cases["irregular times"] = dict(c, times=np.array([-7200.0, -7000.0, 1.0e-3, 5400.5]))
    return cases


@functools.lru_cache(maxsize=None)
def cases():
    """name -> the arguments of htraj_restate.run(); shared, not to be written to."""
    built = _build()
    for c in built.values():
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return built


NAMES = tuple(_build())


@functools.lru_cache(maxsize=None)
def expected(name):
    return ht.run(**cases()[name])
