"""The cases that tests/test_vparcel_cpu.py (the stability condition) and tests/test_gpu_vparcel.py (the kernel) share:
small soundings whose LCL, LFC and EL move across a row, with every kind of hole, for every phase of the kernel's slot
rotation (nlev 2, 3, 4, 7, 12), both cell-per-lane forms (9 x 16: four cells per lane, 9 x 13: one), both walk
directions and the three kinds of source.  Two cases of 10 x 206 = 2 060 cells fill several workgroups and a tail.

A case is a dict of float32 arrays in LEVEL order (what the entries take).  Its three coordinate forms:
  hyb: ps, al, bl                 lev: plev (one pressure per level)
  fld: p, the hybrid pressure with holes of its own (undef, NaN, <= 0, not falling)
reference(case, form) runs the restatement once un-nudged (R0) and once per member of the nudge family, and keeps it."""
import functools

import numpy as np

import vparcel_restate as vp

F = np.float32
U = vp.UNDEF
A, S_ = vp.ALL_DEFINED, vp.SOME_DEFINED
NLEVS = (2, 3, 4, 7, 12)
SHAPES = ((9, 16), (9, 13))
SOURCES = ("first", "middle", "planes")
FORMS = ("hyb", "fld", "lev")
PLANES = vp.OUTPUTS[:5]


def _qsat(T, p):
    ok, q = vp.sat_test((vp.CP * T.astype(F)).astype(F), p.astype(F))
    return np.where(ok, q, F(1e-3)).astype(F)


def make(nlev, ny, nx, from_, source, seed=0, factor=1.0):
    """factor: every pressure of the case (ps, alevel, the fields form's p, the levels, p_src) times this number, q_src from
    the saturation value at the scaled pressure (tests/vparcel_range_cases.py); 1: the cases as they always were."""
    rng = np.random.default_rng(1000 * nlev + 10 * ny + nx + seed)
    k = F(factor)
    top = 300.0 if nlev <= 3 else 240.0  # (the coldest, driest parcels leave the saturation table below it)
    P = (1000.0 * (top / 1000.0) ** (np.arange(nlev) / (nlev - 1))).astype(F)  # position order: the surface first
    bl = ((P / F(1000.0)) ** 2).astype(F)
    al = (P - F(1000.0) * bl).astype(F)
    al[0], bl[0] = F(0.0), F(1.0)
    P, al = (P * k).astype(F), (al * k).astype(F)
    x = np.broadcast_to(np.arange(nx)[None, :], (ny, nx))
    y = np.broadcast_to(np.arange(ny)[:, None], (ny, nx))
    ps = ((985.0 + 3.0 * (x % 11) + 1.7 * y + rng.uniform(-0.5, 0.5, (ny, nx))).astype(F) * k).astype(F)
    p = vp.hybrid_pressure(ps, al, bl, A)
    Ts = (250.0 + 56.0 *((x * 7 + y * 3) % nx) / max(nx - 1, 1) + rng.uniform(-0.4, 0.4, (ny, nx))).astype(F)
    g = (0.10 + 0.17 * ((x * 5 + y) % 7) / 6.0).astype(F)  # d ln T / d ln p: 0.286 is the dry adiabat
    strat = np.where((x + 2 * y) % 5 == 0, 0.0, 204.0 + 1.5 * (x % 8)).astype(F)  # 0: no cap, B may stay > 0 to the top
    t = np.maximum(Ts[None] * (p / ps[None]) ** g[None], strat[None]).astype(F)
    t = (t + rng.uniform(-0.3, 0.3, t.shape)).astype(F)
    t[:, :, 1 % nx] = (Ts[:, 1 % nx] - F(1.0))[None]  # an isothermal column: no LFC
    rh = np.choose((x + 3 * y) % 6, [1e-4, 0.25, 0.55, 0.8, 0.96, 1.15]).astype(F)

    order = np.arange(nlev) if from_ == "first" else np.arange(nlev)[::-1]  # order[j] = the level of position j
    to_level = np.argsort(order)                                             # arrays in position order -> level order
    c = {"name": "n%d_%dx%d_%s_%s" % (nlev, ny, nx, from_, source), "nlev": nlev, "ny": ny, "nx": nx, "from": from_, "source": source}
    if source == "planes":
        c["src_level"] = None
        c["p_src"] = np.where((x + y) % 3 == 0, ps + F(4.0) * k, ps * F(0.97)).astype(F)  # below the ground / between two levels
        c["t_src"] = (Ts + F(0.5)).astype(F)
        c["q_src"] = (rh * _qsat(c["t_src"], c["p_src"])).astype(F)
        js = -1
    else:
        js = 0 if source == "first" else nlev // 2
        c["src_level"] = int(order[js])
        c["p_src"] = c["t_src"] = None
        c["q_src"] = (rh * _qsat(t[js], p[js])).astype(F)
    fdin = np.where(np.arange(nlev) % 3 == 1, A, S_).astype(np.int32)  # mixed flags, in position order

    # ---- holes, in position order; j1: a position behind the source (where there is one)
    j1 = min(js + 2, nlev - 1)
    col = lambda k: k % nx  # noqa: E731
    t[j1, 0, col(3)] = U                          # undef t in mid-column: a hole under SOME_DEFINED, a (huge) value under ALL
    t[j1, 1, col(5)] = np.nan                     # NaN t: a hole under any flag
    t[min(js + 1, nlev - 1), 2, col(6)] = U
    if js >= 0:
        t[js, 3, col(2)] = U                      # an undef source level
    c["q_src"][4, col(7)] = U                     # an undef source humidity
    c["q_src"][5, col(8)] = np.nan
    if source == "planes":
        c["t_src"][6, col(4)] = U
        c["p_src"][7, col(9)] = U
        c["p_src"][8, col(10)] = F(-5.0)
    ps_h = ps.copy()
    ps_h[6, col(1)] = U                           # the hybrid form's hole: no pressure in the whole column
    pf = p.copy()
    pf[j1, 2, col(0)] = U                         # the fields form's holes
    pf[j1, 3, col(9)] = np.nan
    pf[j1, 4, col(11)] = pf[j1 - 1, 4, col(11)]   # not falling
    pf[j1, 5, col(12)] = F(-1.0)
    pf[nlev - 1, 7, col(2)] = F(0.0)
    fdc = np.where(np.arange(nlev) % 2 == 0, A, S_).astype(np.int32)

    c.update(t=np.ascontiguousarray(t[to_level]), ps=ps_h, al=np.ascontiguousarray(al[to_level]), bl=np.ascontiguousarray(bl[to_level]),
             p=np.ascontiguousarray(pf[to_level]), plev=np.ascontiguousarray(P[to_level]), fdefined_in=np.ascontiguousarray(fdin[to_level]),
             fdef_coord=np.ascontiguousarray(fdc[to_level]))
    return c


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    i = 0
    for nlev in NLEVS:
        for from_ in ("first", "last"):
            for source in SOURCES:
                ny, nx = SHAPES[i % 2]
                out.append(make(nlev, ny, nx, from_, source))
                i += 1
    out.append(make(7, 10, 206, "last", "first"))  # 2 060 cells: three workgroups of four-cell lanes with a tail, nine of one-cell lanes
    out.append(make(4, 10, 206, "first", "planes"))
    return tuple(out)


def case_names():
    return [c["name"] for c in cases()]


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def nudge_family(nlev, ny, nx):
    """The members of the pi nudge family: all -1, all +1, alternating by level in both phases, two seeded random patterns."""
    shape = (nlev + 1, ny, nx)
    alt = np.where(np.arange(nlev + 1) % 2 == 0, 1, -1)[:, None, None] * np.ones(shape, np.int64)
    rng = np.random.default_rng(77 + nlev)
    return [np.full(shape, -1), np.full(shape, 1), alt, -alt, rng.integers(-1, 2, shape), rng.integers(-1, 2, shape)]


def run_restatement(c, form, pi_nudge=None, diag=None, host_pi=False):
    kw = dict(from_=c["from"], src_level=c["src_level"], t_src=c["t_src"], p_src=c["p_src"], fdefined_in=c["fdefined_in"], pi_nudge=pi_nudge, diag=diag)
    if form == "hyb":
        return vp.hlevels(c["t"], c["ps"], c["al"], c["bl"], c["q_src"], **kw)
    if form == "fld":
        return vp.fields(c["t"], c["p"], c["q_src"], fdef_coord=c["fdef_coord"], **kw)
    return vp.levels(c["t"], c["plev"], c["q_src"], host_pi=host_pi, **kw)


class Reference:
    """R0, the family's members, and per cell whether the case is stable there (tests/test_vparcel_cpu.py asserts how few
    cells are not): no member differs from R0 in the undef-ness of an output, in the piece that holds LCL, LFC or EL, or
    in whether the adjustment ran at a level."""

    def __init__(self, c, form):
        d0 = {}
        self.r0 = run_restatement(c, form, diag=d0)
        self.members = []
        stable = np.ones((c["ny"], c["nx"]), bool)
        for nudge in nudge_family(c["nlev"], c["ny"], c["nx"]):
            d = {}
            r = run_restatement(c, form, pi_nudge=nudge, diag=d)
            self.members.append(r)
            for n in vp.OUTPUTS:
                same = (r[n] == U) == (self.r0[n] == U)
                stable &= same if same.ndim == 2 else same.all(axis=0)
            for n in ("lcl_pos", "lfc_pos", "el_pos"):
                stable &= d[n] == d0[n]
            stable &= (d["adjusted"] == d0["adjusted"]).all(axis=0)
        self.stable = stable
        self.diag = d0

    def bound(self, name):
        """2 * max_j |R_j - R0| + 2 ulp_float32(R0), per value (meaningful on stable cells)."""
        r0 = self.r0[name].astype(np.float64)
        with np.errstate(all="ignore"):
            spread = np.max([np.abs(m[name].astype(np.float64) - r0) for m in self.members], axis=0)
            return 2.0 * spread + 2.0 * np.spacing(np.abs(self.r0[name])).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(name, form):
    return Reference(by_name(name), form)
