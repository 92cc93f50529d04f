"""Seeded cases of mifc_vregrid_* that tests/test_vregrid_cpu.py (restatement, rules header) and tests/test_gpu_vregrid.py
share.  A case is a dict: kind ("hybrid" | "field" | "levels"), fields, coord (ps, the coordinate batch or the levels), ab
(hybrid), tcoord, and optionally flags, fdef_c (fdef_ps or fdef_coord), fdef_t, undef.  expected(case, method, from_,
outside) runs the restatement."""
import functools

import numpy as np

import vinterp_restate as vi
import vregrid_restate as vg

METHODS = {"linear": vg.LINEAR, "log": vg.LOG}
FROM = {"first": vg.FROM_FIRST, "last": vg.FROM_LAST}
OUTSIDE = {"undef": vg.OUTSIDE_UNDEF, "clamp": vg.OUTSIDE_CLAMP}
MIXED = [vg.ALL_DEFINED, vg.SOME_DEFINED, vg.NONE_DEFINED]


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, tuple):
            for a in v:
                a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def main(kind="hybrid", nf=3, nlev=12, ny=9, nx=13, nt=5, seed=1, bottom_up=False):
    """vinterp's main generator (ps in 700..1050, 3 % of ps and of every field undef) with nt target planes that follow the
    levels of a second surface pressure, some of them beyond both ends of the column, 3 % of the targets undef."""
    fields, ps, alevel, blevel = vi.main_case(nf, nlev, ny, nx, seed)
    if bottom_up:
        fields, alevel, blevel = np.ascontiguousarray(fields[:, ::-1]), np.ascontiguousarray(alevel[::-1]), np.ascontiguousarray(blevel[::-1])
    coord = vi.hybrid_coordinate(np.where(ps == vi.UNDEF, np.float32(900), ps), alevel, blevel)
    tcoord = vg.target_planes(coord, nt, seed + 100)
    if kind == "hybrid":
        return _frozen(dict(kind=kind, fields=fields, coord=ps, ab=(alevel, blevel), tcoord=tcoord))
    if kind == "levels":
        lv = np.ascontiguousarray(coord[:, 0, 0])
        return _frozen(dict(kind=kind, fields=fields, coord=lv, tcoord=tcoord))
    coord[:, ps == vi.UNDEF] = vi.UNDEF
    return _frozen(dict(kind=kind, fields=fields, coord=coord, tcoord=tcoord))


@functools.lru_cache(maxsize=None)
def wavy(nf=2, nlev=12, ny=9, nx=13, nt=5, seed=11):
    """Non-monotone pressures, built as in test_gpu_vinterp.py: pairs overlap, the first and the last bracket differ."""
    base = main("field", nf, nlev, ny, nx, nt, 1)
    rng = np.random.default_rng(seed)
    c = (base["coord"] * rng.uniform(0.5, 1.5, base["coord"].shape)).astype(np.float32)
    c[base["coord"] == vi.UNDEF] = vi.UNDEF
    return _frozen(dict(kind="field", fields=base["fields"], coord=c, tcoord=base["tcoord"]))


@functools.lru_cache(maxsize=None)
def heights(nf=2, nlev=7, ny=9, nx=13, nt=6, seed=5, holes=0.08):
    """Signed heights in steps of 100 with zeros (of both signs), equal neighbours, ties for the extremes and holes; the
    targets on the same steps -- exactly on levels, beyond both ends, undef and NaN among them.  LINEAR's ground."""
    rng = np.random.default_rng(seed)
    z = np.round(rng.uniform(-3, 3, (nlev, ny, nx))).astype(np.float32) * 100
    z[(z == 0) & (rng.random(z.shape) < 0.5)] = np.float32(-0.0)
    z = vi.sprinkle(z, rng, holes, vi.UNDEF)
    fields = np.stack([vi.sprinkle(rng.normal(0, 10, (nlev, ny, nx)).astype(np.float32), rng, 0.05, vi.UNDEF) for _ in range(nf)])
    t = np.round(rng.uniform(-4.4, 4.4, (nt, ny, nx))).astype(np.float32) * 100
    t = vi.sprinkle(vi.sprinkle(t, rng, 0.04, vi.UNDEF), rng, 0.03, np.nan)
    return _frozen(dict(kind="field", fields=fields, coord=z, tcoord=t))


@functools.lru_cache(maxsize=None)
def flagged(seed=3):
    """Mixed fdefined_in, fdef_coord and fdef_tcoord tables over stored undef and NaN."""
    base = main("field", 3, 12, 9, 13, 5, 1)
    rng = np.random.default_rng(seed)
    return _frozen(dict(kind="field", fields=vi.sprinkle(base["fields"], rng, 0.03, np.nan), coord=vi.sprinkle(base["coord"], rng, 0.03, np.nan),
                        tcoord=vi.sprinkle(base["tcoord"], rng, 0.03, np.nan), flags=rng.choice(MIXED, size=(3, 12)).astype(np.int32),
                        fdef_c=rng.choice(MIXED, size=12).astype(np.int32), fdef_t=rng.choice(MIXED, size=5).astype(np.int32)))


def with_nan_undef(case):
    """The same case with NaN for undef."""
    nan = np.float32(np.nan)
    swap = lambda a: np.where(a == vi.UNDEF, nan, a)  # noqa: E731
    out = dict(case, fields=swap(case["fields"]), tcoord=swap(case["tcoord"]), undef=nan)
    if case["kind"] != "levels":
        out["coord"] = swap(case["coord"])
    return out


def expected(case, method, from_="first", outside="undef", **kw):
    m, fr, o = METHODS[method], FROM[from_], OUTSIDE[outside]
    undef = case.get("undef", vi.UNDEF)
    flags = case.get("flags")
    if flags is not None and np.ndim(flags) == 1:
        flags = np.repeat(np.asarray(flags).reshape(-1, 1), case["fields"].shape[1], axis=1)
    if case["kind"] == "hybrid":
        return vg.hlevels(case["fields"], case["coord"], case["ab"][0], case["ab"][1], case["tcoord"], m, fr, o, flags,
                          vg.SOME_DEFINED if case.get("fdef_c") is None else case["fdef_c"], case.get("fdef_t"), undef, **kw)
    if case["kind"] == "field":
        return vg.coord_fields(case["fields"], case["coord"], case["tcoord"], m, fr, o, flags, case.get("fdef_c"), case.get("fdef_t"), undef, **kw)
    return vg.levels(case["fields"], case["coord"], case["tcoord"], m, fr, o, flags, case.get("fdef_t"), undef, **kw)
