"""Seeded cases that put the stencil operators at the ends of the float range (numpy only: no GPU, nothing read from the
reference).  tests/test_stencil_seams_cpu.py asserts on the CPU that the cases reach what they are meant to reach and pins
the oracle to the compiled reference on them; tests/test_gpu_stencil_seams.py runs them through every kernel form that has
its own copy of the point formulas.

A case is a dict:
  op       key of OPS                          label   "<op>-<class>-maps-<placement>[-nan-undef]-<nx>x<ny>": names the seam
  nx, ny, nlev                                 fields  list of (nlev, ny, nx) float32 arrays, in the operator's argument order
  xm, ym, fc   (ny, nx) map factors, Coriolis  flags   int32[nlev]: ALL_DEFINED, SOME_DEFINED, SOME_DEFINED
  undef    1e35, or NaN in the "-nan-undef" variant
  hours / pres   advection's scalar, plevelqvector's pressure per level

What the ingredients are for (the kernels replace the reference's expressions by cheaper ones that are equal under
conditions on the operands; the cases sit where those conditions end):
  fcoriolis  a row of +0 (the equator of a global grid) and a sprinkled quarter (plevelqvector: an eighth, see make_case) of
             zeros, denormals, huge values, infinities and NaN: the f64 divisions of the geostrophic operators, done through
             a shared reciprocal
  map factors  a sprinkled eighth (placement "some") of zeros, denormals, values around 2^-125 (below it half a map factor
             is not exact), values whose squares leave the float range, +inf and a negative one; placement "all": every
             map factor below 2^-125; "none": ordinary ones -- waves with no, one and only inexact halves
  fields     per magnitude class: differences that overflow, inf - inf, differences that are denormal, plateaus, signed
             zeros; for the operators that multiply partials the decades are chosen so that the partials lie near
             sqrt(FLT_MAX) or sqrt(FLT_MIN) and their products straddle the ends of the range; +inf, -inf, +0 and -0
             sprinkled in (2 % each and 2.5 % each; fewer infinities for the operators with wide footprints, see INF_FRACTION),
             a plateau over the equator row, a patch of signed zeros, and on the SOME_DEFINED levels 3 % undef with some NaN

The rates and decades are tuned until the conditions asserted in tests/test_stencil_seams_cpu.py hold: a case must not
degrade into comparing NaN with NaN.
"""
import numpy as np

import mi_fieldcalc_amd.synth as synth

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
UNDEF = np.float32(1.0e35)
NX_FORMS = (68, 260, 258)  # below one segment | one 256-column segment and a group | ragged, remainder 2
NY, NLEV = 13, 3
FLAGS = np.array([ALL_DEFINED, SOME_DEFINED, SOME_DEFINED], np.int32)
HOURS = 3.0
PRESSURES = np.array([850.0, 500.0, 300.0], np.float32)

_F = np.float32
FLT_MAX, FLT_MIN, DENORM_MIN = np.finfo(np.float32).max, np.finfo(np.float32).tiny, _F(2.0) ** _F(-149)

FC_SPECIALS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, 1e-40, FLT_MIN, -FLT_MIN, 1e-20, -1e20, 3e38, -FLT_MAX, np.inf, -np.inf, np.nan],
                       np.float32)
# 1.9e19 and 3e38: their squares leave the float range (not the double range); 2^-149, 1e-39, 3*2^-127, 2^-126: below 2^-125
MAP_SPECIALS = np.array([0.0, -0.0, DENORM_MIN, 1e-39, 2.0 ** -126, 3 * 2.0 ** -127, 2.0 ** -125, 1e-20, 1e19, 1.9e19, 3e38, np.inf, -1.7e-5],
                        np.float32)

# operator key -> (oracle operator(s), number of input fields, takes fcoriolis, compute or None)
OPS = {
    "relvort": (("relvort",), 2, False, None), "divergence": (("divergence",), 2, False, None), "absvort": (("absvort",), 2, True, None),
    "vortdiv": (("relvort", "divergence"), 2, False, None), "vortdiv_ff": (("relvort", "divergence", "vectorabs"), 2, False, None),
    "gradient1": (("gradient",), 1, False, 1), "gradient2": (("gradient",), 1, False, 2), "gradient3": (("gradient",), 1, False, 3),
    "gradient4": (("gradient",), 1, False, 4),
    "plevelgwind_xcomp": (("plevelgwind_xcomp",), 1, True, None), "plevelgwind_ycomp": (("plevelgwind_ycomp",), 1, True, None),
    "plevelgvort": (("plevelgvort",), 1, True, None), "ilevelgwind": (("ilevelgwind",), 1, True, None),
    "jacobian": (("jacobian",), 2, False, None), "advection": (("advection",), 3, False, None),
    "thermalFrontParameter": (("thermalFrontParameter",), 1, False, None),
    "plevelqvector1": (("plevelqvector",), 2, True, 1), "plevelqvector2": (("plevelqvector",), 2, True, 2),
    "plevelqvector3": (("plevelqvector",), 2, True, 3), "plevelqvector4": (("plevelqvector",), 2, True, 4),
    "shapiro2_filter": (("shapiro2_filter",), 1, False, None),
}
FAMILIES = {
    "wind": ("relvort", "divergence", "absvort", "vortdiv"), "wind_ff": ("vortdiv_ff",),
    "scalar": ("gradient1", "gradient2", "gradient3", "gradient4", "plevelgwind_xcomp", "plevelgwind_ycomp", "plevelgvort", "ilevelgwind"),
    "jacobian": ("jacobian",), "advection": ("advection",), "tfp": ("thermalFrontParameter",),
    "qvector": ("plevelqvector1", "plevelqvector2", "plevelqvector3", "plevelqvector4"), "shapiro": ("shapiro2_filter",),
}
GEOSTROPHIC = ("plevelgwind_xcomp", "plevelgwind_ycomp", "plevelgvort", "ilevelgwind") + FAMILIES["qvector"]

# Result classes an operator's arithmetic cannot produce (tests/test_stencil_seams_cpu.py skips them):
EXEMPT = {
    # sqrtf(x*x + y*y): never negative, and -0 only from sqrtf(-0), which a sum of two squares is not
    # and its largest finite value is sqrtf(FLT_MAX) = 1.8e19, its smallest non-zero one sqrtf(2^-149) = 3.7e-23
    "gradient3": ("-inf", "-0", ">1e30", "denormal"),
    # the filter's first sweep copies its input where it does not smooth; -0 comes out only where a cell and its neighbours
    # are all -0 (x + 0.25 * (sum - 2x) with x = -0 needs sum = -0), which sprinkled zeros do not line up to
    "shapiro2_filter": ("-0",),
}


def _rand(shape, seed):
    return synth.uniform(shape, seed)


def _sprinkle(a, seed, values, frac):
    """frac of the cells of `a` (any shape) take a value of `values`, chosen per cell."""
    flat = a.reshape(-1)
    r = _rand(flat.shape, seed)
    idx = np.nonzero(r < frac)[0]
    pick = (synth.splitmix64(idx, seed + 77) % np.uint64(len(values))).astype(np.int64)
    flat[idx] = np.asarray(values, np.float32)[pick]
    return a


def maps(nx, ny, placement, seed, h=27800.0, fc_frac=0.25):
    """(xm, ym, fc): synth.grid_maps with the equator row and the special values on top."""
    xm, ym, fc = synth.grid_maps(nx, ny, h=h)
    fc = fc.copy()
    _sprinkle(fc, seed + 1, FC_SPECIALS, fc_frac)
    fc[ny // 2, :] = _F(0.0)  # the equator
    fc[2, nx - 16:nx - 4] = _F(-0.0)  # over the fields' patch of signed zeros: -0 + -0 in absvort, 0 / 0 in the geostrophic operators
    if placement == "some":
        _sprinkle(xm, seed + 2, MAP_SPECIALS, 0.125)
        _sprinkle(ym, seed + 3, MAP_SPECIALS, 0.125)
    elif placement == "all":
        # every map factor below 2^-125: half of it is a denormal whose last bit is lost (for the odd ones)
        scale = _F(2.0) ** _F(-126) / _F(max(xm.max(), ym.max()))
        jitter = (1.0 + 0.25 * _rand(xm.shape, seed + 4)).astype(np.float32)
        xm = (xm * scale * jitter).astype(np.float32)
        ym = (ym * scale * jitter[::-1]).astype(np.float32)
        assert xm.max() < 2.0 ** -125 and ym.max() < 2.0 ** -125
    else:
        assert placement == "none"
    return xm, ym, fc


def _smooth(kind, nx, ny, nlev, seed):
    """Zero-centred smooth fields of order 1 with noise: the wind of synth.wind / 20, the geopotential wave of
    synth.scalar_field / 120."""
    if kind == "u":
        return (synth.wind(nx, ny, seed, nlev=nlev)[0] / _F(20.0)).astype(np.float32)
    if kind == "v":
        return (synth.wind(nx, ny, seed, nlev=nlev)[1] / _F(15.0)).astype(np.float32)
    return np.stack([synth.scalar_field(nx, ny, seed + 13 * l, base=0.0, amp=1.0, noise=0.3) for l in range(nlev)]).astype(np.float32)


def field(kind, nx, ny, nlev, seed, cls, decades, undef=UNDEF, plateau=(3, 8), zeros=3, base=0.0, inf_frac=0.02):
    """One input field of a case, (nlev, ny, nx).
    cls: "ordinary" (base + smooth * 10^decades[l]), "huge" / "tiny" (smooth * 10^decades[l]; the tiny class with a decade at
    or below -38 is built from bit patterns instead: neighbours a few ulps apart near 1e-38, or denormal themselves),
    "mixed" (every cell draws its decade from decades[0]..decades[1])."""
    s = _smooth(kind, nx, ny, nlev, seed).astype(np.float64)
    out = np.empty((nlev, ny, nx), np.float32)
    with np.errstate(all="ignore"):
        if cls == "mixed":
            lo, hi = decades
            dec = np.floor(lo + (hi - lo + 1) * _rand(s.shape, seed + 5))
            out[...] = (s * 10.0 ** dec).astype(np.float32)
        else:
            for l in range(nlev):
                d = decades[l % len(decades)]
                if cls == "tiny" and d <= -38:
                    steps = np.floor(16 * _rand((ny, nx), seed + 6 + l)).astype(np.int32)
                    if d == -38:  # a few ulps apart near 1e-38: the differences are denormal
                        bits = np.float32(1e-38).view(np.int32) + steps
                    else:  # denormal themselves
                        bits = np.int32(int(10.0 ** (d + 45) / 1.4)) + steps * np.int32(max(1, int(10.0 ** (d + 44)))) + 1
                    v = bits.astype(np.int32).view(np.float32)
                    out[l] = np.where(s[l] < 0, -v, v)
                else:
                    out[l] = (base + s[l] * 10.0 ** d).astype(np.float32)
    big = FLT_MAX / _F(1.1)
    for l in range(nlev):
        _sprinkle(out[l], seed + 100 + l, [np.inf], inf_frac)
        _sprinkle(out[l], seed + 200 + l, [-np.inf], inf_frac)
        _sprinkle(out[l], seed + 300 + l, [0.0], 0.025)
        _sprinkle(out[l], seed + 400 + l, [-0.0], 0.025)
        if cls == "huge":  # neighbours of opposite sign at the end of the range: differences that overflow
            _sprinkle(out[l], seed + 500 + l, [big, -big], inf_frac)
    # the plateau: equal values, centred on the equator row
    pr, pc = plateau
    j0, i0 = ny // 2 - pr // 2, 9
    for l in range(nlev):
        ordinary = out[l][np.isfinite(out[l]) & (out[l] != 0)]
        out[l, j0:j0 + pr, i0:i0 + pc] = ordinary[l]
    # a patch of signed zeros: differences and sums of zeros of every sign (rows 1..zeros, 12 columns)
    for l in range(nlev):
        z = np.where((np.arange(12) + l) % 3 == 0, _F(-0.0), _F(0.0)).astype(np.float32)
        out[l, 1:1 + zeros, nx - 16:nx - 4] = z[None, :]
        out[l, 2, nx - 16:nx - 4:2] = _F(-0.0)
    for l in range(nlev):
        if FLAGS[l] == ALL_DEFINED:
            if undef == undef:
                out[l][out[l] == undef] = _F(0.5) * undef  # no undef under ALL_DEFINED (inf and NaN are allowed)
        else:
            out[l] = synth.sprinkle_undef(out[l], seed + 600 + l, 0.03, undef=undef, nan_every=4)
    return out


# Per operator: class -> decades of the field(s), h of synth.grid_maps, map placement.  The linear operators keep one scaling
# per class.  The operators that multiply partials get decades that put the partials (after the map factor: 1.8e-5 at
# h = 27800, of order 1 at h = 0.5) near 1e17..1e20 or 1e-22..1e-18, so that the products straddle the ends of the float range;
# a smooth field of order 1 has differences of 0.01..0.6.  "dec2": the second input's decades where they differ.
def _spec(dec, h, maps, dec2=None):
    return dict(dec=dec, h=h, maps=maps, dec2=dec2 or dec)


_LINEAR = {
    "ordinary": _spec((1.3, 1.3, 1.3), 27800.0, "some"),
    "huge": _spec((36.0, 37.0, 37.8), 27800.0, "all"),
    "tiny": _spec((-38, -41, -43), 0.5, "some"),
    "mixed": _spec((-42, 36), 27800.0, "none"),
}
_PRODUCT = {  # jacobian, gradient 3: partial = 0.5 * m * difference
    "ordinary": _spec((1.3, 1.3, 1.3), 27800.0, "some"),
    "huge": _spec((19.0, 19.7, 20.3), 0.5, "none"),
    "tiny": _spec((-18.0, -19.5, -21.0), 0.5, "some"),
    "mixed": _spec((-22, 20), 0.5, "none"),
    "huge-tinymaps": _spec((36.5, 37.5, 38.0), 27800.0, "all"),
}
# advection rounds once, after u * partial * (-3600 * hours): the product of two inputs straddles the range
_ADVECTION = dict(_PRODUCT, huge=_spec((16.6, 17.2, 17.8), 0.5, "none"), **{"huge-tinymaps": _spec((35.5, 36.2, 36.6), 27800.0, "all")})
# thermalFrontParameter: |grad t| overflows at partials of 1.8e19; its own partials times a ratio below 1 reach the end of the
# range only with large map factors (h = 1e-13: 5e12).  Its divisor |grad t| is a sqrtf: infinite in the huge class, zero on the
# plateau, never denormal (the smallest non-zero value is sqrtf(2^-149) = 3.7e-23)
_TFP = dict(_PRODUCT, huge=_spec((6.0, 6.6, 7.1), 1e-13, "none"))
# plevelqvector: the geostrophic wind is the geopotential's partial times g / f (1e5), so z stays four to five decades below t
_QVECTOR = dict(_PRODUCT, huge=_spec((14.0, 14.7, 15.3), 0.5, "none", dec2=(18.5, 19.1, 19.7)),
                tiny=_spec((-22.5, -24.0, -25.5), 0.5, "some", dec2=(-17.5, -19.0, -20.5)), mixed=_spec((-26, 16), 0.5, "none", dec2=(-22, 20)))
# shapiro2_filter: f[i-1] + f[i+1] overflows where f[i-1] - 2 f[i] + f[i+1] does not
_SHAPIRO = dict(_LINEAR, huge=_spec((37.5, 38.2, 38.4), 27800.0, "all"))
TABLE = {}
for _op in OPS:
    TABLE[_op] = _LINEAR
for _op in ("jacobian", "gradient3"):
    TABLE[_op] = _PRODUCT
TABLE["advection"] = _ADVECTION
TABLE["thermalFrontParameter"] = _TFP
for _op in FAMILIES["qvector"]:
    TABLE[_op] = _QVECTOR
TABLE["shapiro2_filter"] = _SHAPIRO
NAN_UNDEF_CLASS = "ordinary"  # the extra variant with undef = NaN
# thermalFrontParameter and plevelqvector are stencils of stencils (13 input cells per result) and the filter's four sweeps
# reach two cells each way (25): with +inf and -inf at 2 % each fewer than 30 % of their results would be finite, so their
# fields get 1 % each -- and 0.5 % for plevelqvector, where the equator row alone (f = 0: an infinite geostrophic wind) takes the
# results of three rows of eleven in the two components that difference across rows
INF_FRACTION = dict.fromkeys(OPS, 0.02)
INF_FRACTION.update({"thermalFrontParameter": 0.01, "shapiro2_filter": 0.01}, **dict.fromkeys(FAMILIES["qvector"], 0.005))


def _seed(op, cls, nx):
    return 7000 + 131 * sorted(OPS).index(op) + 17 * sorted(_PRODUCT).index(cls) + nx


def make_case(op, cls, nx, ny=NY, nlev=NLEV, undef=UNDEF):
    spec = TABLE[op][cls]
    names, nfields, _, compute = OPS[op]
    qvec = op.startswith("plevelqvector")
    seed = _seed(op, cls, nx)
    # (plevelqvector differences the geostrophic wind again: a special fcoriolis cell takes five results, and an eighth of the
    # cells is what leaves 30 % of them finite)
    xm, ym, fc = maps(nx, ny, spec["maps"], seed, h=spec["h"], fc_frac=0.125 if qvec else 0.25)
    kw = dict(undef=undef, inf_frac=INF_FRACTION[op])
    if op == "thermalFrontParameter":
        kw["plateau"] = (5, 10)  # large enough for |grad t| == 0 inside
    if op == "shapiro2_filter":
        kw["zeros"] = 5  # a zero survives the four sweeps only two cells away from anything else
    base = 5500.0 if cls == "ordinary" and (nfields == 1 or qvec) else 0.0
    kinds = {"jacobian": "zu", "advection": "zuv"}.get(op, "zz" if qvec else "uv" if nfields == 2 else "z")
    fields = [field(k, nx, ny, nlev, seed + 1000 * n, cls, spec["dec2"] if n else spec["dec"],
                    base=(250.0 if qvec and n and base else base if k == "z" else 0.0), **kw) for n, k in enumerate(kinds)]
    if qvec:  # the temperature is undefined where the geopotential is, as in tests/cases.py
        z, t = fields
        bad = np.isnan(z) | (z == undef)
        fields = [z, np.where(bad, z, t).astype(np.float32)]
    label = "%s-%s-maps-%s%s-%dx%d" % (op, cls, spec["maps"], "" if undef == undef else "-nan-undef", nx, ny)
    return dict(op=op, nx=nx, ny=ny, nlev=nlev, fields=fields, xm=xm, ym=ym, fc=fc, flags=FLAGS[:nlev].copy(), undef=_F(undef), label=label,
                hours=HOURS, pres=PRESSURES[:nlev].copy(), compute=compute, cls=cls, maps=spec["maps"])


_CACHE = {}


def cases_for(op, nx=NX_FORMS[0]):
    """The cases of one operator at one width: one per magnitude class, and the undef = NaN variant.  Cached; treat as read-only."""
    key = (op, nx)
    if key not in _CACHE:
        cs = [make_case(op, cls, nx) for cls in TABLE[op]]
        cs.append(make_case(op, NAN_UNDEF_CLASS, nx, undef=np.nan))
        for c in cs:
            for a in c["fields"] + [c["xm"], c["ym"], c["fc"]]:
                a.setflags(write=False)
        _CACHE[key] = cs
    return _CACHE[key]


def oracle_calls(case, l):
    """[(oracle operator, argument list)] for level l, in the order of the operator's outputs."""
    names, nfields, use_fc, compute = OPS[case["op"]]
    f = [a[l] for a in case["fields"]]
    xm, ym, fc = case["xm"], case["ym"], case["fc"]
    out = []
    for name in names:
        if name == "vectorabs":
            args = [f[0], f[1]]
        elif name == "advection":
            args = [f[0], f[1], f[2], xm, ym, case["hours"]]
        elif name == "plevelqvector":
            args = [f[0], f[1], xm, ym, fc, float(case["pres"][l]), compute]
        elif name == "shapiro2_filter":
            args = [f[0]]
        else:
            args = f + [xm, ym] + ([fc] if use_fc else []) + ([compute] if compute else [])
        out.append((name, args))
    return out


def expect(lib, case):
    """The per-level single-field calls of a CpuLib: (outputs[level][k] as arrays, flags[level][k], ok)."""
    outs, flags, ok_all = [], [], True
    for l in range(case["nlev"]):
        o_l, f_l = [], []
        for name, args in oracle_calls(case, l):
            ok, o, f = lib.call(name, case["nx"], case["ny"], *args, fdefined=int(case["flags"][l]), undef=case["undef"])
            ok_all = ok_all and ok
            for a in (o if isinstance(o, tuple) else (o,)):
                o_l.append(a)
                f_l.append(f)
        outs.append(o_l)
        flags.append(f_l)
    return outs, flags, ok_all


def interior(a):
    return a[1:-1, 1:-1]


CLASSES = ("+inf", "-inf", "nan", "+0", "-0", ">1e30", "denormal")


def classify_results(a, undef):
    """Counts of the result classes over the interior of one output, and the count of finite, non-zero, not-undef cells."""
    x = interior(np.asarray(a, np.float32))
    notu = ~(x == undef) if undef == undef else ~np.isnan(x)
    fin = np.isfinite(x) & notu
    ax = np.abs(x)
    counts = {
        "+inf": int(np.count_nonzero(x == np.inf)), "-inf": int(np.count_nonzero(x == -np.inf)),
        "nan": int(np.count_nonzero(np.isnan(x))) if undef == undef else 0,
        "+0": int(np.count_nonzero((x == 0) & ~np.signbit(x))), "-0": int(np.count_nonzero((x == 0) & np.signbit(x))),
        ">1e30": int(np.count_nonzero(fin & (ax > 1e30))), "denormal": int(np.count_nonzero(fin & (ax > 0) & (ax < FLT_MIN))),
    }
    good = int(np.count_nonzero(fin & (x != 0)))
    return counts, good, int(x.size)
