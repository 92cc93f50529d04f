"""Ertel potential vorticity of level batches (include/mifc.h, mifc_pvort_*; EXTENSION): free functions that take a
Context, built from the helpers of _args and Context._launch like the functions of vcumul.

    from mi_fieldcalc_amd import pvort
    pv, flags = pvort.potential_vorticity_hlevels(ctx, u, v, t, ps, alevel, blevel, xmapr, ymapr, fcoriolis)
    p_trop, _ = ctx.vinterp_fields(p, pv, [2.0], fdef_coord=flags)   # the pressure of the 2 PVU surface

Fields are numpy arrays (host memory) or CUDA tensors (device); the result lives where the fields live."""
import numpy as np

from ._args import _Arg, _coord_flags, _hybrid_levels, _level_batches, _level_coord, _level_flags, _output, _parse_form
from ._consts import GRAVITY, SOME_DEFINED, UNDEF, VDERIV_METHODS
from .vcumul import Refused

__all__ = ["Refused", "pvort_hlevels", "pvort_fields", "pvort_levels", "potential_vorticity_hlevels", "last_pvort_form", "PVU_SCALE"]

# with the coordinate in hPa: -g * 1e4 gives PVU (1e-6 K m^2 / (kg s)); 1e-2 for hPa -> Pa, 1e6 for the unit
PVU_SCALE = -GRAVITY * 1e4


def _plane(x, shape, what):
    a = _Arg(x)
    if tuple(a.shape) != tuple(shape[1:]):
        raise ValueError("%s must have the shape %s" % (what, tuple(shape[1:])))
    return a


def _pvort(ctx, name, u, v, th, coord, coord_args, xmapr, ymapr, fcoriolis, method, scale, fdefined_in, undef, out):
    code = VDERIV_METHODS.get(method, -1) if isinstance(method, str) else int(method)
    _, batches, fa, shape = _level_batches([u, v, th])
    nlev, ny, nx = shape
    others = []
    if name == "mifc_pvort_levels":
        lv = np.ascontiguousarray(np.asarray(coord, dtype=np.float32).ravel())
        if lv.size != nlev:
            raise ValueError("levels must hold one value per level")
        coord_arg = lv
    else:
        ca = _level_coord(coord, name == "mifc_pvort_hlevels", shape)
        coord_arg = ca.addr
        others.append(ca)
    xa, ya = _plane(xmapr, shape, "xmapr"), _plane(ymapr, shape, "ymapr")
    others += [xa, ya]
    fca = None if fcoriolis is None else _plane(fcoriolis, shape, "fcoriolis")
    if fca is not None:
        others.append(fca)
    res, oa = _output(out, batches[0], shape)
    fd = np.zeros(nlev, np.int32)
    try:
        ctx._launch(name, fa + others + [oa],
                    [nx, ny, nlev, fa[0].addr, fa[1].addr, fa[2].addr, _level_flags(fdefined_in, 3, nlev), coord_arg] + coord_args
                    + [xa.addr, ya.addr, None if fca is None else fca.addr, code, float(scale), oa.addr, fd, float(undef)])
    except RuntimeError as e:
        raise Refused(str(e)) from None
    return res, fd


def pvort_hlevels(ctx, u, v, th, ps, alevel, blevel, xmapr, ymapr, fcoriolis=None, method="centred", scale=1.0, fdefined_in=None, fdef_ps=SOME_DEFINED,
                  out=None, undef=UNDEF):
    """EXTENSION (include/mifc.h, mifc_pvort_hlevels): scale * [(fcoriolis + dv/dx - du/dy) dth/dc - dv/dc dth/dx +
    du/dc dth/dy] on hybrid levels, c = alevel[k] + blevel[k] * ps, in one pass: the vertical derivatives by the rules of
    vderiv_hlevels ("centred" or "weighted"), the horizontal ones by the reference's centred differences with the map
    ratios xmapr, ymapr, along the surfaces of the batch; the outer ring is a copy of its interior neighbour.  u, v, th:
    (nlev, ny, nx) numpy arrays (host memory) or CUDA tensors (device); ps, xmapr, ymapr, fcoriolis: (ny, nx), fcoriolis
    None: relative instead of absolute vorticity.  fdefined_in: flags (3, nlev) in the order u, v, th, or one per field;
    None: SOME_DEFINED.  Returns (pv (nlev, ny, nx), flags int32 (nlev,)), the flags counted over the interior cells.  A
    refused call raises Refused (a ValueError) with the library's reason."""
    al, bl = _hybrid_levels(u, alevel, blevel)
    return _pvort(ctx, "mifc_pvort_hlevels", u, v, th, ps, [int(fdef_ps), al, bl], xmapr, ymapr, fcoriolis, method, scale, fdefined_in, undef, out)


def pvort_fields(ctx, u, v, th, p, xmapr, ymapr, fcoriolis=None, method="centred", scale=1.0, fdefined_in=None, fdef_coord=None, out=None, undef=UNDEF):
    """EXTENSION (include/mifc.h, mifc_pvort_fields): as pvort_hlevels, the coordinate given as a batch (nlev, ny, nx)
    like the fields; fdef_coord: one flag per level, None: SOME_DEFINED."""
    return _pvort(ctx, "mifc_pvort_fields", u, v, th, p, [_coord_flags(fdef_coord, p)], xmapr, ymapr, fcoriolis, method, scale, fdefined_in, undef, out)


def pvort_levels(ctx, u, v, th, levels, xmapr, ymapr, fcoriolis=None, method="centred", scale=1.0, fdefined_in=None, out=None, undef=UNDEF):
    """EXTENSION (include/mifc.h, mifc_pvort_levels): as pvort_hlevels, the coordinate one constant per level (pressure
    levels): `levels` holds nlev numbers."""
    return _pvort(ctx, "mifc_pvort_levels", u, v, th, levels, [], xmapr, ymapr, fcoriolis, method, scale, fdefined_in, undef, out)


def potential_vorticity_hlevels(ctx, u, v, t, ps, alevel, blevel, xmapr, ymapr, fcoriolis, method="weighted", fdef_wind=None, fdef_thermo=None,
                                fdef_ps=SOME_DEFINED, undef=UNDEF, out=None):
    """Ertel potential vorticity in PVU on hybrid levels from the wind, the temperature t (Kelvin) and ps (hPa): the
    potential temperature by the fused derived batch (hleveltemp, compute 3), then pvort_hlevels with scale = -g * 1e4.
    fdef_wind, fdef_thermo: one flag per level for u and v / for t, None: SOME_DEFINED.  Returns (pv (nlev, ny, nx), flags
    int32 (nlev,))."""
    nlev = int(_Arg(t).shape[0])
    got = ctx.hlevel_derived_batch(None, None, t, None, ps, alevel, blevel, temp=("", 3), ff=False, fdef_thermo=fdef_thermo, undef=undef)
    if got is None:
        raise Refused("mifc_hlevel_derived_batch: " + ctx.last_error())
    th, th_flags = got[0]["temp"], got[1]["temp"]
    wind = np.full(nlev, SOME_DEFINED, np.int32) if fdef_wind is None else np.asarray(fdef_wind, np.int32).reshape(nlev)
    return pvort_hlevels(ctx, u, v, th, ps, alevel, blevel, xmapr, ymapr, fcoriolis, method, PVU_SCALE, fdefined_in=np.stack([wind, wind, th_flags]),
                         fdef_ps=fdef_ps, out=out, undef=undef)


def last_pvort_form(ctx):
    """The launch shape of this thread's last pvort call as a dict (mifc_last_pvort_form; a diagnostic for tests): kind,
    method and tile as strings, the other keys as ints."""
    return _parse_form(ctx._lib.mifc_last_pvort_form(), ("kind", "method", "tile"))
