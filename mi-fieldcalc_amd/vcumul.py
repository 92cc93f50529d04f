"""Running vertical integrals of level batches (include/mifc.h, mifc_vcumul_*; EXTENSION): free functions that take a
Context, built from the helpers of _args and Context._launch like the methods of _levelbatch.

    from mi_fieldcalc_amd import vcumul
    z, flags = vcumul.geopotential_height_hlevels(ctx, t, q, ps, alevel, blevel, zs)

Fields are numpy arrays (host memory) or CUDA tensors (device); the result lives where the fields live."""
import ctypes

import numpy as np

from ._args import (_Arg, _coord_flags, _drop_one, _field_tables, _hybrid_levels, _is_torch, _level_batches, _level_coord, _level_flags, _output,
                    _parse_form, _pointer_table)
from ._consts import GRAVITY, R_DRY, SOME_DEFINED, UNDEF, VCUMUL_FROM, VCUMUL_METHODS  # noqa: F401  (the tables are this module's to export)

__all__ = ["VCUMUL_METHODS", "VCUMUL_FROM", "Refused", "vcumul_hlevels", "vcumul_fields", "vcumul_levels", "geopotential_height_hlevels",
           "last_vcumul_form"]


class Refused(ValueError, RuntimeError):
    """A call the library refused, with its reason: a ValueError (the arguments were wrong) that the handlers of the
    Context methods' RuntimeError catch too."""


def _plane(x, shape, what):
    a = _Arg(x)
    if tuple(a.shape) != tuple(shape[1:]):
        raise ValueError("%s must have the shape %s" % (what, tuple(shape[1:])))
    return a


def _vcumul(ctx, name, fields, coord, coord_args, method, from_, start, fdef_start, base, fdef_base, scale, fdefined_in, undef, out):
    code = VCUMUL_METHODS.get(method, -1) if isinstance(method, str) else int(method)
    walk = VCUMUL_FROM.get(from_, -1) if isinstance(from_, str) else int(from_)
    one, batches, fa, shape = _level_batches(fields)
    nlev, ny, nx = shape
    nf = len(fa)
    others = []
    if name == "mifc_vcumul_levels":
        lv = np.ascontiguousarray(np.asarray(coord, dtype=np.float32).ravel())
        if lv.size != nlev:
            raise ValueError("levels must hold one value per level")
        coord_arg = lv
    else:
        ca = _level_coord(coord, name == "mifc_vcumul_hlevels", shape)
        coord_arg = ca.addr
        others.append(ca)
    sa = None if start is None else _plane(start, shape, "start")
    if sa is not None:
        others.append(sa)
    # base: one (ny, nx) plane per field, a stacked (nf, ny, nx), or -- for ONE batch -- the plane itself; entries may be None
    btab = bfd = None
    if base is not None:
        if hasattr(base, "shape"):
            planes = [base] if one and len(base.shape) == 2 else [base[f] for f in range(base.shape[0])]
        else:
            planes = list(base)
        if len(planes) != nf:
            raise ValueError("base must hold one plane (or None) per field")
        ba = [None if p is None else _plane(p, shape, "a base plane") for p in planes]
        others += [a for a in ba if a is not None]
        btab = _pointer_table([None if a is None else a.addr for a in ba])
        if fdef_base is not None:
            bfd = np.ascontiguousarray(np.broadcast_to(np.asarray(fdef_base, dtype=np.int32).reshape(-1), (nf,)), dtype=np.int32)
    sc = None
    if scale is not None:
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64).reshape(-1), (nf,)), dtype=np.float64)
    res, oa = _output(out, batches[0], shape if one else (nf,) + shape)
    table, outs = _field_tables(fa, oa, nlev * ny * nx * 4)
    fd = np.zeros((nf, nlev), np.int32)
    try:
        ctx._launch(name, fa + others + [oa],
                    [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, coord_arg] + coord_args
                    + [code, walk, None if sa is None else sa.addr, int(fdef_start), None if btab is None else ctypes.addressof(btab), bfd, sc,
                       ctypes.addressof(outs), fd, float(undef)])
    except RuntimeError as e:
        raise Refused(str(e)) from None
    return _drop_one(one, res, fd)


def vcumul_hlevels(ctx, fields, ps, alevel, blevel, method="linear", from_="first", start=None, base=None, scale=None, fdefined_in=None, fdef_ps=SOME_DEFINED,
                   fdef_start=SOME_DEFINED, fdef_base=None, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vcumul_hlevels): the integral of hybrid-level batches over the coordinate
    c = alevel[k] + blevel[k] * ps ("linear") or over its logarithm ("log") from the start of the walk to every level, by
    trapezoids: one value per input level.  from_: "first" walks k = 0, 1, ...; "last" walks k = nlev - 1, ..., 0.
    fields: a list of (nlev, ny, nx) numpy arrays (host memory) or CUDA tensors (device), or one stacked
    (nf, nlev, ny, nx); ps: (ny, nx); fdefined_in: flags (nf, nlev), or one per field; None: SOME_DEFINED.  start: None, or
    a (ny, nx) coordinate at which the integral begins (fdef_start: its flag).  base: None, or per field a (ny, nx) plane
    (or None) that is added to the result (fdef_base: one flag, or one per field).  scale: None, one factor or one per
    field.  Returns (out (nf, nlev, ny, nx), flags int32 (nf, nlev)); with ONE (nlev, ny, nx) batch for `fields` the leading
    axis is dropped from both (and base may be the plane itself).  From the first level in walk order that is missing, a
    column is undef.  A refused call raises Refused (a ValueError) with the library's reason."""
    al, bl = _hybrid_levels(fields, alevel, blevel)
    return _vcumul(ctx, "mifc_vcumul_hlevels", fields, ps, [int(fdef_ps), al, bl], method, from_, start, fdef_start, base, fdef_base, scale, fdefined_in,
                   undef, out)


def vcumul_fields(ctx, fields, coord, method="linear", from_="first", start=None, base=None, scale=None, fdefined_in=None, fdef_coord=None,
                  fdef_start=SOME_DEFINED, fdef_base=None, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vcumul_fields): as vcumul_hlevels, the coordinate given as a batch (nlev, ny, nx)
    like the fields (pressure, height ...); fdef_coord: one flag per level, None: SOME_DEFINED."""
    fc_ = _coord_flags(fdef_coord, coord)
    return _vcumul(ctx, "mifc_vcumul_fields", fields, coord, [fc_], method, from_, start, fdef_start, base, fdef_base, scale, fdefined_in, undef, out)


def vcumul_levels(ctx, fields, levels, method="linear", from_="first", start=None, base=None, scale=None, fdefined_in=None, fdef_start=SOME_DEFINED,
                  fdef_base=None, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vcumul_levels): as vcumul_hlevels, the coordinate one constant per level (pressure
    levels): `levels` holds nlev numbers."""
    return _vcumul(ctx, "mifc_vcumul_levels", fields, levels, [], method, from_, start, fdef_start, base, fdef_base, scale, fdefined_in, undef, out)


def geopotential_height_hlevels(ctx, t, q, ps, alevel, blevel, zs=None, surface_last=True, fdefined_in=None, fdef_ps=SOME_DEFINED, undef=UNDEF,
                                out=None):
    """The height of hybrid levels by the hydrostatic integration of virtual temperature over ln p from the surface:
    z_k = zs - (Rd / g) * integral from ps to p_k of Tv d ln p, with Tv = t * (1 + 0.608 * q) formed here (torch on device
    tensors, numpy on host arrays; q=None: dry air).  t, q: (nlev, ny, nx); ps, zs: (ny, nx), zs=None: heights above the
    surface.  surface_last: the levels are stored top-down (the walk starts at level nlev - 1).  Where t or q is undef
    (or NaN) Tv is undef: the column is undef from that level on.  Returns (z (nlev, ny, nx), flags int32 (nlev,))."""
    if q is None:
        tv = t
    elif _is_torch(t):
        import torch

        bad = (t == float(undef)) | (q == float(undef)) | torch.isnan(t) | torch.isnan(q)
        tv = torch.where(bad, torch.full_like(t, float(undef)), t * (1 + 0.608 * q))
    else:
        t32, q32 = np.asarray(t, np.float32), np.asarray(q, np.float32)
        bad = (t32 == np.float32(undef)) | (q32 == np.float32(undef)) | np.isnan(t32) | np.isnan(q32)
        with np.errstate(all="ignore"):
            tv = np.where(bad, np.float32(undef), t32 * (1 + np.float32(0.608) * q32)).astype(np.float32)
    return vcumul_hlevels(ctx, tv, ps, alevel, blevel, "log", "last" if surface_last else "first", start=ps, base=zs, scale=-R_DRY / GRAVITY, fdefined_in=fdefined_in, fdef_ps=fdef_ps,
                          fdef_start=fdef_ps, undef=undef, out=out)


def last_vcumul_form(ctx):
    """The launch shape of this thread's last vcumul call as a dict (mifc_last_vcumul_form; a diagnostic for tests):
    method and from as strings, the other keys as ints."""
    return _parse_form(ctx._lib.mifc_last_vcumul_form(), ("method", "from"))
