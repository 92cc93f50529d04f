"""Level batches interpolated to per-cell target surfaces (include/mifc.h, mifc_vregrid_*; EXTENSION): free functions that
take a Context, built from the helpers of _args and Context._launch like the functions of vcumul.

    from mi_fieldcalc_amd import vregrid
    out, flags = vregrid.hybrid_to_hybrid(ctx, [t, q, u, v], ps, alevel, blevel, alevel_dst, blevel_dst, ps_dst)
    wind_at_lcl, flags = vregrid.vregrid_hlevels(ctx, [u, v], ps, alevel, blevel, plcl[None], method="log")

Fields are numpy arrays (host memory) or CUDA tensors (device); the result lives where the fields live."""
import ctypes

import numpy as np

from ._args import _Arg, _coord_flags, _drop_one, _field_tables, _hybrid_levels, _is_torch, _level_batches, _level_coord, _level_flags, _output, _parse_form
from ._consts import SOME_DEFINED, UNDEF, VREGRID_METHODS, VREGRID_FROM, VREGRID_OUTSIDE  # noqa: F401  (the tables are this module's to export)
from .vcumul import Refused

__all__ = ["VREGRID_METHODS", "VREGRID_FROM", "VREGRID_OUTSIDE", "Refused", "vregrid_hlevels", "vregrid_fields", "vregrid_levels", "hybrid_to_hybrid", "last_vregrid_form"]


def _target_planes(tcoord, shape):
    """tcoord as one contiguous (ntargets, ny, nx) batch: a stacked array / tensor, one (ny, nx) plane, or a sequence of planes."""
    if not (isinstance(tcoord, np.ndarray) or _is_torch(tcoord)):
        planes = list(tcoord)
        if not planes:
            raise ValueError("no target planes")
        if _is_torch(planes[0]):
            import torch

            tcoord = torch.stack(planes)
        else:
            tcoord = np.stack([np.asarray(p, dtype=np.float32) for p in planes])
    if len(tcoord.shape) == 2:
        tcoord = tcoord[None]
    if _is_torch(tcoord) and not tcoord.is_contiguous():
        tcoord = tcoord.contiguous()
    ta = _Arg(tcoord)
    if len(ta.shape) != 3 or tuple(ta.shape[1:]) != tuple(shape[1:]):
        raise ValueError("tcoord must be (ntargets, ny, nx) planes of the shape %s" % (tuple(shape[1:]),))
    return ta


def _vregrid(ctx, name, fields, coord, coord_args, tcoord, method, from_, outside, fdefined_in, fdef_tcoord, undef, out):
    code = VREGRID_METHODS.get(method, -1) if isinstance(method, str) else int(method)
    walk = VREGRID_FROM.get(from_, -1) if isinstance(from_, str) else int(from_)
    beyond = VREGRID_OUTSIDE.get(outside, -1) if isinstance(outside, str) else int(outside)
    one, batches, fa, shape = _level_batches(fields)
    nlev, ny, nx = shape
    nf = len(fa)
    others = []
    if name == "mifc_vregrid_levels":
        lv = np.ascontiguousarray(np.asarray(coord, dtype=np.float32).ravel())
        if lv.size != nlev:
            raise ValueError("levels must hold one value per level")
        coord_arg = lv
    else:
        ca = _level_coord(coord, name == "mifc_vregrid_hlevels", shape)
        coord_arg = ca.addr
        others.append(ca)
    ta = _target_planes(tcoord, shape)
    others.append(ta)
    nt = int(ta.shape[0])
    tfd = None
    if fdef_tcoord is not None:
        tfd = np.ascontiguousarray(np.broadcast_to(np.asarray(fdef_tcoord, dtype=np.int32).reshape(-1), (nt,)), dtype=np.int32)
    res, oa = _output(out, batches[0], (nt, ny, nx) if one else (nf, nt, ny, nx))
    table, outs = _field_tables(fa, oa, nt * ny * nx * 4)
    fd = np.zeros((nf, nt), np.int32)
    try:
        ctx._launch(name, fa + others + [oa],
                    [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, coord_arg] + coord_args
                    + [ta.addr, tfd, nt, code, walk, beyond, ctypes.addressof(outs), fd, float(undef)])
    except RuntimeError as e:
        raise Refused(str(e)) from None
    return _drop_one(one, res, fd)


def vregrid_hlevels(ctx, fields, ps, alevel, blevel, tcoord, method="linear", from_="first", outside="undef", fdefined_in=None, fdef_ps=SOME_DEFINED,
                    fdef_tcoord=None, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vregrid_hlevels): hybrid-level batches, coordinate c = alevel[k] + blevel[k] * ps,
    interpolated to the target planes tcoord (ntargets, ny, nx): per cell the value where the column's coordinate equals
    the cell's own target.  method: "linear" in c or "log" in its logarithm; from_: "first" takes the first bracketing
    pair of levels in index order, "last" the last one; outside: "undef", or "clamp" -- a target beyond the column's
    smallest / largest coordinate takes the value of that level.  fields: a list of (nlev, ny, nx) numpy arrays (host
    memory) or CUDA tensors (device), or one stacked (nf, nlev, ny, nx); ps: (ny, nx); tcoord: stacked, one (ny, nx) plane or
    a list of planes, where the fields live; fdefined_in: flags (nf, nlev), or one per field; fdef_tcoord: one flag, or
    one per target plane; None: SOME_DEFINED.  Returns (out (nf, ntargets, ny, nx), flags int32 (nf, ntargets)); with ONE
    (nlev, ny, nx) batch for `fields` the leading axis is dropped from both.  A refused call raises Refused (a ValueError)
    with the library's reason."""
    al, bl = _hybrid_levels(fields, alevel, blevel)
    return _vregrid(ctx, "mifc_vregrid_hlevels", fields, ps, [int(fdef_ps), al, bl], tcoord, method, from_, outside, fdefined_in, fdef_tcoord, undef, out)


def vregrid_fields(ctx, fields, coord, tcoord, method="linear", from_="first", outside="undef", fdefined_in=None, fdef_coord=None, fdef_tcoord=None,
                   undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vregrid_fields): as vregrid_hlevels, the coordinate given as a batch (nlev, ny, nx)
    like the fields (pressure, height, potential vorticity ...); fdef_coord: one flag per level, None: SOME_DEFINED."""
    fc_ = _coord_flags(fdef_coord, coord)
    return _vregrid(ctx, "mifc_vregrid_fields", fields, coord, [fc_], tcoord, method, from_, outside, fdefined_in, fdef_tcoord, undef, out)


def vregrid_levels(ctx, fields, levels, tcoord, method="linear", from_="first", outside="undef", fdefined_in=None, fdef_tcoord=None, undef=UNDEF,
                   out=None):
    """EXTENSION (include/mifc.h, mifc_vregrid_levels): as vregrid_hlevels, the coordinate one constant per level (pressure
    levels): `levels` holds nlev numbers."""
    return _vregrid(ctx, "mifc_vregrid_levels", fields, levels, [], tcoord, method, from_, outside, fdefined_in, fdef_tcoord, undef, out)


def hybrid_to_hybrid(ctx, fields, ps, alevel, blevel, alevel_dst, blevel_dst, ps_dst=None, method="log", outside="clamp", from_="first",
                     fdefined_in=None, fdef_ps=SOME_DEFINED, undef=UNDEF, out=None):
    """Model levels to model levels: the fields on the hybrid levels (alevel, blevel) over ps, interpolated to the levels
    (alevel_dst, blevel_dst) over ps_dst (None: ps itself -- another level set over the same orography).  The target
    pressure batch is alevel_dst[t] + blevel_dst[t] * ps_dst in float32, the product rounded first like the reference's
    p_hlevel; where ps_dst is undef (or NaN) it is undef, and so is every result there.  Target levels under the lowest
    source level take that level's values with outside="clamp".  Returns what vregrid_hlevels returns."""
    pd = ps if ps_dst is None else ps_dst
    a = np.ascontiguousarray(np.asarray(alevel_dst, dtype=np.float32).ravel())
    b = np.ascontiguousarray(np.asarray(blevel_dst, dtype=np.float32).ravel())
    if a.size != b.size or a.size == 0:
        raise ValueError("alevel_dst and blevel_dst must hold one value per target level")
    if _is_torch(pd):
        import torch

        ta, tb = (torch.from_numpy(x).to(pd.device)[:, None, None] for x in (a, b))
        bad = (pd == float(undef)) | torch.isnan(pd)
        tcoord = torch.where(bad[None], torch.full((), float(undef), dtype=torch.float32, device=pd.device), ta + tb * pd[None])
    else:
        p32 = np.asarray(pd, dtype=np.float32)
        bad = (p32 == np.float32(undef)) | np.isnan(p32)
        with np.errstate(all="ignore"):
            prod = (b[:, None, None] * p32[None]).astype(np.float32)
            tcoord = np.where(bad[None], np.float32(undef), (a[:, None, None] + prod).astype(np.float32)).astype(np.float32)
    return vregrid_hlevels(ctx, fields, ps, alevel, blevel, tcoord, method, from_, outside, fdefined_in=fdefined_in, fdef_ps=fdef_ps, undef=undef, out=out)


def last_vregrid_form(ctx):
    """The launch shape of this thread's last vregrid call as a dict (mifc_last_vregrid_form; a diagnostic for tests):
    from, outside, coord and method as strings, the other keys as ints."""
    return _parse_form(ctx._lib.mifc_last_vregrid_form(), ("from", "outside", "coord", "method"))
