"""Parcel ascent over level batches: CAPE, CIN, LCL, LFC, EL and the parcel temperature (include/mifc.h,
mifc_vparcel_*; EXTENSION): free functions that take a Context, built from the helpers of _args and Context._launch like
the functions of vcumul.

    from mi_fieldcalc_amd import vparcel
    r = vparcel.vparcel_hlevels(ctx, t, ps, alevel, blevel, q_src=q[-1], src_level=nlev - 1, from_="last")
    r["cape"], r["plcl"], r["flags"]["cape"]

t is a numpy array (host memory) or a CUDA tensor (device); the results live where t lives."""
import numpy as np

from ._args import _Arg, _coord_flags, _hybrid_levels, _level_batches, _level_coord, _output, _parse_form
from ._consts import SOME_DEFINED, UNDEF, VPARCEL_FROM, VPARCEL_OUTPUTS  # noqa: F401  (the tables are this module's to export)

__all__ = ["VPARCEL_FROM", "VPARCEL_OUTPUTS", "Refused", "vparcel_hlevels", "vparcel_fields", "vparcel_levels", "last_vparcel_form"]

_PLANES = VPARCEL_OUTPUTS[:5]


class Refused(ValueError, RuntimeError):
    """A call the library refused, with its reason: a ValueError (the arguments were wrong) that the handlers of the
    Context methods' RuntimeError catch too."""


def _plane(x, shape, what):
    a = _Arg(x)
    if tuple(a.shape) != tuple(shape[1:]):
        raise ValueError("%s must have the shape %s" % (what, tuple(shape[1:])))
    return a


def _vparcel(ctx, name, t, coord, coord_args, q_src, src_level, from_, t_src, p_src, outputs, fdefined_in, fdef_tsrc, fdef_qsrc, fdef_psrc, undef,
             out):
    walk = VPARCEL_FROM.get(from_, -1) if isinstance(from_, str) else int(from_)
    one, batches, fa, shape = _level_batches(t)
    if not one:
        raise ValueError("t must be one (nlev, ny, nx) batch")
    nlev, ny, nx = shape
    ta = fa[0]
    others = []
    if name == "mifc_vparcel_levels":
        lv = np.ascontiguousarray(np.asarray(coord, dtype=np.float32).ravel())
        if lv.size != nlev:
            raise ValueError("levels must hold one value per level")
        coord_arg = lv
    else:
        ca = _level_coord(coord, name == "mifc_vparcel_hlevels", shape)
        coord_arg = ca.addr
        others.append(ca)
    src = -1 if src_level is None else int(src_level)
    qa = _plane(q_src, shape, "q_src")
    tsa = None if t_src is None else _plane(t_src, shape, "t_src")
    psa = None if p_src is None else _plane(p_src, shape, "p_src")
    if src < 0 and (tsa is None or psa is None):
        raise ValueError("a source given by planes (src_level None or -1) needs t_src, q_src and p_src")
    others += [a for a in (qa, tsa, psa) if a is not None]
    names = [outputs] if isinstance(outputs, str) else list(outputs)
    for n in names:
        if n not in VPARCEL_OUTPUTS:
            raise ValueError("unknown output %r: one of %s" % (n, ", ".join(VPARCEL_OUTPUTS)))
    given = dict(out or {})
    res, oas = {}, {}
    for n in VPARCEL_OUTPUTS:
        if n in names:
            want = shape if n == "tparcel" else shape[1:]
            res[n], oas[n] = _output(given.get(n), batches[0], want, "out[%r] must have shape %s" % (n, want))
    fdin = None if fdefined_in is None else np.ascontiguousarray(np.broadcast_to(np.asarray(fdefined_in, dtype=np.int32).reshape(-1), (nlev,)), dtype=np.int32)
    fd = np.full(5 + nlev, SOME_DEFINED, np.int32)
    addr = lambda a: None if a is None else a.addr  # noqa: E731
    try:
        ctx._launch(name, [ta] + others + list(oas.values()),
                    [nx, ny, nlev, ta.addr, fdin, coord_arg] + coord_args
                    + [walk, src, addr(tsa), int(fdef_tsrc), qa.addr, int(fdef_qsrc), addr(psa), int(fdef_psrc)]
                    + [addr(oas.get(n)) for n in VPARCEL_OUTPUTS] + [fd, float(undef)])
    except RuntimeError as e:
        raise Refused(str(e)) from None
    flags = {n: (fd[5:].copy() if n == "tparcel" else int(fd[_PLANES.index(n)])) for n in res}
    res["flags"] = flags
    return res


def vparcel_hlevels(ctx, t, ps, alevel, blevel, q_src, src_level=0, from_="first", t_src=None, p_src=None, outputs=_PLANES, fdefined_in=None,
                    fdef_ps=SOME_DEFINED, fdef_tsrc=SOME_DEFINED, fdef_qsrc=SOME_DEFINED, fdef_psrc=SOME_DEFINED, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vparcel_hlevels): lifts a parcel through the hybrid-level batch t (nlev, ny, nx; K),
    pressure alevel[k] + blevel[k] * ps (hPa), by the reference's moist adjustment stepped from level to level, and
    returns a dict of the outputs asked for -- "cape", "cin" (J/kg), "plcl", "plfc", "pel" (hPa): (ny, nx); "tparcel":
    (nlev, ny, nx) -- plus "flags": per plane an int, for "tparcel" int32 (nlev,).  from_: "first" walks k = 0, 1, ...;
    "last" walks k = nlev - 1, ..., 0 (pressure must fall along the walk).  The source: src_level, a level of the batch,
    with the specific humidity q_src (ny, nx; kg/kg); or src_level=None with the planes t_src, q_src, p_src (a mixed-layer
    parcel).  fdefined_in: one flag, or one per level.  out: a dict of arrays / tensors to write into.  No
    virtual-temperature correction.  A refused call raises Refused (a ValueError) with the library's reason."""
    al, bl = _hybrid_levels(t, alevel, blevel)
    return _vparcel(ctx, "mifc_vparcel_hlevels", t, ps, [int(fdef_ps), al, bl], q_src, src_level, from_, t_src, p_src, outputs, fdefined_in, fdef_tsrc,
                    fdef_qsrc, fdef_psrc, undef, out)


def vparcel_fields(ctx, t, p, q_src, src_level=0, from_="first", t_src=None, p_src=None, outputs=_PLANES, fdefined_in=None, fdef_coord=None,
                   fdef_tsrc=SOME_DEFINED, fdef_qsrc=SOME_DEFINED, fdef_psrc=SOME_DEFINED, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vparcel_fields): as vparcel_hlevels, the pressure given as a batch (nlev, ny, nx)
    like t; fdef_coord: one flag per level, None: SOME_DEFINED."""
    fc_ = _coord_flags(fdef_coord, p)
    return _vparcel(ctx, "mifc_vparcel_fields", t, p, [fc_], q_src, src_level, from_, t_src, p_src, outputs, fdefined_in, fdef_tsrc, fdef_qsrc,
                    fdef_psrc, undef, out)


def vparcel_levels(ctx, t, levels, q_src, src_level=0, from_="first", t_src=None, p_src=None, outputs=_PLANES, fdefined_in=None,
                   fdef_tsrc=SOME_DEFINED, fdef_qsrc=SOME_DEFINED, fdef_psrc=SOME_DEFINED, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_vparcel_levels): as vparcel_hlevels, the pressure one constant per level (pressure
    levels): `levels` holds nlev numbers."""
    return _vparcel(ctx, "mifc_vparcel_levels", t, levels, [], q_src, src_level, from_, t_src, p_src, outputs, fdefined_in, fdef_tsrc, fdef_qsrc,
                    fdef_psrc, undef, out)


def last_vparcel_form(ctx):
    """The launch shape of this thread's last vparcel call as a dict (mifc_last_vparcel_form; a diagnostic for tests):
    form and from as strings, the other keys as ints."""
    return _parse_form(ctx._lib.mifc_last_vparcel_form(), ("form", "from"))
