"""Trajectories through a series of wind level batches (include/mifc.h, mifc_htraj_levels; EXTENSION): points carried
by the wind of a level from time slice to time slice, forward or backward -- where the air of a plume came from, an origin
map (a backward trajectory from every grid cell), temperature or humidity along the path -- without a round trip of the
positions per evaluation.  Every level carries its own copy of the particles; positions are in grid-index units, as
hinterp_levels takes them.  The results are bit for bit the definition of the header, whatever the memory kind or the
staging.  A free function that takes a Context, built from the helpers of _args and Context._launch like the functions of
hdist.

    from mi_fieldcalc_amd import htraj
    back = htraj.trajectories(ctx, u, v, times, xmapr, ymapr, xs, ys, start=-1, end=0)           # u, v: one batch per time
    path = htraj.trajectories(ctx, u, v, times, xmapr, ymapr, xs, ys, trace=[t, q], nsub=6)
    path["x"], path["y"]            # (nslots, nlev, npos): slot n is slice start + n * dir
    path["trace"][0]                # t along the path, (nslots, nlev, npos)
    path["flags"]                   # int32 (1 + ntrace, nslots, nlev): [0] the positions, [1 + f] trace field f

Fields are numpy arrays (host memory) or CUDA tensors (device); the results live where the fields live."""
import ctypes

import numpy as np

from ._args import _Arg, _empty_like, _memkind, _parse_form, _pointer_table, _same_shape
from ._consts import SOME_DEFINED, UNDEF
from .vcumul import Refused

__all__ = ["Refused", "trajectories", "last_htraj_form", "MAX_NSUB", "MAX_NITER", "MAX_TRACE"]

# the limits of mifc_htraj_levels
MAX_NSUB = 64
MAX_NITER = 8
MAX_TRACE = 4


def _slices(batches, what, nt=None, shape=None):
    """One (nlev, ny, nx) batch per time slice as _Arg: (the arguments, the shape of a batch)."""
    fa = [_Arg(b) for b in batches]
    if not fa or (nt is not None and len(fa) != nt):
        raise ValueError("%s must hold one (nlev, ny, nx) batch per time" % what)
    shape = tuple(fa[0].shape) if shape is None else shape
    if len(shape) != 3 or not _same_shape(fa, shape):
        raise ValueError("every batch of %s must have the shape %s" % (what, shape if len(shape) == 3 else "(nlev, ny, nx)"))
    return fa, shape


def _flags(flags, n, what):
    """Flags as the flat int32 table of the C entry, None as it is: one flag for everything, or the full table of n."""
    if flags is None:
        return None
    f = np.asarray(flags, dtype=np.int32)
    if f.size == 1:
        f = np.full(n, int(f.reshape(())), np.int32)
    if f.size != n:
        raise ValueError("%s must hold one flag, or %d" % (what, n))
    return np.ascontiguousarray(f.reshape(n), dtype=np.int32)


def trajectories(ctx, u, v, times, xmapr, ymapr, xpos, ypos, start=0, end=-1, nsub=4, niter=2, trace=(), fdefined_in=None,
                 fdef_map=SOME_DEFINED, fdef_trace=None, undef=UNDEF):
    """EXTENSION (include/mifc.h, mifc_htraj_levels): the particles that start at (xpos, ypos) on every level of slice
    `start`, carried by the wind of their level to slice `end` -- nsub substeps per interval between two slices, each an
    Euler predictor and niter Petterssen corrections, the winds linear in time between the slices; every operation in
    double, the state rounded to float at every slice.  u, v: sequences of nt (nlev, ny, nx) arrays or tensors, one per
    time; times: nt seconds (double), strictly increasing; xmapr, ymapr: the (ny, nx) map-ratio planes of the stencil
    operators; xpos, ypos: npos positions in grid-index units.  start, end: slices, a negative one counts from the last
    (end < start runs backward).  trace: fields sampled along the path (bilinear, as hinterp_levels does), each a sequence
    of nt batches.  fdefined_in: one flag, or (2, nt, nlev) for u and v; fdef_trace: one flag, or (ntrace, nt, nlev).
    Returns a dict: "x", "y" float32 (nslots, nlev, npos), undef from the slot on at which a particle is lost (it left the
    grid, or met a hole in the winds or the map planes); "trace" a list of (nslots, nlev, npos); "flags" int32
    (1 + ntrace, nslots, nlev).  The launch shape is in last_htraj_form().  A refused call raises Refused (a ValueError)
    with the library's reason."""
    ua, shape = _slices(u, "u")
    nt = len(ua)
    va, _ = _slices(v, "v", nt, shape)
    nlev, ny, nx = shape
    fields = [list(f) for f in trace]
    if len(fields) > MAX_TRACE:
        raise ValueError("trace must hold 0..%d fields" % MAX_TRACE)
    ta = [_slices(f, "a trace field", nt, shape)[0] for f in fields]
    ntrace = len(ta)
    t = np.ascontiguousarray(np.asarray(times, dtype=np.float64).ravel())
    if t.size != nt:
        raise ValueError("times must hold one value per time slice of u")
    xm, ym = _Arg(xmapr), _Arg(ymapr)
    if tuple(xm.shape) != (ny, nx) or tuple(ym.shape) != (ny, nx):
        raise ValueError("xmapr and ymapr must have the shape %s" % ((ny, nx),))
    xa, ya = _Arg(xpos), _Arg(ypos)
    if len(xa.shape) != 1 or tuple(xa.shape) != tuple(ya.shape):
        raise ValueError("xpos and ypos must be one-dimensional and equally long")
    npos = int(xa.shape[0])
    j_start, j_end = (int(j) + nt if int(j) < 0 else int(j) for j in (start, end))
    nslots = abs(j_end - j_start) + 1
    every = ua + va + [a for f in ta for a in f] + [xm, ym, xa, ya]
    _memkind(every, ctx.device)  # (before anything is allocated: host and device arguments do not mix)
    out_shape = (nslots, nlev, npos)
    outs = [_empty_like(u[0], out_shape) for _ in range(2 + ntrace)]
    oa = [_Arg(o, output=True) for o in outs]
    fd = np.zeros((1 + ntrace, nslots, nlev), np.int32)
    tu, tv = _pointer_table([a.addr for a in ua]), _pointer_table([a.addr for a in va])
    tt = _pointer_table([a.addr for f in ta for a in f]) if ntrace else None
    tr = _pointer_table([a.addr for a in oa[2:]]) if ntrace else None
    try:
        ctx._launch("mifc_htraj_levels", every + oa,
                    [nx, ny, nlev, nt, ctypes.addressof(tu), ctypes.addressof(tv), _flags(fdefined_in, 2 * nt * nlev, "fdefined_in"), t, xm.addr, ym.addr,
                     int(fdef_map), npos, xa.addr, ya.addr, j_start, j_end, int(nsub), int(niter), ctypes.addressof(tt) if ntrace else None,
                     _flags(fdef_trace, ntrace * nt * nlev, "fdef_trace") if ntrace else None, ntrace, oa[0].addr, oa[1].addr,
                     ctypes.addressof(tr) if ntrace else None, fd, float(undef)])
    except RuntimeError as err:
        raise Refused(str(err)) from None
    return {"x": outs[0], "y": outs[1], "trace": outs[2:], "flags": fd}


def last_htraj_form(ctx):
    """The launch shape of this thread's last trajectories call as a dict of ints (mifc_last_htraj_form; a diagnostic for
    tests)."""
    return _parse_form(ctx._lib.mifc_last_htraj_form())
