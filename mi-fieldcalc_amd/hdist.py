"""Area histograms and exact percentiles of level batches (include/mifc.h, mifc_hdist_*; EXTENSION): the shape of the
distribution that hstats_levels stops short of -- a robust colour scale, the area fraction above a threshold, an empirical
CDF, the median of a field or of an error field -- without a copy of the batch to the host.  Counts are integers and
percentiles are order statistics: the results are exact, the same bits whatever the launch, the memory kind or the staging.
Free functions that take a Context, built from the helpers of _args and Context._launch like the functions of hremap.

    from mi_fieldcalc_amd import hdist
    counts = hdist.histogram_levels(ctx, t2m, edges=np.arange(230, 320, 5))             # (nlev, 1, nedges + 2) int32
    rows = hdist.histogram_levels(ctx, [rr, cc], [[0.1, 1, 10], [0.5]], mode="rows")    # edges per field: equally many
    scale, flags = hdist.quantile_levels(ctx, t2m, [2, 98])                             # a robust colour scale per level: (nlev, 2)
    q, flags = hdist.quantile_levels(ctx, err, [25, 50, 75], mask=sea, box=(i0, i1, j0, j1))

Fields are numpy arrays (host memory) or CUDA tensors (device); the result lives where the fields live."""
import ctypes

import numpy as np

from ._args import _Arg, _is_torch, _level_batches, _level_flags, _output, _parse_form, _pointer_table
from ._consts import HSTATS_MODES, SOME_DEFINED, UNDEF
from .vcumul import Refused

__all__ = ["Refused", "histogram_levels", "quantile_levels", "last_hdist_form", "QUANTILE_METHODS", "MAX_EDGES", "MAX_PERCENTILES"]

# the methods of mifc_hdist_quantile_levels (MIFC_QUANTILE_*), the limits of the two entries
QUANTILE_METHODS = {"lower": 0, "linear": 1}
MAX_EDGES = 1024
MAX_PERCENTILES = 16


def _edges(edges, nf):
    """edges as the (nf, nedges) float32 table of the C entry: one list for every field, or one list per field."""
    e = np.asarray(edges, dtype=np.float32)
    if e.ndim == 1:
        e = np.broadcast_to(e, (nf, e.size))
    if e.ndim != 2 or e.shape[0] != nf:
        raise ValueError("edges must be one list of edges, or one list per field, all of the same length")
    if not 1 <= e.shape[1] <= MAX_EDGES:
        raise ValueError("edges must hold 1..%d values per field" % MAX_EDGES)
    return np.ascontiguousarray(e, dtype=np.float32)


def _area(fa, mask, box, shape):
    """The mask plane and the box of a call: (the mask's _Arg, the int32 box or None, the rows of the box)."""
    nlev, ny, nx = shape
    ma = _Arg(mask, allow_none=True)
    if mask is not None and tuple(ma.shape) != (ny, nx):
        raise ValueError("mask must have the shape %s" % ((ny, nx),))
    bx = None
    if box is not None:
        bx = np.ascontiguousarray(np.asarray(box, dtype=np.int32).ravel())
        if bx.size != 4:
            raise ValueError("box is (i0, i1, j0, j1)")
    return ma, bx, (int(bx[3] - bx[2]) if bx is not None else ny)


def _int_output(ref, shape):
    """An int32 result of `shape` where `ref` lives, pre-filled with -1 (a refused call writes nothing): (object, address)."""
    if _is_torch(ref):
        import torch

        out = torch.full(shape, -1, dtype=torch.int32, device=ref.device)
        return out, out.data_ptr()
    out = np.full(shape, -1, np.int32)
    return out, out.ctypes.data


def histogram_levels(ctx, fields, edges, mask=None, box=None, mode="area", fdefined_in=None, fdef_mask=SOME_DEFINED, undef=UNDEF):
    """EXTENSION (include/mifc.h, mifc_hdist_histogram_levels): the included cells of every (field, level) counted into
    the bins of `edges` -- strictly ascending, bin b = the number of edges <= x (numpy.searchsorted(edges, x, "right")),
    -0.0 with +0.0, a NaN (under ALL_DEFINED) in the last slot.  fields, fdefined_in: as hstats_levels takes them.  edges:
    one list for all fields, or one per field (equally many).  mask: (ny, nx), like the fields, a stored undef excludes a
    cell (fdef_mask: its flag); box: (i0, i1, j0, j1), half-open.  mode "area": one histogram per field and level, "rows":
    one per grid row of the box.  Returns the int32 counts (nf, nlev, nrows, nedges + 2) where the fields live -- slots
    0..nedges the bins, slot nedges + 1 the NaN count --; with ONE (nlev, ny, nx) batch for `fields` the leading axis is
    dropped.  The launch shape is in last_hdist_form().  A refused call raises Refused (a ValueError) with the reason."""
    code = HSTATS_MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
    one, batches, fa, shape = _level_batches(fields)
    nlev, ny, nx = shape
    nf = len(fa)
    e = _edges(edges, nf)
    ma, bx, box_rows = _area(fa, mask, box, shape)
    nrows = 1 if code == 0 else max(box_rows, 0)
    hist, addr = _int_output(batches[0], (nf, nlev, nrows, e.shape[1] + 2))
    table = _pointer_table([a.addr for a in fa])
    try:
        ctx._launch("mifc_hdist_histogram_levels", fa + [ma], [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, e,
                                                                 int(e.shape[1]), ma.addr, int(fdef_mask), bx, code, addr, float(undef)])
    except RuntimeError as err:
        raise Refused(str(err)) from None
    return hist[0] if one else hist


def quantile_levels(ctx, fields, percentiles, method="linear", mask=None, box=None, fdefined_in=None, fdef_mask=SOME_DEFINED, undef=UNDEF, out=None):
    """EXTENSION (include/mifc.h, mifc_hdist_quantile_levels): exact percentiles of the included cells of every (field,
    level), by the order and the rank rules of ensembleQuantiles -- IEEE total order, -0 < +0, NaN above +inf; "lower":
    x[(int)(n * p / 100)] in float, clamped; "linear": numpy's default, in double.  percentiles: 1..16 values in [0, 100].
    mask, box, fdefined_in: as histogram_levels takes them.  Returns (quant, flags) where the fields live: quant float32
    (nf, nlev, nq), undef where no cell is included -- quant[f].reshape(nlev, 1, nq) is a level batch --, flags int32
    (nf, nlev), ALL_DEFINED or NONE_DEFINED; with ONE (nlev, ny, nx) batch for `fields` the leading axis is dropped from
    both.  A refused call raises Refused (a ValueError) with the library's reason."""
    code = QUANTILE_METHODS.get(method, -1) if isinstance(method, str) else int(method)
    one, batches, fa, shape = _level_batches(fields)
    nlev, ny, nx = shape
    nf = len(fa)
    p = np.ascontiguousarray(np.asarray(percentiles, dtype=np.float32).ravel())
    if not 1 <= p.size <= MAX_PERCENTILES:
        raise ValueError("percentiles must hold 1..%d values" % MAX_PERCENTILES)
    ma, bx, _ = _area(fa, mask, box, shape)
    lead = () if one else (nf,)
    res, oa = _output(out, batches[0], lead + (nlev, int(p.size)))
    fd = np.zeros(lead + (nlev,), np.int32)
    table = _pointer_table([a.addr for a in fa])
    try:
        ctx._launch("mifc_hdist_quantile_levels", fa + [ma, oa], [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, p,
                                                                    int(p.size), code, ma.addr, int(fdef_mask), bx, oa.addr, fd, float(undef)])
    except RuntimeError as err:
        raise Refused(str(err)) from None
    return res, fd


def last_hdist_form(ctx):
    """The launch shape of this thread's last histogram_levels / quantile_levels call as a dict (mifc_last_hdist_form; a
    diagnostic for tests): entry and mode as strings, the other keys as ints."""
    return _parse_form(ctx._lib.mifc_last_hdist_form(), ("entry", "mode"))
