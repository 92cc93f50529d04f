"""Level batches regridded by a sparse weight table (include/mifc.h, mifc_hremap_*; EXTENSION): conservative remapping,
region averages and any other linear horizontal operator that a regridding tool delivers as (destination, source, weight)
triples.  Free functions that take a Context, built from the helpers of _args and Context._launch like the functions of
pvort.

    from mi_fieldcalc_amd import hremap
    rowptr, col, w = hremap.conservative_weights_regular(src_xedges, src_yedges, dst_xedges, dst_yedges)
    with hremap.Plan(ctx, rowptr, col, w, nsrc=ny * nx) as plan:          # once per grid pair
        coarse, flags = hremap.hremap_levels(ctx, plan, precip, dst_shape=(ny2, nx2))   # every time step
    plan = hremap.Plan.from_coo(ctx, row, col, S, nsrc, ndst, one_based=True)           # ESMF weight files as they are

Fields are numpy arrays (host memory) or CUDA tensors (device); the result lives where the fields live."""
import ctypes
import weakref

import numpy as np

from ._args import _field_tables, _is_torch, _level_batches, _level_flags, _output, _parse_form
from ._consts import MEM_DEVICE, MEM_HOST, UNDEF
from .vcumul import Refused

__all__ = ["Refused", "Plan", "hremap_levels", "last_hremap_form", "conservative_weights_regular", "HREMAP_MODES"]

# the modes of mifc_hremap_levels (MIFC_HREMAP_*)
HREMAP_MODES = {"strict": 0, "renorm": 1}


def _table(x, dtype, what):
    """One array of a weight table: (address or numpy array, keep-alive, on the device?, length)."""
    if _is_torch(x):
        import torch

        want = torch.int32 if dtype == np.int32 else torch.float32
        if x.dtype != want or not x.is_cuda or not x.is_contiguous() or x.dim() != 1:
            raise ValueError("%s on the device must be a contiguous 1-D %s CUDA tensor" % (what, want))
        return x.data_ptr(), x, True, int(x.shape[0])
    a = np.ascontiguousarray(np.asarray(x).ravel(), dtype=dtype)
    return a, a, False, int(a.size)


class Plan:
    """A weight table on the device (mifc_hremap_plan): ndst rows over nsrc source cells in CSR form -- rowptr int32
    (ndst + 1,), col int32 (nnz,) the flat source index j * nx + i, w float32 (nnz,) --, all three numpy arrays (host
    memory) or all three CUDA tensors.  The library validates and copies the table: the arrays may be freed or overwritten
    afterwards.  The entries of a row are summed in the given order.  close() destroys the handle, once; a Plan is a context
    manager.  A plan belongs to its Context, which closes the plans it still has when it is closed itself: a plan closed
    or collected after its context no longer calls the library.  A refused table raises Refused with the library's
    reason."""

    def __init__(self, ctx, rowptr, col, w, nsrc, ndst=None):
        tabs = [_table(rowptr, np.int32, "rowptr"), _table(col, np.int32, "col"), _table(w, np.float32, "w")]
        if len({t[2] for t in tabs}) != 1:
            raise ValueError("rowptr, col and w must be all numpy arrays (host) or all CUDA tensors (device)")
        if tabs[1][3] != tabs[2][3]:
            raise ValueError("col and w must have the same length")
        self.nsrc, self.ndst = int(nsrc), int(tabs[0][3] - 1 if ndst is None else ndst)
        if tabs[0][3] != self.ndst + 1:
            raise ValueError("rowptr must hold ndst + 1 values")
        mk = MEM_DEVICE if tabs[0][2] else MEM_HOST
        self._ctx, self._handle = ctx, None
        ctx._bind_stream(mk)
        try:
            handle = ctx._call("mifc_hremap_plan_create", [self.nsrc, self.ndst, tabs[0][0], tabs[1][0], tabs[2][0], mk])
        except RuntimeError as e:
            raise Refused(str(e)) from None
        if not handle:
            raise Refused("mifc_hremap_plan_create: " + ctx.last_error())
        self._handle = handle
        ctx.__dict__.setdefault("_plans", []).append(weakref.ref(self))  # Context.close() closes what is left

    @classmethod
    def from_coo(cls, ctx, rows, cols, w, nsrc, ndst, one_based=False):
        """A plan from (destination, source, weight) triples in any order, the ESMF / SCRIP `row`, `col`, `S` of a weight
        file as they are (one_based=True).  The triples are sorted by row with a stable sort: the entries of a row keep
        their order."""
        rowptr, c, s = coo_to_csr(rows, cols, w, ndst, one_based)
        return cls(ctx, rowptr, c, s, nsrc, ndst)

    @property
    def handle(self):
        if self._handle is None:
            raise ValueError("the plan is closed")
        return self._handle

    def info(self):
        """{"nnz", "max_row", "empty_rows"} of the table (mifc_hremap_plan_info)."""
        nnz, longest, empty = ctypes.c_longlong(0), ctypes.c_int(0), ctypes.c_int(0)
        self._ctx._lib.mifc_hremap_plan_info(self.handle, ctypes.addressof(nnz), ctypes.addressof(longest), ctypes.addressof(empty))
        return {"nnz": int(nnz.value), "max_row": int(longest.value), "empty_rows": int(empty.value)}

    def close(self):
        if self._handle is not None:
            handle, self._handle = self._handle, None
            plans = self._ctx.__dict__.get("_plans")
            if plans:
                plans[:] = [r for r in plans if r() is not None and r() is not self]
            if getattr(self._ctx, "_ctx", None):  # (a closed context took the plan with it: its mifc_ctx is gone)
                self._ctx._lib.mifc_hremap_plan_destroy(handle)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (the interpreter is shutting down)
            pass


def coo_to_csr(rows, cols, w, ndst, one_based=False):
    """(rowptr, col, w) of triples in any order: a stable sort by row."""
    r = np.asarray(rows).astype(np.int64).ravel()
    c = np.asarray(cols).astype(np.int64).ravel()
    s = np.asarray(w, dtype=np.float32).ravel()
    if not (r.size == c.size == s.size):
        raise ValueError("rows, cols and w must have the same length")
    if one_based:
        r, c = r - 1, c - 1
    if r.size and (r.min() < 0 or r.max() >= ndst):
        raise ValueError("a row outside [0, ndst)")
    order = np.argsort(r, kind="stable")
    rowptr = np.zeros(int(ndst) + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=int(ndst)), out=rowptr[1:])
    if r.size and (np.abs(c).max() > 2**31 - 1 or rowptr[-1] > 2**31 - 1):
        raise ValueError("the table does not fit int32")
    return rowptr.astype(np.int32), c[order].astype(np.int32), s[order]


def hremap_levels(ctx, plan, fields, mode="strict", min_frac=0.0, fdefined_in=None, out=None, undef=UNDEF, dst_shape=None):
    """EXTENSION (include/mifc.h, mifc_hremap_levels): the plan's weight table applied to every level of the fields.  Per
    destination the entries of its row are summed in double in the table's order; "strict": a destination with an
    undefined source value (or an empty row) is undef; "renorm": the sum over the defined entries is rescaled by
    Wall / Wdef where |Wdef| >= min_frac * |Wall| (for non-negative weights), undef otherwise.  fields, fdefined_in: as
    hinterp_levels takes them, (nlev, ny, nx) batches with ny * nx the plan's nsrc.  Returns (res, flags) where the fields
    live: res (nf, nlev, ndst) -- (nf, nlev) + dst_shape when a shape is given, itself a level batch --, flags int32
    (nf, nlev); with ONE (nlev, ny, nx) batch for `fields` the leading axis is dropped from both.  The launch shape is in
    last_hremap_form().  A refused call raises Refused (a ValueError) with the library's reason."""
    code = HREMAP_MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
    one, batches, fa, shape = _level_batches(fields)
    nlev, ny, nx = shape
    nf = len(fa)
    ndst = plan.ndst
    where = (ndst,) if dst_shape is None else tuple(int(n) for n in dst_shape)
    if int(np.prod(where, dtype=np.int64)) != ndst:
        raise ValueError("dst_shape %s does not hold the plan's %d destinations" % (where, ndst))
    lead = () if one else (nf,)
    res, oa = _output(out, batches[0], lead + (nlev,) + where)
    table, outs = _field_tables(fa, oa, nlev * ndst * 4)
    fd = np.zeros(lead + (nlev,), np.int32)
    try:
        ctx._launch("mifc_hremap_levels", fa + [oa], [plan.handle, nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, code,
                                                      float(min_frac), ctypes.addressof(outs), fd, float(undef)])
    except RuntimeError as e:
        raise Refused(str(e)) from None
    return res, fd


def last_hremap_form(ctx):
    """The launch shape of this thread's last hremap_levels call as a dict (mifc_last_hremap_form; a diagnostic for
    tests): mode as a string, the other keys as ints."""
    return _parse_form(ctx._lib.mifc_last_hremap_form(), ("mode",))


def _overlap_1d(src_edges, dst_edges):
    """Per destination interval the source intervals it overlaps: (destination, source, overlap length) triples, ordered by
    destination, then source."""
    s, d = np.asarray(src_edges, np.float64), np.asarray(dst_edges, np.float64)
    if s.ndim != 1 or d.ndim != 1 or s.size < 2 or d.size < 2 or not (np.all(np.diff(s) > 0) and np.all(np.diff(d) > 0)):
        raise ValueError("cell edges must be 1-D, ascending, at least two")
    lo = np.maximum(d[:-1, None], s[None, :-1])
    hi = np.minimum(d[1:, None], s[None, 1:])
    di, si = np.nonzero(hi > lo)
    return di, si, (hi - lo)[di, si]


def conservative_weights_regular(src_xedges, src_yedges, dst_xedges, dst_yedges):
    """First-order conservative weights between two rectilinear grids given by their cell edges (ascending; nx + 1 and
    ny + 1 values): the weight of a source cell in a destination cell is their overlap in x times their overlap in y,
    over the destination cell's area.  Destination parts outside the source count as missing area: such a row sums to
    the covered fraction, a destination outside the source has an empty row.  Entries are ordered by ascending source
    index j * nx + i.  Returns (rowptr int32 (ndst + 1,), col int32, w float32) for Plan, destinations in row-major
    order of the destination grid.  A latitude axis is weighted by passing sin(lat) edges.  numpy only."""
    dxi, sxi, lx = _overlap_1d(src_xedges, dst_xedges)
    dyi, syi, ly = _overlap_1d(src_yedges, dst_yedges)
    nx_s = len(src_xedges) - 1
    nx_d, ny_d = len(dst_xedges) - 1, len(dst_yedges) - 1
    dx, dy = np.diff(np.asarray(dst_xedges, np.float64)), np.diff(np.asarray(dst_yedges, np.float64))
    # every y pair with every x pair; y outer, x inner: ascending (destination, source) in both flat indices
    d = (dyi[:, None] * nx_d + dxi[None, :]).ravel()
    c = (syi[:, None] * nx_s + sxi[None, :]).ravel()
    w = ((ly[:, None] * lx[None, :]) / (dy[dyi][:, None] * dx[dxi][None, :])).ravel()
    order = np.lexsort((c, d))
    rowptr = np.zeros(nx_d * ny_d + 1, np.int64)
    np.cumsum(np.bincount(d, minlength=nx_d * ny_d), out=rowptr[1:])
    return rowptr.astype(np.int32), c[order].astype(np.int32), w[order].astype(np.float32)
