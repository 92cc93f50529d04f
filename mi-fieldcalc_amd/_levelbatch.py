"""The EXTENSION entries that take whole level batches (include/mifc.h): ensemble statistics and percentiles, vertical
interpolation, layer products and derivatives, sampling, rotation, horizontal statistics, and the batched neighbourhood
and icing functions.  Each method is what differs between them; the mechanics are in _args and Context._launch."""
import ctypes

import numpy as np

from . import _capi
from ._args import (_Arg, _coord_flags, _drop_one, _empty_like, _field_tables, _flag_table, _hybrid_levels, _is_torch, _kept, _level_batches,
                    _level_coord, _level_flags, _member_batch, _output, _pairs, _pointer_table, _same_shape, _stacked_table)
from ._consts import (ALL_DEFINED, ENS_EXTREME, ENS_MEAN, ENS_PROBABILITY, ENS_STDDEV, ENS_SUM, HINTERP_METHODS, HSTATS_MODES, HSTATS_PRODUCTS,
                      SOME_DEFINED, UNDEF, VDERIV_METHODS, VLAYER_PRODUCTS)

_ENS_EXTREMES = {"max": 1, "min": 2, "argmax": 3, "argmin": 4}
_ENS_MAX_PROBABILITIES = 8


def ensemble_products(products):
    """The product specs of Context.ensembleStatistics as a list of (stat, compute, limits, flag_in) tuples, validated
    the way mifc_ensemble_levels validates its list (a bad list raises ValueError here, before anything is allocated).
    A spec is "mean", "stddev", "sum", "max", "min", "argmax", "argmin" (a bare name or a 1-tuple), ("sum", flag_in),
    ("max", flag_in) ... with flag_in one ValuesDefined flag or one per level (default SOME_DEFINED), ("extreme", compute,
    flag_in), or ("probability", compute, limits) with the reference's compute 1..6 and one or two limits.  flag_in is
    None where the statistic has no input flag of its own."""
    out, seen, nprob = [], set(), 0
    for spec in products:
        try:
            spec = (spec,) if isinstance(spec, str) else tuple(spec)
        except TypeError:
            spec = ()
        if not spec or not isinstance(spec[0], str):
            raise ValueError("a product is a name or a tuple that starts with one: %r" % (spec,))
        name, rest = spec[0].lower(), spec[1:]
        if name in ("mean", "stddev"):
            if rest:
                raise ValueError("%r takes no arguments (the member flags are fdefined_in)" % name)
            item = (ENS_MEAN if name == "mean" else ENS_STDDEV, 0, (), None)
            key = name
        elif name == "sum" or name in _ENS_EXTREMES or name == "extreme":
            if name == "extreme":
                if not rest:
                    raise ValueError('("extreme", compute[, flag_in])')
                compute, rest = int(rest[0]), rest[1:]
                if compute not in (1, 2, 3, 4):
                    raise ValueError("extreme: compute %d outside 1..4" % compute)
            else:
                compute = _ENS_EXTREMES.get(name, 0)
            if len(rest) > 1:
                raise ValueError("%r takes one argument, the input flag" % name)
            item = (ENS_SUM if name == "sum" else ENS_EXTREME, compute, (), rest[0] if rest else SOME_DEFINED)
            key = "sum" if name == "sum" else ("extreme", compute)
        elif name == "probability":
            if len(rest) != 2:
                raise ValueError('("probability", compute, limits)')
            compute = int(rest[0])
            limits = tuple(float(x) for x in np.atleast_1d(np.asarray(rest[1], dtype=np.float32)))
            if compute not in (1, 2, 3, 4, 5, 6):
                raise ValueError("probability: compute %d outside 1..6" % compute)
            if len(limits) not in (1, 2):
                raise ValueError("probability: one or two limits, not %d" % len(limits))
            if compute in (3, 6) and len(limits) == 1:
                raise ValueError("probability: between (compute %d) needs two limits" % compute)
            nprob += 1
            if nprob > _ENS_MAX_PROBABILITIES:
                raise ValueError("more than %d probability products" % _ENS_MAX_PROBABILITIES)
            item = (ENS_PROBABILITY, compute, limits, None)
            key = None
        else:
            raise ValueError("unknown statistic %r" % (spec[0],))
        if key is not None:
            if key in seen:
                raise ValueError("%r is in the list twice" % (spec[0],))
            seen.add(key)
        out.append(item)
    if not out:
        raise ValueError("no products")
    return out


class HstatsResult:
    """What Context.hstats_levels returns: `stats`, the raw float64 array (nf, nlev, nrows, 8) of mifc_hstats_levels -- a
    numpy array for host fields, a CUDA tensor for device fields, the leading axis dropped for ONE batch -- with the named
    views n, w, s1, s2, min, max, imin, imax (the slots of a product group that was not requested hold NaN), `pivot`
    (float64, shaped like a view without the row axis, or None), and, when the call asked for them, the float32 batch
    `mean_batch` (nf, nlev, nrows) and its flags `mean_flags` int32 (nf, nlev).  mean(), variance() and rms() are computed
    in float64 on the host from stats."""

    _SLOTS = ("n", "w", "s1", "s2", "min", "max", "imin", "imax")

    def __init__(self, stats, pivot, mean_batch, mean_flags):
        self.stats, self.pivot, self.mean_batch, self.mean_flags = stats, pivot, mean_batch, mean_flags

    def __getattr__(self, name):
        if name in HstatsResult._SLOTS:
            return self.stats[..., HstatsResult._SLOTS.index(name)]
        raise AttributeError(name)

    def _host(self, slot):
        v = self.stats[..., slot]
        return v.cpu().numpy() if _is_torch(v) else np.asarray(v)

    def mean(self):
        """pivot + S1 / W, float64 (NaN where W is 0)."""
        p = 0.0 if self.pivot is None else np.asarray(self.pivot, np.float64)[..., None]
        with np.errstate(all="ignore"):
            return p + self._host(2) / self._host(1)

    def variance(self):
        """S2 / W - (S1 / W)^2, about the mean whatever the pivot; float64."""
        with np.errstate(all="ignore"):
            m = self._host(2) / self._host(1)
            return self._host(3) / self._host(1) - m * m

    def rms(self):
        """sqrt(S2 / W): with `minus` and no pivot the RMSE of x - y; float64."""
        with np.errstate(all="ignore"):
            return np.sqrt(self._host(3) / self._host(1))


class _LevelBatchOps:
    """Mixin of Context: the level-batch extension methods.  A refused call raises RuntimeError with the reason, except in
    neighbour_levels and vesselIcing_levels, which return None like the reference functions they batch."""

    # ------------------------------------------------------ statistics over ensemble members (EXTENSION)
    def ensembleQuantiles(self, fields, percentiles, fdefined_in=None, method="lower", undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_ensembleQuantiles): per-cell percentiles across ensemble members.
        fields: a sequence of members, each (ny, nx) or (nlev, ny, nx), or one stacked array / tensor whose axis 0 is the
        members (numpy: host memory, CUDA tensors: device).  percentiles: one value or a sequence in [0, 100].
        fdefined_in: member flags, (nmem,) or (nmem, nlev); None: SOME_DEFINED.  method: "lower" (the reference's
        neighbourFunctions rule) or "linear" (numpy's default).  out: (nq,) + the member shape, may be the members
        themselves.  Returns (out, fdefined): an int for 2-D members, an int32 array of nlev flags otherwise.  A refused
        call raises RuntimeError with the reason."""
        code = {"lower": 0, "linear": 1}.get(method, -1) if isinstance(method, str) else int(method)
        pct = np.ascontiguousarray(np.asarray(percentiles, dtype=np.float32).ravel())
        nq = int(pct.size)
        fallback = None if out is None else tuple(_Arg(out, output=True).shape)[1:]
        members, fa, shape, nlev, ny, nx, table, flags = _member_batch(fields, fdefined_in, fallback)
        res, oa = _output(out, members[0] if members else None, (nq,) + shape)
        outs = _stacked_table(oa.addr, nq, nlev * ny * nx * 4, 1)
        fd = np.zeros(nlev, np.int32)
        self._launch("mifc_ensembleQuantiles", fa + [oa],
                     [code, nx, ny, nlev, ctypes.addressof(table), flags, len(fa), pct, nq, ctypes.addressof(outs), fd, float(undef)])
        return res, (int(fd[0]) if len(shape) == 2 else fd)

    def ensembleStatistics(self, fields, products, fdefined_in=None, undef=UNDEF, out=None):
        """mifc_ensemble_levels (include/mifc.h): several of sumFields, meanValue, stddevValue, extremeValue and probability
        over the same members in one pass, each bit for bit what its single-field function returns per level.
        fields: as ensembleQuantiles takes them.  products: see ensemble_products().  fdefined_in: member flags, (nmem,)
        or (nmem, nlev); None: SOME_DEFINED.  out: one array or tensor of shape (len(products),) + the member shape, or a
        sequence of one per product.  Returns a list of (array, flags) in product order: flags an int for 2-D members,
        an int32 array of nlev flags otherwise.  A refused call raises RuntimeError with the reason."""
        specs = ensemble_products(products)
        if out is not None and (isinstance(out, np.ndarray) or _is_torch(out)):
            out = [out[k] for k in range(out.shape[0])]
        if out is not None and len(out) != len(specs):
            raise ValueError("out must hold one array per product")
        fallback = None if out is None else tuple(_Arg(out[0], output=True).shape)
        members, fa, shape, nlev, ny, nx, table, flags = _member_batch(fields, fdefined_in, fallback)
        if out is None:
            out = [_empty_like(members[0], shape) for _ in specs]
        oa = [_Arg(o, output=True) for o in out]
        if not _same_shape(oa, shape):
            raise ValueError("every output must have the shape %s" % (shape,))
        fds = []
        prods = (_capi.EnsProduct * len(specs))()
        for k, (stat, compute, limits, flag_in) in enumerate(specs):
            fd = _flag_table(None, nlev)
            if flag_in is not None:
                fd[:] = np.asarray(flag_in, dtype=np.int32).reshape(-1) if np.ndim(flag_in) else int(flag_in)
            fds.append(fd)
            prods[k].stat, prods[k].compute, prods[k].nlimits = stat, compute, len(limits)
            for i, v in enumerate(limits):
                prods[k].limits[i] = v
            prods[k].out, prods[k].fdefined = oa[k].addr, fd.ctypes.data
        self._launch("mifc_ensemble_levels", fa + oa,
                     [nx, ny, nlev, ctypes.addressof(table), flags, len(fa), ctypes.addressof(prods), len(specs), float(undef)])
        return [(_kept(o, a), (int(fd[0]) if len(shape) == 2 else fd)) for o, a, fd in zip(out, oa, fds)]

    # ------------------------------------------------------ level batches to constant surfaces (EXTENSION)
    def _vinterp(self, name, fields, coord, coord_args, targets, method, fdefined_in, undef, out):
        code = {"linear": 0, "log": 1}.get(method, -1) if isinstance(method, str) else int(method)
        one, batches, fa, shape = _level_batches(fields)
        nlev, ny, nx = shape
        ca = _level_coord(coord, name == "mifc_vinterp_hlevels", shape)
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.float32).ravel())
        nt, nf = int(tg.size), len(fa)
        res, oa = _output(out, batches[0], (nt, ny, nx) if one else (nf, nt, ny, nx))
        table, outs = _field_tables(fa, oa, nt * ny * nx * 4)
        fd = np.zeros((nf, nt), np.int32)
        self._launch(name, fa + [ca, oa], [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, ca.addr] + coord_args
                     + [tg, nt, code, ctypes.addressof(outs), fd, float(undef)])
        return _drop_one(one, res, fd)

    def vinterp_hlevels(self, fields, ps, alevel, blevel, targets, method="linear", fdefined_in=None, fdef_ps=SOME_DEFINED, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_vinterp_hlevels): hybrid-level batches interpolated to the surfaces where the
        coordinate alevel[k] + blevel[k] * ps takes the values `targets` (pressure surfaces, say), linearly in the
        coordinate ("linear") or in its logarithm ("log").  fields: a list of (nlev, ny, nx) numpy arrays (host memory)
        or CUDA tensors (device), or one stacked (nf, nlev, ny, nx); ps: (ny, nx); fdefined_in: flags (nf, nlev), or one
        per field; None: SOME_DEFINED.  Returns (out (nf, ntargets, ny, nx), flags int32 (nf, ntargets)); with ONE
        (nlev, ny, nx) batch for `fields` the leading axis is dropped from both.  A refused call raises RuntimeError."""
        al, bl = _hybrid_levels(fields, alevel, blevel)
        return self._vinterp("mifc_vinterp_hlevels", fields, ps, [int(fdef_ps), al, bl], targets, method, fdefined_in, undef, out)

    def vinterp_fields(self, fields, coord, targets, method="linear", fdefined_in=None, fdef_coord=None, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_vinterp_fields): as vinterp_hlevels, the coordinate given as a batch
        (nlev, ny, nx) like the fields (pressure on other level types, height, potential temperature ...);
        fdef_coord: one flag per level, None: SOME_DEFINED."""
        fc_ = _coord_flags(fdef_coord, coord)
        return self._vinterp("mifc_vinterp_fields", fields, coord, [fc_], targets, method, fdefined_in, undef, out)

    # ------------------------------------------ layer integrals, means and extremes of level batches (EXTENSION)
    def _vlayer(self, name, fields, coord, coord_args, products, lo, hi, fdefined_in, undef, out):
        codes = [VLAYER_PRODUCTS.get(p, -1) if isinstance(p, str) else int(p) for p in ([products] if isinstance(products, (str, int)) else products)]
        one, batches, fa, shape = _level_batches(fields)
        nlev, ny, nx = shape
        ca = _level_coord(coord, name == "mifc_vlayer_hlevels", shape)
        bounds, scalars, ptrs = [], [], []
        for b in (lo, hi):  # a number, or a (ny, nx) field of per-cell bounds
            if (isinstance(b, np.ndarray) and b.ndim > 0) or _is_torch(b):
                ba = _Arg(b)
                if tuple(ba.shape) != (ny, nx):
                    raise ValueError("a bound given as a field must have the shape %s" % ((ny, nx),))
                bounds.append(ba)
                scalars.append(0.0)
                ptrs.append(ba.addr)
            else:
                scalars.append(float(b))
                ptrs.append(None)
        np_, nf = len(codes), len(fa)
        res, oa = _output(out, batches[0], (np_, ny, nx) if one else (nf, np_, ny, nx))
        table, outs = _field_tables(fa, oa, np_ * ny * nx * 4)
        pc = np.ascontiguousarray(codes, dtype=np.int32)
        fd = np.zeros((nf, np_), np.int32)
        self._launch(name, fa + [ca, oa] + bounds, [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, ca.addr] + coord_args
                     + scalars + ptrs + [pc, np_, ctypes.addressof(outs), fd, float(undef)])
        return _drop_one(one, res, fd)

    def vlayer_hlevels(self, fields, ps, alevel, blevel, products, lo=-np.inf, hi=np.inf, fdefined_in=None, fdef_ps=SOME_DEFINED, undef=UNDEF,
                       out=None):
        """EXTENSION (include/mifc.h, mifc_vlayer_hlevels): integrals, means and extremes of hybrid-level batches over
        the layer lo <= c <= hi of the coordinate c = alevel[k] + blevel[k] * ps, in one pass over the levels.
        fields, ps, fdefined_in: as vinterp_hlevels takes them.  products: names ("integral", "mean", "max", "min",
        "coord_of_max", "coord_of_min") or MIFC_VLAYER_* codes, each at most once.  lo, hi: a number (+-inf: open) or a
        (ny, nx) array / tensor of per-cell bounds.  Returns (out (nf, nproducts, ny, nx), flags int32
        (nf, nproducts)); with ONE (nlev, ny, nx) batch for `fields` the leading axis is dropped from both.  A refused
        call raises RuntimeError."""
        al, bl = _hybrid_levels(fields, alevel, blevel)
        return self._vlayer("mifc_vlayer_hlevels", fields, ps, [int(fdef_ps), al, bl], products, lo, hi, fdefined_in, undef, out)

    def vlayer_fields(self, fields, coord, products, lo=-np.inf, hi=np.inf, fdefined_in=None, fdef_coord=None, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_vlayer_fields): as vlayer_hlevels, the coordinate given as a batch
        (nlev, ny, nx) like the fields; fdef_coord: one flag per level, None: SOME_DEFINED."""
        fc_ = _coord_flags(fdef_coord, coord)
        return self._vlayer("mifc_vlayer_fields", fields, coord, [fc_], products, lo, hi, fdefined_in, undef, out)

    # ------------------------------------------ vertical derivatives of level batches, vector magnitude (EXTENSION)
    def _vderiv(self, name, fields, coord, coord_args, method, magnitude, fdefined_in, undef, out):
        code = VDERIV_METHODS.get(method, -1) if isinstance(method, str) else int(method)
        if magnitude not in (None, "also", "only"):
            raise ValueError('magnitude must be None, "also" or "only"')
        one, batches, fa, shape = _level_batches(fields)
        nlev, ny, nx = shape
        nf = len(fa)
        nm = nf // 2
        others = []
        if name == "mifc_vderiv_levels":
            lv = np.ascontiguousarray(np.asarray(coord, dtype=np.float32).ravel())
            if lv.size != nlev:
                raise ValueError("levels must hold one value per level")
            coord_arg = lv
        else:
            ca = _level_coord(coord, name == "mifc_vderiv_hlevels", shape)
            coord_arg = ca.addr
            others.append(ca)
        want_out, want_mag = magnitude != "only", magnitude is not None
        given = list(out) if isinstance(out, (tuple, list)) else [out]
        if want_out and want_mag and len(given) == 1:
            given = [given[0], None]
        if len(given) != (2 if want_out and want_mag else 1):
            raise ValueError('out must be one array or tensor, or (out, mag) with magnitude="also"')
        shapes = ([shape if one else (nf,) + shape] if want_out else []) + ([(nm,) + shape] if want_mag else [])
        res = [_output(o, batches[0], s) for o, s in zip(given, shapes)]  # (what to hand back, its _Arg): the derivative, the magnitude
        batch_bytes = nlev * ny * nx * 4
        table = _pointer_table([a.addr for a in fa])
        outs = mags = fd = mfd = None
        if want_out:
            outs = _stacked_table(res[0][1].addr, nf, batch_bytes)
            fd = np.zeros((nf, nlev), np.int32)
        if want_mag:
            mags = _stacked_table(res[-1][1].addr, nm, batch_bytes, 1)
            mfd = np.zeros((nm, nlev), np.int32)
        self._launch(name, fa + others + [oa for _, oa in res],
                     [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, coord_arg] + coord_args
                     + [code, ctypes.addressof(outs) if want_out else None, fd, ctypes.addressof(mags) if want_mag else None, mfd, float(undef)])
        return (_drop_one(one, res[0][0], fd) if want_out else ()) + ((res[-1][0], mfd) if want_mag else ())

    def vderiv_hlevels(self, fields, ps, alevel, blevel, method="centred", magnitude=None, fdefined_in=None, fdef_ps=SOME_DEFINED, undef=UNDEF,
                       out=None):
        """EXTENSION (include/mifc.h, mifc_vderiv_hlevels): the derivative of hybrid-level batches along the coordinate
        c = alevel[k] + blevel[k] * ps, one value per input level: centred differences ("centred") or the second-order
        form for uneven spacing ("weighted"), one-sided at the ends and next to holes.  fields, ps, fdefined_in: as
        vinterp_hlevels takes them.  magnitude: None returns (out (nf, nlev, ny, nx), flags int32 (nf, nlev)); "also"
        returns (out, flags, mag (nf / 2, nlev, ny, nx), mag_flags (nf / 2, nlev)), mag[j] the magnitude of the derivatives
        of the fields 2j and 2j + 1; "only" returns (mag, mag_flags) and writes no derivative.  With ONE (nlev, ny, nx)
        batch for `fields` the leading axis is dropped from out and flags.  out: an array or tensor to write into (with
        "also": (out, mag)).  A refused call raises RuntimeError."""
        al, bl = _hybrid_levels(fields, alevel, blevel)
        return self._vderiv("mifc_vderiv_hlevels", fields, ps, [int(fdef_ps), al, bl], method, magnitude, fdefined_in, undef, out)

    def vderiv_fields(self, fields, coord, method="centred", magnitude=None, fdefined_in=None, fdef_coord=None, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_vderiv_fields): as vderiv_hlevels, the coordinate given as a batch
        (nlev, ny, nx) like the fields (height, pressure, potential temperature ...); fdef_coord: one flag per level,
        None: SOME_DEFINED."""
        fc_ = _coord_flags(fdef_coord, coord)
        return self._vderiv("mifc_vderiv_fields", fields, coord, [fc_], method, magnitude, fdefined_in, undef, out)

    def vderiv_levels(self, fields, levels, method="centred", magnitude=None, fdefined_in=None, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_vderiv_levels): as vderiv_hlevels, the coordinate one constant per level
        (pressure levels, the targets of an earlier vinterp call): `levels` holds nlev numbers."""
        return self._vderiv("mifc_vderiv_levels", fields, levels, [], method, magnitude, fdefined_in, undef, out)

    # ------------------------------------------ level batches sampled at arbitrary points (EXTENSION)
    def _hinterp(self, name, sources, points, message, rotation, method, fdefined_in, undef, out):
        """hinterp_levels and hinterp_vector_levels.  sources: what _level_batches or _pairs made of the fields; points: xpos,
        ypos and whatever else holds one value per position; rotation: the scalars that follow them in a pair call."""
        code = HINTERP_METHODS.get(method, -1) if isinstance(method, str) else int(method)
        one, batches, fa, shape = sources
        nlev, ny, nx = shape
        nf = len(fa)
        count, lead = (nf, (nf,)) if rotation is None else (nf // 2, (nf // 2, 2))  # the fields, or their pairs
        pa = [_Arg(p) for p in points]
        where = tuple(pa[0].shape)
        if not _same_shape(pa[1:], where):
            raise ValueError(message)
        npos = int(np.prod(where, dtype=np.int64))
        res, oa = _output(out, batches[0], (lead[1:] if one else lead) + (nlev,) + where)
        table, outs = _field_tables(fa, oa, nlev * npos * 4)
        fd = np.zeros(lead + (nlev,), np.int32)
        self._launch(name, fa + pa + [oa], [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), count, npos]
                     + [p.addr for p in pa] + (rotation or []) + [code, ctypes.addressof(outs), fd, float(undef)])
        return _drop_one(one, res, fd)

    def hinterp_levels(self, fields, xpos, ypos, method="bilinear", fdefined_in=None, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_hinterp_levels): level batches sampled at arbitrary positions -- a section line,
        stations, the grid of another projection -- by "nearest", "bilinear" or "bicubic" (Catmull-Rom, bilinear next to
        holes and in the outer ring of cells) interpolation, or a MIFC_HINTERP_* code.  fields, fdefined_in: as
        vderiv_fields takes them.  xpos, ypos: numpy arrays (host memory) or CUDA tensors (device), like the fields, of any
        one shape S, in grid-index units (x = 0 is column 0, x = nx - 1 the last column); a position outside the grid, NaN
        or equal to undef gives undef.  Returns (out (nf, nlev) + S, flags int32 (nf, nlev)); with ONE (nlev, ny, nx)
        batch for `fields` the leading axis is dropped from both.  A 2-D S is a regrid; a 1-D S gives (nlev, npos), which
        reshaped to (nlev, 1, npos) is a level batch for vinterp_*, vlayer_* and vderiv_*.  Vector components are not
        rotated: hinterp_vector_levels does that in the same pass.  A refused call raises RuntimeError."""
        return self._hinterp("mifc_hinterp_levels", _level_batches(fields), [xpos, ypos], "xpos and ypos must have the same shape", None, method,
                             fdefined_in, undef, out)

    def hinterp_vector_levels(self, pairs, xpos, ypos, cosa, sina, method="bilinear", fdefined_in=None, fdef_rot=SOME_DEFINED, undef=UNDEF,
                              out=None):
        """EXTENSION (include/mifc.h, mifc_hinterp_vector_levels): hinterp_levels of vector pairs and their rotation by rule R
        in one pass -- wind regridded to another projection, along- and across-section wind.  pairs, fdefined_in, fdef_rot:
        as vrotate_levels takes them; xpos, ypos, method: as hinterp_levels takes them; cosa, sina: one value per position,
        shaped like xpos.  A position with undefined coefficients gives undef like an unusable one.  Returns (out
        (npairs, 2, nlev) + S, flags int32 (npairs, 2, nlev)), bit for bit hinterp_levels followed by vrotate_levels; with
        ONE pair the leading axis is dropped from both.  The launch shape is in last_hinterp_form().  A refused call raises
        RuntimeError."""
        return self._hinterp("mifc_hinterp_vector_levels", _pairs(pairs), [xpos, ypos, cosa, sina], "xpos, ypos, cosa and sina must have the same shape",
                             [int(fdef_rot)], method, fdefined_in, undef, out)

    # ------------------------------------------ vector pairs rotated on the grid (EXTENSION)
    def vrotate_levels(self, pairs, cosa, sina, fdefined_in=None, fdef_rot=SOME_DEFINED, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_vrotate_levels, rule R): vector pairs of level batches rotated cell by cell,
        u' = c u - s v, v' = s u + c v in double, rounded to float once.  pairs: one pair (2, nlev, ny, nx), up to four
        stacked (npairs, 2, nlev, ny, nx), or a sequence of (u, v) batches; numpy arrays (host memory) or CUDA tensors.
        cosa, sina: (ny, nx), like the fields; the library does not normalise them; fdef_rot: their flag.  fdefined_in: one
        flag per component or per component and level, None: SOME_DEFINED.  Returns (out, flags): out shaped like the
        stacked pairs, flags int32 (npairs, 2, nlev) -- the two components of a pair carry the same flag; with ONE pair the
        leading axis is dropped from both.  A refused call raises RuntimeError."""
        one, batches, fa, shape = _pairs(pairs)
        nlev, ny, nx = shape
        nf = len(fa)
        ca, sa = _Arg(cosa), _Arg(sina)
        if tuple(ca.shape) != (ny, nx) or tuple(sa.shape) != (ny, nx):
            raise ValueError("cosa and sina must have the shape %s" % ((ny, nx),))
        res, oa = _output(out, batches[0], ((2,) if one else (nf // 2, 2)) + shape)
        table, outs = _field_tables(fa, oa, nlev * ny * nx * 4)
        fd = np.zeros((nf // 2, 2, nlev), np.int32)
        self._launch("mifc_vrotate_levels", fa + [ca, sa, oa], [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf // 2,
                                                                ca.addr, sa.addr, int(fdef_rot), ctypes.addressof(outs), fd, float(undef)])
        return _drop_one(one, res, fd)

    # ------------------------------------------ horizontal statistics of level batches (EXTENSION)
    def hstats_levels(self, fields, minus=None, pivot=None, weight=None, box=None, mode="area", products=("moments", "extremes"), want_mean=False,
                      fdefined_in=None, fdefined_minus=None, fdef_weight=SOME_DEFINED, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_hstats_levels): area ("area": one result per field and level) or row-wise
        ("rows": one per grid row of the box) statistics of level batches, reproducible bit for bit -- the count N, the sums
        W, S1, S2 of w, w * d and w * d * d (products "moments") and the minimum and maximum of d with the flat index
        j * nx + i of their first cell (products "extremes"), d = (x - y) - pivot in double.  fields, fdefined_in: as
        vderiv_fields takes them.  minus: batches y like the fields (bias, RMSE), with fdefined_minus; pivot: float64, one
        per field and level; weight: (ny, nx), like the fields, a stored undef masks a cell (fdef_weight: its flag);
        box: (i0, i1, j0, j1), half-open.  products: names or a MIFC_HSTATS_* bit mask.  out: a float64 array / tensor
        (nf, nlev, nrows, 8) to write into.  Returns an HstatsResult; want_mean adds the float32 batch of means
        (nf, nlev, nrows) -- reshaped to (nlev, nrows, 1) a level batch for vinterp_* -- and its flags.  With ONE
        (nlev, ny, nx) batch for `fields` the leading axis is dropped everywhere.  A refused call raises RuntimeError."""
        code = HSTATS_MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
        if isinstance(products, str):
            products = (products,)
        mask = int(products) if isinstance(products, (int, np.integer)) else sum({HSTATS_PRODUCTS.get(p, 4) if isinstance(p, str) else int(p) for p in products})
        one, batches, fa, shape = _level_batches(fields)
        nlev, ny, nx = shape
        nf = len(fa)
        ma = []
        if minus is not None:
            _, _, ma, mshape = _level_batches(minus)
            if len(ma) != nf or mshape != shape:
                raise ValueError("minus must hold one batch like the fields per field")
        wa = _Arg(weight, allow_none=True)
        if weight is not None and tuple(wa.shape) != (ny, nx):
            raise ValueError("weight must have the shape %s" % ((ny, nx),))
        bx = None
        if box is not None:
            bx = np.ascontiguousarray(np.asarray(box, dtype=np.int32).ravel())
            if bx.size != 4:
                raise ValueError("box is (i0, i1, j0, j1)")
        nrows = 1 if code == 0 else (int(bx[3] - bx[2]) if bx is not None else ny)
        pv = None
        if pivot is not None:
            pv = np.ascontiguousarray(np.broadcast_to(np.asarray(pivot, dtype=np.float64), (nlev,) if one else (nf, nlev)))
        # the statistics are float64 and pre-filled with NaN: not an output as _output makes them
        device = fa[0].device
        stats_shape = (nf, nlev, max(nrows, 0), 8)
        if out is None:
            if device:
                import torch

                stats = torch.full(stats_shape, float("nan"), dtype=torch.float64, device=batches[0].device)
            else:
                stats = np.full(stats_shape, np.nan, np.float64)
        else:
            stats = out
            ok = (_is_torch(out) and out.is_cuda and out.is_contiguous() and str(out.dtype) == "torch.float64") if device else (
                isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags["C_CONTIGUOUS"])
            if not ok or tuple(out.shape) not in (stats_shape, stats_shape[1:] if one else stats_shape):
                raise ValueError("out must be a contiguous float64 array (host fields) or CUDA tensor (device fields) of shape %s" % (stats_shape,))
        stats_addr = stats.data_ptr() if _is_torch(stats) else stats.ctypes.data
        mean = mean_table = mfd = None
        means = []
        if want_mean:
            mean, ma_out = _output(None, batches[0], (nf, nlev, max(nrows, 0)))
            means = [ma_out]
            mean_table = _stacked_table(ma_out.addr, nf, nlev * nrows * 4)
            mfd = np.zeros((nf, nlev), np.int32)
        table = _pointer_table([a.addr for a in fa])
        mtable = _pointer_table([a.addr for a in ma]) if ma else None
        self._launch("mifc_hstats_levels", fa + ma + [wa] + means, [
            nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, ctypes.addressof(mtable) if ma else None,
            _level_flags(fdefined_minus, nf, nlev) if ma else None, pv, wa.addr, int(fdef_weight), bx, code, mask, stats_addr,
            ctypes.addressof(mean_table) if want_mean else None, mfd, float(undef)])
        if one:
            stats = stats.reshape(stats_shape[1:])
        return HstatsResult(stats, pv, None if mean is None else (mean[0] if one else mean), None if mfd is None else (mfd[0] if one else mfd))

    # ------------------------------------------------------ the neighbourhood and icing functions over a level batch
    def neighbour_levels(self, which, compute, field, constants, fdefined=None, undef=UNDEF, out=None):
        """Either function over a (nlev, ny, nx) batch in one launch.  which: "prob" (neighbourProbFunctions) or
        "functions".  fdefined: per-level flags (default ALL_DEFINED).  Returns (out, flags ndarray) or None."""
        codes = {"prob": 0, "functions": 1}
        if which not in codes:
            raise ValueError("which must be 'prob' or 'functions'")
        fa = _Arg(field)
        if len(fa.shape) != 3:
            raise ValueError("field must have shape (nlev, ny, nx)")
        nlev, ny, nx = fa.shape
        res, oa = _output(out, field, tuple(fa.shape), "out must have the shape of field", fill=undef)  # see _ReferenceOps._neighbour
        flags = _flag_table(fdefined, nlev, ALL_DEFINED)
        consts = np.ascontiguousarray(constants, dtype=np.float32).ravel()
        if not self._launch("mifc_neighbour_levels", [fa, oa], [codes[which], int(compute), nx, ny, nlev, fa.addr, consts.ctypes.data, int(consts.size),
                                                                oa.addr, flags, float(undef)], raises=False):
            return None
        return res, flags

    def vesselIcing_levels(self, model, fields, vs, alpha, zmin, zmax, alt=1, fdefined=None, undef=UNDEF, out=None):
        """Either model over a (nlev, ny, nx) batch (ensemble members, lead times) in one launch.  model: "modstall" or
        "mincog".  fields: the 11 inputs in reference order (sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice,
        depth), each (nlev, ny, nx) or -- shared by every level, bathymetry say -- (ny, nx).  fdefined: per-level flags
        (default SOME_DEFINED).  Returns (out, flags ndarray) or None."""
        codes = {"modstall": 1, "mincog": 2}
        if model not in codes:
            raise ValueError("model must be 'modstall' or 'mincog'")
        fields = list(fields)
        if len(fields) != 11:
            raise ValueError("vesselIcing_levels takes the 11 input fields of the models")
        fa = [_Arg(f) for f in fields]
        per_level = [a for a in fa if len(a.shape) == 3]
        if not per_level:
            raise ValueError("at least one input must be a (nlev, ny, nx) batch")
        shape = tuple(per_level[0].shape)
        nlev, ny, nx = shape
        mask = 0
        for k, a in enumerate(fa):
            if tuple(a.shape) == shape[1:]:
                mask |= 1 << k
            elif tuple(a.shape) != shape:
                raise ValueError("input %d must have shape %s or %s" % (k, shape, shape[1:]))
        res, oa = _output(out, fields[fa.index(per_level[0])], shape, "out must have shape (nlev, ny, nx)")
        flags = _flag_table(fdefined, nlev)
        if not self._launch("mifc_vesselIcing_levels", fa + [oa], [codes[model], nlev, nx, ny] + [a.addr for a in fa]
                            + [mask, float(vs), float(alpha), float(zmin), float(zmax), int(alt), oa.addr, flags, float(undef)], raises=False):
            return None
        return res, flags
