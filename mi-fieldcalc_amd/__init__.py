"""mi_fieldcalc_amd -- MI355X (gfx950) implementation of the mi-fieldcalc hot
path: the elementwise derived-variable operators and the 5-point-stencil
operators of ``miutil::fieldcalc`` (reference: src/mi_fieldcalc/FieldCalculations.h).

This Python layer is plumbing over the C ABI in ``include/mifc.h``: it picks
pointers out of numpy arrays (host memory, the legacy calling convention) or
PyTorch CUDA tensors (fields resident in HBM), forwards to ``libmifc.so`` and
hands back ``(result, fDefined)``.  Operator names, argument order and failure
behaviour follow the reference: where the C++ function returns ``false`` the
wrapper returns ``None`` (as the reference's pybind11 layer does,
python/py_mi_fieldcalc.cc:92-93).

There is no CPU compute path here.  Without the HIP library the import fails,
without a GPU ``Context()`` raises.
"""
import ctypes

import numpy as np

from . import _capi

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2  # miutil::ValuesDefined, FieldDefined.h:41
UNDEF = np.float32(1.0e35)  # miutil::UNDEF, FieldDefined.cc:34
MEM_HOST, MEM_DEVICE = 0, 1

__all__ = ["Context", "SlabPlan", "Graph", "PreparedCalls", "HstatsResult", "ALL_DEFINED", "NONE_DEFINED", "SOME_DEFINED", "UNDEF", "classify",
           "ensemble_products"]

# mifc_ens_product.stat (include/mifc.h), and the names Context.ensembleStatistics takes for them
ENS_SUM, ENS_MEAN, ENS_STDDEV, ENS_EXTREME, ENS_PROBABILITY = 0, 1, 2, 3, 4
_ENS_EXTREMES = {"max": 1, "min": 2, "argmax": 3, "argmin": 4}
_ENS_MAX_PROBABILITIES = 8
# the product codes of mifc_vlayer_* (include/mifc.h, MIFC_VLAYER_*) and the names Context.vlayer_* takes for them
VLAYER_PRODUCTS = {"integral": 1, "mean": 2, "max": 3, "min": 4, "coord_of_max": 5, "coord_of_min": 6}
# the methods of mifc_vderiv_* (MIFC_VDERIV_*)
VDERIV_METHODS = {"centred": 0, "weighted": 1}
# the methods of mifc_hinterp_levels (MIFC_HINTERP_*)
HINTERP_METHODS = {"nearest": 0, "bilinear": 1, "bicubic": 2}
# the modes and product groups of mifc_hstats_levels (MIFC_HSTATS_*)
HSTATS_MODES = {"area": 0, "rows": 1}
HSTATS_PRODUCTS = {"moments": 1, "extremes": 2}


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


def classify(n_undefined, n):
    """miutil::checkDefined(size_t, size_t), FieldDefined.cc:62-70."""
    return _capi.lib().mifc_classify(int(n_undefined), int(n))


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class _Arg:
    """Address + keep-alive of one field argument.

    levels=True accepts a (nlev, ny, nx) device tensor whose levels are padded
    (stride(0) >= ny*nx, every level itself contiguous): ``lstride`` is that
    level stride in floats.  output=True refuses host arrays that would have to
    be converted (the caller's array would never be written)."""

    __slots__ = ("addr", "keep", "device", "shape", "dev_index", "lstride")

    def __init__(self, x, allow_none=False, levels=False, output=False):
        self.dev_index, self.lstride = None, None
        if x is None:
            if not allow_none:
                raise ValueError("missing field argument")
            self.addr, self.keep, self.device, self.shape = None, None, None, None
            return
        if _is_torch(x):
            import torch

            if x.dtype != torch.float32:
                raise ValueError("device fields must be float32 tensors")
            if not x.is_cuda:
                raise ValueError("torch tensors must live on the GPU; pass numpy arrays for host memory")
            if levels and x.dim() == 3 and not x.is_contiguous():
                nlev, ny, nx = x.shape
                if x.stride(2) != 1 or x.stride(1) != nx or x.stride(0) < ny * nx or x.stride(0) % 4 != 0:
                    raise ValueError("a level batch must be (nlev, ny, nx) with contiguous levels and a level stride that is a multiple of 4")
            elif not x.is_contiguous():
                raise ValueError("device fields must be contiguous float32 tensors")
            self.addr, self.keep, self.device, self.shape = x.data_ptr(), x, True, tuple(x.shape)
            self.dev_index = x.device.index
            if levels and x.dim() == 3:
                self.lstride = int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1] * x.shape[2])
        else:
            if output and not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags["C_CONTIGUOUS"]):
                raise ValueError("an output array must be a C-contiguous float32 numpy array (or a CUDA tensor)")
            a = np.ascontiguousarray(x, dtype=np.float32)  # forcecast, like py_mi_fieldcalc.cc:40
            self.addr, self.keep, self.device, self.shape = a.ctypes.data, a, False, a.shape
            if levels and a.ndim == 3:
                self.lstride = int(a.shape[1] * a.shape[2])


def _memkind(args, ctx_device=None):
    present = [a for a in args if a.addr is not None]
    kinds = {a.device for a in present}
    if len(kinds) != 1:
        raise ValueError("all fields of one call must be either numpy (host) or CUDA tensors (device)")
    if ctx_device is not None:
        for a in present:
            if a.device and a.dev_index is not None and a.dev_index != ctx_device:
                raise ValueError("a tensor lives on cuda:%d but this Context was created on device %d" % (a.dev_index, ctx_device))
    return MEM_DEVICE if kinds.pop() else MEM_HOST


def _same_shape(args, shape):
    return all(a.addr is None or tuple(a.shape) == tuple(shape) for a in args)


def _empty_like(ref, shape=None):
    if _is_torch(ref):
        import torch

        return torch.empty(shape or ref.shape, dtype=torch.float32, device=ref.device)
    return np.empty(shape or np.shape(ref), dtype=np.float32)


# ------------------------------------------------ what the level-batch methods (vinterp, vlayer, vderiv) take alike
def _level_batches(fields):
    """One (nlev, ny, nx) batch, a stacked (nf, nlev, ny, nx) array / tensor or a sequence of batches: (was it one, the
    batches, their _Arg, the shape of a batch)."""
    one = (isinstance(fields, np.ndarray) or _is_torch(fields)) and len(fields.shape) == 3
    if one:
        batches = [fields]
    elif isinstance(fields, np.ndarray) or _is_torch(fields):
        batches = [fields[f] for f in range(fields.shape[0])]
    else:
        batches = list(fields)
    if not batches:
        raise ValueError("no fields")
    fa = [_Arg(b) for b in batches]
    shape = tuple(fa[0].shape)
    if len(shape) != 3:
        raise ValueError("fields must be (nlev, ny, nx) batches")
    if not _same_shape(fa, shape):
        raise ValueError("every field must have the shape %s" % (shape,))
    return one, batches, fa, shape


def _member_batch(fields, fdefined_in, fallback):
    """What ensembleQuantiles and ensembleStatistics take alike: `fields` and `fdefined_in` as their docstrings say; fallback: the
    member shape taken from the output, for a call without members, or None.  Returns (the members, their _Arg, shape, nlev,
    ny, nx, the pointer table, the (nmem, nlev) int32 flags or None)."""
    members = [fields[j] for j in range(fields.shape[0])] if isinstance(fields, np.ndarray) or _is_torch(fields) else list(fields)
    fa = [_Arg(m) for m in members]
    if fa:
        shape = tuple(fa[0].shape)
    elif fallback is not None:
        shape = tuple(fallback)
    else:
        raise ValueError("no member fields and no output to take the shape from")
    if len(shape) not in (2, 3):
        raise ValueError("members must be (ny, nx) or (nlev, ny, nx) fields")
    if not _same_shape(fa, shape):
        raise ValueError("every member must have the shape %s" % (shape,))
    nlev = shape[0] if len(shape) == 3 else 1
    table = (ctypes.c_void_p * max(len(fa), 1))(*[a.addr for a in fa])
    flags = None
    if fdefined_in is not None:
        f = np.asarray(fdefined_in, dtype=np.int32)
        if f.ndim == 1:
            f = np.repeat(f[:, None], nlev, axis=1)
        flags = np.ascontiguousarray(f.reshape(len(fa), nlev), dtype=np.int32)
    return members, fa, shape, nlev, shape[-2], shape[-1], table, flags


def _level_coord(coord, hybrid, shape):
    """The coordinate argument: ps (ny, nx) of the hybrid form, else a batch like the fields."""
    ca = _Arg(coord)
    want = shape[1:] if hybrid else shape
    if tuple(ca.shape) != want:
        raise ValueError("the coordinate must have the shape %s" % (want,))
    return ca


def _level_flags(fdefined_in, nf, nlev):
    """fdefined_in as the (nf, nlev) table the C entries take, None as it is."""
    if fdefined_in is None:
        return None
    f = np.asarray(fdefined_in, dtype=np.int32)
    if f.size == nf:  # one flag per field stands for every level (nlev >= 2: never mistaken for the full table)
        f = np.repeat(f.reshape(nf, 1), nlev, axis=1)
    return np.ascontiguousarray(f.reshape(nf, nlev), dtype=np.int32)


def _hybrid_levels(fields, alevel, blevel):
    al = np.ascontiguousarray(np.asarray(alevel, dtype=np.float32).ravel())
    bl = np.ascontiguousarray(np.asarray(blevel, dtype=np.float32).ravel())
    nlev = int(fields[0].shape[-3]) if not hasattr(fields, "shape") else int(fields.shape[-3])
    if al.size != nlev or bl.size != nlev:
        raise ValueError("alevel and blevel must hold one value per level")
    return al, bl


def _coord_flags(fdef_coord, coord):
    if fdef_coord is None:
        return None
    fc_ = np.ascontiguousarray(np.asarray(fdef_coord, dtype=np.int32).ravel())
    if fc_.size != int(_Arg(coord).shape[0]):
        raise ValueError("fdef_coord must hold one flag per level")
    return fc_


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


class Context:
    """One mifc_ctx: a HIP device, a stream, staging scratch.  Not thread-safe;
    create one per thread (the reference is re-entrant)."""

    def __init__(self, device=0, stream=None):
        self._recording = None  # prepare(): the C calls made while it runs
        self._lib = _capi.lib()
        self._ctx = self._lib.mifc_create(int(device))
        if not self._ctx:
            raise RuntimeError(
                "mifc_create(%d) failed: no usable HIP device (visible devices: %d). "
                "The operators run on the GPU only; there is no CPU fallback." % (device, self._lib.mifc_device_count())
            )
        self.device = device
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.mifc_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ misc
    def last_error(self):
        s = self._lib.mifc_last_error(self._ctx)
        return s.decode() if s else ""

    def set_stream(self, stream):
        """stream: raw hipStream_t address (0 = HIP's default stream), a
        torch.cuda.Stream, or None to go back to the context's own stream."""
        if stream is None:
            self._lib.mifc_use_own_stream(self._ctx)
            return
        if hasattr(stream, "cuda_stream"):
            stream = stream.cuda_stream
        self._lib.mifc_set_stream(self._ctx, ctypes.c_void_p(int(stream)))

    def use_torch_stream(self):
        import torch

        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def reload_env(self):
        """Re-read the MIFC_* tuning / diagnostic variables (they are read when a context is created)."""
        self._lib.mifc_reload_env(self._ctx)

    def synchronize(self):
        if not self._lib.mifc_synchronize(self._ctx):
            raise RuntimeError(self.last_error())

    def _measure_entry(self, name):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise RuntimeError("%s exists in the measurement build of the library only (tools/ select it through MIFC_LIB_PATH)" % name)
        return fn

    def timing_begin(self):
        """Measurement build only: bracket every kernel launch of the following calls with HIP events."""
        if not self._measure_entry("mifc_timing_begin")(self._ctx):
            raise RuntimeError(self.last_error())

    def timing_end_ms(self):
        """Summed kernel time (ms) of the calls since timing_begin(); -1 if unavailable."""
        return float(self._measure_entry("mifc_timing_end_ms")(self._ctx))

    def hold_field(self, host_array):
        """Uploads a constant host field (map ratios, Coriolis parameter) once;
        host-pointer calls that are handed the same array then skip its upload.
        The array must stay alive and unchanged until release_field()."""
        a = _Arg(host_array)
        if a.device:
            raise ValueError("hold_field is for host arrays")
        if a.keep is not host_array:
            raise ValueError("hold_field needs a C-contiguous float32 array (a converted copy would have another address)")
        self._held = getattr(self, "_held", {})
        self._held[a.addr] = a.keep
        if not self._lib.mifc_hold_field(self._ctx, a.addr, int(a.keep.size)):
            raise RuntimeError(self.last_error())
        return a.keep

    def release_field(self, host_array):
        a = _Arg(host_array)
        self._lib.mifc_release_field(self._ctx, a.addr)
        getattr(self, "_held", {}).pop(a.addr, None)

    # ------------------------------------------------------------ call helper
    def _bind_stream(self, memkind):
        """Fields resident on the device come from PyTorch: run on torch's
        current stream so that the kernels are ordered after whatever produced
        the inputs (and before whatever consumes the outputs).  Host-pointer
        calls use the context's own stream."""
        if getattr(self, "_frozen_stream", False):
            return  # a graph capture is open (Graph): the recorded calls go to the capture stream
        if memkind == MEM_DEVICE:
            self.use_torch_stream()
        else:
            self.set_stream(None)

    def _call(self, name, args):
        # numpy arrays among the arguments are host tables (flags, per-level coefficients): passed by address
        cargs = [a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]
        fn = getattr(self._lib, name)
        if self._recording is not None:
            self._recording.append((name, fn, cargs, [a for a in args if isinstance(a, np.ndarray)]))
        rc = fn(self._ctx, *cargs)
        if not rc and self.last_error():
            err = self.last_error()
            raise RuntimeError("%s: %s" % (name, err))
        return rc

    def prepare(self, fn):
        """Runs fn() -- asynchronous *_enqueue wrapper calls on device tensors -- once and returns a PreparedCalls whose launch()
        repeats exactly the C calls it made (same addresses, same scalars, the host tables kept alive) without the wrapper's
        shape checks, array conversions and stream lookup: ~3 us per call instead of ~30.  The tensors must stay alive and in
        place; the context must be on the stream the launches are meant for (use_torch_stream)."""
        self._recording = []
        try:
            fn()
        finally:
            rec, self._recording = self._recording, None
        return PreparedCalls(self, rec)

    @staticmethod
    def _nxny(a):
        ny, nx = a.shape[-2], a.shape[-1]
        return nx, ny

    def _single(self, name, fields, scalars, outs, fdefined, undef, n_out=1, out_like=None, lead=(), pre=(), tail=()):
        """fields: input arrays (None allowed), scalars: list placed between
        inputs and outputs in reference order, outs: preallocated or None.
        lead: arguments before (nx, ny) (fieldOPER*'s compute), pre: scalars
        before the fields, tail: arguments between the outputs and the flag."""
        fa = [_Arg(f, allow_none=True) for f in fields]
        ref = next(f for f in fields if f is not None)
        ra = _Arg(ref)
        if len(ra.shape) != 2:
            return None  # like the reference's binding (py_mi_fieldcalc.cc:82-83): not a 2-D field
        nx, ny = self._nxny(ra)
        outs = list(outs)
        for k in range(n_out):
            if outs[k] is None:
                outs[k] = _empty_like(ref)
        oa = [_Arg(o, output=True) for o in outs]
        # every field of the call has the shape of the first one; the reference's binding returns None
        # otherwise (same_dims, py_mi_fieldcalc.cc:82-83) -- here it also keeps the kernels inside the buffers
        if not _same_shape(fa + oa, ra.shape):
            return None
        mk = _memkind(fa + oa, self.device)
        self._bind_stream(mk)
        fd = ctypes.c_int(int(fdefined))
        args = (list(lead) + [nx, ny] + list(pre) + [a.addr for a in fa] + list(scalars) + [a.addr for a in oa] + list(tail)
                + [ctypes.addressof(fd), float(undef), mk])
        if not self._call(name, args):
            return None
        res = [o if _is_torch(o) else a.keep for o, a in zip(outs, oa)]
        return (res[0] if n_out == 1 else tuple(res)), fd.value

    # ---------------------------------------------------- elementwise operators
    def vectorabs(self, u, v, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """ff = sqrt(u*u+v*v); FieldCalculations.cc:1819."""
        return self._single("mifc_vectorabs", [u, v], [], [out], fdefined, undef)

    def pleveltemp(self, tinp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pleveltemp", [tinp], [float(p), unit.encode(), int(compute)], [out], fdefined, undef)

    def hleveltemp(self, tinp, ps, alevel, blevel, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single(
            "mifc_hleveltemp", [tinp, ps], [float(alevel), float(blevel), unit.encode(), int(compute)], [out], fdefined, undef
        )

    def aleveltemp(self, tinp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_aleveltemp", [tinp, p], [unit.encode(), int(compute)], [out], fdefined, undef)

    def plevelhum(self, t, huminp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelhum", [t, huminp], [float(p), unit.encode(), int(compute)], [out], fdefined, undef)

    def hlevelhum(self, t, huminp, ps, alevel, blevel, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single(
            "mifc_hlevelhum", [t, huminp, ps], [float(alevel), float(blevel), unit.encode(), int(compute)], [out], fdefined, undef
        )

    def alevelhum(self, t, huminp, p, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_alevelhum", [t, huminp, p], [unit.encode(), int(compute)], [out], fdefined, undef)

    def cvhum(self, t, huminp, unit, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_cvhum", [t, huminp], [unit.encode(), int(compute)], [out], fdefined, undef)

    # -------------------------------------------------------- stencil operators
    def relvort(self, u, v, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_relvort", [u, v, xmapr, ymapr], [], [out], fdefined, undef)

    def absvort(self, u, v, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_absvort", [u, v, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def divergence(self, u, v, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_divergence", [u, v, xmapr, ymapr], [], [out], fdefined, undef)

    def gradient(self, field, xmapr, ymapr, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_gradient", [field, xmapr, ymapr], [int(compute)], [out], fdefined, undef)

    def plevelgwind_xcomp(self, z, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelgwind_xcomp", [z, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def plevelgwind_ycomp(self, z, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelgwind_ycomp", [z, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def plevelgvort(self, z, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelgvort", [z, xmapr, ymapr, fcoriolis], [], [out], fdefined, undef)

    def ilevelgwind(self, mpot, xmapr, ymapr, fcoriolis, fdefined=SOME_DEFINED, undef=UNDEF, out=(None, None)):
        return self._single("mifc_ilevelgwind", [mpot, xmapr, ymapr, fcoriolis], [], list(out), fdefined, undef, n_out=2)

    # ------------------------------------------ next operators
    def advection(self, f, u, v, xmapr, ymapr, hours, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_advection", [f, u, v, xmapr, ymapr], [float(hours)], [out], fdefined, undef)

    def jacobian(self, field1, field2, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_jacobian", [field1, field2, xmapr, ymapr], [], [out], fdefined, undef)

    def momentumXcoordinate(self, v, xmapr, fcoriolis, fcoriolisMin, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_momentumXcoordinate", [v, xmapr, fcoriolis], [float(fcoriolisMin)], [out], fdefined, undef)

    def momentumYcoordinate(self, u, ymapr, fcoriolis, fcoriolisMin, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_momentumYcoordinate", [u, ymapr, fcoriolis], [float(fcoriolisMin)], [out], fdefined, undef)

    def thermalFrontParameter(self, tx, xmapr, ymapr, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_thermalFrontParameter", [tx, xmapr, ymapr], [], [out], fdefined, undef)

    def plevelqvector(self, z, t, xmapr, ymapr, fcoriolis, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelqvector", [z, t, xmapr, ymapr, fcoriolis], [float(p), int(compute)], [out], fdefined, undef)

    # ---------------------------- the rest of the pointwise catalogue
    # Same argument order as miutil::fieldcalc; (result, flag) or None like the others.
    def plevelthe(self, t, rh, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelthe", [t, rh], [float(p), int(compute)], [out], fdefined, undef)

    def hlevelthe(self, t, q, ps, alevel, blevel, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_hlevelthe", [t, q, ps], [float(alevel), float(blevel), int(compute)], [out], fdefined, undef)

    def alevelthe(self, t, q, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_alevelthe", [t, q, p], [int(compute)], [out], fdefined, undef)

    def plevelducting(self, t, h, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_plevelducting", [t, h], [float(p), int(compute)], [out], fdefined, undef)

    def hlevelducting(self, t, h, ps, alevel, blevel, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_hlevelducting", [t, h, ps], [float(alevel), float(blevel), int(compute)], [out], fdefined, undef)

    def alevelducting(self, t, h, p, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_alevelducting", [t, h, p], [int(compute)], [out], fdefined, undef)

    def hlevelpressure(self, ps, alevel, blevel, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_hlevelpressure", [ps], [float(alevel), float(blevel)], [out], fdefined, undef)

    def pleveldz2tmean(self, z1, z2, p1, p2, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pleveldz2tmean", [z1, z2], [float(p1), float(p2), int(compute)], [out], fdefined, undef)

    def kIndex(self, t500, t700, rh700, t850, rh850, p500, p700, p850, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_kIndex", [t500, t700, rh700, t850, rh850], [float(p500), float(p700), float(p850), int(compute)], [out],
                            fdefined, undef)

    def ductingIndex(self, t850, rh850, p850, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_ductingIndex", [t850, rh850], [float(p850), int(compute)], [out], fdefined, undef)

    def showalterIndex(self, t500, t850, rh850, p500, p850, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_showalterIndex", [t500, t850, rh850], [float(p500), float(p850), int(compute)], [out], fdefined, undef)

    def boydenIndex(self, t700, z700, z1000, p700, p1000, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_boydenIndex", [t700, z700, z1000], [float(p700), float(p1000), int(compute)], [out], fdefined, undef)

    def sweatIndex(self, t850, t500, td850, td500, u850, v850, u500, v500, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_sweatIndex", [t850, t500, td850, td500, u850, v850, u500, v500], [], [out], fdefined, undef)

    def seaSoundSpeed(self, t, s, z, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_seaSoundSpeed", [t, s], [float(z), int(compute)], [out], fdefined, undef)

    def cvtemp(self, tinp, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_cvtemp", [tinp], [int(compute)], [out], fdefined, undef)

    def abshum(self, t, rhum, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_abshum", [t, rhum], [], [out], fdefined, undef)

    def windCooling(self, t, u, v, compute, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_windCooling", [t, u, v], [int(compute)], [out], fdefined, undef)

    def underCooledRain(self, precip, snow, tk, precipMin, snowRateMax, tcMax, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_underCooledRain", [precip, snow, tk], [float(precipMin), float(snowRateMax), float(tcMax)], [out], fdefined, undef)

    def pressure2FlightLevel(self, pressure, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pressure2FlightLevel", [pressure], [], [out], fdefined, undef)

    def snow_in_cm(self, snow_water, tk2m, td2m, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_snow_in_cm", [snow_water, tk2m, td2m], [], [out], fdefined, undef)

    def values2classes(self, fvalue, values, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """values: the class limits (host sequence).  C order: fvalue, fclass (output), values, nvalues."""
        vals = np.ascontiguousarray(values, dtype=np.float32)
        return self._single("mifc_values2classes", [fvalue], [], [out], fdefined, undef, tail=[vals.ctypes.data, int(vals.size)])

    def shapiro2_filter(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """Second-order Shapiro filter; pass out=field to smooth in place."""
        return self._single("mifc_shapiro2_filter", [field], [], [out], fdefined, undef)

    def vesselIcingOverland(self, airtemp, seatemp, u, v, sal, aice, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_vesselIcingOverland", [airtemp, seatemp, u, v, sal, aice], [], [out], fdefined, undef)

    def vesselIcingMertins(self, airtemp, seatemp, u, v, sal, aice, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_vesselIcingMertins", [airtemp, seatemp, u, v, sal, aice], [], [out], fdefined, undef)

    def winddir(self, u, v, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        """EXTENSION (no reference function): meteorological wind direction, degrees the wind blows FROM,
        dd = 270 - atan2(v, u) * 180 / pi in [0, 360), calm -> 0; see include/mifc.h."""
        return self._single("mifc_winddir", [u, v], [], [out], fdefined, undef)

    def minvalueFields(self, field1, field2, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_minvalueFields", [field1, field2], [], [out], fdefined, undef)

    def maxvalueFields(self, field1, field2, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_maxvalueFields", [field1, field2], [], [out], fdefined, undef)

    def minvalueFieldConst(self, field1, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_minvalueFieldConst", [field1], [float(value)], [out], fdefined, undef)

    def maxvalueFieldConst(self, field1, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_maxvalueFieldConst", [field1], [float(value)], [out], fdefined, undef)

    def absvalueField(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_absvalueField", [field], [], [out], fdefined, undef)

    def log10Field(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_log10Field", [field], [], [out], fdefined, undef)

    def pow10Field(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_pow10Field", [field], [], [out], fdefined, undef)

    def logField(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_logField", [field], [], [out], fdefined, undef)

    def expField(self, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_expField", [field], [], [out], fdefined, undef)

    def powerField(self, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_powerField", [field], [float(value)], [out], fdefined, undef)

    def replaceUndefined(self, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_replaceUndefined", [field], [float(value)], [out], fdefined, undef)

    def replaceDefined(self, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_replaceDefined", [field], [float(value)], [out], fdefined, undef)

    def fieldOPERfield(self, compute, field1, field2, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_fieldOPERfield", [field1, field2], [], [out], fdefined, undef, lead=[int(compute)])

    def fieldOPERconstant(self, compute, field, value, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_fieldOPERconstant", [field], [float(value)], [out], fdefined, undef, lead=[int(compute)])

    def constantOPERfield(self, compute, value, field, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._single("mifc_constantOPERfield", [field], [], [out], fdefined, undef, lead=[int(compute)], pre=[float(value)])

    # ---------------------------------- reductions over ensemble members
    def _ensemble(self, name, fields, fdefined_in, lead, tail, fdefined, undef, out):
        """fields: sequence of member fields (all numpy or all CUDA tensors)."""
        fa = [_Arg(f) for f in fields]
        ref = fields[0] if len(fields) else out
        if ref is None:
            raise ValueError("no member fields and no output to take the shape from")
        ra = _Arg(ref)
        if len(ra.shape) != 2:
            return None
        nx, ny = self._nxny(ra)
        if out is None:
            out = _empty_like(ref)
        oa = _Arg(out, output=True)
        if not _same_shape(fa + [oa], ra.shape):
            return None
        mk = _memkind(fa + [oa], self.device)
        self._bind_stream(mk)
        table = (ctypes.c_void_p * max(len(fa), 1))(*[a.addr for a in fa])
        args = list(lead) + [nx, ny, ctypes.addressof(table)]
        if fdefined_in is not None:
            flags = (ctypes.c_int * max(len(fa), 1))(*[int(x) for x in fdefined_in])
            args.append(ctypes.addressof(flags))
        fd = ctypes.c_int(int(fdefined))
        args += [len(fa)] + list(tail) + [oa.addr, ctypes.addressof(fd), float(undef), mk]
        if not self._call(name, args):
            return None
        return (out if _is_torch(out) else oa.keep), fd.value

    def sumFields(self, fields, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_sumFields", fields, None, [], [], fdefined, undef, out)

    def meanValue(self, fields, fdefined_in, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_meanValue", fields, fdefined_in, [], [], fdefined, undef, out)

    def stddevValue(self, fields, fdefined_in, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_stddevValue", fields, fdefined_in, [], [], fdefined, undef, out)

    def extremeValue(self, compute, fields, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        return self._ensemble("mifc_extremeValue", fields, None, [int(compute)], [], fdefined, undef, out)

    def probability(self, compute, fields, fdefined_in, limits, fdefined=SOME_DEFINED, undef=UNDEF, out=None):
        lim = np.ascontiguousarray(limits, dtype=np.float32)
        return self._ensemble("mifc_probability", fields, fdefined_in, [int(compute)], [lim.ctypes.data, int(lim.size)], fdefined, undef, out)

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
        if out is None:
            out = _empty_like(members[0], (nq,) + shape)
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != (nq,) + shape:
            raise ValueError("out must have shape %s" % (((nq,) + shape),))
        mk = _memkind(fa + [oa], self.device)
        self._bind_stream(mk)
        level_bytes = nlev * ny * nx * 4
        outs = (ctypes.c_void_p * max(nq, 1))(*[oa.addr + q * level_bytes for q in range(nq)])
        fd = np.zeros(nlev, np.int32)
        if not self._call("mifc_ensembleQuantiles", [code, nx, ny, nlev, ctypes.addressof(table), flags, len(fa), pct, nq, ctypes.addressof(outs), fd,
                                                      float(undef), mk]):
            raise RuntimeError("mifc_ensembleQuantiles: " + self.last_error())
        return (out if _is_torch(out) else oa.keep), (int(fd[0]) if len(shape) == 2 else fd)

    # ------------------------------------------------------ level batches to constant surfaces (EXTENSION)
    def _vinterp(self, name, fields, coord, coord_args, targets, method, fdefined_in, undef, out):
        code = {"linear": 0, "log": 1}.get(method, -1) if isinstance(method, str) else int(method)
        one, batches, fa, shape = _level_batches(fields)
        nlev, ny, nx = shape
        ca = _level_coord(coord, name == "mifc_vinterp_hlevels", shape)
        tg = np.ascontiguousarray(np.asarray(targets, dtype=np.float32).ravel())
        nt, nf = int(tg.size), len(fa)
        out_shape = (nt, ny, nx) if one else (nf, nt, ny, nx)
        if out is None:
            out = _empty_like(batches[0], out_shape)
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != out_shape:
            raise ValueError("out must have shape %s" % (out_shape,))
        mk = _memkind(fa + [ca, oa], self.device)
        self._bind_stream(mk)
        table = (ctypes.c_void_p * nf)(*[a.addr for a in fa])
        outs = (ctypes.c_void_p * nf)(*[oa.addr + f * nt * ny * nx * 4 for f in range(nf)])
        flags = _level_flags(fdefined_in, nf, nlev)
        fd = np.zeros((nf, nt), np.int32)
        args = [nx, ny, nlev, ctypes.addressof(table), flags, nf, ca.addr] + coord_args + [tg, nt, code, ctypes.addressof(outs), fd, float(undef), mk]
        if not self._call(name, args):
            raise RuntimeError(name + ": " + self.last_error())
        res = out if _is_torch(out) else oa.keep
        return (res, fd[0]) if one else (res, fd)

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
        out_shape = (np_, ny, nx) if one else (nf, np_, ny, nx)
        if out is None:
            out = _empty_like(batches[0], out_shape)
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != out_shape:
            raise ValueError("out must have shape %s" % (out_shape,))
        mk = _memkind(fa + [ca, oa] + bounds, self.device)
        self._bind_stream(mk)
        table = (ctypes.c_void_p * nf)(*[a.addr for a in fa])
        outs = (ctypes.c_void_p * nf)(*[oa.addr + f * np_ * ny * nx * 4 for f in range(nf)])
        flags = _level_flags(fdefined_in, nf, nlev)
        pc = np.ascontiguousarray(codes, dtype=np.int32)
        fd = np.zeros((nf, np_), np.int32)
        args = [nx, ny, nlev, ctypes.addressof(table), flags, nf, ca.addr] + coord_args + scalars + ptrs + [pc, np_, ctypes.addressof(outs), fd, float(undef), mk]
        if not self._call(name, args):
            raise RuntimeError(name + ": " + self.last_error())
        res = out if _is_torch(out) else oa.keep
        return (res, fd[0]) if one else (res, fd)

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
        res = []
        for o, s in zip(given, shapes):
            if o is None:
                o = _empty_like(batches[0], s)
            oa = _Arg(o, output=True)
            if tuple(oa.shape) != tuple(s):
                raise ValueError("out must have shape %s" % (s,))
            res.append((o, oa))
        mk = _memkind(fa + others + [oa for _, oa in res], self.device)
        self._bind_stream(mk)
        batch_bytes = nlev * ny * nx * 4
        table = (ctypes.c_void_p * nf)(*[a.addr for a in fa])
        outs = mags = fd = mfd = None
        if want_out:
            outs = (ctypes.c_void_p * nf)(*[res[0][1].addr + f * batch_bytes for f in range(nf)])
            fd = np.zeros((nf, nlev), np.int32)
        if want_mag:
            mags = (ctypes.c_void_p * max(nm, 1))(*[res[-1][1].addr + j * batch_bytes for j in range(nm)])
            mfd = np.zeros((nm, nlev), np.int32)
        flags = _level_flags(fdefined_in, nf, nlev)
        args = [nx, ny, nlev, ctypes.addressof(table), flags, nf, coord_arg] + coord_args + [
            code, ctypes.addressof(outs) if want_out else None, fd, ctypes.addressof(mags) if want_mag else None, mfd, float(undef), mk]
        if not self._call(name, args):
            raise RuntimeError(name + ": " + self.last_error())
        ret = []
        if want_out:
            ret += [res[0][0] if _is_torch(res[0][0]) else res[0][1].keep, fd[0] if one else fd]
        if want_mag:
            ret += [res[-1][0] if _is_torch(res[-1][0]) else res[-1][1].keep, mfd]
        return tuple(ret)

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
        code = HINTERP_METHODS.get(method, -1) if isinstance(method, str) else int(method)
        one, batches, fa, shape = _level_batches(fields)
        nlev, ny, nx = shape
        nf = len(fa)
        xa, ya = _Arg(xpos), _Arg(ypos)
        where = tuple(xa.shape)
        if tuple(ya.shape) != where:
            raise ValueError("xpos and ypos must have the same shape")
        npos = int(np.prod(where, dtype=np.int64))
        out_shape = ((nlev,) if one else (nf, nlev)) + where
        if out is None:
            out = _empty_like(batches[0], out_shape)
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != out_shape:
            raise ValueError("out must have shape %s" % (out_shape,))
        mk = _memkind(fa + [xa, ya, oa], self.device)
        self._bind_stream(mk)
        table = (ctypes.c_void_p * nf)(*[a.addr for a in fa])
        outs = (ctypes.c_void_p * nf)(*[oa.addr + f * nlev * npos * 4 for f in range(nf)])
        flags = _level_flags(fdefined_in, nf, nlev)
        fd = np.zeros((nf, nlev), np.int32)
        args = [nx, ny, nlev, ctypes.addressof(table), flags, nf, npos, xa.addr, ya.addr, code, ctypes.addressof(outs), fd, float(undef), mk]
        if not self._call("mifc_hinterp_levels", args):
            raise RuntimeError("mifc_hinterp_levels: " + self.last_error())
        res = out if _is_torch(out) else oa.keep
        return (res, fd[0]) if one else (res, fd)

    def last_hinterp_form(self):
        """The launch shape of this thread's last hinterp_levels call as a dict (mifc_last_hinterp_form; a diagnostic for
        tests): method as a string, the other keys as ints."""
        form = dict(word.split("=", 1) for word in self._lib.mifc_last_hinterp_form().decode().split())
        return {k: (v if k == "method" else int(v)) for k, v in form.items()}

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
        mean = ma_out = mean_table = mfd = None
        if want_mean:
            mean = _empty_like(batches[0], (nf, nlev, max(nrows, 0)))
            ma_out = _Arg(mean, output=True)
            mean_table = (ctypes.c_void_p * nf)(*[ma_out.addr + f * nlev * nrows * 4 for f in range(nf)])
            mfd = np.zeros((nf, nlev), np.int32)
        mk = _memkind(fa + ma + [wa] + ([ma_out] if want_mean else []), self.device)
        self._bind_stream(mk)
        table = (ctypes.c_void_p * nf)(*[a.addr for a in fa])
        mtable = (ctypes.c_void_p * nf)(*[a.addr for a in ma]) if ma else None
        args = [nx, ny, nlev, ctypes.addressof(table), _level_flags(fdefined_in, nf, nlev), nf, ctypes.addressof(mtable) if ma else None,
                _level_flags(fdefined_minus, nf, nlev) if ma else None, pv, wa.addr, int(fdef_weight), bx, code, mask, stats_addr,
                ctypes.addressof(mean_table) if want_mean else None, mfd, float(undef), mk]
        if not self._call("mifc_hstats_levels", args):
            raise RuntimeError("mifc_hstats_levels: " + self.last_error())
        if one:
            stats = stats.reshape(stats_shape[1:])
        return HstatsResult(stats, pv, None if mean is None else (mean[0] if one else mean), None if mfd is None else (mfd[0] if one else mfd))

    def last_hstats_form(self):
        """The launch shape of this thread's last hstats_levels call as a dict (mifc_last_hstats_form; a diagnostic for
        tests): mode as a string, the other keys as ints."""
        form = dict(word.split("=", 1) for word in self._lib.mifc_last_hstats_form().decode().split())
        return {k: (v if k == "mode" else int(v)) for k, v in form.items()}

    # ------------------------------------------ vector pairs rotated, on the grid and while sampling (EXTENSION)
    @staticmethod
    def _pairs(pairs):
        """The components u0, v0, u1, v1 ... of `pairs` -- one pair (2, nlev, ny, nx), stacked pairs (npairs, 2, nlev, ny, nx),
        a sequence of (u, v) or the flat sequence u0, v0, u1, v1 ... of (nlev, ny, nx) batches -- as _level_batches takes
        them: (was it one pair, the batches, their _Arg, the shape of a batch)."""
        stacked = isinstance(pairs, np.ndarray) or _is_torch(pairs)
        if stacked and len(pairs.shape) not in (4, 5):
            raise ValueError("pairs must be (2, nlev, ny, nx), (npairs, 2, nlev, ny, nx) or a sequence of (u, v)")
        items = [pairs[j] for j in range(pairs.shape[0])] if stacked else list(pairs)
        if items and all(hasattr(i, "shape") and len(i.shape) == 3 for i in items):
            comps, one = items, len(items) == 2  # u, v (, u1, v1 ...)
        else:
            comps, one = [], False
            for pair in items:
                if len(pair) != 2:
                    raise ValueError("a pair is (u, v)")
                comps += [pair[0], pair[1]]
        if len(comps) < 2 or len(comps) % 2:
            raise ValueError("pairs must hold u and v of every pair")
        _, batches, fa, shape = _level_batches(comps)
        return one, batches, fa, shape

    @staticmethod
    def _pair_flags(fdefined_in, npairs, nlev):
        """fdefined_in of a pair call -- (2,), (2, nlev), (npairs, 2) or (npairs, 2, nlev) -- as the (2 * npairs, nlev) table."""
        if fdefined_in is None:
            return None
        f = np.asarray(fdefined_in, dtype=np.int32)
        if f.size == 2 * npairs:
            f = np.repeat(f.reshape(2 * npairs, 1), nlev, axis=1)
        return np.ascontiguousarray(f.reshape(2 * npairs, nlev), dtype=np.int32)

    def vrotate_levels(self, pairs, cosa, sina, fdefined_in=None, fdef_rot=SOME_DEFINED, undef=UNDEF, out=None):
        """EXTENSION (include/mifc.h, mifc_vrotate_levels, rule R): vector pairs of level batches rotated cell by cell,
        u' = c u - s v, v' = s u + c v in double, rounded to float once.  pairs: one pair (2, nlev, ny, nx), up to four
        stacked (npairs, 2, nlev, ny, nx), or a sequence of (u, v) batches; numpy arrays (host memory) or CUDA tensors.
        cosa, sina: (ny, nx), like the fields; the library does not normalise them; fdef_rot: their flag.  fdefined_in: one
        flag per component or per component and level, None: SOME_DEFINED.  Returns (out, flags): out shaped like the
        stacked pairs, flags int32 (npairs, 2, nlev) -- the two components of a pair carry the same flag; with ONE pair the
        leading axis is dropped from both.  A refused call raises RuntimeError."""
        one, batches, fa, shape = self._pairs(pairs)
        nlev, ny, nx = shape
        nf = len(fa)
        ca, sa = _Arg(cosa), _Arg(sina)
        if tuple(ca.shape) != (ny, nx) or tuple(sa.shape) != (ny, nx):
            raise ValueError("cosa and sina must have the shape %s" % ((ny, nx),))
        out_shape = ((2,) if one else (nf // 2, 2)) + shape
        if out is None:
            out = _empty_like(batches[0], out_shape)
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != out_shape:
            raise ValueError("out must have shape %s" % (out_shape,))
        mk = _memkind(fa + [ca, sa, oa], self.device)
        self._bind_stream(mk)
        table = (ctypes.c_void_p * nf)(*[a.addr for a in fa])
        outs = (ctypes.c_void_p * nf)(*[oa.addr + f * nlev * ny * nx * 4 for f in range(nf)])
        flags = self._pair_flags(fdefined_in, nf // 2, nlev)
        fd = np.zeros((nf // 2, 2, nlev), np.int32)
        args = [nx, ny, nlev, ctypes.addressof(table), flags, nf // 2, ca.addr, sa.addr, int(fdef_rot), ctypes.addressof(outs), fd, float(undef), mk]
        if not self._call("mifc_vrotate_levels", args):
            raise RuntimeError("mifc_vrotate_levels: " + self.last_error())
        res = out if _is_torch(out) else oa.keep
        return (res, fd[0]) if one else (res, fd)

    def last_vrotate_form(self):
        """The launch shape of this thread's last vrotate_levels call as a dict of ints (mifc_last_vrotate_form; a diagnostic
        for tests)."""
        return {k: int(v) for k, v in (word.split("=", 1) for word in self._lib.mifc_last_vrotate_form().decode().split())}

    def hinterp_vector_levels(self, pairs, xpos, ypos, cosa, sina, method="bilinear", fdefined_in=None, fdef_rot=SOME_DEFINED, undef=UNDEF,
                              out=None):
        """EXTENSION (include/mifc.h, mifc_hinterp_vector_levels): hinterp_levels of vector pairs and their rotation by rule R
        in one pass -- wind regridded to another projection, along- and across-section wind.  pairs, fdefined_in, fdef_rot:
        as vrotate_levels takes them; xpos, ypos, method: as hinterp_levels takes them; cosa, sina: one value per position,
        shaped like xpos.  A position with undefined coefficients gives undef like an unusable one.  Returns (out
        (npairs, 2, nlev) + S, flags int32 (npairs, 2, nlev)), bit for bit hinterp_levels followed by vrotate_levels; with
        ONE pair the leading axis is dropped from both.  The launch shape is in last_hinterp_form().  A refused call raises
        RuntimeError."""
        code = HINTERP_METHODS.get(method, -1) if isinstance(method, str) else int(method)
        one, batches, fa, shape = self._pairs(pairs)
        nlev, ny, nx = shape
        nf = len(fa)
        xa, ya, ca, sa = _Arg(xpos), _Arg(ypos), _Arg(cosa), _Arg(sina)
        where = tuple(xa.shape)
        if not _same_shape([ya, ca, sa], where):
            raise ValueError("xpos, ypos, cosa and sina must have the same shape")
        npos = int(np.prod(where, dtype=np.int64))
        out_shape = ((2, nlev) if one else (nf // 2, 2, nlev)) + where
        if out is None:
            out = _empty_like(batches[0], out_shape)
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != out_shape:
            raise ValueError("out must have shape %s" % (out_shape,))
        mk = _memkind(fa + [xa, ya, ca, sa, oa], self.device)
        self._bind_stream(mk)
        table = (ctypes.c_void_p * nf)(*[a.addr for a in fa])
        outs = (ctypes.c_void_p * nf)(*[oa.addr + f * nlev * npos * 4 for f in range(nf)])
        flags = self._pair_flags(fdefined_in, nf // 2, nlev)
        fd = np.zeros((nf // 2, 2, nlev), np.int32)
        args = [nx, ny, nlev, ctypes.addressof(table), flags, nf // 2, npos, xa.addr, ya.addr, ca.addr, sa.addr, int(fdef_rot), code,
                ctypes.addressof(outs), fd, float(undef), mk]
        if not self._call("mifc_hinterp_vector_levels", args):
            raise RuntimeError("mifc_hinterp_vector_levels: " + self.last_error())
        res = out if _is_torch(out) else oa.keep
        return (res, fd[0]) if one else (res, fd)

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
        mk = _memkind(fa + oa, self.device)
        self._bind_stream(mk)
        fds = []
        prods = (_capi.EnsProduct * len(specs))()
        for k, (stat, compute, limits, flag_in) in enumerate(specs):
            fd = np.full(nlev, SOME_DEFINED, np.int32)
            if flag_in is not None:
                fd[:] = np.asarray(flag_in, dtype=np.int32).reshape(-1) if np.ndim(flag_in) else int(flag_in)
            fds.append(fd)
            prods[k].stat, prods[k].compute, prods[k].nlimits = stat, compute, len(limits)
            for i, v in enumerate(limits):
                prods[k].limits[i] = v
            prods[k].out, prods[k].fdefined = oa[k].addr, fd.ctypes.data
        if not self._call("mifc_ensemble_levels", [nx, ny, nlev, ctypes.addressof(table), flags, len(fa), ctypes.addressof(prods), len(specs),
                                                    float(undef), mk]):
            raise RuntimeError("mifc_ensemble_levels: " + self.last_error())
        return [((o if _is_torch(o) else a.keep), (int(fd[0]) if len(shape) == 2 else fd)) for o, a, fd in zip(out, oa, fds)]

    # ------------------------------------------------------ neighbourhood statistics
    # out=None allocates an output pre-filled with `undef`: the reference leaves some cells unwritten (neighbourFunctions:
    # interior cells that no step x step block covers; neighbourProbFunctions with range 0 and a compute other than 5 / 6:
    # every cell), and these come back as `undef` instead of uninitialised memory.  With out= given they keep its values.
    # Refusals where the reference is undefined raise RuntimeError with the reason (include/mifc.h); the reference's
    # own `false` gives None.
    def _neighbour(self, name, field, constants, compute, fdefined, undef, out):
        if out is None:
            out = _empty_like(field)
            out[...] = float(np.float32(undef))
        consts = np.ascontiguousarray(constants, dtype=np.float32).ravel()
        return self._single(name, [field], [consts.ctypes.data, int(consts.size), int(compute)], [out], fdefined, undef)

    def neighbourProbFunctions(self, field, constants, compute, fdefined=ALL_DEFINED, undef=UNDEF, out=None):
        """constants = [limit, range]; compute 5: fraction of the (2r+1)^2 box above limit, 6: below.  out=field works in place."""
        return self._neighbour("mifc_neighbourProbFunctions", field, constants, compute, fdefined, undef, out)

    def neighbourFunctions(self, field, constants, compute, fdefined=ALL_DEFINED, undef=UNDEF, out=None):
        """compute 1 mean, 2 max, 3 min (constants = [range(, step)]), 4 percentile, 5 / 6 fraction above / below
        (constants = [percentile or limit, range(, step)]); each computed centre fills its step x step block."""
        return self._neighbour("mifc_neighbourFunctions", field, constants, compute, fdefined, undef, out)

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
        if out is None:
            out = _empty_like(field)
            out[...] = float(np.float32(undef))
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != tuple(fa.shape):
            raise ValueError("out must have the shape of field")
        mk = _memkind([fa, oa], self.device)
        self._bind_stream(mk)
        flags = np.full(nlev, ALL_DEFINED, np.int32) if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        consts = np.ascontiguousarray(constants, dtype=np.float32).ravel()
        if not self._call("mifc_neighbour_levels", [codes[which], int(compute), nx, ny, nlev, fa.addr, consts.ctypes.data, int(consts.size),
                                                     oa.addr, flags, float(undef), mk]):
            return None
        return (out if _is_torch(out) else oa.keep), flags

    # ------------------------------------------------------ iterative vessel icing
    # FieldCalculationsVesselIcing.cc:182 / :677.  The reference's `false` gives None; a level count that overflows an
    # int raises RuntimeError with the reason.  out may be any input (each cell reads only its own index).
    def vesselIcingModStall(self, sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth, vs, alpha, zmin, zmax, fdefined=SOME_DEFINED,
                            undef=UNDEF, out=None):
        """Modified Stallabrass freezing-spray icing rate (cm/h)."""
        return self._single("mifc_vesselIcingModStall", [sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth],
                            [float(vs), float(alpha), float(zmin), float(zmax)], [out], fdefined, undef)

    def vesselIcingMincog(self, sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth, vs, alpha, zmin, zmax, alt, fdefined=SOME_DEFINED,
                          undef=UNDEF, out=None):
        """MINCOG icing rate (cm/h); alt == 1: MINCOG org, anything else: MINCOG adj."""
        return self._single("mifc_vesselIcingMincog", [sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth],
                            [float(vs), float(alpha), float(zmin), float(zmax), int(alt)], [out], fdefined, undef)

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
        if out is None:
            out = _empty_like(fields[fa.index(per_level[0])])
        oa = _Arg(out, output=True)
        if tuple(oa.shape) != shape:
            raise ValueError("out must have shape (nlev, ny, nx)")
        mk = _memkind(fa + [oa], self.device)
        self._bind_stream(mk)
        flags = np.full(nlev, SOME_DEFINED, np.int32) if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        if not self._call("mifc_vesselIcing_levels", [codes[model], nlev, nx, ny] + [a.addr for a in fa]
                          + [mask, float(vs), float(alpha), float(zmin), float(zmax), int(alt), oa.addr, flags, float(undef), mk]):
            return None
        return (out if _is_torch(out) else oa.keep), flags

    # ------------------------------------------------------------------ batched
    def vortdiv_levels(self, u, v, xmapr, ymapr, fdefined=None, undef=UNDEF, rvort=None, diverg=None, want=("rvort", "diverg")):
        """Fused relvort + divergence over u, v of shape (nlev, ny, nx).
        fdefined: int sequence per level (default SOME_DEFINED).  Returns
        ((rvort, diverg), flags ndarray) or None."""
        au, av, ax, ay = _Arg(u), _Arg(v), _Arg(xmapr), _Arg(ymapr)
        if len(au.shape) != 3:
            raise ValueError("u, v must have shape (nlev, ny, nx)")
        nlev, ny, nx = au.shape
        if rvort is None and "rvort" in want:
            rvort = _empty_like(u)
        if diverg is None and "diverg" in want:
            diverg = _empty_like(u)
        ar, ad = _Arg(rvort, allow_none=True, output=True), _Arg(diverg, allow_none=True, output=True)
        if not _same_shape([av, ar, ad], au.shape) or not _same_shape([ax, ay], (ny, nx)):
            raise ValueError("u, v, rvort, diverg must be (nlev, ny, nx) and xmapr, ymapr (ny, nx)")
        mk = _memkind([au, av, ax, ay, ar, ad], self.device)
        self._bind_stream(mk)
        flags = np.full(nlev, SOME_DEFINED, dtype=np.int32) if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        rc = self._call(
            "mifc_vortdiv_levels",
            [nx, ny, nlev, au.addr, av.addr, ax.addr, ay.addr, ar.addr, ad.addr, flags.ctypes.data, float(undef), mk],
        )
        if not rc:
            return None
        outs = tuple(o if (o is None or _is_torch(o)) else a.keep for o, a in ((rvort, ar), (diverg, ad)))
        return outs, flags

    OPS = {"relvort": 0, "absvort": 1, "divergence": 2, "vortdiv": 3, "gradient1": 4, "gradient2": 5, "gradient3": 6, "gradient4": 7,
           "plevelgwind_xcomp": 8, "plevelgwind_ycomp": 9, "plevelgvort": 10, "ilevelgwind": 11, "jacobian": 13}

    def stencil_levels(self, op, f0, f1, xmapr, ymapr, fcoriolis=None, fdefined=None, undef=UNDEF, out0=None, out1=None):
        """Any stencil operator (name from Context.OPS) over f0/f1 of shape (nlev, ny, nx).
        Returns ((out0, out1-or-None), flags) or None."""
        code = self.OPS[op]
        a0, a1 = _Arg(f0), _Arg(f1, allow_none=True)
        ax, ay, af = _Arg(xmapr, allow_none=True), _Arg(ymapr, allow_none=True), _Arg(fcoriolis, allow_none=True)
        nlev, ny, nx = a0.shape
        two = code in (3, 11)
        if out0 is None:
            out0 = _empty_like(f0)
        if two and out1 is None:
            out1 = _empty_like(f0)
        o0, o1 = _Arg(out0, output=True), _Arg(out1 if two else None, allow_none=True, output=True)
        if len(a0.shape) != 3 or not _same_shape([a1, o0, o1], a0.shape) or not _same_shape([ax, ay, af], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and the map / Coriolis fields (ny, nx)")
        mk = _memkind([a0, a1, ax, ay, af, o0, o1], self.device)
        self._bind_stream(mk)
        flags = np.full(nlev, SOME_DEFINED, dtype=np.int32) if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        rc = self._call("mifc_stencil_levels", [code, nx, ny, nlev, a0.addr, a1.addr, ax.addr, ay.addr, af.addr, o0.addr, o1.addr,
                                                flags.ctypes.data, float(undef), mk])
        if not rc:
            return None
        r0 = out0 if _is_torch(out0) else o0.keep
        r1 = None if not two else (out1 if _is_torch(out1) else o1.keep)
        return (r0, r1), flags

    OPS_EX = {"advection": 12, "thermalFrontParameter": 14, "plevelqvector": 15, "shapiro2_filter": 17}

    def stencil_levels_ex(self, op, f0, f1=None, f2=None, xmapr=None, ymapr=None, fcoriolis=None, level_scalars=None, scalar=0.0, compute=0,
                          fdefined=None, undef=UNDEF, out0=None):
        """The f1 operators over a level batch (mifc_stencil_levels_ex): op in OPS_EX; fields (nlev, ny, nx),
        map / Coriolis fields (ny, nx) shared.  advection: f0 = f, f1 = u, f2 = v, scalar = hours;
        thermalFrontParameter: f0 = tx; plevelqvector: f0 = z, f1 = t, level_scalars = p per level, compute 1..4;
        shapiro2_filter: f0 = field.  Returns (out0, flags) or None."""
        code = self.OPS_EX[op]
        a0, a1, a2 = _Arg(f0), _Arg(f1, allow_none=True), _Arg(f2, allow_none=True)
        ax, ay, af = _Arg(xmapr, allow_none=True), _Arg(ymapr, allow_none=True), _Arg(fcoriolis, allow_none=True)
        if len(a0.shape) != 3:
            raise ValueError("level fields must be (nlev, ny, nx)")
        nlev, ny, nx = a0.shape
        if out0 is None:
            out0 = _empty_like(f0)
        o0 = _Arg(out0, output=True)
        if not _same_shape([a1, a2, o0], a0.shape) or not _same_shape([ax, ay, af], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and the map / Coriolis fields (ny, nx)")
        mk = _memkind([a0, a1, a2, ax, ay, af, o0], self.device)
        self._bind_stream(mk)
        flags = np.full(nlev, SOME_DEFINED, dtype=np.int32) if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        ls = None if level_scalars is None else np.ascontiguousarray(level_scalars, dtype=np.float32).reshape(nlev)
        rc = self._call("mifc_stencil_levels_ex", [code, nx, ny, nlev, a0.addr, a1.addr, a2.addr, ax.addr, ay.addr, af.addr,
                                                   None if ls is None else ls.ctypes.data, float(scalar), int(compute), o0.addr, None,
                                                   flags.ctypes.data, float(undef), mk])
        if not rc:
            return None
        return (out0 if _is_torch(out0) else o0.keep), flags

    def vortdiv_levels_enqueue(self, u, v, xmapr, ymapr, rvort, diverg, fdefined=None, undef=UNDEF, n_undefined=None):
        """Asynchronous form on device tensors; n_undefined: int64 CUDA tensor[nlev] or None.
        u, v and rvort, diverg may be level-padded batches (see batch_empty)."""
        au, av, ax, ay = _Arg(u, levels=True), _Arg(v, levels=True), _Arg(xmapr), _Arg(ymapr)
        ar, ad = _Arg(rvort, allow_none=True, levels=True), _Arg(diverg, allow_none=True, levels=True)
        if len(au.shape) != 3:
            raise ValueError("u, v must have shape (nlev, ny, nx)")
        nlev, ny, nx = au.shape
        if not _same_shape([av, ar, ad], au.shape) or not _same_shape([ax, ay], (ny, nx)):
            raise ValueError("u, v, rvort, diverg must be (nlev, ny, nx) and xmapr, ymapr (ny, nx)")
        if _memkind([au, av, ax, ay, ar, ad], self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        outs = [a for a in (ar, ad) if a.addr is not None]
        if not outs:
            raise ValueError("at least one of rvort, diverg is required")
        if av.lstride != au.lstride or (len(outs) == 2 and outs[0].lstride != outs[1].lstride):
            raise ValueError("u and v (and rvort and diverg) must share one level stride")
        flags = None if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        self._bind_stream(MEM_DEVICE)
        rc = self._call(
            "mifc_vortdiv_levels_strided_enqueue",
            [
                nx, ny, nlev, au.addr, av.addr, ax.addr, ay.addr, ar.addr, ad.addr, au.lstride, outs[0].lstride,
                flags, float(undef),
                None if n_undefined is None else n_undefined.data_ptr(),
            ],
        )
        return bool(rc)

    def vortdiv_ff_levels_enqueue(self, u, v, xmapr, ymapr, rvort, diverg, ff, fdefined=None, undef=UNDEF, n_undefined=None, n_undefined_ff=None):
        """Vorticity, divergence and the wind speed of a level batch in one pass (mifc_vortdiv_ff_levels_enqueue); device tensors
        (nlev, ny, nx); n_undefined / n_undefined_ff: int64[nlev] (classify against nx*ny - 2*nx / nx*ny), None allowed when every
        level is ALL_DEFINED."""
        a = [_Arg(x) for x in (u, v, xmapr, ymapr, rvort, diverg, ff)]
        if len(a[0].shape) != 3:
            raise ValueError("u, v must have shape (nlev, ny, nx)")
        nlev, ny, nx = a[0].shape
        if not _same_shape([a[1], a[4], a[5], a[6]], a[0].shape) or not _same_shape(a[2:4], (ny, nx)):
            raise ValueError("u, v, rvort, diverg, ff must be (nlev, ny, nx) and xmapr, ymapr (ny, nx)")
        if _memkind(a, self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        flags = None if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        self._bind_stream(MEM_DEVICE)
        rc = self._call("mifc_vortdiv_ff_levels_enqueue", [nx, ny, nlev] + [x.addr for x in a] + [
            flags, float(undef), None if n_undefined is None else n_undefined.data_ptr(),
            None if n_undefined_ff is None else n_undefined_ff.data_ptr()])
        return bool(rc)

    def stencil_levels_enqueue(self, op, f0, f1, xmapr, ymapr, fcoriolis, out0, out1=None, fdefined=None, undef=UNDEF, n_undefined=None):
        """Asynchronous form of stencil_levels on device tensors (mifc_stencil_levels_enqueue): nothing is read back;
        n_undefined: int64 CUDA tensor[nlev] (None allowed when every level is ALL_DEFINED).  The flag of level l is
        classify(n_undefined[l], stencil_count_domain(op, nx, ny)) once the stream has drained."""
        code = self.OPS[op]
        a0, a1 = _Arg(f0), _Arg(f1, allow_none=True)
        ax, ay, af = _Arg(xmapr), _Arg(ymapr), _Arg(fcoriolis, allow_none=True)
        o0, o1 = _Arg(out0, allow_none=True, output=True), _Arg(out1, allow_none=True, output=True)
        if len(a0.shape) != 3:
            raise ValueError("level fields must be (nlev, ny, nx)")
        nlev, ny, nx = a0.shape
        if not _same_shape([a1, o0, o1], a0.shape) or not _same_shape([ax, ay, af], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and the map / Coriolis fields (ny, nx)")
        if _memkind([a0, a1, ax, ay, af, o0, o1], self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        flags = None if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()
        self._bind_stream(MEM_DEVICE)
        rc = self._call("mifc_stencil_levels_enqueue", [code, nx, ny, nlev, a0.addr, a1.addr, ax.addr, ay.addr, af.addr, o0.addr, o1.addr,
                                                        flags, float(undef),
                                                        None if n_undefined is None else n_undefined.data_ptr()])
        return bool(rc)

    def last_stencil_form(self):
        """The kernel form this thread's last stencil launch took (mifc_last_stencil_form; a diagnostic for tests)."""
        return self._lib.mifc_last_stencil_form().decode()

    def last_host_chunks(self):
        """(number of chunks, levels per chunk) of this thread's last synchronous level-batch call from host memory; (0, 0) when
        the batch was staged whole (mifc_last_host_chunks; a diagnostic for tests)."""
        per_chunk = ctypes.c_int(0)
        nchunks = self._lib.mifc_last_host_chunks(ctypes.addressof(per_chunk))
        return int(nchunks), int(per_chunk.value)

    def last_pointwise_form(self):
        """The launch shape of this thread's last elementwise, catalogue or derived-batch launch as a dict
        (mifc_last_pointwise_form; a diagnostic for tests): family, form, inst as strings, the other keys as ints."""
        text = self._lib.mifc_last_pointwise_form().decode()
        form = dict(word.split("=", 1) for word in text.split())
        return {k: (v if k in ("family", "form", "inst") else int(v)) for k, v in form.items()}

    def stencil_count_domain(self, op, nx, ny):
        return int(self._lib.mifc_stencil_count_domain(self.OPS[op], nx, ny))

    def batch_level_stride(self, nx, ny):
        """Recommended distance (floats) between the levels of a device-resident batch (mifc_batch_level_stride)."""
        return int(self._lib.mifc_batch_level_stride(int(nx), int(ny)))

    def batch_empty(self, nlev, ny, nx, level_stride=None):
        """Uninitialised (nlev, ny, nx) float32 device batch whose levels are level_stride floats apart
        (default: batch_level_stride).  The padding between levels is never read or written."""
        import torch

        ls = self.batch_level_stride(nx, ny) if level_stride is None else int(level_stride)
        if ls < ny * nx or ls % 4 != 0:
            raise ValueError("level stride must be a multiple of 4 and at least ny*nx")
        base = torch.empty(nlev * ls, dtype=torch.float32, device=torch.device("cuda", self.device))
        return torch.as_strided(base, (nlev, ny, nx), (ls, nx, 1))

    def hlevel_derived_levels(self, u, v, t, q, ps, alevel, blevel, fdef_wind=None, fdef_thermo=None, undef=UNDEF,
                              want=("ff", "rh", "theta"), out=None):
        """Fused ff / RH(%) / theta on hybrid levels; u, v, t, q: (nlev, ny, nx), ps: (ny, nx).
        Returns ({name: array}, {name: flags}) or None."""
        ref = next(x for x in (u, t) if x is not None)
        nlev, ny, nx = _Arg(ref).shape
        out = dict(out or {})
        for k in want:
            if out.get(k) is None:
                out[k] = _empty_like(ref)
        a = {k: _Arg(x, allow_none=True) for k, x in dict(u=u, v=v, t=t, q=q, ps=ps).items()}
        o = {k: _Arg(out.get(k), allow_none=True) for k in ("ff", "rh", "theta")}
        if not _same_shape([a[k] for k in ("u", "v", "t", "q")] + list(o.values()), (nlev, ny, nx)) or not _same_shape([a["ps"]], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and ps (ny, nx)")
        mk = _memkind(list(a.values()) + list(o.values()), self.device)
        self._bind_stream(mk)
        al = np.ascontiguousarray(alevel if alevel is not None else np.zeros(nlev), dtype=np.float32).reshape(nlev)
        bl = np.ascontiguousarray(blevel if blevel is not None else np.ones(nlev), dtype=np.float32).reshape(nlev)
        fw = np.full(nlev, SOME_DEFINED, np.int32) if fdef_wind is None else np.array(fdef_wind, np.int32).reshape(nlev).copy()
        ft = np.full(nlev, SOME_DEFINED, np.int32) if fdef_thermo is None else np.array(fdef_thermo, np.int32).reshape(nlev).copy()
        fo = {k: np.full(nlev, -1, np.int32) for k in ("ff", "rh", "theta")}
        rc = self._call(
            "mifc_hlevel_derived_levels",
            [
                nx, ny, nlev, a["u"].addr, a["v"].addr, a["t"].addr, a["q"].addr, a["ps"].addr, al, bl,
                o["ff"].addr, o["rh"].addr, o["theta"].addr, fw, ft,
                fo["ff"].ctypes.data, fo["rh"].ctypes.data, fo["theta"].ctypes.data, float(undef), mk,
            ],
        )
        if not rc:
            return None
        res = {k: (out[k] if _is_torch(out[k]) else o[k].keep) for k in want}
        return res, {k: fo[k] for k in want}

    def hlevel_derived_batch(self, u, v, t, h, ps, alevel, blevel, temp=None, hum=None, hum2=None, ff=True, dd=False, fdef_wind=None,
                             fdef_thermo=None, undef=UNDEF, out=None, enqueue_counts=None):
        """The general fused derived batch (mifc_hlevel_derived_batch): per level any of
          ff   = vectorabs(u, v)                         (ff=True)
          temp = hleveltemp(t, ps, a, b, unit, compute)  (temp=(unit, compute))
          hum  = hlevelhum(t, h, ps, a, b, unit, compute)   (hum=(unit, compute))
          hum2 = a second hlevelhum variant of the same inputs (hum2=(unit, compute))
          dd   = wind direction from u, v (dd=True) -- EXTENSION, not a reference function
        u, v, t, h: (nlev, ny, nx); ps: (ny, nx).  out: optional dict of preallocated outputs.
        Returns ({name: array}, {name: flags}) or None.  With enqueue_counts (int64 CUDA tensor[5*nlev]) the call is
        asynchronous on device tensors and returns the outputs only (counts: ff | temp | hum | hum2 | dd)."""
        ref = next(x for x in (u, t) if x is not None)
        nlev, ny, nx = _Arg(ref).shape
        names = [k for k, w in (("ff", ff), ("temp", temp), ("hum", hum), ("hum2", hum2), ("dd", dd)) if w]
        out = dict(out or {})
        for k in names:
            if out.get(k) is None:
                out[k] = _empty_like(ref)
        a = {k: _Arg(x, allow_none=True) for k, x in dict(u=u, v=v, t=t, h=h, ps=ps).items()}
        o = {k: _Arg(out.get(k) if k in names else None, allow_none=True, output=True) for k in ("ff", "temp", "hum", "hum2", "dd")}
        if not _same_shape([a[k] for k in ("u", "v", "t", "h")] + list(o.values()), (nlev, ny, nx)) or not _same_shape([a["ps"]], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and ps (ny, nx)")
        mk = _memkind(list(a.values()) + list(o.values()), self.device)
        self._bind_stream(mk)
        al = np.ascontiguousarray(alevel if alevel is not None else np.zeros(nlev), dtype=np.float32).reshape(nlev)
        bl = np.ascontiguousarray(blevel if blevel is not None else np.ones(nlev), dtype=np.float32).reshape(nlev)
        fw = np.full(nlev, SOME_DEFINED, np.int32) if fdef_wind is None else np.array(fdef_wind, np.int32).reshape(nlev).copy()
        ft = np.full(nlev, SOME_DEFINED, np.int32) if fdef_thermo is None else np.array(fdef_thermo, np.int32).reshape(nlev).copy()
        unit = lambda w: (w[0] if w else "").encode()
        comp = lambda w: int(w[1]) if w else 0
        common = [nx, ny, nlev, a["u"].addr, a["v"].addr, a["t"].addr, a["h"].addr, a["ps"].addr, al, bl,
                  o["ff"].addr, o["temp"].addr, unit(temp), comp(temp), o["hum"].addr, unit(hum), comp(hum), o["hum2"].addr, unit(hum2), comp(hum2),
                  o["dd"].addr, fw, ft]
        if enqueue_counts is not None:
            if mk != MEM_DEVICE:
                raise ValueError("the *_enqueue calls take device tensors only")
            rc = self._call("mifc_hlevel_derived_batch_enqueue", common + [float(undef), enqueue_counts.data_ptr()])
            return {k: out[k] for k in names} if rc else None
        fo = {k: np.full(nlev, -1, np.int32) for k in ("ff", "temp", "hum", "hum2", "dd")}
        rc = self._call("mifc_hlevel_derived_batch", common + [fo[k].ctypes.data for k in ("ff", "temp", "hum", "hum2", "dd")] + [float(undef), mk])
        if not rc:
            return None
        res = {k: (out[k] if _is_torch(out[k]) else o[k].keep) for k in names}
        return res, {k: fo[k] for k in names}

    def hlevel_derived_levels_enqueue(self, u, v, t, q, ps, alevel, blevel, ff, rh, theta, n_undefined, fdef_wind=None,
                                      fdef_thermo=None, undef=UNDEF):
        ref = next(x for x in (u, t) if x is not None)
        nlev, ny, nx = _Arg(ref).shape
        a = [_Arg(x, allow_none=True) for x in (u, v, t, q, ps)]
        o = [_Arg(x, allow_none=True) for x in (ff, rh, theta)]
        al = np.ascontiguousarray(alevel, dtype=np.float32).reshape(nlev)
        bl = np.ascontiguousarray(blevel, dtype=np.float32).reshape(nlev)
        fw = None if fdef_wind is None else np.array(fdef_wind, np.int32).reshape(nlev).copy()
        ft = None if fdef_thermo is None else np.array(fdef_thermo, np.int32).reshape(nlev).copy()
        if not _same_shape(a[:4] + o, (nlev, ny, nx)) or not _same_shape([a[4]], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and ps (ny, nx)")
        if _memkind(a + o, self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        self._bind_stream(MEM_DEVICE)
        rc = self._call(
            "mifc_hlevel_derived_levels_enqueue",
            [nx, ny, nlev] + [x.addr for x in a] + [al, bl] + [x.addr for x in o]
            + [fw, ft, float(undef), n_undefined.data_ptr()],
        )
        return bool(rc)

    def vortdiv_slab_enqueue(self, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in=SOME_DEFINED,
                             undef=UNDEF, n_undefined=None, rows=None, accumulate=False):
        """Row-slab form (see include/mifc.h); all tensors on the device.  rows=(begin, end) restricts the
        launch to those owned rows (halo overlap); accumulate=True adds to n_undefined instead of zeroing it."""
        a = [_Arg(x, allow_none=True) for x in (u_halo, v_halo, xmapr, ymapr, rvort, diverg)]
        if not _same_shape(a[:2], (ny_local + 2, nx)) or not _same_shape(a[2:], (ny_local, nx)):
            raise ValueError("u_halo, v_halo must be (ny_local + 2, nx); xmapr, ymapr, rvort, diverg (ny_local, nx)")
        if _memkind(a, self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        self._bind_stream(MEM_DEVICE)
        r0, r1 = (0, int(ny_local)) if rows is None else (int(rows[0]), int(rows[1]))
        rc = self._call(
            "mifc_vortdiv_slab_rows_enqueue",
            [int(nx), int(ny_global), int(j0), int(ny_local), r0, r1] + [x.addr for x in a]
            + [int(fdefined_in), float(undef), None if n_undefined is None else n_undefined.data_ptr(), 1 if accumulate else 0],
        )
        return bool(rc)

    # ---- a sequence of *_enqueue calls as one launch (include/mifc.h: mifc_graph_*)
    def counts_accumulate(self, on=True):
        """The *_enqueue entries add to the counters they are given instead of zeroing them first (mifc_counts_accumulate)."""
        return bool(self._lib.mifc_counts_accumulate(self._ctx, 1 if on else 0))

    def zero_counts_enqueue(self, counts):
        """One asynchronous fill of an int64 CUDA tensor of counters (mifc_zero_counts_enqueue)."""
        self._bind_stream(MEM_DEVICE)
        return bool(self._call("mifc_zero_counts_enqueue", [counts.data_ptr(), counts.numel()]))

    def graph_capture(self, max_levels_per_call=0, lanes=1):
        """with ctx.graph_capture() as g: ... *_enqueue calls ...   ->  g.launch() replays them with one runtime call.
        lanes > 1: g.lane(k) before a call records it in lane k; calls in different lanes must be independent."""
        return Graph(self, max_levels_per_call, lanes)

    # ---- the decomposed step as one call (include/mifc.h: mifc_comm_*, mifc_slab_plan_*)
    def comm_unique_id(self):
        """mifc_comm_unique_id: the bytes rank 0 hands to every rank of a new communicator."""
        ident = ctypes.create_string_buffer(128)
        if not self._lib.mifc_comm_unique_id(ctypes.cast(ident, ctypes.c_void_p)):
            raise RuntimeError("mifc_comm_unique_id failed (RCCL not loadable?)")
        return ident.raw

    def comm_init(self, ident, rank, world):
        """mifc_comm_init: a communicator of the library's own for `world` processes, this one being `rank`."""
        buf = ctypes.create_string_buffer(bytes(ident), 128)
        if not self._call("mifc_comm_init", [ctypes.cast(buf, ctypes.c_void_p), int(rank), int(world)]):
            raise RuntimeError("mifc_comm_init: " + self.last_error())
        return True

    def comm_init_from_torch(self, group=None):
        """A communicator for the ranks of a torch.distributed group: rank 0's id is broadcast through the group."""
        import torch.distributed as dist

        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [self.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return self.comm_init(box[0], rank, world)

    def comm_adopt(self, nccl_comm_ptr):
        """Use an ncclComm_t the caller owns (an integer address, e.g. ProcessGroupNCCL._comm_ptr())."""
        return bool(self._call("mifc_comm_adopt", [int(nccl_comm_ptr)]))

    def comm_release(self):
        return bool(self._lib.mifc_comm_release(self._ctx))

    def comm_info(self):
        """(has a communicator, rank, world)"""
        r, w = ctypes.c_int(0), ctypes.c_int(1)
        has = self._lib.mifc_comm_info(self._ctx, ctypes.cast(ctypes.pointer(r), ctypes.c_void_p), ctypes.cast(ctypes.pointer(w), ctypes.c_void_p))
        return bool(has), r.value, w.value

    def slab_plan(self, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in=SOME_DEFINED, undef=UNDEF,
                  n_undefined=None):
        """mifc_slab_plan_create on device tensors: u_halo, v_halo (nlev, ny_local + 2, nx) or (ny_local + 2, nx); xmapr, ymapr
        (ny_local, nx); rvort, diverg (nlev, ny_local, nx) or (ny_local, nx); n_undefined int64[nlev].  -> SlabPlan"""
        return SlabPlan(self, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in, undef, n_undefined)

    def halo_copy_enqueue(self, dst, src_ctx, src):
        """dst (tensor on this context's device) <- src (tensor on src_ctx's device), see mifc_halo_copy_enqueue."""
        if dst.numel() != src.numel() or not dst.is_contiguous() or not src.is_contiguous():
            raise ValueError("halo rows must be contiguous and of equal length")
        return bool(self._call("mifc_halo_copy_enqueue", [dst.data_ptr(), src_ctx._ctx, src.data_ptr(), dst.numel()]))

    def diag_division(self, a, b, g, shared, plain):
        """Measurement build only (include/mifc_measure.h): arithmetic self-check; device tensors of equal length."""
        self._measure_entry("mifc_diag_division")
        self._bind_stream(MEM_DEVICE)
        return bool(self._call("mifc_diag_division", [a.data_ptr(), b.data_ptr(), g.data_ptr(), shared.data_ptr(), plain.data_ptr(), a.numel()]))

    def bench_stream2(self, variant, blocks, dst0, dst1, src0, src1):
        """Measurement build only (include/mifc_measure.h): bandwidth yardstick; device tensors."""
        self._measure_entry("mifc_bench_stream2")
        self._bind_stream(MEM_DEVICE)
        n = src0.numel()
        return bool(self._call("mifc_bench_stream2", [int(variant), int(blocks), dst0.data_ptr(), dst1.data_ptr(), src0.data_ptr(), src1.data_ptr(), n]))


class SlabPlan:
    """One rank's row slab of a horizontally decomposed level batch, bound to its buffers (mifc_slab_plan_*): step() enqueues
    the whole decomposed step -- RCCL halo exchange, interior rows meanwhile, boundary strips, count all-reduce -- as one
    call that replays a HIP graph; begin() / finish() bracket a halo exchange the caller does itself."""

    def __init__(self, ctx, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in, undef, n_undefined):
        a = [_Arg(x, allow_none=True) for x in (u_halo, v_halo, xmapr, ymapr, rvort, diverg)]
        nlev = u_halo.shape[0] if u_halo.dim() == 3 else 1
        halo_shape = (nlev, ny_local + 2, nx) if u_halo.dim() == 3 else (ny_local + 2, nx)
        out_shape = (nlev, ny_local, nx) if u_halo.dim() == 3 else (ny_local, nx)
        if not _same_shape(a[:2], halo_shape) or not _same_shape(a[2:4], (ny_local, nx)) or not _same_shape(a[4:], out_shape):
            raise ValueError("u_halo, v_halo must be ([nlev,] ny_local + 2, nx); xmapr, ymapr (ny_local, nx); rvort, diverg ([nlev,] ny_local, nx)")
        if _memkind(a, ctx.device) != MEM_DEVICE:
            raise ValueError("a slab plan takes device tensors only")
        if n_undefined is not None and n_undefined.numel() < nlev:
            raise ValueError("n_undefined needs one int64 per level")
        self._ctx, self._keep = ctx, (u_halo, v_halo, xmapr, ymapr, rvort, diverg, n_undefined)
        ctx._bind_stream(MEM_DEVICE)
        self._plan = ctx._lib.mifc_slab_plan_create(ctx._ctx, int(nx), int(ny_global), int(j0), int(ny_local), int(nlev), *[x.addr for x in a],
                                                    int(fdefined_in), float(undef), None if n_undefined is None else n_undefined.data_ptr())
        if not self._plan:
            raise RuntimeError("mifc_slab_plan_create: " + (ctx.last_error() or "invalid arguments"))

    def _run(self, name):
        self._ctx._bind_stream(MEM_DEVICE)
        if not getattr(self._ctx._lib, name)(self._plan):
            raise RuntimeError("%s: %s" % (name, self._ctx.last_error()))
        return True

    def step(self):
        return self._run("mifc_slab_plan_step")

    def begin(self):
        return self._run("mifc_slab_plan_begin")

    def finish(self):
        return self._run("mifc_slab_plan_finish")

    @property
    def uses_graph(self):
        return bool(self._ctx._lib.mifc_slab_plan_uses_graph(self._plan))

    def close(self):
        if self._plan:
            self._ctx._lib.mifc_slab_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Graph:
    """A recorded sequence of asynchronous calls (mifc_graph_begin / _end / _launch).  The tensors passed to the recorded
    calls must stay alive and in place for as long as the graph is launched: the graph holds their addresses."""

    def __init__(self, ctx, max_levels_per_call=0, lanes=1):
        self._ctx, self._graph, self._max, self._lanes = ctx, None, int(max_levels_per_call), int(lanes)

    def __enter__(self):
        self._ctx._bind_stream(MEM_DEVICE)
        self._ctx._frozen_stream = True  # the recorded calls must not re-bind the stream
        if not self._ctx._lib.mifc_graph_begin_lanes(self._ctx._ctx, self._max, self._lanes):
            self._ctx._frozen_stream = False
            raise RuntimeError("mifc_graph_begin: " + self._ctx.last_error())
        return self

    def __exit__(self, *exc):
        self._graph = self._ctx._lib.mifc_graph_end(self._ctx._ctx)
        self._ctx._frozen_stream = False
        if exc[0] is None and not self._graph:
            raise RuntimeError("mifc_graph_end: " + self._ctx.last_error())
        return False

    def lane(self, k):
        if not self._ctx._lib.mifc_graph_lane(self._ctx._ctx, int(k)):
            raise RuntimeError("mifc_graph_lane: " + self._ctx.last_error())

    def launch(self):
        self._ctx._bind_stream(MEM_DEVICE)
        if not self._ctx._lib.mifc_graph_launch(self._graph):
            raise RuntimeError("mifc_graph_launch: " + self._ctx.last_error())
        return True

    def close(self):
        if self._graph:
            self._ctx._lib.mifc_graph_destroy(self._graph)
            self._graph = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedCalls:
    """The C calls of a recorded wrapper sequence (Context.prepare), ready to be repeated: launch() is one ctypes call per
    recorded call, with the arguments converted once."""

    def __init__(self, ctx, recorded):
        self._ctx = ctx
        self._keep = [k for _, _, _, k in recorded]
        self._calls = []
        for name, fn, cargs, _ in recorded:
            conv = tuple(t(a) if a is not None else None for t, a in zip(fn.argtypes[1:], cargs))
            self._calls.append((name, fn, conv))
        self._ctxp = ctypes.c_void_p(ctx._ctx) if not isinstance(ctx._ctx, ctypes.c_void_p) else ctx._ctx

    def launch(self):
        c = self._ctxp
        for name, fn, cargs in self._calls:
            if not fn(c, *cargs):
                raise RuntimeError("%s: %s" % (name, self._ctx.last_error()))
        return True

    def __len__(self):
        return len(self._calls)
