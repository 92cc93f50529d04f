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

The package is split by family: this file holds the core of ``Context`` (lifetime, stream binding, the C call,
diagnostics), ``_reference`` the reference's 2-D functions, ``_levelbatch`` the level-batch extensions, ``_batched``
the batched stencil and derived entries with their asynchronous forms; ``_args`` has what they share and ``_consts``
the constants.
"""
import ctypes

import numpy as np

from . import _capi
from ._args import _Arg, _memkind, _parse_form
from ._batched import Graph, PreparedCalls, SlabPlan, _BatchedOps
from ._consts import MEM_DEVICE
from ._levelbatch import HstatsResult, _LevelBatchOps, ensemble_products  # noqa: F401  (re-exported)
from ._reference import _ReferenceOps

# the constants, re-exported (they live in a leaf module that the method families share)
from ._consts import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, MEM_HOST  # noqa: F401
from ._consts import ENS_SUM, ENS_MEAN, ENS_STDDEV, ENS_EXTREME, ENS_PROBABILITY  # noqa: F401
from ._consts import VLAYER_PRODUCTS, VDERIV_METHODS, HINTERP_METHODS, HSTATS_MODES, HSTATS_PRODUCTS  # noqa: F401

__all__ = ["Context", "SlabPlan", "Graph", "PreparedCalls", "HstatsResult", "ALL_DEFINED", "NONE_DEFINED", "SOME_DEFINED", "UNDEF", "classify",
           "ensemble_products"]


def classify(n_undefined, n):
    """miutil::checkDefined(size_t, size_t), FieldDefined.cc:62-70."""
    return _capi.lib().mifc_classify(int(n_undefined), int(n))


class Context(_ReferenceOps, _LevelBatchOps, _BatchedOps):
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
            for ref in self.__dict__.pop("_plans", ()):  # handles that belong to this context go first (hremap.Plan)
                plan = ref()
                if plan is not None:
                    plan.close()
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

    def _launch(self, name, fields, args, raises=True):
        """A synchronous field call: where its fields (_Arg) live decides the stream and is the last argument of the C entry.
        A refusal comes with its reason from _call; one without a reason raises RuntimeError too (the extension methods) or,
        with raises=False, gives False (the reference-style methods, which then return None)."""
        mk = _memkind(fields, self.device)
        self._bind_stream(mk)
        if self._call(name, args + [mk]):
            return True
        if raises:
            raise RuntimeError(name + ": " + self.last_error())
        return False

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

    # ------------------------------------------------------------ diagnostics for tests
    def last_hinterp_form(self):
        """The launch shape of this thread's last hinterp_levels call as a dict (mifc_last_hinterp_form; a diagnostic for
        tests): method as a string, the other keys as ints."""
        return _parse_form(self._lib.mifc_last_hinterp_form(), ("method",))

    def last_hstats_form(self):
        """The launch shape of this thread's last hstats_levels call as a dict (mifc_last_hstats_form; a diagnostic for
        tests): mode as a string, the other keys as ints."""
        return _parse_form(self._lib.mifc_last_hstats_form(), ("mode",))

    def last_ensemble_form(self):
        """The launch shape of this thread's last call of one of the five ensemble reductions, ensembleStatistics or
        ensembleQuantiles as a dict (mifc_last_ensemble_form; a diagnostic for tests): entry as a string ("single",
        "levels", "quantiles"), the other keys as ints."""
        return _parse_form(self._lib.mifc_last_ensemble_form(), ("entry",))

    def last_vrotate_form(self):
        """The launch shape of this thread's last vrotate_levels call as a dict of ints (mifc_last_vrotate_form; a diagnostic
        for tests)."""
        return _parse_form(self._lib.mifc_last_vrotate_form())

    def last_pointwise_form(self):
        """The launch shape of this thread's last elementwise, catalogue or derived-batch launch as a dict
        (mifc_last_pointwise_form; a diagnostic for tests): family, form, inst as strings, the other keys as ints."""
        return _parse_form(self._lib.mifc_last_pointwise_form(), ("family", "form", "inst"))

    def last_stencil_form(self):
        """The kernel form this thread's last stencil launch took (mifc_last_stencil_form; a diagnostic for tests)."""
        return self._lib.mifc_last_stencil_form().decode()

    def last_host_chunks(self):
        """(number of chunks, levels per chunk) of this thread's last synchronous level-batch call from host memory; (0, 0) when
        the batch was staged whole (mifc_last_host_chunks; a diagnostic for tests)."""
        per_chunk = ctypes.c_int(0)
        nchunks = self._lib.mifc_last_host_chunks(ctypes.addressof(per_chunk))
        return int(nchunks), int(per_chunk.value)

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

    # ------------------------------------------------------------ the measurement build (include/mifc_measure.h)
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
