"""The Python front's marshalling, pinned without a GPU and without libmifc.so.

A Context is built around a stub library whose every entry records the C call it is handed and returns 1.  Each case
below makes one wrapper call on small host arrays; the recorded calls -- pointers named by the test array they fall
into, pointer tables and mifc_ens_product lists decoded while they are alive, host value tables by dtype and values,
scalars as they are -- and a summary of what came back (or the exception) are compared with
tests/golden/python_front_calls.json.  That file also holds the signature and docstring digest of every public Context
method and the module's public names.

    python tests/test_python_front_cpu.py --record

rewrites the file from the code as it stands and stamps it with `git rev-parse HEAD`: it is meant to be run on the
commit whose behaviour is to be kept, before the wrapper is touched.  Device tensors cannot be driven here (_Arg
refuses torch tensors that are not on the GPU); tests/test_gpu_python_front.py covers that road.
"""
import ctypes
import hashlib
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "python_front_calls.json")
NLEV, NY, NX, NPOS, NT = 3, 4, 5, 7, 2
BATCH, PLANE = (NLEV, NY, NX), (NY, NX)
AL, BL, TG, LV = [0.0, 10.0, 20.0], [1.0, 0.5, 0.0], [50.0, 60.0], [100.0, 200.0, 300.0]


def _fc():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import mi_fieldcalc_amd as fc

    return fc


# ------------------------------------------------------------------------------------------------ the named arrays
def _data():
    shapes = {
        "F4": (4,) + BATCH, "F2": (2,) + BATCH, "B": BATCH, "V": BATCH, "T": BATCH, "Q": BATCH, "MINUS2": (2,) + BATCH, "MINUS1": BATCH,
        "COORD": BATCH, "P5": (2, 2) + BATCH, "MEM": (4,) + BATCH, "MEM2": (4,) + PLANE, "ICE": (11,) + BATCH,
        "PS": PLANE, "XM": PLANE, "YM": PLANE, "FCOR": PLANE, "COSA": PLANE, "SINA": PLANE, "W": PLANE, "LO": PLANE, "HI": PLANE, "DEPTH": PLANE,
        "XP": (NPOS,), "YP": (NPOS,), "COSP": (NPOS,), "SINP": (NPOS,),
        "OUT": (2 * 4 * NLEV * NY * NX,), "OUT2": (2 * 4 * NLEV * NY * NX,),
    }
    d = {k: (np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) % 17.0 + 1.0) for k, s in shapes.items()}
    d["OUT64"] = np.zeros(4 * NLEV * NY * 8, np.float64)
    return d


def _o(d, *shape, buf="OUT"):
    """An output of the given shape at the start of a named buffer."""
    return d[buf][: int(np.prod(shape))].reshape(shape)


class _Where:
    """Names a pointer by the test array it falls into."""

    def __init__(self, d):
        self.ranges = [(k, a.ctypes.data, a.nbytes) for k, a in d.items()]

    def add(self, name, a):
        self.ranges.append((name, a.ctypes.data, a.nbytes))

    def __call__(self, addr):
        if addr is None:
            return None
        for name, base, n in self.ranges:
            if base <= addr < base + max(n, 1):
                return [name, addr - base]
        return "<other>"


# --------------------------------------------------------------------- which arguments of an entry are host tables
# Positions count the arguments after the context.  (position, kind, length): kind "ptr" a table of pointers, "i32" /
# "f32" a table of values handed over as a bare address, "ens" the mifc_ens_product list; length from the other arguments.
def _at(i, scale=1, least=0):
    return lambda a: max(a[i] * scale, least)


_ONE = lambda a: 1  # noqa: E731
_FD = (-3, "i32", _ONE)  # the in/out flag of a 2-D call
SPEC = {
    "mifc_vinterp_hlevels": [(3, "ptr", _at(5)), (13, "ptr", _at(5))],
    "mifc_vinterp_fields": [(3, "ptr", _at(5)), (11, "ptr", _at(5))],
    "mifc_vlayer_hlevels": [(3, "ptr", _at(5)), (16, "ptr", _at(5))],
    "mifc_vlayer_fields": [(3, "ptr", _at(5)), (14, "ptr", _at(5))],
    "mifc_vderiv_hlevels": [(3, "ptr", _at(5)), (11, "ptr", _at(5)), (13, "ptr", lambda a: max(a[5] // 2, 1))],
    "mifc_vderiv_fields": [(3, "ptr", _at(5)), (9, "ptr", _at(5)), (11, "ptr", lambda a: max(a[5] // 2, 1))],
    "mifc_vderiv_levels": [(3, "ptr", _at(5)), (8, "ptr", _at(5)), (10, "ptr", lambda a: max(a[5] // 2, 1))],
    "mifc_hinterp_levels": [(3, "ptr", _at(5)), (10, "ptr", _at(5))],
    "mifc_hinterp_vector_levels": [(3, "ptr", _at(5, 2)), (13, "ptr", _at(5, 2))],
    "mifc_vrotate_levels": [(3, "ptr", _at(5, 2)), (9, "ptr", _at(5, 2))],
    "mifc_hstats_levels": [(3, "ptr", _at(5)), (6, "ptr", _at(5)), (15, "ptr", _at(5))],
    "mifc_ensembleQuantiles": [(4, "ptr", _at(6, least=1)), (9, "ptr", _at(8, least=1))],
    "mifc_ensemble_levels": [(3, "ptr", _at(5, least=1)), (6, "ens", _at(7))],
    "mifc_neighbour_levels": [(6, "f32", _at(7))],
    "mifc_vortdiv_levels": [(9, "i32", _at(2))],
    "mifc_stencil_levels": [(11, "i32", _at(3))],
    "mifc_stencil_levels_ex": [(10, "f32", _at(3)), (15, "i32", _at(3))],
    "mifc_hlevel_derived_levels": [(15, "i32", _at(2)), (16, "i32", _at(2)), (17, "i32", _at(2))],
    "mifc_hlevel_derived_batch": [(k, "i32", _at(2)) for k in range(23, 28)],
    "mifc_sumFields": [(2, "ptr", _at(3, least=1)), _FD],
    "mifc_meanValue": [(2, "ptr", _at(4, least=1)), (3, "i32", _at(4, least=1)), _FD],
    "mifc_probability": [(3, "ptr", _at(5, least=1)), (4, "i32", _at(5, least=1)), (6, "f32", _at(7)), _FD],
    "mifc_extremeValue": [(3, "ptr", _at(4, least=1)), _FD],
    "mifc_values2classes": [(4, "f32", _at(5)), _FD],
    "mifc_neighbourFunctions": [(3, "f32", _at(4)), _FD],
    "mifc_neighbourProbFunctions": [(3, "f32", _at(4)), _FD],
}
for _name in ("relvort", "fieldOPERfield", "constantOPERfield", "ilevelgwind", "pleveltemp", "vesselIcingMincog"):
    SPEC["mifc_" + _name] = [_FD]


class _Entry:
    def __init__(self, lib, name, capi):
        self.lib, self.name = lib, name
        sig = capi.SIGNATURES.get(name) or capi.MEASURE_SIGNATURES.get(name)
        self.kinds = sig[1] if sig else []
        self.argtypes = [capi._T[k] for k in self.kinds]

    def __call__(self, *cargs):
        return self.lib.record(self.name, self.kinds, cargs)


class _StubLib:
    """Every mifc_* attribute is an entry that records (name, normalised arguments) and returns `rc`."""

    def __init__(self, capi, where, rc=1):
        self.capi, self.where, self.rc, self.calls, self.np_args, self.tables_alive = capi, where, rc, [], {}, True

    def __getattr__(self, name):
        if not name.startswith("mifc_"):
            raise AttributeError(name)
        entry = self.__dict__[name] = _Entry(self, name, self.capi)
        return entry

    def _decode(self, kind, addr, n, args):
        if addr is None:
            return None
        if kind == "ptr":
            return [self.where(p) for p in (ctypes.c_void_p * n).from_address(addr)]
        if kind == "i32":
            return {"int32": list((ctypes.c_int * n).from_address(addr))}
        if kind == "f32":
            return {"float32": list((ctypes.c_float * n).from_address(addr))}
        assert kind == "ens"
        return [{"stat": p.stat, "compute": p.compute, "limits": list(p.limits)[: p.nlimits], "out": self.where(p.out),
                 "fdefined": list((ctypes.c_int * args[2]).from_address(p.fdefined))} for p in (self.capi.EnsProduct * n).from_address(addr)]

    def record(self, name, kinds, cargs):
        if name == "mifc_last_error":
            return b""
        vals = [v.value if isinstance(v, ctypes._SimpleCData) else v for v in cargs]
        has_ctx = bool(kinds) and kinds[0] == "ctx"
        args, kinds = (vals[1:], kinds[1:]) if has_ctx else (vals, kinds)
        tables = {pos % len(args): (kind, n) for pos, kind, n in SPEC.get(name, ())}
        out = []
        for i, v in enumerate(args):
            if i in self.np_args:
                a = self.np_args[i]
                assert v == a.ctypes.data
                out.append({"numpy": str(a.dtype), "shape": list(a.shape), "values": a.ravel().tolist()})
            elif i in tables and not self.tables_alive:
                out.append("<table>")
            elif i in tables:
                out.append(self._decode(tables[i][0], v, tables[i][1](args), args))
            elif i < len(kinds) and kinds[i] in ("p", "pi", "pu", "ctx"):
                out.append(self.where(v))
            elif isinstance(v, bytes):
                out.append("bytes:" + v.decode())
            else:
                out.append(v)
        self.calls.append([name, out])
        return self.rc


def _stub_context(d, rc=1):
    fc = _fc()
    lib = _StubLib(fc._capi, _Where(d), rc)
    ctx = fc.Context.__new__(fc.Context)
    ctx._recording, ctx._ctx, ctx.device, ctx._lib = None, 1, 0, lib

    def call(name, args):  # tells the stub which arguments were numpy tables before _call took their addresses
        lib.np_args = {i: a for i, a in enumerate(args) if isinstance(a, np.ndarray)}
        try:
            return fc.Context._call(ctx, name, args)
        finally:
            lib.np_args = {}

    ctx._call = call
    return ctx, lib


# ------------------------------------------------------------------------------------------------ what came back
def _arrays_in(x, found):
    if isinstance(x, np.ndarray):
        found.add(id(x))
    elif isinstance(x, (tuple, list)):
        for y in x:
            _arrays_in(y, found)
    elif isinstance(x, dict):
        for y in x.values():
            _arrays_in(y, found)
    return found


def _summary(x, given, where, fill):
    if isinstance(x, np.ndarray):
        s = {"dtype": str(x.dtype), "shape": list(x.shape), "at": where(x.ctypes.data) if x.size else None, "is_given": id(x) in given}
        if x.dtype == np.int32:
            s["values"] = x.ravel().tolist()
        elif fill and x.size:
            s["fill"] = float(x.flat[0]) if bool((x == x.flat[0]).all()) else None
        return s
    if isinstance(x, (np.integer, np.floating)):
        return x.item()
    if isinstance(x, (tuple, list)):
        return [type(x).__name__] + [_summary(y, given, where, fill) for y in x]
    if isinstance(x, dict):
        return {k: _summary(y, given, where, fill) for k, y in x.items()}
    if type(x).__name__ == "HstatsResult":
        return {"HstatsResult": {k: _summary(getattr(x, k), given, where, fill) for k in ("stats", "pivot", "mean_batch", "mean_flags")}}
    return x


# ------------------------------------------------------------------------------------------------------ the cases
CASES = []


def case(ident, method, build, rc0=False, fill=False):
    """build(d) -> (args, kwargs) of ctx.<method>.  rc0: run it once more against a library whose entry returns 0."""
    CASES.append((ident, method, build, 1, fill))
    if rc0:
        CASES.append((ident + "@refused", method, build, 0, fill))


def _pairs_layouts(d):
    p = d["P5"]
    return {"one": p[0], "stacked": p, "tuples": [(p[0, 0], p[0, 1]), (p[1, 0], p[1, 1])], "flat": [p[0, 0], p[0, 1], p[1, 0], p[1, 1]],
            "flat_one": [p[1, 0], p[1, 1]]}


_PAIR_FLAGS = {"one": [0, 2], "stacked": [[0, 2], [2, 2]], "tuples": [[[0, 1, 2], [2, 2, 2]], [[0, 0, 0], [2, 0, 2]]], "flat": None,
               "flat_one": [[0, 2, 2], [2, 2, 0]]}
_FULL2 = [[0, 1, 2], [2, 2, 0]]

# --- the reference's 2-D operators: one per shape of _single, the ensemble functions, the neighbour functions
case("relvort", "relvort", lambda d: ((d["B"][0], d["V"][0], d["XM"], d["YM"]), dict(out=_o(d, NY, NX))), rc0=True)
case("relvort_alloc", "relvort", lambda d: ((d["B"][0], d["V"][0], d["XM"], d["YM"]), dict(fdefined=0, undef=-1.0)))
case("relvort_not_2d", "relvort", lambda d: ((d["B"], d["V"], d["XM"], d["YM"]), {}))
case("relvort_shapes_differ", "relvort", lambda d: ((d["B"][0], d["V"][0], d["XM"], d["XP"]), {}))
case("fieldOPERfield", "fieldOPERfield", lambda d: ((2, d["B"][0], d["V"][0]), dict(out=_o(d, NY, NX))))
case("constantOPERfield", "constantOPERfield", lambda d: ((3, 2.5, d["B"][1]), dict(out=_o(d, NY, NX))))
case("values2classes", "values2classes", lambda d: ((d["B"][0], [1.0, 5.0, 9.0]), dict(out=_o(d, NY, NX))))
case("ilevelgwind", "ilevelgwind", lambda d: ((d["B"][0], d["XM"], d["YM"], d["FCOR"]), dict(out=(_o(d, NY, NX), _o(d, NY, NX, buf="OUT2")))))
case("ilevelgwind_alloc", "ilevelgwind", lambda d: ((d["B"][0], d["XM"], d["YM"], d["FCOR"]), {}))
case("pleveltemp", "pleveltemp", lambda d: ((d["B"][0], 850.0, "celsius", 3), dict(out=_o(d, NY, NX))))
case("vesselIcingMincog", "vesselIcingMincog", lambda d: (tuple(d["ICE"][k, 0] for k in range(11)) + (5.0, 0.5, 1.0, 9.0, 2), dict(out=_o(d, NY, NX))))
case("sumFields", "sumFields", lambda d: (([d["MEM2"][0], d["MEM2"][2]],), dict(out=_o(d, NY, NX))), rc0=True)
case("meanValue", "meanValue", lambda d: (([d["MEM2"][k] for k in range(4)], [0, 2, 2, 0]), dict(out=_o(d, NY, NX))))
case("meanValue_no_members", "meanValue", lambda d: (([], []), dict(out=_o(d, NY, NX))))
case("extremeValue_alloc", "extremeValue", lambda d: ((1, [d["MEM2"][1], d["MEM2"][3]]), {}))
case("probability", "probability", lambda d: ((3, [d["MEM2"][0], d["MEM2"][1]], [2, 0], [2.0, 8.0]), dict(out=_o(d, NY, NX))))
case("err_ensemble_nothing", "sumFields", lambda d: (([],), {}))
case("neighbourFunctions", "neighbourFunctions", lambda d: ((d["B"][0], [50.0, 1, 2], 4), dict(out=_o(d, NY, NX))))
case("neighbourFunctions_alloc", "neighbourFunctions", lambda d: ((d["B"][0], [1], 1), dict(undef=-7.0)), fill=True)
case("neighbourProbFunctions_alloc", "neighbourProbFunctions", lambda d: ((d["B"][0], [3.0, 1], 5), {}), rc0=True, fill=True)

# --- vinterp
case("vinterp_h_one", "vinterp_hlevels", lambda d: ((d["B"], d["PS"], AL, BL, TG), dict(out=_o(d, NT, NY, NX))), rc0=True)
case("vinterp_h_stack_flags_per_field", "vinterp_hlevels",
     lambda d: ((d["F2"], d["PS"], AL, BL, TG), dict(method="log", fdefined_in=[0, 2], fdef_ps=0, undef=-9.0, out=_o(d, 2, NT, NY, NX))))
case("vinterp_h_list_flags_full", "vinterp_hlevels",
     lambda d: (([d["F4"][0], d["F4"][2]], d["PS"], AL, BL, TG), dict(fdefined_in=_FULL2, out=_o(d, 2, NT, NY, NX))))
case("vinterp_h_alloc", "vinterp_hlevels", lambda d: ((d["F4"], d["PS"], AL, BL, [70.0]), dict(method="cubic")))
case("vinterp_f_one", "vinterp_fields", lambda d: ((d["B"], d["COORD"], TG), dict(fdef_coord=[0, 2, 0], out=_o(d, NT, NY, NX))), rc0=True)
case("vinterp_f_stack", "vinterp_fields", lambda d: ((d["F2"], d["COORD"], TG), dict(method=1, fdefined_in=[2, 2], out=_o(d, 2, NT, NY, NX))))
case("vinterp_f_alloc", "vinterp_fields", lambda d: ((d["B"], d["COORD"], TG), {}))
case("err_vinterp_h_coord", "vinterp_hlevels", lambda d: ((d["B"], d["COORD"], AL, BL, TG), {}))
case("err_vinterp_f_coord", "vinterp_fields", lambda d: ((d["B"], d["PS"], TG), {}))
case("err_vinterp_out_shape", "vinterp_hlevels", lambda d: ((d["F2"], d["PS"], AL, BL, TG), dict(out=_o(d, NT, NY, NX))))
case("err_vinterp_out_dtype", "vinterp_hlevels", lambda d: ((d["B"], d["PS"], AL, BL, TG), dict(out=np.zeros((NT, NY, NX), np.float64))))
case("err_vinterp_levels", "vinterp_hlevels", lambda d: ((d["B"], d["PS"], AL[:2], BL, TG), {}))
case("err_vinterp_fdef_coord", "vinterp_fields", lambda d: ((d["B"], d["COORD"], TG), dict(fdef_coord=[0, 2])))
case("err_batches_none", "vinterp_fields", lambda d: (([], d["COORD"], TG), {}))
case("err_batches_not_3d", "vinterp_fields", lambda d: ((d["PS"], d["COORD"], TG), {}))
case("err_batches_differ", "vinterp_fields", lambda d: (([d["B"], d["F2"][0][:2]], d["COORD"], TG), {}))

# --- vlayer
case("vlayer_h_one_scalar_bounds", "vlayer_hlevels", lambda d: ((d["B"], d["PS"], AL, BL, ["integral", "mean"], 10.0, 90.0), dict(out=_o(d, 2, NY, NX))),
     rc0=True)
case("vlayer_h_stack_field_bounds", "vlayer_hlevels",
     lambda d: ((d["F2"], d["PS"], AL, BL, "max"), dict(lo=d["LO"], hi=d["HI"], fdefined_in=[2, 0], fdef_ps=0, out=_o(d, 2, 1, NY, NX))))
case("vlayer_f_stack_mixed_bounds", "vlayer_fields",
     lambda d: ((d["F2"], d["COORD"], [3, "coord_of_min", "nonsense"]), dict(lo=d["LO"], fdefined_in=_FULL2, fdef_coord=[2, 2, 0], out=_o(d, 2, 3, NY, NX))))
case("vlayer_f_one_open", "vlayer_fields", lambda d: ((d["B"], d["COORD"], 2), dict(out=_o(d, 1, NY, NX))), rc0=True)
case("vlayer_h_alloc", "vlayer_hlevels", lambda d: ((d["F2"], d["PS"], AL, BL, ["min", "max"]), {}))
case("vlayer_f_alloc", "vlayer_fields", lambda d: ((d["B"], d["COORD"], "integral"), dict(hi=d["HI"])))
case("err_vlayer_bound", "vlayer_fields", lambda d: ((d["B"], d["COORD"], "mean"), dict(lo=d["XP"])))
case("err_vlayer_out_shape", "vlayer_hlevels", lambda d: ((d["B"], d["PS"], AL, BL, ["mean"]), dict(out=_o(d, 2, NY, NX))))
case("err_vlayer_coord", "vlayer_hlevels", lambda d: ((d["B"], d["XP"], AL, BL, ["mean"]), {}))

# --- vderiv: the three coordinate kinds, every magnitude
_VDERIV = {"h": ("vderiv_hlevels", lambda d: (d["PS"], AL, BL)), "f": ("vderiv_fields", lambda d: (d["COORD"],)), "l": ("vderiv_levels", lambda d: (LV,))}
for _k, (_m, _coord) in _VDERIV.items():
    case("vderiv_%s_stack_none" % _k, _m, lambda d, c=_coord: ((d["F2"],) + c(d), dict(fdefined_in=[0, 2], out=_o(d, 2, *BATCH))), rc0=True)
    case("vderiv_%s_stack_also" % _k, _m, lambda d, c=_coord: ((d["F4"],) + c(d), dict(method="weighted", magnitude="also", fdefined_in=[_FULL2[0]] * 4,
                                                                                     out=(_o(d, 4, *BATCH), _o(d, 2, *BATCH, buf="OUT2")))))
    case("vderiv_%s_stack_only" % _k, _m, lambda d, c=_coord: ((d["F2"],) + c(d), dict(magnitude="only", out=_o(d, 1, *BATCH, buf="OUT2"))))
    case("vderiv_%s_one_none" % _k, _m, lambda d, c=_coord: ((d["B"],) + c(d), dict(method=7, out=_o(d, *BATCH))))
    case("vderiv_%s_alloc_also" % _k, _m, lambda d, c=_coord: (([d["B"], d["V"]],) + c(d), dict(magnitude="also")))
case("vderiv_l_one_also_no_pair", "vderiv_levels", lambda d: ((d["B"], LV), dict(magnitude="also", out=_o(d, *BATCH))))
case("vderiv_f_also_out_alone", "vderiv_fields", lambda d: ((d["F2"], d["COORD"]), dict(magnitude="also", fdef_coord=[0, 0, 2], out=_o(d, 2, *BATCH))))
case("vderiv_h_alloc_only", "vderiv_hlevels", lambda d: ((d["F2"], d["PS"], AL, BL), dict(magnitude="only", fdef_ps=0)))
case("vderiv_l_alloc_none", "vderiv_levels", lambda d: ((d["B"], LV), {}))
case("err_vderiv_magnitude", "vderiv_levels", lambda d: ((d["F2"], LV), dict(magnitude="too")))
case("err_vderiv_levels", "vderiv_levels", lambda d: ((d["F2"], LV[:2]), {}))
case("err_vderiv_out_count", "vderiv_levels", lambda d: ((d["F2"], LV), dict(out=(_o(d, 2, *BATCH), _o(d, 1, *BATCH, buf="OUT2")))))
case("err_vderiv_out_shape", "vderiv_fields", lambda d: ((d["F2"], d["COORD"]), dict(out=_o(d, *BATCH))))
case("err_vderiv_mag_shape", "vderiv_fields", lambda d: ((d["F2"], d["COORD"]), dict(magnitude="only", out=_o(d, 2, *BATCH))))
case("err_vderiv_coord", "vderiv_hlevels", lambda d: ((d["F2"], d["COORD"], AL, BL), {}))

# --- hinterp
case("hinterp_one", "hinterp_levels", lambda d: ((d["B"], d["XP"], d["YP"]), dict(out=_o(d, NLEV, NPOS))), rc0=True)
case("hinterp_stack_flags_per_field", "hinterp_levels",
     lambda d: ((d["F2"], d["XP"], d["YP"]), dict(method="bicubic", fdefined_in=[2, 0], undef=-3.0, out=_o(d, 2, NLEV, NPOS))))
case("hinterp_list_flags_full_2d_positions", "hinterp_levels",
     lambda d: (([d["F4"][1], d["F4"][3]], d["XP"].reshape(NPOS, 1), d["YP"].reshape(NPOS, 1)), dict(method=0, fdefined_in=_FULL2, out=_o(d, 2, NLEV, NPOS, 1))))
case("hinterp_alloc", "hinterp_levels", lambda d: ((d["F2"], d["XP"], d["YP"]), dict(method="spline")))
case("hinterp_alloc_one", "hinterp_levels", lambda d: ((d["B"], d["XP"], d["YP"]), {}))
case("err_hinterp_positions", "hinterp_levels", lambda d: ((d["B"], d["XP"], d["YP"][:3]), {}))
case("err_hinterp_out_shape", "hinterp_levels", lambda d: ((d["B"], d["XP"], d["YP"]), dict(out=_o(d, 1, NLEV, NPOS))))

# --- the pair methods: every layout of `pairs`
for _lay in ("one", "stacked", "tuples", "flat", "flat_one"):
    _np = 1 if _lay in ("one", "flat_one") else 2
    _lead = (2,) if _np == 1 else (2, 2)
    case("vrotate_" + _lay, "vrotate_levels", lambda d, l=_lay, s=_lead: (
        (_pairs_layouts(d)[l], d["COSA"], d["SINA"]), dict(fdefined_in=_PAIR_FLAGS[l], out=_o(d, *(s + BATCH)))), rc0=_lay == "one")
    case("hinterp_vector_" + _lay, "hinterp_vector_levels", lambda d, l=_lay, s=_lead: (
        (_pairs_layouts(d)[l], d["XP"], d["YP"], d["COSP"], d["SINP"]), dict(fdefined_in=_PAIR_FLAGS[l], out=_o(d, *(s + (NLEV, NPOS))))), rc0=_lay == "one")
case("vrotate_alloc", "vrotate_levels", lambda d: ((d["P5"], d["COSA"], d["SINA"]), dict(fdef_rot=0, undef=-2.0)))
case("vrotate_alloc_one", "vrotate_levels", lambda d: ((d["P5"][1], d["COSA"], d["SINA"]), {}))
case("hinterp_vector_alloc", "hinterp_vector_levels", lambda d: ((d["P5"], d["XP"], d["YP"], d["COSP"], d["SINP"]), dict(method="nearest", fdef_rot=0)))
case("hinterp_vector_alloc_one", "hinterp_vector_levels", lambda d: ((d["P5"][0], d["XP"], d["YP"], d["COSP"], d["SINP"]), dict(method=2)))
case("err_vrotate_rotation", "vrotate_levels", lambda d: ((d["P5"], d["COSA"], d["XP"]), {}))
case("err_vrotate_out_shape", "vrotate_levels", lambda d: ((d["P5"], d["COSA"], d["SINA"]), dict(out=_o(d, 2, *BATCH))))
case("err_pairs_rank", "vrotate_levels", lambda d: ((d["B"], d["COSA"], d["SINA"]), {}))
case("err_pairs_triple", "vrotate_levels", lambda d: (([(d["B"], d["V"], d["T"])], d["COSA"], d["SINA"]), {}))
case("err_pairs_odd", "vrotate_levels", lambda d: (([d["B"], d["V"], d["T"]], d["COSA"], d["SINA"]), {}))
case("err_pairs_none", "hinterp_vector_levels", lambda d: (([], d["XP"], d["YP"], d["COSP"], d["SINP"]), {}))
case("err_hinterp_vector_positions", "hinterp_vector_levels", lambda d: ((d["P5"], d["XP"], d["YP"], d["COSP"], d["SINA"]), {}))
case("err_hinterp_vector_out_shape", "hinterp_vector_levels", lambda d: ((d["P5"], d["XP"], d["YP"], d["COSP"], d["SINP"]), dict(out=_o(d, 2, NLEV, NPOS))))

# --- hstats
case("hstats_area_one", "hstats_levels", lambda d: ((d["B"],), dict(out=_o(d, NLEV, 1, 8, buf="OUT64"))), rc0=True)
case("hstats_area_stack_everything", "hstats_levels", lambda d: ((d["F2"],), dict(
    minus=d["MINUS2"], pivot=2.5, weight=d["W"], box=(1, 4, 0, 3), want_mean=True, fdefined_in=[0, 2], fdefined_minus=_FULL2, fdef_weight=0, undef=-5.0,
    out=_o(d, 2, NLEV, 1, 8, buf="OUT64"))))
case("hstats_rows_box", "hstats_levels", lambda d: ((d["F2"],), dict(mode="rows", box=[0, 5, 1, 3], products="moments", pivot=[[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]],
                                                                     out=_o(d, 2, NLEV, 2, 8, buf="OUT64"))))
case("hstats_rows_one_minus_mean", "hstats_levels", lambda d: ((d["B"],), dict(mode=1, minus=d["MINUS1"], products=3, want_mean=True, pivot=[1.0, 2.0, 3.0],
                                                                               out=_o(d, 1, NLEV, NY, 8, buf="OUT64"))))
case("hstats_list_weight", "hstats_levels", lambda d: (([d["B"], d["V"]],), dict(minus=[d["T"], d["Q"]], weight=d["W"], products=("extremes", "other"), mode="columns")))
case("hstats_alloc_rows_mean", "hstats_levels", lambda d: ((d["F2"],), dict(mode="rows", want_mean=True)))
case("hstats_alloc_one", "hstats_levels", lambda d: ((d["B"],), dict(pivot=1.0)))
case("err_hstats_minus", "hstats_levels", lambda d: ((d["F2"],), dict(minus=d["MINUS1"])))
case("err_hstats_weight", "hstats_levels", lambda d: ((d["F2"],), dict(weight=d["XP"])))
case("err_hstats_box", "hstats_levels", lambda d: ((d["F2"],), dict(box=(0, 1, 2))))
case("err_hstats_out_dtype", "hstats_levels", lambda d: ((d["B"],), dict(out=_o(d, NLEV, 1, 8))))
case("err_hstats_out_shape", "hstats_levels", lambda d: ((d["F2"],), dict(out=_o(d, NLEV, 1, 8, buf="OUT64"))))

# --- the ensemble extensions
case("quantiles_levels_stacked", "ensembleQuantiles", lambda d: ((d["MEM"], [10.0, 50.0]), dict(fdefined_in=[0, 2, 2, 0], method="linear", out=_o(d, 2, *BATCH))),
     rc0=True)
case("quantiles_2d_list", "ensembleQuantiles", lambda d: (([d["MEM2"][k] for k in (0, 2, 3)], 50.0), dict(undef=-4.0, out=_o(d, 1, NY, NX))))
case("quantiles_flags_full", "ensembleQuantiles", lambda d: (([d["MEM"][0], d["MEM"][1]], [25.0, 75.0, 100.0]), dict(fdefined_in=_FULL2, method=5, out=_o(d, 3, *BATCH))))
case("quantiles_no_members", "ensembleQuantiles", lambda d: (([], 50.0), dict(out=_o(d, 1, NY, NX))))
case("quantiles_alloc", "ensembleQuantiles", lambda d: ((d["MEM"], [10.0, 90.0]), dict(method="nearest")))
case("quantiles_alloc_2d", "ensembleQuantiles", lambda d: ((d["MEM2"], 50.0), {}))
case("err_quantiles_out_shape", "ensembleQuantiles", lambda d: ((d["MEM"], [10.0, 50.0]), dict(out=_o(d, 1, *BATCH))))
case("err_quantiles_nothing", "ensembleQuantiles", lambda d: (([], 50.0), {}))
case("err_members_rank", "ensembleQuantiles", lambda d: (([d["XP"], d["YP"]], 50.0), {}))
case("err_members_differ", "ensembleQuantiles", lambda d: (([d["MEM2"][0], d["B"]], 50.0), {}))
_PRODUCTS = ["mean", ("sum", 0), ("max", [0, 2, 2]), ("probability", 1, [3.0]), ("extreme", 2), ("probability", 6, (2.0, 8.0)), "stddev"]
case("statistics_levels_stacked", "ensembleStatistics", lambda d: ((d["MEM"], _PRODUCTS), dict(fdefined_in=[0, 2, 2, 0], out=_o(d, 7, *BATCH))), rc0=True)
case("statistics_2d_out_list", "ensembleStatistics", lambda d: (([d["MEM2"][1], d["MEM2"][2]], ["sum", "argmin"]),
                                                               dict(undef=-6.0, out=[_o(d, NY, NX), _o(d, NY, NX, buf="OUT2")])))
case("statistics_flags_full", "ensembleStatistics", lambda d: (([d["MEM"][2], d["MEM"][3]], [("mean",), ("min", 0)]), dict(fdefined_in=_FULL2, out=_o(d, 2, *BATCH))))
case("statistics_no_members", "ensembleStatistics", lambda d: (([], ["mean"]), dict(out=[_o(d, NY, NX)])))
case("statistics_alloc", "ensembleStatistics", lambda d: ((d["MEM"], ["mean", "max"]), {}))
case("statistics_alloc_2d", "ensembleStatistics", lambda d: ((d["MEM2"], ["stddev"]), {}))
case("err_statistics_out_count", "ensembleStatistics", lambda d: ((d["MEM"], ["mean", "max"]), dict(out=_o(d, 1, *BATCH))))
case("err_statistics_out_shape", "ensembleStatistics", lambda d: ((d["MEM"], ["mean", "max"]), dict(out=[_o(d, *BATCH), _o(d, NY, NX, buf="OUT2")])))
case("err_statistics_unknown", "ensembleStatistics", lambda d: ((d["MEM"], ["median"]), {}))
case("err_statistics_no_products", "ensembleStatistics", lambda d: ((d["MEM"], []), {}))
case("err_statistics_twice", "ensembleStatistics", lambda d: ((d["MEM"], ["mean", "mean"]), {}))

# --- neighbour and icing batches
case("neighbour_levels_prob", "neighbour_levels", lambda d: (("prob", 5, d["B"], [3.0, 1]), dict(out=_o(d, *BATCH))), rc0=True)
case("neighbour_levels_functions_flags", "neighbour_levels", lambda d: (("functions", 4, d["B"], [50.0, 1, 2]), dict(fdefined=[0, 2, 0], undef=-8.0, out=_o(d, *BATCH))))
case("neighbour_levels_alloc", "neighbour_levels", lambda d: (("functions", 1, d["B"], [1]), dict(undef=-8.0)), fill=True)
case("err_neighbour_which", "neighbour_levels", lambda d: (("both", 1, d["B"], [1]), {}))
case("err_neighbour_rank", "neighbour_levels", lambda d: (("prob", 5, d["PS"], [3.0, 1]), {}))
case("err_neighbour_out_shape", "neighbour_levels", lambda d: (("prob", 5, d["B"], [3.0, 1]), dict(out=_o(d, NY, NX))))
case("icing_levels_modstall", "vesselIcing_levels", lambda d: (("modstall", d["ICE"], 5.0, 0.5, 1.0, 9.0), dict(out=_o(d, *BATCH))), rc0=True)
case("icing_levels_mincog_shared_depth", "vesselIcing_levels",
     lambda d: (("mincog", [d["ICE"][k] for k in range(9)] + [d["PS"], d["DEPTH"]], 5.0, 0.5, 1.0, 9.0), dict(alt=2, fdefined=[0, 2, 2], undef=-1.5, out=_o(d, *BATCH))))
case("icing_levels_alloc", "vesselIcing_levels", lambda d: (("mincog", [d["DEPTH"]] + [d["ICE"][k] for k in range(1, 11)], 5.0, 0.5, 1.0, 9.0), {}))
case("err_icing_model", "vesselIcing_levels", lambda d: (("overland", d["ICE"], 5.0, 0.5, 1.0, 9.0), {}))
case("err_icing_count", "vesselIcing_levels", lambda d: (("mincog", d["ICE"][:10], 5.0, 0.5, 1.0, 9.0), {}))
case("err_icing_no_batch", "vesselIcing_levels", lambda d: (("mincog", [d["DEPTH"]] * 11, 5.0, 0.5, 1.0, 9.0), {}))
case("err_icing_input_shape", "vesselIcing_levels", lambda d: (("mincog", [d["ICE"][k] for k in range(10)] + [d["XP"]], 5.0, 0.5, 1.0, 9.0), {}))
case("err_icing_out_shape", "vesselIcing_levels", lambda d: (("mincog", d["ICE"], 5.0, 0.5, 1.0, 9.0), dict(out=_o(d, NY, NX))))

# --- the batched stencil and derived methods
_WIND = lambda d: (d["B"], d["V"], d["XM"], d["YM"])  # noqa: E731
case("vortdiv_levels", "vortdiv_levels", lambda d: (_WIND(d), dict(rvort=_o(d, *BATCH), diverg=_o(d, *BATCH, buf="OUT2"))), rc0=True)
case("vortdiv_levels_rvort_only_flags", "vortdiv_levels", lambda d: (_WIND(d), dict(fdefined=[0, 2, 0], undef=-2.0, rvort=_o(d, *BATCH), want=("rvort",))))
case("vortdiv_levels_alloc", "vortdiv_levels", lambda d: (_WIND(d), {}))
case("vortdiv_levels_alloc_diverg_only", "vortdiv_levels", lambda d: (_WIND(d), dict(want=("diverg",))))
case("err_vortdiv_rank", "vortdiv_levels", lambda d: ((d["PS"], d["PS"], d["XM"], d["YM"]), {}))
case("err_vortdiv_shapes", "vortdiv_levels", lambda d: ((d["B"], d["V"], d["XM"], d["XP"]), {}))
case("stencil_levels_relvort", "stencil_levels", lambda d: (("relvort",) + _WIND(d), dict(out0=_o(d, *BATCH))), rc0=True)
case("stencil_levels_vortdiv_flags", "stencil_levels", lambda d: (("vortdiv",) + _WIND(d), dict(fdefined=[2, 0, 2], undef=-2.0, out0=_o(d, *BATCH),
                                                                                              out1=_o(d, *BATCH, buf="OUT2"))))
case("stencil_levels_absvort", "stencil_levels", lambda d: (("absvort",) + _WIND(d), dict(fcoriolis=d["FCOR"], out0=_o(d, *BATCH), out1=_o(d, *BATCH, buf="OUT2"))))
case("stencil_levels_gradient", "stencil_levels", lambda d: (("gradient1", d["B"], None, d["XM"], d["YM"]), dict(out0=_o(d, *BATCH))))
case("stencil_levels_alloc_two", "stencil_levels", lambda d: (("ilevelgwind", d["B"], None, d["XM"], d["YM"], d["FCOR"]), {}))
case("stencil_levels_alloc", "stencil_levels", lambda d: (("jacobian",) + _WIND(d), {}))
case("err_stencil_levels_shapes", "stencil_levels", lambda d: (("relvort", d["B"], d["V"], d["XM"], d["XP"]), {}))
case("err_stencil_levels_rank", "stencil_levels", lambda d: (("relvort", d["PS"], d["PS"], d["XM"], d["YM"]), {}))
case("stencil_levels_ex_advection", "stencil_levels_ex", lambda d: (("advection", d["T"], d["B"], d["V"], d["XM"], d["YM"]), dict(scalar=6.0, out0=_o(d, *BATCH))),
     rc0=True)
case("stencil_levels_ex_qvector", "stencil_levels_ex", lambda d: (("plevelqvector", d["B"], d["T"]), dict(
    xmapr=d["XM"], ymapr=d["YM"], fcoriolis=d["FCOR"], level_scalars=[850.0, 700.0, 500.0], compute=3, fdefined=[0, 0, 2], undef=-2.0, out0=_o(d, *BATCH))))
case("stencil_levels_ex_shapiro_alloc", "stencil_levels_ex", lambda d: (("shapiro2_filter", d["B"]), {}))
case("err_stencil_levels_ex_rank", "stencil_levels_ex", lambda d: (("shapiro2_filter", d["PS"]), {}))
case("err_stencil_levels_ex_shapes", "stencil_levels_ex", lambda d: (("advection", d["T"], d["B"], d["V"], d["XM"], d["XP"]), {}))
_HYB = lambda d: (d["B"], d["V"], d["T"], d["Q"], d["PS"], AL, BL)  # noqa: E731
case("derived_levels", "hlevel_derived_levels", lambda d: (_HYB(d), dict(out={"ff": _o(d, *BATCH), "rh": _o(d, *BATCH, buf="OUT2")})), rc0=True)
case("derived_levels_subset_flags", "hlevel_derived_levels", lambda d: ((None, None, d["T"], d["Q"], d["PS"], None, None), dict(
    fdef_wind=[0, 0, 0], fdef_thermo=[2, 0, 2], undef=-2.0, want=("theta",), out={"theta": _o(d, *BATCH)})))
case("derived_levels_alloc", "hlevel_derived_levels", lambda d: (_HYB(d), {}))
case("err_derived_levels_shapes", "hlevel_derived_levels", lambda d: ((d["B"], d["V"], d["T"], d["Q"], d["XP"], AL, BL), {}))
case("derived_batch", "hlevel_derived_batch", lambda d: (_HYB(d), dict(temp=("celsius", 2), hum=("percent", 1), hum2=("kg/kg", 4), dd=True, fdef_wind=[0, 2, 0],
                                                                        fdef_thermo=[2, 2, 0], undef=-2.0, out={"ff": _o(d, *BATCH), "dd": _o(d, *BATCH, buf="OUT2")})),
     rc0=True)
case("derived_batch_ff_only", "hlevel_derived_batch", lambda d: ((d["B"], d["V"], None, None, d["PS"], None, None), dict(out={"ff": _o(d, *BATCH)})))
case("derived_batch_alloc", "hlevel_derived_batch", lambda d: (_HYB(d), dict(ff=False, temp=("kelvin", 1))))
case("err_derived_batch_shapes", "hlevel_derived_batch", lambda d: ((d["B"], d["V"], d["T"], d["Q"], d["XP"], AL, BL), {}))
case("err_derived_batch_enqueue_host", "hlevel_derived_batch", lambda d: (_HYB(d), dict(enqueue_counts=object())))

# --- the *_enqueue methods refuse host arrays after their shape checks; their device road is for the GPU test
case("err_vortdiv_enqueue_host", "vortdiv_levels_enqueue", lambda d: (_WIND(d) + (_o(d, *BATCH), None), {}))
case("err_vortdiv_enqueue_rank", "vortdiv_levels_enqueue", lambda d: ((d["PS"], d["PS"], d["XM"], d["YM"], None, None), {}))
case("err_vortdiv_enqueue_shapes", "vortdiv_levels_enqueue", lambda d: (_WIND(d) + (_o(d, NY, NX), None), {}))
case("err_vortdiv_ff_enqueue_host", "vortdiv_ff_levels_enqueue", lambda d: (_WIND(d) + (_o(d, *BATCH), _o(d, *BATCH, buf="OUT2"), d["T"]), {}))
case("err_stencil_enqueue_host", "stencil_levels_enqueue", lambda d: (("relvort",) + _WIND(d) + (None, _o(d, *BATCH)), {}))
case("err_stencil_enqueue_shapes", "stencil_levels_enqueue", lambda d: (("relvort",) + _WIND(d) + (None, _o(d, NY, NX)), {}))
case("err_derived_enqueue_host", "hlevel_derived_levels_enqueue", lambda d: (_HYB(d) + (_o(d, *BATCH), None, None, None), {}))
case("err_slab_enqueue_shapes", "vortdiv_slab_enqueue", lambda d: ((NX, NY, 0, NY, d["PS"], d["PS"], d["XM"], d["YM"], None, None), {}))

IDS = [c[0] for c in CASES]
assert len(set(IDS)) == len(IDS)


def _run(ident, method, build, rc, fill, d):
    ctx, lib = _stub_context(d, rc)
    args, kwargs = build(d)
    given = _arrays_in((args, kwargs), set())
    try:
        outcome = {"result": _summary(getattr(ctx, method)(*args, **kwargs), given, lib.where, fill)}
    except (ValueError, RuntimeError) as e:
        outcome = {"raises": type(e).__name__, "message": str(e)}
    outcome["calls"] = lib.calls
    ctx._ctx = None  # nothing to destroy
    return outcome


def _run_prepare(d):
    """prepare() around two wrapper calls: the recorded tuples (the kept-alive tables among them) and the replayed calls."""
    ctx, lib = _stub_context(d)
    prepared = ctx.prepare(lambda: (ctx.vinterp_hlevels(d["F2"], d["PS"], AL, BL, TG, fdefined_in=[0, 2], out=_o(d, 2, NT, NY, NX)),
                                    ctx.vortdiv_levels(d["B"], d["V"], d["XM"], d["YM"], rvort=_o(d, *BATCH), diverg=_o(d, *BATCH, buf="OUT2"))))
    direct, lib.calls = lib.calls, []
    keep = []
    for k, tables in enumerate(prepared._keep):
        keep.append([{"numpy": str(a.dtype), "shape": list(a.shape), "values": a.ravel().tolist()} for a in tables])
        for j, a in enumerate(tables):
            lib.where.add("keep%d.%d" % (k, j), a)
    assert ctx._recording is None
    lib.tables_alive = False  # prepare() keeps the numpy tables alive, not the ctypes pointer tables of the extension methods
    prepared.launch()
    ctx._ctx = None  # nothing to destroy
    return {"direct": direct, "len": len(prepared), "keep": keep, "replayed": lib.calls}


def _surface():
    fc = _fc()
    methods = {}
    for name, member in inspect.getmembers(fc.Context):
        if not name.startswith("_") and callable(member):
            methods[name] = {"signature": str(inspect.signature(member)), "doc": hashlib.sha1((inspect.getdoc(member) or "").encode()).hexdigest()}
    names = sorted(n for n in dir(fc) if not n.startswith("_") and not inspect.ismodule(getattr(fc, n)))
    tables = {n: getattr(fc, n) for n in ("VLAYER_PRODUCTS", "VDERIV_METHODS", "HINTERP_METHODS", "HSTATS_MODES", "HSTATS_PRODUCTS")}
    values = {n: float(getattr(fc, n)) for n in names if isinstance(getattr(fc, n), (int, np.float32))}
    return {"methods": methods, "public_names": names, "all": list(fc.__all__), "OPS": fc.Context.OPS, "OPS_EX": fc.Context.OPS_EX, "tables": tables,
            "values": values, "class_docs": {n: hashlib.sha1((inspect.getdoc(getattr(fc, n)) or "").encode()).hexdigest()
                                             for n in ("Context", "SlabPlan", "Graph", "PreparedCalls", "HstatsResult", "classify", "ensemble_products")}}


def _plain(x):
    return json.loads(json.dumps(x))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def data():
    return _data()


def test_every_case_is_in_the_golden_file(golden):
    assert sorted(golden["cases"]) == sorted(IDS)
    assert len(golden["parent"]) == 40


@pytest.mark.parametrize("ident,method,build,rc,fill", CASES, ids=IDS)
def test_call_is_marshalled_as_recorded(golden, data, ident, method, build, rc, fill):
    got, want = _plain(_run(ident, method, build, rc, fill, data)), golden["cases"][ident]
    if ident.startswith("err_"):
        assert got.get("raises") == "ValueError", got
    assert got.get("raises") == want.get("raises") and got.get("message") == want.get("message")
    assert len(got["calls"]) == len(want["calls"]), [c[0] for c in got["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g[0] == w[0]
        for k, (ga, wa) in enumerate(zip(g[1], w[1])):
            assert ga == wa, "%s argument %d" % (g[0], k)
        assert len(g[1]) == len(w[1])
    assert got.get("result") == want.get("result")


def test_prepare_records_and_replays_the_same_calls(golden, data):
    assert _plain(_run_prepare(data)) == golden["prepare"]


def test_public_surface_is_unchanged(golden):
    got, want = _plain(_surface()), golden["surface"]
    assert sorted(got["methods"]) == sorted(want["methods"])
    for name in want["methods"]:
        assert got["methods"][name] == want["methods"][name], name
    for key in want:
        assert got[key] == want[key], key
    fc = _fc()
    for name in ("ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, MEM_HOST, MEM_DEVICE, ENS_SUM, ENS_MEAN, ENS_STDDEV, ENS_EXTREME, ENS_PROBABILITY, "
                 "VLAYER_PRODUCTS, VDERIV_METHODS, HINTERP_METHODS, HSTATS_MODES, HSTATS_PRODUCTS, Context, SlabPlan, Graph, PreparedCalls, HstatsResult, "
                 "classify, ensemble_products").split(", "):
        assert hasattr(fc, name), name


def test_no_module_of_the_package_imports_the_package_back():
    """The modules below __init__ import each other and never the package itself: `from . import x` names a module file."""
    import ast

    pkg = os.path.join(ROOT, "mi-fieldcalc_amd")
    modules = {f[:-3] for f in os.listdir(pkg) if f.endswith(".py") and f != "__init__.py"}
    for m in sorted(modules):
        for node in ast.walk(ast.parse(open(os.path.join(pkg, m + ".py")).read())):
            if isinstance(node, ast.ImportFrom):
                assert node.level <= 1 and (node.module or "").split(".")[0] != "mi_fieldcalc_amd", (m, node.lineno)
                if node.level == 1 and node.module is None:
                    assert {a.name for a in node.names} <= modules, (m, node.lineno)
            elif isinstance(node, ast.Import):
                assert all(a.name.split(".")[0] != "mi_fieldcalc_amd" for a in node.names), (m, node.lineno)


def record():
    d = _data()
    parent = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    doc = {"parent": parent, "cases": {c[0]: _run(*c, d) for c in CASES}, "prepare": _run_prepare(d), "surface": _surface()}
    with open(GOLDEN, "w") as f:
        json.dump(_plain(doc), f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("%d cases recorded from %s into %s (%d bytes)" % (len(CASES), parent, GOLDEN, os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    if "--record" in sys.argv[1:]:
        record()
    else:
        sys.exit("usage: python tests/test_python_front_cpu.py --record")
