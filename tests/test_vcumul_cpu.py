"""CPU checks of mifc_vcumul_hlevels / mifc_vcumul_fields / mifc_vcumul_levels: the semantics through their numpy
restatement (tests/vcumul_restate.py, the oracle of the GPU tests) on hand-worked columns, the restatement against the
sibling definition of the layer integral, the constants of the header against the Python front, that the entries are
declared, bound and configured where the others are, and the front's marshalling against a recording stub library."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import vcumul_restate as vc
import vlayer_restate as vl
from test_python_front_cpu import _data, _stub_context

U = vc.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, S_, N = vc.ALL_DEFINED, vc.SOME_DEFINED, vc.NONE_DEFINED


def column(coord, values, method=vc.LINEAR, from_=vc.FROM_FIRST, fdef_coord=None, start=None, base=None, **kw):
    """One column (ny = nx = 1), one or several fields: returns (out[nf][nlev], flags[nf][nlev])."""
    v = np.atleast_2d(np.asarray(values, np.float32))
    c = np.asarray(coord, np.float32)
    if start is not None:
        kw["start"] = np.full((1, 1), start, np.float32)
    if base is not None:
        kw["base"] = [None if b is None else np.full((1, 1), b, np.float32) for b in np.atleast_1d(np.asarray(base, object))]
    out, fd = vc.coord_fields(v[:, :, None, None], c[:, None, None], method, from_, fdef_coord=fdef_coord, **kw)
    return out[:, :, 0, 0], fd


def f32(*xs):
    return [np.float32(x) for x in xs]


def test_two_levels():
    out, fd = column([100, 300], [1, 5])
    assert list(out[0]) == f32(0, 3 * 200) and (fd == A).all()
    out, fd = column([100, 300], [1, 5], from_="last")
    assert list(out[0]) == f32(3 * -200, 0) and (fd == A).all()  # the integral is signed: walked downward in the coordinate
    assert np.signbit(column([100, 300], [-1, 5])[0][0, 0]) == False  # noqa: E712  (S starts at +0.0)


def test_three_uneven_levels_scale_and_base():
    out, _ = column([100, 200, 400], [[1, 3, 9], [2, 2, 2]], scale=[0.5, -1.0], base=[10, None])
    assert list(out[0]) == f32(10, 10 + 0.5 * 200, 10 + 0.5 * (200 + 1200)) and list(out[1]) == f32(-0.0, -200, -600)
    assert np.signbit(out[1, 0])  # no base: the product alone, -1 * +0


def test_start_given_and_not_given():
    out, _ = column([100, 200, 400], [1, 3, 9], start=50)
    assert list(out[0]) == f32(50, 50 + 200, 50 + 200 + 1200)  # x_0 held constant from 50 to 100
    out, _ = column([100, 200, 400], [1, 3, 9], start=450, from_="last")
    assert list(out[0]) == f32(-450 - 1200 - 200, -450 - 1200, 9 * -50)
    out, fd = column([100, 200, 400], [1, 3, 9], start=U)  # the start must be usable: every level undef
    assert (out == U).all() and (fd == N).all()
    out, fd = column([100, 200, 400], [1, 3, 9], start=U, fdef_start=A)  # ... a stored undef under ALL_DEFINED is a value
    assert out[0, 0] == np.float32(np.float64(100) - np.float64(U)) and (fd == A).all()
    out, fd = column([100, 200, 400], [1, 3, 9], start=np.nan, fdef_start=A)  # ... a NaN never is
    assert (out == U).all() and (fd == N).all()
    out, _ = column([100, 200, 400], [-1, 3, 9], start=100)  # x * 0 keeps the sign of x: S = -0.0
    assert np.signbit(out[0, 0]) and out[0, 0] == 0


def test_a_hole_in_the_middle_in_both_directions():
    c, x = [100, 200, 400, 500, 700], [1, 3, U, 4, 8]
    out, fd = column(c, x)
    assert list(out[0]) == f32(0, 200, U, U, U) and list(fd[0]) == [A, A, N, N, N]
    out, fd = column(c, x, from_=vc.FROM_LAST)
    assert list(out[0]) == f32(U, U, U, 6 * -200, 0) and list(fd[0]) == [N, N, N, A, A]
    # per field: the other field of the call walks on
    out, fd = column(c, [x, [1, 1, 1, 1, 1]])
    assert list(out[1]) == f32(0, 100, 300, 400, 600) and (fd[1] == A).all()
    # a hole at the first walked level: nothing is left
    assert (column(c, [U, 3, 2, 4, 8])[0] == U).all() and (column(c, [1, 3, 2, 4, U], from_="last")[0] == U).all()
    # under ALL_DEFINED the stored undef is a value
    out, fd = column(c, x, flags=[[S_, S_, A, S_, S_]])
    assert out[0, 2] == np.float32(200 + ((3 + np.float64(U)) * 0.5) * 200) and (fd == A).all()


def test_base_undef():
    out, fd = column([100, 200], [[1, 3], [1, 3]], base=[U, 7])
    assert (out[0] == U).all() and list(out[1]) == f32(7, 207) and list(fd[0]) == [N, N] and list(fd[1]) == [A, A]
    out, fd = column([100, 200], [[1, 3], [1, 3]], base=[U, np.nan], fdef_base=[A, A])
    assert list(out[0]) == f32(U, np.float32(np.float64(U) + 200)) and (fd[0] == A).all() and (out[1] == U).all() and (fd[1] == N).all()


def test_log_and_a_coordinate_that_is_not_positive():
    out, fd = column([100, 200, 400], [2, 2, 4], "log")
    l = np.log(np.array([100, 200, 400], np.float64))
    e1 = (np.float64(4) * 0.5) * (l[1] - l[0])
    assert list(out[0]) == f32(0, e1, e1 + (np.float64(6) * 0.5) * (l[2] - l[1])) and (fd == A).all()
    for bad in (0.0, -0.0, -3.0):
        out, fd = column([100, bad, 400], [2, 2, 4], vc.LOG)
        assert list(out[0]) == f32(0, U, U) and list(fd[0]) == [A, N, N]
        out, fd = column([100, bad, 400], [2, 2, 4], vc.LINEAR)
        assert (out != U).all() and (fd == A).all()
    out, fd = column([100, 200, 400], [2, 2, 4], "log", start=0.0)
    assert (out == U).all() and (fd == N).all()
    out, _ = column([100, 200], [2, 2], "log", start=400, scale=-1.0, base=5)  # upward from the surface: height grows
    assert list(out[0]) == f32(5 + -1.0 * (2 * (l[0] - l[2])), 5 + -1.0 * (2 * (l[0] - l[2]) + 2 * (l[1] - l[0])))


def test_a_non_monotone_column():
    out, fd = column([100, 300, 200, 200, 500], [1, 3, 5, 7, 1])
    assert list(out[0]) == f32(0, 400, 400 - 400, 0, 1200) and (fd == A).all()


def test_a_nan_coordinate_through_an_all_defined_flag():
    for fc in (None, [A] * 4):
        out, fd = column([100, 200, np.nan, 400], [1, 3, 5, 7], fdef_coord=fc)
        assert list(out[0]) == f32(0, 200, U, U) and list(fd[0]) == [A, A, N, N]
    out, fd = column([100, 200, U, 400], [1, 3, 5, 7], fdef_coord=[S_, S_, A, S_])  # a stored undef under ALL_DEFINED is a coordinate
    assert out[0, 2] == np.float32(200 + 4.0 * (np.float64(U) - 200)) and (fd == A).all()
    # an undefined ps: every level of that cell, no other cell
    x = np.arange(1, 7, dtype=np.float32).reshape(1, 3, 1, 2)
    al, bl = vc.hybrid_levels(3)
    out, fd = vc.hlevels(x, np.array([[1000, U]], np.float32), al, bl)
    assert (out[0, :, 0, 1] == U).all() and (out[0, :, 0, 0] != U).all() and (fd == S_).all()


def test_nan_as_undef_and_flags_per_level():
    nan = np.float32(np.nan)
    out, fd = column([100, 200, 400], [1, 3, nan], undef=nan)
    assert list(out[0, :2]) == f32(0, 200) and np.isnan(out[0, 2]) and list(fd[0]) == [A, A, N]
    x = np.ones((1, 3, 1, 3), np.float32)
    x[0, 1, 0, 1] = U
    out, fd = vc.levels(x, [10, 20, 40])
    assert list(fd[0]) == [A, S_, S_] and list(out[0, :, 0, 1]) == f32(0, U, U) and list(out[0, :, 0, 0]) == f32(0, 10, 30)
    # a result that happens to equal undef, or is not finite, is a value: not counted
    out, fd = column([0, 1], [U, U], flags=[[A, A]])
    assert out[0, 1] == U and (fd == A).all()
    out, fd = column([0, 1], [np.inf, 1], flags=[[A, A]])
    assert np.isinf(out[0, 1]) and (fd == A).all()


@pytest.mark.parametrize("kind", ["hybrid", "field"])
def test_last_level_is_the_layer_integral_of_the_sibling_definition(kind):
    """Strictly ascending coordinate, everything defined, from the first level, no start, base or scale: the same additions
    in the same order as vlayer_restate's INTEGRAL over the open layer -- bit for bit."""
    fields, ps, alevel, blevel = vc.main_case(3, 12, 9, 13, 5, frac=0.0)
    if kind == "hybrid":
        out, fd = vc.hlevels(fields, ps, alevel, blevel)
        exp, efd = vl.hlevels(fields, ps, alevel, blevel, [vl.INTEGRAL])
    else:
        coord = vc.hybrid_coordinate(ps, alevel, blevel)
        assert (np.diff(coord, axis=0) > 0).all()
        out, fd = vc.coord_fields(fields, coord)
        exp, efd = vl.coord_fields(fields, coord, [vl.INTEGRAL])
    assert out[:, -1].tobytes() == exp[:, 0].tobytes() and (fd == A).all() and (efd == A).all()
    assert (out[:, -1] != 0).all()


def test_main_generator_reaches_holes_starts_and_bases():
    fields, ps, ab, coord, starts, base = vc.cumul_case()
    for from_ in (vc.FROM_FIRST, vc.FROM_LAST):
        out, fd = vc.coord_fields(fields, coord, vc.LOG, from_, start=starts[from_], base=list(base), scale=[1.0, -2.0, 0.5])
        defined = (out != U).mean(axis=(0, 2, 3))
        print("from", from_, "defined per level", np.round(defined, 3))
        assert 0.2 < defined.min() < defined.max() < 1 and (fd == S_).all()
        first, last = (0, -1) if from_ == vc.FROM_FIRST else (-1, 0)
        assert defined[first] > defined[last] + 0.1  # holes accumulate along the walk


def test_header_constants_and_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi
    from mi_fieldcalc_amd import vcumul

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_vcumul_hlevels", "mifc_vcumul_fields", "mifc_vcumul_levels", "mifc_last_vcumul_form"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert [len(capi.SIGNATURES["mifc_vcumul_" + k][1]) for k in ("hlevels", "fields", "levels")] == [22, 20, 19]
    enums = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bMIFC_VCUMUL_([A-Z_]+) = (\d+)\b", header)}
    assert enums == {"LINEAR": 0, "LOG": 1, "FROM_FIRST": 0, "FROM_LAST": 1}
    assert vcumul.VCUMUL_METHODS == {"linear": enums["LINEAR"], "log": enums["LOG"]} == vc.METHODS
    assert vcumul.VCUMUL_FROM == {"first": enums["FROM_FIRST"], "last": enums["FROM_LAST"]} == vc.FROM
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(csrc, "*"))) if '"MIFC_VCUMUL_CHUNK_MIB"' in open(p, errors="replace").read()]
    assert readers == ["mifc_env.hip"], readers
    host = open(os.path.join(csrc, "mifc_capi_vcumul.hip")).read()
    assert "getenv" not in host and re.search(r"vcumul_chunk_mib > 0 \? mifc::env\(\)\.vcumul_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_vcumul.hip") == 1 and makefile.count("mifc_capi_vcumul.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    kernel = open(os.path.join(csrc, "mifc_vcumul.hip")).read()
    assert kernel.count("__global__") == 1  # one kernel for both directions


# ------------------------------------------------------------------------------- the front against a recording stub
B = 3 * 4 * 5 * 4  # bytes of a batch of the stub's arrays


def _tables(lib, args, nf, at_fields, at_base, at_scale, at_fres):
    """The host tables of the last recorded call, decoded from the raw arguments the stub was handed."""
    ptrs = lambda addr: None if addr is None else [lib.where(p) for p in (ctypes.c_void_p * nf).from_address(addr)]  # noqa: E731
    scale = None if args[at_scale] is None else list((ctypes.c_double * nf).from_address(args[at_scale]))
    return ptrs(args[at_fields]), ptrs(args[at_base]), scale, ptrs(args[at_fres])


class _Raw:
    """Wraps the stub library: keeps the raw C arguments of every entry call before the stub normalises them."""

    def __init__(self, lib):
        self.lib, self.raw, self.seen = lib, [], {}

    def __getattr__(self, name):
        entry = getattr(self.lib, name)

        def call(*cargs):
            vals = [v.value if isinstance(v, ctypes._SimpleCData) else v for v in cargs]
            self.raw.append((name, vals[1:]))
            if name.startswith("mifc_vcumul_"):
                self.seen = self.decode(name, vals[1:])
            return entry(*cargs)

        return call

    def decode(self, name, a):
        nf = a[5]
        tail = {"mifc_vcumul_hlevels": 10, "mifc_vcumul_fields": 8, "mifc_vcumul_levels": 7}[name]  # where `method` sits
        fields, base, scale, fres = _tables(self.lib, a, nf, 3, tail + 4, tail + 6, tail + 7)
        fdb = None if a[tail + 5] is None else list((ctypes.c_int * nf).from_address(a[tail + 5]))
        floats = lambda addr: list((ctypes.c_float * a[2]).from_address(addr))  # noqa: E731  (the tables live as long as the call)
        more = {"fdefined_in": None if a[4] is None else list((ctypes.c_int * (nf * a[2])).from_address(a[4]))}
        if name == "mifc_vcumul_hlevels":
            more.update(fdef_ps=a[7], alevel=floats(a[8]), blevel=floats(a[9]))
        elif name == "mifc_vcumul_fields":
            more.update(fdef_coord=None if a[7] is None else list((ctypes.c_int * a[2]).from_address(a[7])))
        else:
            more.update(levels=floats(a[6]))
        return {"head": a[:3] + [nf], "fields": fields, "coord": a[6] if name.endswith("levels") and "hlevels" not in name else self.lib.where(a[6]),
                "method": a[tail], "from": a[tail + 1], "start": self.lib.where(a[tail + 2]), "fdef_start": a[tail + 3], "base": base,
                "fdef_base": fdb, "scale": scale, "fres": fres, "undef": a[tail + 9], "memkind": a[tail + 10], "nargs": len(a), **more}


def _front(rc=1):
    from mi_fieldcalc_amd import vcumul

    d = _data()
    ctx, lib = _stub_context(d, rc)
    raw = _Raw(lib)
    ctx._lib = raw
    return vcumul, d, ctx, raw


def test_front_marshals_the_hybrid_form_in_header_order():
    vcumul, d, ctx, raw = _front()
    out, fd = vcumul.vcumul_hlevels(ctx, d["F2"], d["PS"], [0.0, 10.0, 20.0], [1.0, 0.5, 0.0], "log", "last", start=d["XM"], base=[d["LO"], None],
                                    scale=[2.0, -3.0], fdef_ps=A, fdef_start=A, fdef_base=[A, S_], fdefined_in=[A, S_])
    s = raw.seen
    assert s["head"] == [5, 4, 3, 2] and s["fields"] == [["F2", 0], ["F2", B]] and s["coord"] == ["PS", 0]
    assert s["method"] == 1 and s["from"] == 1 and s["start"] == ["XM", 0] and s["fdef_start"] == A
    assert s["base"] == [["LO", 0], None] and s["fdef_base"] == [A, S_] and s["scale"] == [2.0, -3.0]
    assert s["undef"] == float(U) and s["memkind"] == 0 and s["nargs"] == 21
    assert raw.raw[-1][0] == "mifc_vcumul_hlevels" and s["fdef_ps"] == A and s["alevel"] == [0.0, 10.0, 20.0] and s["blevel"] == [1.0, 0.5, 0.0]
    assert s["fdefined_in"] == [A, A, A, S_, S_, S_]  # one flag per field stands for every level
    assert out.shape == (2, 3, 4, 5) and out.dtype == np.float32 and fd.shape == (2, 3) and fd.dtype == np.int32
    assert s["fres"] == [lib_at(out, 0, raw), lib_at(out, B, raw)]


def lib_at(arr, off, raw):
    return raw.lib.where(arr.ctypes.data + off)


def test_front_keeps_null_tables_null_and_honours_out():
    vcumul, d, ctx, raw = _front()
    o = d["OUT"][: 3 * 4 * 5].reshape(3, 4, 5)
    out, fd = vcumul.vcumul_fields(ctx, d["B"], d["COORD"], out=o)
    s = raw.seen
    assert out is o and fd.shape == (3,) and s["fres"] == [["OUT", 0]] and s["fields"] == [["B", 0]] and s["coord"] == ["COORD", 0]
    assert s["method"] == 0 and s["from"] == 0 and s["start"] is None and s["fdef_start"] == S_
    assert s["base"] is None and s["fdef_base"] is None and s["scale"] is None and s["nargs"] == 19
    assert s["fdefined_in"] is None and s["fdef_coord"] is None
    # ONE batch: the base may be the plane itself; one scale stands for every field
    out, fd = vcumul.vcumul_levels(ctx, d["B"], [100.0, 200.0, 300.0], base=d["HI"], scale=0.25, from_=vc.FROM_LAST, method=vc.LOG)
    s = raw.seen
    assert s["base"] == [["HI", 0]] and s["scale"] == [0.25] and s["from"] == 1 and s["method"] == 1 and s["nargs"] == 18 and out.shape == (3, 4, 5)
    assert s["levels"] == [100.0, 200.0, 300.0]
    out, fd = vcumul.vcumul_fields(ctx, [d["B"], d["V"], d["T"]], d["COORD"], base=np.stack([d["LO"], d["HI"], d["W"]]), fdef_base=A)
    assert raw.seen["fdef_base"] == [A, A, A] and raw.seen["base"] == ["<other>"] * 3  # (the planes of the stacked copy)
    with pytest.raises(ValueError, match="out must have shape"):
        vcumul.vcumul_fields(ctx, d["F2"], d["COORD"], out=o)
    with pytest.raises(ValueError, match="one plane"):
        vcumul.vcumul_fields(ctx, d["F2"], d["COORD"], base=[d["LO"]])
    with pytest.raises(ValueError, match="start must have the shape"):
        vcumul.vcumul_fields(ctx, d["F2"], d["COORD"], start=d["COORD"])


def test_geopotential_height_forms_tv_and_calls_the_hybrid_entry():
    vcumul, d, ctx, raw = _front()
    from mi_fieldcalc_amd._consts import GRAVITY, R_DRY

    seen = {}
    launch = ctx._launch

    def spy(name, fields, args, raises=True):
        seen["tv"] = fields[0].keep.copy()
        return launch(name, fields, args, raises)

    ctx._launch = spy
    t, q = d["T"] + 250, d["Q"] / 1000
    t[1, 2, 3] = U
    z, fd = vcumul.geopotential_height_hlevels(ctx, t, q, d["PS"], [0.0, 10.0, 20.0], [1.0, 0.5, 0.0], zs=d["DEPTH"])
    s = raw.seen
    assert s["method"] == vc.LOG and s["from"] == vc.FROM_LAST and s["start"] == ["PS", 0] and s["coord"] == ["PS", 0] and s["base"] == [["DEPTH", 0]]
    assert s["scale"] == [-R_DRY / GRAVITY] and z.shape == (3, 4, 5) and fd.shape == (3,)
    with np.errstate(over="ignore"):
        e = (t * (1 + np.float32(0.608) * q)).astype(np.float32)
    e[1, 2, 3] = U
    assert seen["tv"].tobytes() == e.tobytes()
    vcumul.geopotential_height_hlevels(ctx, t, None, d["PS"], [0.0, 10.0, 20.0], [1.0, 0.5, 0.0], surface_last=False)
    assert raw.seen["from"] == vc.FROM_FIRST and raw.seen["base"] is None and seen["tv"].tobytes() == t.tobytes()


def test_a_refused_call_raises_value_error_with_the_librarys_message():
    vcumul, d, ctx, raw = _front(rc=0)
    raw.lib.__dict__["mifc_last_error"] = lambda c: b"mifc_vcumul_fields: scale[1] is NaN"
    with pytest.raises(ValueError, match=r"mifc_vcumul_fields: scale\[1\] is NaN") as info:
        vcumul.vcumul_fields(ctx, d["F2"], d["COORD"], scale=[1.0, np.nan])
    assert isinstance(info.value, RuntimeError)  # what the Context methods raise for a refusal is caught by the same handler
    with pytest.raises(ValueError, match="every field must have the shape"):
        vcumul.vcumul_fields(ctx, [d["B"], d["PS"]], d["COORD"])
