"""CPU checks of mifc_hremap_*: the semantics through their numpy restatement (tests/hremap_restate.py, the oracle of the
GPU tests) on hand-worked rows, the row and value seams, an independent scalar loop, the conservative weights of
hremap.conservative_weights_regular, the CSR conversion of Plan.from_coo, the plan header (validation, Wall, the
sliced-ELL layout) compiled with the host compiler -- through a shim and, under the address and undefined-behaviour
sanitizers, as a stand-alone program --, that the entries are declared, bound and configured where the others are, and the
front's marshalling against a recording stub library."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hremap_restate as hr
import test_python_front_cpu as front
from mi_fieldcalc_amd import hremap as hremap_module  # (without the feature the file fails here)
from test_python_front_cpu import _data, _stub_context

U = hr.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
A, S_, N = hr.ALL_DEFINED, hr.SOME_DEFINED, hr.NONE_DEFINED
# the host tables of mifc_hremap_levels for the recording stub: positions after the context
front.SPEC.setdefault("mifc_hremap_levels", [(4, "ptr", front._at(6)), (9, "ptr", front._at(6))])


def one_row(values, weights, cols=None, **kw):
    """One destination over len(values) source cells, one field, one level: (result, flag)."""
    x = np.asarray(values, np.float32).reshape(1, 1, -1)
    n = len(weights)
    out, fd = hr.remap(x, [0, n], np.arange(n) if cols is None else cols, weights, **kw)
    return out[0, 0, 0], int(fd[0, 0])


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


# ------------------------------------------------------------------------------------------------- hand-worked rows
def test_hand_worked_strict_and_renorm():
    r, f = one_row([1, 2, 3, 4], [0.25] * 4)
    assert r == np.float32(2.5) and f == A
    r, f = one_row([1, U, 3, 4], [0.25] * 4)
    assert r == U and f == N  # STRICT: one hole
    r, f = one_row([1, U, 3, 4], [0.25] * 4, mode=hr.RENORM)
    assert r == np.float32((2.0 / 0.75) * 1.0) and f == A  # S = 2, Wdef = 0.75, Wall = 1
    r, f = one_row([1, 2, 3, 4], [0.25] * 4, mode="renorm", min_frac=1.0)
    assert bits(r) == bits(one_row([1, 2, 3, 4], [0.25] * 4)[0])  # nbad == 0: the bits of STRICT, whatever min_frac
    # min_frac 0: one defined entry is enough; 1: any hole is too many
    assert one_row([U, U, U, 8], [0.25] * 4, mode=hr.RENORM, min_frac=0.0) == (np.float32(8), A)
    assert one_row([1, 2, 3, U], [0.25] * 4, mode=hr.RENORM, min_frac=1.0) == (U, N)
    assert one_row([U, U, U, U], [0.25] * 4, mode=hr.RENORM, min_frac=0.0) == (U, N)  # every entry undefined
    # exactly on the threshold: Wdef = 0.5 >= 0.5 * 1.0
    r, f = one_row([U, 2, U, 4], [0.25] * 4, mode=hr.RENORM, min_frac=0.5)
    assert r == np.float32(3) and f == A
    assert one_row([U, 2, U, U], [0.25] * 4, mode=hr.RENORM, min_frac=0.5) == (U, N)
    # Wdef == 0.0 from weights that cancel
    assert one_row([1, 2, U], [0.5, -0.5, 1.0], mode=hr.RENORM) == (U, N)
    # a partly covered destination (Wall = 0.5) keeps its partial sum scale
    r, f = one_row([4, U], [0.25, 0.25], mode=hr.RENORM)
    assert r == np.float32((1.0 / 0.25) * 0.5) and f == A


def test_row_seams():
    x = np.arange(1, 7, dtype=np.float32).reshape(1, 1, 6)
    out, fd = hr.remap(x, [0, 2, 2, 3], [0, 1, 5], [0.5, 0.5, 2.0])
    assert out[0, 0].tolist() == [1.5, float(U), 12.0] and fd[0, 0] == S_  # the empty row is undef, and counted
    out, fd = hr.remap(x, [0, 2, 2, 3], [0, 1, 5], [0.5, 0.5, 2.0], mode=hr.RENORM)
    assert out[0, 0].tolist() == [1.5, float(U), 12.0] and fd[0, 0] == S_
    out, fd = hr.remap(x, [0, 0, 0], [], [])
    assert (out == U).all() and fd[0, 0] == N  # nnz == 0
    assert one_row([3, 5], [0.25, 0.5, 0.25], cols=[1, 0, 1]) == (np.float32(4.0), A)  # a repeated column: 1.25 + 1.5 + 1.25
    # the order of the entries changes the last bits: 2^60 + 1 is 2^60 in double
    big = np.float32(2.0 ** 60)
    assert one_row([big, 1, -big], [1, 1, 1])[0] == np.float32(0) and one_row([big, -big, 1], [1, 1, 1])[0] == np.float32(1)
    assert one_row([big, 1, -big], [1, 1, 1], cols=[0, 2, 1])[0] == np.float32(1)  # the same cells, another order


def test_value_seams():
    neg0 = np.float32(-0.0)
    r, f = one_row([neg0], [1.0])
    assert bits(r) == bits(0.0) and f == A  # -0.0 comes back as +0.0: the sum starts from +0.0
    for v in (1.5, -3.25e-40, 3.4e38, np.inf):
        assert bits(one_row([v], [1.0])[0]) == bits(v)  # a one-entry row of weight 1: the value bit for bit
    # a stored undef under ALL_DEFINED is a value, and a result that equals undef is not counted
    assert one_row([U, 1], [1.0, 0.0], flags=[[A]]) == (U, A)
    assert one_row([U, 1], [0.5, 0.5], flags=[[A]]) == (np.float32(0.5 * float(U) + 0.5), A)
    assert one_row([np.float32(2) * U], [0.5]) == (U, A)  # undef by arithmetic: computed, never counted
    assert one_row([np.float32(2) * U, U], [0.25, 0.25], mode=hr.RENORM, min_frac=0.5) == (U, A)  # (0.5 U / 0.25) * 0.5
    r, f = one_row([np.nan, 1], [0.5, 0.5], flags=[[A]])
    assert np.isnan(r) and f == A  # a NaN under ALL_DEFINED
    assert one_row([np.nan, 1], [0.5, 0.5]) == (U, N)  # tested: NaN is a hole
    assert one_row([np.nan, 1], [0.5, 0.5], flags=[[N]]) == (U, N)  # NONE_DEFINED is tested like SOME_DEFINED
    r, f = one_row([np.inf, 1], [0.5, -0.5])
    assert r == np.inf and f == A
    nan = np.float32(np.nan)  # a non-default undef
    r, f = one_row([nan, 4], [0.5, 0.5], mode=hr.RENORM, undef=nan)
    assert r == np.float32(4) and f == A
    r, f = one_row([U, 4], [0.5, 0.5], undef=np.float32(-999))
    assert r == np.float32(0.5 * float(U) + 2) and f == A


def _scalar_loop(fields, rowptr, col, w, mode, min_frac, flags, undef):
    """The definition of include/mifc.h entry by entry in Python floats (doubles)."""
    nf, nlev = fields.shape[:2]
    f = fields.reshape(nf, nlev, -1)
    ndst = len(rowptr) - 1
    out = np.empty((nf, nlev, ndst), np.float32)
    fd = np.empty((nf, nlev), np.int32)
    for g in range(nf):
        for k in range(nlev):
            holes = 0
            for d in range(ndst):
                s = wdef = wall = 0.0
                nbad = 0
                for e in range(rowptr[d], rowptr[d + 1]):
                    x, we = f[g, k, col[e]], float(w[e])
                    wall = wall + we
                    if flags[g, k] == A or not (np.isnan(x) or x == undef):
                        s = s + we * float(x)
                        wdef = wdef + we
                    else:
                        nbad += 1
                n = rowptr[d + 1] - rowptr[d]
                if n == 0 or (nbad > 0 and mode == hr.STRICT):
                    res = None
                elif nbad == 0:
                    res = np.float32(s)
                elif nbad == n or wdef == 0.0 or not (abs(wdef) >= min_frac * abs(wall)):
                    res = None
                else:
                    with np.errstate(all="ignore"):
                        res = np.float32(np.float64(s) / np.float64(wdef) * np.float64(wall))
                holes += res is None
                out[g, k, d] = undef if res is None else res
            fd[g, k] = A if holes == 0 else (N if holes == ndst else S_)
    return out, fd


@pytest.mark.parametrize("mode,min_frac", [(hr.STRICT, 0.0), (hr.RENORM, 0.0), (hr.RENORM, 0.5), (hr.RENORM, 1.0)])
def test_the_restatement_against_an_independent_scalar_loop(mode, min_frac):
    fields, (rowptr, col, w) = hr.main_case(nf=2, nlev=3, ndst=150, seed=7, frac=0.15)
    fields[0, 1, 2, 3] = np.nan
    rowptr, col, w = hr.table_from_lengths(hr.main_lengths(150, 7), 117, 7, negative=True)
    flags = np.array([[A, S_, N], [S_, A, S_]], np.int32)
    with np.errstate(all="ignore"):
        want, wfd = _scalar_loop(fields, rowptr, col, w, mode, min_frac, flags, U)
    got, gfd = hr.remap(fields, rowptr, col, w, mode, min_frac, flags)
    assert got.tobytes() == want.tobytes() and (gfd == wfd).all()
    assert (got == U).any() and (got != U).any() and (gfd == S_).all()  # (the table has empty rows)


# ---------------------------------------------------------------------------- conservative_weights_regular, from_coo
def _hremap():
    return hremap_module


def _apply(rowptr, col, w, field):
    out, fd = hr.remap(field[None, None], rowptr, col, w, flags=[[A]])
    return out[0, 0], fd


@pytest.mark.parametrize("by,bx", [(2, 2), (3, 2)], ids=["2x2", "3x2"])
def test_conservative_coarsening_reproduces_block_means(by, bx):
    hremap = _hremap()
    ny, nx = 12, 18
    rowptr, col, w = hremap.conservative_weights_regular(np.arange(nx + 1), np.arange(ny + 1), np.arange(0, nx + 1, bx), np.arange(0, ny + 1, by))
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and w.dtype == np.float32
    assert (np.diff(rowptr) == by * bx).all() and all((np.diff(col[rowptr[d]:rowptr[d + 1]]) > 0).all() for d in range(rowptr.size - 1))
    x = np.random.default_rng(3).integers(-50, 50, (ny, nx)).astype(np.float32)
    got, _ = _apply(rowptr, col, w, x)
    blocks = x.reshape(ny // by, by, nx // bx, bx)
    if by * bx == 4:  # weights of 1/4 are exact: the block mean bit for bit
        want = (blocks.astype(np.float64).sum(axis=(1, 3)) / 4).astype(np.float32)
        assert got.reshape(ny // by, nx // bx).tobytes() == want.tobytes()
    else:  # 1/6 is rounded to float: the mean within the rounding of six weights
        want = blocks.astype(np.float64).mean(axis=(1, 3))
        assert np.abs(got.reshape(want.shape) - want).max() <= 2.0 ** -24 * (np.abs(blocks).sum(axis=(1, 3)) / 6 + np.abs(want)).max()


def test_conservative_weights_rows_areas_and_half_cover():
    hremap = _hremap()
    rng = np.random.default_rng(5)
    sx, sy = np.cumsum(rng.uniform(0.5, 1.5, 19)), np.cumsum(rng.uniform(0.5, 1.5, 13))  # 18 x 12 cells, uneven
    dx, dy = np.linspace(sx[0], sx[-1], 8), np.linspace(sy[0], sy[-1], 6)  # 7 x 5 cells over the same extent, non-aligned
    rowptr, col, w = hremap.conservative_weights_regular(sx, sy, dx, dy)
    nrow = np.diff(rowptr)
    assert rowptr.size == 36 and nrow.min() >= 4
    sums = np.array([w[rowptr[d]:rowptr[d + 1]].astype(np.float64).sum() for d in range(35)])
    # Every entry is its exact value rounded to float once, within 2^-24 of it (relative, the unit roundoff); the exact
    # values of a covered row sum to 1.  Beside that only double roundings: three operations behind every entry before it
    # is rounded to float, and the nrow - 1 additions of this sum.
    wabs = np.array([np.abs(w[rowptr[d]:rowptr[d + 1]].astype(np.float64)).sum() for d in range(35)])
    assert (np.abs(sums - 1.0) <= 2.0 ** -24 * wabs + (nrow + 3) * 2.0 ** -53 * wabs).all()
    x = rng.normal(5, 3, (12, 18)).astype(np.float32)
    got, fd = _apply(rowptr, col, w, x)
    src_area, dst_area = np.outer(np.diff(sy), np.diff(sx)), np.outer(np.diff(dy), np.diff(dx)).ravel()
    absum = np.array([(np.abs(w[rowptr[d]:rowptr[d + 1]].astype(np.float64)) * np.abs(x.ravel()[col[rowptr[d]:rowptr[d + 1]]])).sum() for d in range(35)])
    bound = 2.0 ** -24 * (dst_area * np.abs(got)).sum() + 2.0 ** -24 * (dst_area * absum).sum()
    err = abs((dst_area * got.astype(np.float64)).sum() - (src_area * x).sum())
    print("area integral: error %.3g, bound %.3g" % (err, bound))
    assert err <= bound and fd[0, 0] == A
    # a destination half outside the source carries half the weight; one wholly outside has an empty row
    rowptr, col, w = hremap.conservative_weights_regular([0, 1, 2], [0, 1], [-1, 1, 2, 4, 6], [0, 1])
    assert np.diff(rowptr).tolist() == [1, 1, 0, 0] and col.tolist() == [0, 1] and w.tolist() == [0.5, 1.0]
    with pytest.raises(ValueError, match="ascending"):
        hremap.conservative_weights_regular([0, 2, 1], [0, 1], [0, 1], [0, 1])


def test_from_coo_is_a_stable_sort_by_row_and_takes_one_based_triples():
    hremap = _hremap()
    rows, cols, s = [2, 0, 2, 0, 2], [7, 3, 1, 9, 7], [0.1, 0.2, 0.3, 0.4, 0.5]
    rowptr, col, w = hremap.coo_to_csr(rows, cols, s, 4)
    assert rowptr.tolist() == [0, 2, 2, 5, 5] and col.tolist() == [3, 9, 7, 1, 7] and bits(w) == bits([0.2, 0.4, 0.1, 0.3, 0.5])
    assert rowptr.dtype == np.int32 and col.dtype == np.int32 and w.dtype == np.float32
    r1, c1, w1 = hremap.coo_to_csr(np.array(rows) + 1, np.array(cols) + 1, s, 4, one_based=True)
    assert (r1 == rowptr).all() and (c1 == col).all() and (w1 == w).all()
    with pytest.raises(ValueError, match="a row outside"):
        hremap.coo_to_csr([0, 4], [0, 0], [1, 1], 4)
    with pytest.raises(ValueError, match="a row outside"):
        hremap.coo_to_csr([0, 1], [0, 0], [1, 1], 4, one_based=True)
    d = _data()
    ctx, lib = _stub_context(d)
    plan = hremap.Plan.from_coo(ctx, np.array(rows) + 1, np.array(cols) + 1, s, nsrc=20, ndst=4, one_based=True)
    name, a = lib.calls[-1]
    assert name == "mifc_hremap_plan_create" and a[:2] == [20, 4] and a[2]["values"] == [0, 2, 2, 5, 5] and a[3]["values"] == [3, 9, 7, 1, 7]
    assert bits(a[4]["values"]) == bits(w) and a[5] == 0 and plan.ndst == 4
    plan.close()


# ------------------------------------------------------------------------ the plan header through the host compiler
def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    return cxx


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hremap") / "libhremap_plan_shim.so")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "hremap_plan_shim.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.mifc_test_hremap_check.restype = ctypes.c_int
    lib.mifc_test_hremap_layout.restype = lib.mifc_test_hremap_copy.restype = None
    ip, fp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)

    def tables(rowptr, col, w):
        r, c, s = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(col, np.int32), np.ascontiguousarray(w, np.float32)
        return (r, c, s), (r.ctypes.data_as(ip), c.ctypes.data_as(ip), s.ctypes.data_as(fp))

    def check(nsrc, ndst, rowptr, col, w):
        keep, ptrs = tables(rowptr, col, w)
        why = ctypes.create_string_buffer(160)
        ok = lib.mifc_test_hremap_check(nsrc, ndst, *ptrs, why, 160)
        return ok, why.value.decode()

    def layout(nsrc, rowptr, col, w):
        keep, ptrs = tables(rowptr, col, w)
        ndst = len(rowptr) - 1
        assert check(nsrc, ndst, rowptr, col, w) == (1, "")
        info = (ctypes.c_longlong * 6)()
        lib.mifc_test_hremap_layout(nsrc, ndst, *ptrs, info)
        nnz, max_row, empty, nslices, max_width, entries = (int(v) for v in info)
        off, width = np.zeros(nslices, np.uint64), np.zeros(nslices, np.int32)
        length, wall = np.zeros(nslices * 64, np.int32), np.zeros(nslices * 64, np.float64)
        ec, ew = np.full(max(entries, 1), -7, np.int32), np.zeros(max(entries, 1), np.float32)
        lib.mifc_test_hremap_copy(*(a.ctypes.data_as(ctypes.c_void_p) for a in (off, width, length, wall, ec, ew)))
        return dict(nnz=nnz, max_row=max_row, empty_rows=empty, nslices=nslices, max_width=max_width, entries=entries, slice_off=off, slice_width=width,
                    len=length, wall=wall, col=ec, w=ew)

    return check, layout


def test_plan_header_refusals(shim):
    check, _ = shim
    good = ([0, 1, 2], [0, 4], [0.5, 0.5])
    assert check(5, 2, *good) == (1, "")
    assert check(5, 2, [0, 0, 0], [], []) == (1, "")  # nnz == 0 is legal
    cases = [
        ((0, 2) + good, "nsrc < 1 or ndst < 1"),
        ((-3, 2) + good, "nsrc < 1 or ndst < 1"),
        ((5, 0) + good, "nsrc < 1 or ndst < 1"),
        ((5, 2, [1, 1, 2], [0, 4], [0.5, 0.5]), "rowptr[0] != 0"),
        ((5, 2, [0, 2, 1], [0, 4], [0.5, 0.5]), "rowptr decreases at row 1"),
        ((5, 2, [0, -1, -1], [0, 4], [0.5, 0.5]), "nnz = rowptr[ndst] is negative"),
        ((5, 2, [0, 1, 2], [0, 5], [0.5, 0.5]), "col[1] = 5 outside [0, nsrc)"),
        ((5, 2, [0, 1, 2], [-1, 4], [0.5, 0.5]), "col[0] = -1 outside [0, nsrc)"),
        ((5, 2, [0, 1, 2], [0, 4], [0.5, np.nan]), "w[1] is NaN or infinite"),
        ((5, 2, [0, 1, 2], [0, 4], [-np.inf, 0.5]), "w[0] is NaN or infinite"),
    ]
    for args, why in cases:
        assert check(*args) == (0, why), why


PATTERNS = {"one empty row": [0], "one entry": [1], "64 equal rows": [5] * 64, "65 rows": [5] * 65, "lengths 0..63": list(range(64)),
            "one row of 300 among rows of 2": [2] * 70 + [300] + [2] * 59, "nnz == 0": [0] * 70}


@pytest.mark.parametrize("name", PATTERNS)
def test_plan_header_layout_entry_by_entry(shim, name):
    _, layout = shim
    lengths = np.array(PATTERNS[name])
    nsrc, ndst = 117, len(lengths)
    rowptr, col, w = hr.table_from_lengths(lengths, nsrc, seed=len(name), negative=True)
    L = layout(nsrc, rowptr, col, w)
    assert (L["nnz"], L["max_row"], L["empty_rows"]) == (int(lengths.sum()), int(lengths.max()), int((lengths == 0).sum()))
    assert L["nslices"] == -(-ndst // 64) and L["max_width"] == L["max_row"]
    total = 0
    for s in range(L["nslices"]):
        mine = lengths[64 * s:64 * s + 64]
        assert L["slice_off"][s] == total and L["slice_width"][s] == mine.max()
        for lane in range(64):
            d = 64 * s + lane
            n = int(lengths[d]) if d < ndst else 0
            assert L["len"][d] == n
            at = total + 64 * np.arange(int(mine.max())) + lane  # [r][lane]
            assert (L["col"][at[:n]] == col[rowptr[d]:rowptr[d] + n]).all() and bits(L["w"][at[:n]]) == bits(w[rowptr[d]:rowptr[d] + n]) if d < ndst else n == 0
            pad = col[rowptr[d]] if n else 0  # a valid column: the row's first, 0 for an empty row
            assert (L["col"][at[n:]] == pad).all()
        total += 64 * int(mine.max())
    assert L["entries"] == total
    wall = hr.row_sums(rowptr, w)
    assert L["wall"][:ndst].tobytes() == wall.tobytes() and (L["wall"][ndst:] == 0).all()  # Wall bit for bit


def test_plan_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "hremap_plan_asan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "host", "hremap_plan_main.cc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)  # (the environment as it is: the runtimes are linked in)
    assert run.returncode == 0 and "7 patterns, 0 failures" in run.stdout, run.stdout + run.stderr


# ------------------------------------------------------------------------------- declared, bound and configured
def test_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    hremap = _hremap()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    names = ("mifc_hremap_plan_create", "mifc_hremap_plan_destroy", "mifc_hremap_plan_info", "mifc_hremap_levels", "mifc_last_hremap_form")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert [len(capi.SIGNATURES[n][1]) for n in names] == [7, 1, 4, 14, 0]
    assert capi.SIGNATURES["mifc_hremap_levels"][1][9] == "d" and capi.SIGNATURES["mifc_hremap_plan_create"][0] == "p"  # min_frac is a double
    assert re.search(r"MIFC_HREMAP_STRICT = 0, MIFC_HREMAP_RENORM = 1", header) and hremap.HREMAP_MODES == {"strict": 0, "renorm": 1}
    for var, field in (("MIFC_HREMAP_CHUNK_MIB", "hremap_chunk_mib"), ("MIFC_HREMAP_LEVEL_CHUNK", "hremap_level_chunk")):
        readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if '"%s"' % var in open(p, errors="replace").read()]
        assert readers == ["mifc_env.hip"], (var, readers)
    host = open(os.path.join(CSRC, "mifc_capi_hremap.hip")).read()
    assert "getenv" not in host and re.search(r"hremap_chunk_mib > 0 \? mifc::env\(\)\.hremap_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_hremap.hip") == 1 and makefile.count("mifc_capi_hremap.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    assert makefile.count("mifc_hremap_plan.h") == 1  # HDRS
    kernel = open(os.path.join(CSRC, "mifc_hremap.hip")).read()
    assert kernel.count("__global__") == 1
    plan_header = open(os.path.join(CSRC, "mifc_hremap_plan.h")).read()
    assert "hip" not in re.sub(r"//.*", "", plan_header).lower()  # HIP-free: the host compiler builds it


# ------------------------------------------------------------------------------- the front against a recording stub
def _front(rc=1):
    d = _data()
    d["ROWPTR"], d["COL"], d["WT"] = np.array([0, 2, 2, 3], np.int32), np.array([3, 0, 19], np.int32), np.array([0.5, 0.5, 1.0], np.float32)
    ctx, lib = _stub_context(d, rc)
    return _hremap(), d, ctx, lib


def _entry_calls(lib, name):
    return [a for n, a in lib.calls if n == name]


def test_front_marshals_the_plan_and_the_entry_in_header_order():
    hremap, d, ctx, lib = _front(rc=0)
    lib.rc = d["W"].ctypes.data  # the handle the stub hands out: an address the recorder can name
    plan = hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], nsrc=20)
    a = _entry_calls(lib, "mifc_hremap_plan_create")[-1]
    assert a[:2] == [20, 3] and a[2]["values"] == [0, 2, 2, 3] and a[2]["numpy"] == "int32" and a[3]["values"] == [3, 0, 19]
    assert a[4]["numpy"] == "float32" and a[4]["values"] == [0.5, 0.5, 1.0] and a[5] == 0 and len(a) == 6
    assert plan.ndst == 3 and plan.nsrc == 20 and plan.handle == d["W"].ctypes.data
    lib.rc = 1
    out, fd = hremap.hremap_levels(ctx, plan, d["F2"], "renorm", 0.25, fdefined_in=[A, S_], undef=-5.0)
    a = _entry_calls(lib, "mifc_hremap_levels")[-1]
    assert a[0] == ["W", 0] and a[1:4] == [5, 4, 3]  # the plan's handle, then nx, ny, nlev
    assert a[4] == [["F2", 0], ["F2", 4 * 60]] and a[5]["values"] == [A, A, A, S_, S_, S_] and a[6] == 2 and a[7] == 1 and a[8] == 0.25
    assert a[9] == ["<other>", "<other>"] and a[10]["numpy"] == "int32" and a[10]["shape"] == [2, 3] and a[11] == -5.0 and a[12] == 0 and len(a) == 13
    assert out.shape == (2, 3, 3) and out.dtype == np.float32 and fd.shape == (2, 3)
    # one batch: no leading axis; dst_shape; out= reuse
    o = d["OUT"][:9].reshape(3, 3, 1)
    out, fd = hremap.hremap_levels(ctx, plan, d["B"], out=o, dst_shape=(3, 1))
    a = _entry_calls(lib, "mifc_hremap_levels")[-1]
    assert out is o and a[4] == [["B", 0]] and a[9] == [["OUT", 0]] and a[5] is None and a[6] == 1 and a[7] == 0 and a[8] == 0.0 and a[11] == float(U)
    assert fd.shape == (3,)
    out, fd = hremap.hremap_levels(ctx, plan, [d["B"], d["V"]], out=d["OUT"][:18].reshape(2, 3, 3), mode=hr.RENORM, min_frac=1)
    a = _entry_calls(lib, "mifc_hremap_levels")[-1]
    assert a[4] == [["B", 0], ["V", 0]] and a[9] == [["OUT", 0], ["OUT", 36]] and a[7] == 1 and a[8] == 1.0
    with pytest.raises(ValueError, match="dst_shape"):
        hremap.hremap_levels(ctx, plan, d["B"], dst_shape=(2, 2))
    with pytest.raises(ValueError, match="out must have shape"):
        hremap.hremap_levels(ctx, plan, d["B"], out=d["OUT"][:12].reshape(3, 4))
    # the handle is destroyed once, by close(), the context manager and the collector alike
    assert _entry_calls(lib, "mifc_hremap_plan_destroy") == []
    plan.close()
    plan.close()
    with plan:
        pass
    del plan
    assert len(_entry_calls(lib, "mifc_hremap_plan_destroy")) == 1
    with hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], 20, ndst=3) as p2:
        assert p2.handle == 1
        closed = p2
    assert len(_entry_calls(lib, "mifc_hremap_plan_destroy")) == 2
    with pytest.raises(ValueError, match="closed"):
        hremap.hremap_levels(ctx, closed, d["B"])
    with pytest.raises(ValueError, match="ndst \\+ 1"):
        hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], 20, ndst=5)
    with pytest.raises(ValueError, match="same length"):
        hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"][:2], 20)


def test_a_refused_call_raises_refused_with_the_librarys_message():
    hremap, d, ctx, lib = _front(rc=0)
    lib.__dict__["mifc_last_error"] = lambda c: b"mifc_hremap_plan_create: col[2] = 19 outside [0, nsrc)"
    with pytest.raises(hremap.Refused, match=r"mifc_hremap_plan_create: col\[2\] = 19 outside \[0, nsrc\)") as info:
        hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], nsrc=19)
    assert isinstance(info.value, ValueError) and isinstance(info.value, RuntimeError)
    assert _entry_calls(lib, "mifc_hremap_plan_destroy") == []  # no handle, nothing to destroy
    lib.rc = 1
    plan = hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], nsrc=20)
    lib.rc = 0
    lib.__dict__["mifc_last_error"] = lambda c: b"mifc_hremap_levels: min_frac is NaN or outside [0, 1]"
    with pytest.raises(hremap.Refused, match=r"mifc_hremap_levels: min_frac is NaN or outside \[0, 1\]"):
        hremap.hremap_levels(ctx, plan, d["B"], "renorm", 1.5)
    with pytest.raises(hremap.Refused):
        hremap.hremap_levels(ctx, plan, d["B"], "no such mode")
    assert _entry_calls(lib, "mifc_hremap_levels")[-1][7] == -1
    plan.close()


def test_a_plan_closed_or_collected_after_its_context_does_not_call_the_library():
    import gc

    hremap, d, ctx, lib = _front()
    destroyed = lambda: [n for n, _ in lib.calls if n in ("mifc_hremap_plan_destroy", "mifc_destroy")]  # noqa: E731
    kept = hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], nsrc=20)
    dropped = hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], nsrc=20)
    early = hremap.Plan(ctx, d["ROWPTR"], d["COL"], d["WT"], nsrc=20)
    early.close()  # closed by hand: the context forgets it
    del dropped  # collected while the context lives: destroyed then
    gc.collect()
    assert destroyed() == ["mifc_hremap_plan_destroy"] * 2 and len(ctx._plans) == 1
    ctx.close()  # the context closes the plan it still has, then itself
    assert destroyed() == ["mifc_hremap_plan_destroy"] * 3 + ["mifc_destroy"] and ctx._ctx is None
    with pytest.raises(ValueError, match="closed"):
        hremap.hremap_levels(ctx, kept, d["B"])
    kept.close()
    del kept
    gc.collect()
    assert destroyed() == ["mifc_hremap_plan_destroy"] * 3 + ["mifc_destroy"]  # nothing after the context
    # a plan that outlives a context which never knew it was closed (the handle is dropped, the library is not called)
    ctx2, lib2 = _stub_context(d)
    late = hremap.Plan(ctx2, d["ROWPTR"], d["COL"], d["WT"], nsrc=20)
    ctx2.__dict__.pop("_plans")
    ctx2.close()
    late.close()
    assert [n for n, _ in lib2.calls if "destroy" in n] == ["mifc_destroy"]
