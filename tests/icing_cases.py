"""Seeded inputs of the iterative vessel-icing models and the two host checkers: the compiled reference
(tests/icing_ref_shim.cc against oracle/_ref/libmifc_ref.so) and the host build of the per-cell header
(tests/icing_cell_shim.cc).  Shared by tests/test_vessel_icing_cpu.py, tests/test_gpu_vessel_icing.py and
tools/bench_vessel_icing.py."""
import ctypes
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libmifc_ref.so")
CSRC = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
UNDEF = np.float32(1.0e35)
SENTINEL = np.float32(-4242.5)
ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
MODSTALL, MINCOG = 1, 2
NAMES = ("sal", "wave", "x_wind", "y_wind", "airtemp", "rh", "sst", "p", "Pw", "aice", "depth")
# the issue's realistic set: vs = 5, alpha = 0.7, zmin = 0, zmax = 10
SCALARS = dict(vs=5.0, alpha=0.7, zmin=0.0, zmax=10.0)


def ref_available():
    return os.path.exists(REF_LIB)


def _fptrs(fields):
    arrs = [np.ascontiguousarray(f, dtype=np.float32) for f in fields]
    ptrs = (ctypes.c_void_p * 11)(*[a.ctypes.data for a in arrs])
    return arrs, ptrs


def combine_flags(flags):
    flags = set(flags)
    if flags == {ALL_DEFINED}:
        return ALL_DEFINED
    if flags == {NONE_DEFINED}:
        return NONE_DEFINED
    return SOME_DEFINED


class RefShim:
    """The reference's two models through tests/icing_ref_shim.cc, loaded RTLD_LOCAL | RTLD_DEEPBIND."""

    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libicref_shim.so")
        inc = os.path.join(ROOT, "mi-fieldcalc_amd", "include")
        libdir = os.path.dirname(REF_LIB)
        subprocess.run(["g++", "-std=c++11", "-O2", "-shared", "-fPIC", "-I", inc, os.path.join(HERE, "icing_ref_shim.cc"), "-o", so, "-L", libdir,
                        "-l:libmifc_ref.so", "-Wl,-rpath," + libdir], check=True)
        self.lib = ctypes.CDLL(so, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        common = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float]
        tail = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
        self.lib.icref_modstall.argtypes = common + tail
        self.lib.icref_mincog.argtypes = common + [ctypes.c_int] + tail
        self.lib.icref_modstall.restype = self.lib.icref_mincog.restype = ctypes.c_int

    def run(self, model, fields, vs, alpha, zmin, zmax, alt=1, fdefined=SOME_DEFINED, out=None, undef=UNDEF):
        """fields: 11 arrays of one (ny, nx) shape.  Returns (ok, flag, out)."""
        arrs, ptrs = _fptrs(fields)
        ny, nx = arrs[0].shape
        out = np.full((ny, nx), SENTINEL, np.float32) if out is None else out
        f = ctypes.c_int(int(fdefined))
        if model == MODSTALL:
            ok = self.lib.icref_modstall(nx, ny, ptrs, vs, alpha, zmin, zmax, out.ctypes.data, ctypes.addressof(f), float(undef))
        else:
            ok = self.lib.icref_mincog(nx, ny, ptrs, vs, alpha, zmin, zmax, int(alt), out.ctypes.data, ctypes.addressof(f), float(undef))
        return bool(ok), f.value, out

    def run_rows(self, model, fields, vs, alpha, zmin, zmax, alt=1, fdefined=SOME_DEFINED, threads=16):
        """The same result computed in row bands on `threads` host threads (ctypes releases the GIL; every cell is
        independent of the others, so the bands' values are the whole call's and the flag is combined)."""
        arrs = [np.ascontiguousarray(f, dtype=np.float32) for f in fields]
        ny, nx = arrs[0].shape
        out = np.full((ny, nx), SENTINEL, np.float32)
        bands = [b for b in np.array_split(np.arange(ny), max(1, min(threads, ny))) if b.size]

        def one(b):
            o = np.empty((b.size, nx), np.float32)
            ok, flag, _ = self.run(model, [a[b[0] : b[-1] + 1] for a in arrs], vs, alpha, zmin, zmax, alt, fdefined, out=o)
            return b, ok, flag, o

        with ThreadPoolExecutor(len(bands)) as ex:
            res = list(ex.map(one, bands))
        for b, ok, flag, o in res:
            assert ok
            out[b[0] : b[-1] + 1] = o
        return True, combine_flags([r[2] for r in res]), out


class CellShim:
    """The host build of mi-fieldcalc_amd/csrc/mifc_icing_cell.h through tests/icing_cell_shim.cc."""

    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libiccell_shim.so")
        subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, os.path.join(HERE, "icing_cell_shim.cc"),
                        "-o", so], check=True)
        self.lib = ctypes.CDLL(so, mode=os.RTLD_LOCAL)
        self.lib.iccell_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                        ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p,
                                        ctypes.c_void_p]
        self.lib.iccell_run.restype = ctypes.c_int
        self.lib.iccell_bisect_iterations.restype = ctypes.c_int
        self.lib.iccell_sinhf_mismatches.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
        self.lib.iccell_sinhf_mismatches.restype = ctypes.c_longlong

    def run(self, model, fields, vs, alpha, zmin, zmax, alt=1, fdefined=SOME_DEFINED, undef=UNDEF, trips=False):
        """Returns (status, flag, out[, (dispersion histogram, level histogram)]); status 1 computed, 0 the reference's
        false, -1 refused (level count overflows an int)."""
        arrs, ptrs = _fptrs(fields)
        ny, nx = arrs[0].shape
        out = np.full((ny, nx), SENTINEL, np.float32)
        f = ctypes.c_int(int(fdefined))
        dh, lh = np.zeros(10002, np.int64), np.zeros(1002, np.int64)
        st = self.lib.iccell_run(model, nx, ny, ptrs, vs, alpha, zmin, zmax, int(alt), out.ctypes.data, ctypes.addressof(f), float(undef),
                                 dh.ctypes.data if trips else None, lh.ctypes.data if trips else None)
        return (st, f.value, out, (dh, lh)) if trips else (st, f.value, out)


def make_inputs(nx, ny, seed, nlev=None, specials=False, undef=UNDEF):
    """The 11 input fields (float32, (ny, nx) or (nlev, ny, nx)) in realistic ranges: salinity 30-35, waves 0-8 m,
    winds +-25 m/s, air -25..5 C, SST -1..8 C, rh 0.5-1, p 960-1040 hPa, wave period 2-14 s, sea ice 0-0.5 (some cells
    at or past the 0.4 cut), 20 % shallow water (1-60 m) and the rest 100-3000 m.  specials: sprinkle undefined
    values, NaNs and the edge cases of the models."""
    rng = np.random.default_rng(seed)
    shape = (ny, nx) if nlev is None else (nlev, ny, nx)
    f = {
        "sal": rng.uniform(30, 35, shape),
        "wave": rng.uniform(0, 8, shape),
        "x_wind": rng.uniform(-25, 25, shape),
        "y_wind": rng.uniform(-25, 25, shape),
        "airtemp": rng.uniform(-25, 5, shape),
        "rh": rng.uniform(0.5, 1.0, shape),
        "sst": rng.uniform(-1, 8, shape),
        "p": rng.uniform(960, 1040, shape),
        "Pw": rng.uniform(2, 14, shape),
        "aice": np.where(rng.random(shape) < 0.8, 0.0, rng.uniform(0, 0.5, shape)),
        "depth": np.where(rng.random(shape) < 0.2, rng.uniform(1, 60, shape), rng.uniform(100, 3000, shape)),
    }
    f = {k: v.astype(np.float32) for k, v in f.items()}
    if specials:
        add_specials(f, rng, undef)
    return [f[k] for k in NAMES]


def add_specials(f, rng, undef=UNDEF):
    """Edge cases, each in about 1 % of the cells: undefined / NaN inputs (every input, Pw included, which is not
    tested), Pw = 0, calm wind (v < 1), flat sea (wave < 0.1), aice exactly 0.4 (float, above the double 0.4 cut),
    sst at the freezing threshold (the float below and above it), shallow water down to 1 cm, and negative depth, where
    the shallow-water fixed point flips sign every trip and never converges."""
    shape = f["sal"].shape
    m = rng.random(shape)
    k = 0.0

    def take(frac=0.01):
        nonlocal k
        sel = (m >= k) & (m < k + frac)
        k += frac
        return sel

    for name in NAMES:
        f[name][take(0.004)] = undef
        f[name][take(0.002)] = np.float32(np.nan)
    f["Pw"][take()] = 0.0
    sel = take()
    f["x_wind"][sel] *= np.float32(0.02)
    f["y_wind"][sel] *= np.float32(0.02)
    f["wave"][take()] = np.float32(0.05)
    f["wave"][take()] = np.float32(0.1)  # float 0.1 > double 0.1: computed
    f["aice"][take()] = np.float32(0.4)
    f["aice"][take()] = np.float32(0.39999998)
    sal = f["sal"].astype(np.float64)
    thr = (-54.1126 * sal / (1000 - f["sal"]).astype(np.float64))
    below = thr.astype(np.float32)
    sel = take()
    f["sst"][sel] = below[sel]
    sel = take()
    f["sst"][sel] = np.nextafter(below[sel], np.float32(np.inf))
    f["depth"][take()] = np.float32(0.01)
    f["depth"][take()] = np.float32(-3.0)
    f["airtemp"][take()] = np.float32(-40.0)
    return f


def same_bits(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(a[~an].view(np.uint32), b[~bn].view(np.uint32))


def contract(got, ref, undef=UNDEF):
    """The accuracy contract of the GPU models.  Returns (undef placement equal, fraction of the defined
    cells that are bit-identical, largest excess over 1e-5 |ref| + 5e-5 (<= 0 passes), defined cells)."""
    got, ref = np.asarray(got, np.float32).ravel(), np.asarray(ref, np.float32).ravel()
    ug, ur = got == undef, ref == undef
    if not np.array_equal(ug, ur):
        return False, 0.0, np.inf, int((~ur).sum())
    g, r = got[~ur], ref[~ur]
    if g.size == 0:
        return True, 1.0, 0.0, 0
    gn, rn = np.isnan(g), np.isnan(r)
    if not np.array_equal(gn, rn):
        return True, 0.0, np.inf, int(g.size)
    same = (g.view(np.uint32) == r.view(np.uint32)) | (gn & rn)
    g64, r64 = g[~gn].astype(np.float64), r[~rn].astype(np.float64)
    excess = np.abs(g64 - r64) - (1e-5 * np.abs(r64) + 5e-5)
    return True, float(same.mean()), float(excess.max()) if excess.size else 0.0, int(g.size)
