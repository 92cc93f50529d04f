"""Seeded cases of the neighbourhood statistics and the reference checker (tests/neighbour_ref_shim.cc), shared
by tests/test_neighbour_cpu.py and tests/test_gpu_neighbour.py."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libmifc_ref.so")
SHIM_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "neighbour_ref_shim.cc")
UNDEF = np.float32(1.0e35)
SENTINEL = np.float32(-4242.5)


def ref_available():
    return os.path.exists(REF_LIB)


class RefShim:
    """The reference's two functions through our flat wrapper, loaded RTLD_LOCAL | RTLD_DEEPBIND."""

    def __init__(self, tmpdir):
        so = os.path.join(str(tmpdir), "libnbref_shim.so")
        inc = os.path.join(ROOT, "mi-fieldcalc_amd", "include")
        libdir = os.path.dirname(REF_LIB)
        subprocess.run(["g++", "-std=c++11", "-O2", "-shared", "-fPIC", "-I", inc, SHIM_SRC, "-o", so, "-L", libdir, "-l:libmifc_ref.so",
                        "-Wl,-rpath," + libdir], check=True)
        self.lib = ctypes.CDLL(so, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        for name in ("nbref_neighbourProbFunctions", "nbref_neighbourFunctions"):
            fn = getattr(self.lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                           ctypes.c_void_p, ctypes.c_float]

    def run(self, which, nx, ny, field, constants, compute, fres, fdefined, undef=UNDEF):
        """fres: float32 array, modified in place.  Returns (ok, flag)."""
        fn = self.lib.nbref_neighbourProbFunctions if which == "prob" else self.lib.nbref_neighbourFunctions
        c = np.ascontiguousarray(constants, dtype=np.float32)
        f = ctypes.c_int(int(fdefined))
        field = np.ascontiguousarray(field, dtype=np.float32)
        ok = fn(nx, ny, field.ctypes.data, c.ctypes.data, int(c.size), int(compute), fres.ctypes.data, ctypes.addressof(f), float(undef))
        return bool(ok), f.value


def make_field(nx, ny, seed, specials=False, nlev=None):
    """Values on a 0.25 grid in [-4, 4] (many ties); specials: True sprinkles signed zeros and NaNs, "zeros" signed zeros only."""
    rng = np.random.default_rng(seed)
    shape = (ny, nx) if nlev is None else (nlev, ny, nx)
    f = (np.round(rng.uniform(-4, 4, size=shape) * 4) / 4).astype(np.float32)
    if specials:
        m = rng.random(shape)
        f[m < 0.08] = np.float32(-0.0)
        f[(m >= 0.08) & (m < 0.16)] = np.float32(0.0)
        if specials is True:
            f[(m >= 0.16) & (m < 0.19)] = np.float32(np.nan)
    return f


def sweep(nx=23, ny=17):
    """(which, compute, constants, specials) of the seeded sweep: every compute (0 and 7 too), truncated constants,
    odd and even steps, step / 2 == range, 2r + 1 > nx, percentile index 0 and N - 1, NaN and signed zeros."""
    out = []
    for compute in (5, 6):
        for c in ([0.5, 0], [1.7, 1], [-0.9, 2.9], [2, 3], [0, 8], [1, 11], [0, 17]):
            out.append(("prob", compute, c, compute != 5 or c[1] != 3))
    for compute in (0, 7, -1):
        out.append(("prob", compute, [1.0, 0.0], False))  # range 0: nothing written
    for compute in (1, 2, 3, 0, 7, -2):
        for c in ([1], [2.9], [1, 1], [1, 2], [2, 3], [2, 4], [3.2, 6.9], [4, 1], [11, 2], [12, 3], [2, 5], [3], [1, 2, 9]):
            out.append(("functions", compute, c, compute in (1, 2, 3)))
    for compute in (5, 6):
        for c in ([0.7, 1], [1, 2], [-1.5, 2, 1], [0, 2, 4], [2, 3, 6], [0, 3, 7], [1, 11, 1], [0, 12, 5], [1.9, 1, 2], [1, 2, 3, 4]):
            out.append(("functions", compute, c, True))
    for c in ([0, 1, 1], [99, 1, 1], [50, 2], [90, 2, 1], [-0.9, 3, 2], [99.9, 3, 3], [10, 1, 2], [75, 11, 1], [33, 2, 5]):
        # N = 9: limit 99 gives ii = 8 = N - 1; limit 0 / -0.9 give ii = 0
        out.append(("functions", 4, c, "zeros"))  # NaN: undefined in the reference (std::sort), not tested
    return out


def percentile_zero_equal(a):
    """-0 and +0 as one value: which zero the reference returns depends on std::sort's order of equal elements."""
    a = np.array(a, dtype=np.float32, copy=True)
    a[a == 0] = np.float32(0.0)
    return a


# (which, constants, compute) on a 12 x 10 field where the reference is undefined and the library refuses (DESIGN.md,
# "Neighbourhood statistics"); "alias" = neighbourFunctions with field == fres (range 1, step 1)
NAN = float("nan")
DEVIATIONS = [
    ("prob", [0, -1], 5),  # 1: range < 0
    ("prob", [0, 13], 5),  # 1: range > nx
    ("prob", [0, 11], 6),  # 1: range > ny
    ("prob", [0, 1], 1),  # 2: compute not 5 / 6 with range > 0
    ("prob", [0, 2], 7),
    ("functions", [1, 4], 1),  # 3: step / 2 > range
    ("functions", [0, 1, 5], 5),
    ("functions", [100, 1, 1], 4),  # 4: percentile index N
    ("functions", [-12, 1, 1], 4),  # 4: percentile index < 0
    ("functions", [150, 2], 4),
    ("functions", "alias", 1),  # 5: field == fres
    ("prob", [NAN, 1], 5),  # 6: NaN / out-of-int-range constants
    ("prob", [0, -3e9], 6),
    ("functions", [1, 3e9], 1),
    ("functions", [float("inf")], 2),
    ("functions", [NAN, 1, 1], 4),
]
