"""Numpy restatement of mifc_hdist_histogram_levels and mifc_hdist_quantile_levels (include/mifc.h, "area histograms and
exact percentiles of level batches"): the oracle of tests/test_gpu_hdist.py.  The definition twice: histogram() and
quantiles() are vectorised -- numpy.searchsorted on the keys that fold -0 onto +0, numpy.sort on the keys of the IEEE
total order --, histogram_literal() and quantiles_literal() are loops over the cells in Python floats that know nothing
of keys.  Counts are integers and percentiles are order statistics: every comparison with these functions is for equality."""
import math

import numpy as np

from vinterp_restate import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, is_defined, sprinkle  # noqa: F401

AREA, ROWS = 0, 1
MODES = {"area": AREA, "rows": ROWS}
LOWER, LINEAR = 0, 1
METHODS = {"lower": LOWER, "linear": LINEAR}
MAX_EDGES, MAX_Q, MAX_FIELDS = 1024, 16, 8
NAN_KEY = np.uint32(0xFFFFFFFF)

# Departures from the definition that a test may ask for by name (`mistakes`): what a kernel that is subtly wrong would
# compute.  tests/test_hdist_cpu.py shows that the cases aimed at each tell it from the rules.
MISTAKES = ("binned on the total-order key", "less at an edge", "nan in the last bin", "counters wrap at 2^16", "lower rank in double",
            "no clamp at 100", "sort without signed zeros", "linear with a float difference")


def _check(mistakes):
    assert all(m in MISTAKES for m in mistakes), mistakes


def _box(box, ny, nx):
    i0, i1, j0, j1 = (0, nx, 0, ny) if box is None else (int(b) for b in box)
    assert 0 <= i0 < i1 <= nx and 0 <= j0 < j1 <= ny
    return i0, i1, j0, j1


def _flags(flags, nf, nlev):
    return np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)


def _fields(fields):
    f = np.asarray(fields, np.float32)
    return f[None] if f.ndim == 3 else f


def same(a, b):
    """Equal bit for bit, except that a NaN matches any NaN (floats); equal (integers)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    nan = np.isnan(a) & np.isnan(b)
    return bool((nan | (a.view(np.uint32) == b.view(np.uint32))).all())


# ------------------------------------------------------------------------------------------------------------- keys
def order_key(x):
    """The IEEE total order as uint32: -inf < ... < -0 < +0 < ... < +inf, every NaN on 0xffffffff."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where((b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), NAN_KEY, k).astype(np.uint32)


def key_value(k):
    """The float32 of a key; the NaN key gives a NaN."""
    k = np.asarray(k, np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == NAN_KEY, np.uint32(0x7FC00000), b).astype(np.uint32).view(np.float32)


def bin_key(x):
    """order_key with -0 folded onto +0: for values that are no NaN, bin_key(a) <= bin_key(b) iff a <= b."""
    x = np.ascontiguousarray(x, np.float32).copy()
    x[x == 0] = np.float32(0.0)
    return order_key(x)


def check_edges(edges):
    """-1, or the index of the first edge that is a NaN or not above the edge before it."""
    e = np.asarray(edges, np.float32)
    for i in range(e.size):
        if np.isnan(e[i]) or (i > 0 and not e[i - 1] < e[i]):
            return i
    return -1


def included(x, flag, mask, fdef_mask, box, undef=UNDEF):
    """Rule 1 for one level x (ny, nx): the cells that count."""
    ny, nx = x.shape
    i0, i1, j0, j1 = box
    inc = np.zeros((ny, nx), bool)
    inc[j0:j1, i0:i1] = True
    inc &= is_defined(flag == ALL_DEFINED, x, np.float32(undef))
    if mask is not None:
        inc &= is_defined(fdef_mask == ALL_DEFINED, np.asarray(mask, np.float32), np.float32(undef))
    return inc


# -------------------------------------------------------------------------------------------------------- histogram
def slots(x, edges, mistakes=()):
    """Rules 2 and 3: the slot 0 .. nedges + 1 of every value of x against one field's edges."""
    e = np.asarray(edges, np.float32)
    nan = np.isnan(x)
    key = order_key if "binned on the total-order key" in mistakes else bin_key
    s = np.searchsorted(key(e), key(x), side="left" if "less at an edge" in mistakes else "right")
    return np.where(nan, e.size if "nan in the last bin" in mistakes else e.size + 1, s)


def histogram(fields, edges, mask=None, fdef_mask=SOME_DEFINED, box=None, mode=AREA, flags=None, undef=UNDEF, mistakes=()):
    """int32 (nf, nlev, nrows, nedges + 2).  fields (nf, nlev, ny, nx) or one batch; edges (nedges,) or (nf, nedges)."""
    _check(mistakes)
    f = _fields(fields)
    nf, nlev, ny, nx = f.shape
    e = np.asarray(edges, np.float32)
    e = np.broadcast_to(e, (nf, e.shape[-1]))
    ne = e.shape[1]
    bx = _box(box, ny, nx)
    fl = _flags(flags, nf, nlev)
    mode = MODES.get(mode, mode)
    rows = range(bx[2], bx[3])
    out = np.zeros((nf, nlev, 1 if mode == AREA else len(rows), ne + 2), np.int64)
    for g in range(nf):
        assert check_edges(e[g]) < 0
        for k in range(nlev):
            inc = included(f[g, k], fl[g, k], mask, fdef_mask, bx, undef)
            s = slots(f[g, k], e[g], mistakes)
            for r, j in enumerate(rows):
                out[g, k, 0 if mode == AREA else r] += np.bincount(s[j][inc[j]], minlength=ne + 2)
    if "counters wrap at 2^16" in mistakes:
        out %= 65536
    return out.astype(np.int32)


def histogram_literal(fields, edges, mask=None, fdef_mask=SOME_DEFINED, box=None, mode=AREA, flags=None, undef=UNDEF):
    """The same, cell by cell and edge by edge, in Python floats."""
    f = _fields(fields)
    nf, nlev, ny, nx = f.shape
    e = np.asarray(edges, np.float32)
    e = np.broadcast_to(e, (nf, e.shape[-1]))
    ne = e.shape[1]
    i0, i1, j0, j1 = _box(box, ny, nx)
    fl = _flags(flags, nf, nlev)
    mode = MODES.get(mode, mode)
    u = float(np.float32(undef))
    out = np.zeros((nf, nlev, 1 if mode == AREA else j1 - j0, ne + 2), np.int32)
    for g in range(nf):
        eg = [float(v) for v in e[g]]
        for k in range(nlev):
            for j in range(j0, j1):
                for i in range(i0, i1):
                    x = float(f[g, k, j, i])
                    if fl[g, k] != ALL_DEFINED and (math.isnan(x) or x == u):
                        continue
                    if mask is not None and fdef_mask != ALL_DEFINED:
                        m = float(np.float32(mask[j][i]))
                        if math.isnan(m) or m == u:
                            continue
                    b = ne + 1 if math.isnan(x) else sum(1 for v in eg if v <= x)
                    out[g, k, 0 if mode == AREA else j - j0, b] += 1
    return out


# ------------------------------------------------------------------------------------------------------ percentiles
def rank(method, n, p, mistakes=()):
    """Rule 4 of mifc_ensembleQuantiles for n >= 1: (k, k1, t)."""
    p = np.float32(p)
    if METHODS.get(method, method) == LOWER:
        if "lower rank in double" in mistakes:
            ii = int((float(n) * float(p)) / 100.0)
        else:
            ii = int((np.float32(n) * p) / np.float32(100.0))  # all in float, truncated
        if "no clamp at 100" not in mistakes:
            ii = min(ii, n - 1)
        return ii, ii, 0.0
    h = (np.float64(n - 1) * np.float64(p)) / np.float64(100.0)
    k = int(h)
    t = float(h - np.float64(k))
    return k, (k if t == 0.0 else k + 1), t


def interpolate(xk, xk1, t, mistakes=()):
    if t == 0.0:
        return np.float32(xk)
    with np.errstate(all="ignore"):
        a, b = np.float64(np.float32(xk)), np.float64(np.float32(xk1))
        d = np.float64(np.float32(xk1) - np.float32(xk)) if "linear with a float difference" in mistakes else b - a
        return np.float32(a + np.float64(t) * d)


def quantiles(fields, percentiles, method=LINEAR, mask=None, fdef_mask=SOME_DEFINED, box=None, flags=None, undef=UNDEF, mistakes=()):
    """(quant float32 (nf, nlev, nq), flags int32 (nf, nlev))."""
    _check(mistakes)
    f = _fields(fields)
    nf, nlev, ny, nx = f.shape
    ps = np.asarray(percentiles, np.float32).ravel()
    bx = _box(box, ny, nx)
    fl = _flags(flags, nf, nlev)
    quant = np.full((nf, nlev, ps.size), np.float32(undef), np.float32)
    fd = np.full((nf, nlev), NONE_DEFINED, np.int32)
    for g in range(nf):
        for k in range(nlev):
            v = f[g, k][included(f[g, k], fl[g, k], mask, fdef_mask, bx, undef)]
            n = int(v.size)
            if n == 0:
                continue
            if "sort without signed zeros" in mistakes:  # ordered comparisons: the zeros stay as they came
                nan = np.isnan(v)
                x = np.concatenate([np.sort(v[~nan], kind="stable"), v[nan]])
            else:
                x = key_value(np.sort(order_key(v)))
            x = np.concatenate([x, [np.float32(undef)]])  # (what a rank that is not clamped reads)
            for q, p in enumerate(ps):
                kk, k1, t = rank(method, n, p, mistakes)
                quant[g, k, q] = interpolate(x[kk], x[k1], t, mistakes)
            fd[g, k] = ALL_DEFINED
    return quant, fd


def _total_order(x):
    """A sort key of Python floats for the total order: NaN last, -0 before +0."""
    return (1, 0.0, 0) if math.isnan(x) else (0, x, 0 if math.copysign(1.0, x) < 0 else 1)


def quantiles_literal(fields, percentiles, method=LINEAR, mask=None, fdef_mask=SOME_DEFINED, box=None, flags=None, undef=UNDEF):
    """The same from a Python sort of the included cells, cell by cell."""
    f = _fields(fields)
    nf, nlev, ny, nx = f.shape
    ps = [np.float32(p) for p in np.asarray(percentiles, np.float32).ravel()]
    i0, i1, j0, j1 = _box(box, ny, nx)
    fl = _flags(flags, nf, nlev)
    u = float(np.float32(undef))
    quant = np.full((nf, nlev, len(ps)), np.float32(undef), np.float32)
    fd = np.full((nf, nlev), NONE_DEFINED, np.int32)
    for g in range(nf):
        for k in range(nlev):
            vals = []
            for j in range(j0, j1):
                for i in range(i0, i1):
                    x = float(f[g, k, j, i])
                    if fl[g, k] != ALL_DEFINED and (math.isnan(x) or x == u):
                        continue
                    if mask is not None and fdef_mask != ALL_DEFINED:
                        m = float(np.float32(mask[j][i]))
                        if math.isnan(m) or m == u:
                            continue
                    vals.append(x)
            n = len(vals)
            if n == 0:
                continue
            vals.sort(key=_total_order)
            for q, p in enumerate(ps):
                if METHODS.get(method, method) == LOWER:
                    ii = min(int((np.float32(n) * p) / np.float32(100.0)), n - 1)
                    quant[g, k, q] = np.float32(vals[ii])
                else:
                    h = ((n - 1) * float(p)) / 100.0
                    kk = int(h)
                    t = h - kk
                    with np.errstate(all="ignore"):
                        quant[g, k, q] = np.float32(vals[kk]) if t == 0.0 else np.float32(np.float64(vals[kk]) + np.float64(t) * (np.float64(vals[kk + 1]) - np.float64(vals[kk])))
            fd[g, k] = ALL_DEFINED
    return quant, fd


# ----------------------------------------------------------------------------------------------- the digit plan, restated
DIGIT_BITS = 11


def digit_plan(kmin, kmax):
    """(prefix bits, passes, [(shift, width)] per pass) of the selection between two keys."""
    diff = int(kmin) ^ int(kmax)
    prefix = 32 if diff == 0 else 32 - diff.bit_length()
    left = 32 - prefix
    passes = -(-left // DIGIT_BITS)
    plan = []
    for _ in range(passes):
        w = min(left, DIGIT_BITS)
        left -= w
        plan.append((left, w))
    return prefix, passes, plan


def scan_step(hist, rank_):
    """(digit, rank inside the digit): the smallest d with hist[0] + ... + hist[d] > rank."""
    c = np.cumsum(np.asarray(hist, np.int64))
    d = int(np.searchsorted(c, rank_, side="right"))
    return d, int(rank_ - (c[d - 1] if d else 0))


# ------------------------------------------------------------------------------------------------------------ cases
def smooth_level(ny, nx, seed=0, base=280.0, span=25.0):
    """A synthetic temperature level: a smooth wave plus a little noise, float32."""
    rng = np.random.default_rng(seed)
    j, i = np.mgrid[0:ny, 0:nx]
    return (base + span * np.sin(2 * np.pi * i / max(nx, 2)) * np.cos(np.pi * j / max(ny, 2)) + rng.normal(0, 0.05, (ny, nx))).astype(np.float32)


def two_valued(bit, n=7, seed=0):
    """n float32 values of two kinds whose order keys first differ at `bit` (0 = the lowest), shuffled: (values, the
    smaller, the larger).  The keys are built, not searched: a positive value's key is its bits with the top bit set."""
    rng = np.random.default_rng(seed + bit)
    if bit == 31:  # across the sign
        lo, hi = np.float32(-1.5), np.float32(1.5)
    else:
        base = np.uint32(0x3F800000) if bit < 23 else np.uint32(0x00000001)  # 1.0, or the smallest subnormal for exponent bits
        base = np.uint32(base & ~np.uint32((1 << (bit + 1)) - 1)) | np.uint32(rng.integers(0, 1 << min(bit, 29)) if bit else 0)  # (bit 29 clear: never an infinity or a NaN)
        lo, hi = np.array([base, base | np.uint32(1 << bit)], np.uint32).view(np.float32)
        if np.isnan(hi) or np.isnan(lo):
            raise AssertionError("a NaN")
    kl, kh = int(order_key(np.array([lo]))[0]), int(order_key(np.array([hi]))[0])
    assert kl < kh and ((kl ^ kh).bit_length() - 1) == bit, (bit, hex(kl), hex(kh))
    v = np.array([lo] * (n // 2) + [hi] * (n - n // 2), np.float32)
    rng.shuffle(v)
    return v, lo, hi
