"""Numpy restatement of mifc_ensembleQuantiles (include/mifc.h, "percentiles across ensemble members"): the oracle of
tests/test_gpu_ensemble_quantiles.py.  LOWER in float32 numpy, LINEAR step by step in float64 numpy (every ufunc
rounds once, so nothing is contracted)."""
import numpy as np

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
LOWER, LINEAR = 0, 1
UNDEF = np.float32(1.0e35)
PAD = np.uint32(0xFFFFFFFF)

# not part of the definition: what tests/test_member_range_cpu.py shows the range cases (tests/member_range_cases.py) to
# tell from it.  "linear in float": rule LINEAR's a + t * (b - a) in float32; "linear contracted": t * (b - a) and the sum
# rounded once (an fma); "lerp": (1 - t) * a + t * b; "zeros equal": -0 and +0 share one key, +0 comes back; "flushed":
# subnormal inputs and results become zeros of their sign; "prefix one bit short": the bisection (more than 64 members)
# starts one bit below the true common prefix of the smallest and the largest counted key -- where they differ in their
# last two bits only, every rank comes back as the smallest.
MISTAKES = ("linear in float", "linear contracted", "lerp", "zeros equal", "flushed", "prefix one bit short")
_TINY = np.float32(np.finfo(np.float32).tiny)


def _flush(x):
    x = np.asarray(x, np.float32)
    return np.where((np.abs(x) < _TINY) & (x != 0), np.copysign(np.float32(0), x), x).astype(np.float32)


def _fma(t, d, a):
    """round(t * d + a) for float64 arrays, one rounding: the exact product as a sum of two doubles (Veltkamp / Dekker; every
    operand here is far from the ends of the double range), then the three terms added with the small ones first."""
    split = np.float64(134217729.0)  # 2^27 + 1

    def halves(v):
        c = split * v
        hi = c - (c - v)
        return hi, v - hi

    p = t * d
    th, tl = halves(t)
    dh, dl = halves(d)
    e = ((th * dh - p) + th * dl + tl * dh) + tl * dl  # p + e == t * d exactly
    s = a + p
    bb = s - a
    err = (a - (s - bb)) + (p - bb)  # a + p == s + err exactly
    r = s + (err + e)
    return np.where(np.isfinite(r), r, a + p)  # (an infinite operand: as the plain expression)


def keys(x):
    """Order-preserving uint32 keys: IEEE total order, -0 < +0; every NaN becomes 0xffffffff (above +inf)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32)
    k = np.where((b & np.uint32(0x80000000)) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(x), PAD, k).astype(np.uint32)


def unkeys(k):
    k = np.asarray(k, dtype=np.uint32)
    b = np.where((k & np.uint32(0x80000000)) != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)
    return b.view(np.float32)


def classify(n_undefined, n):
    """miutil::checkDefined, FieldDefined.cc:62-70."""
    if n_undefined == 0:
        return ALL_DEFINED
    return NONE_DEFINED if n_undefined == n else SOME_DEFINED


def quantiles(members, percentiles, method, flags=None, undef=UNDEF, mistakes=(), ranks=None):
    """members: float32 (nmem, nlev, ny, nx), or (nmem, ny, nx) for one level; flags: None (every member SOME_DEFINED),
    (nmem,) or (nmem, nlev).  Returns (out, fdefined): out (nq,) + the member shape, fdefined a list of nlev flags.
    mistakes: names from MISTAKES, not part of the definition.  ranks: a dict that receives what the cases' own tests read:
    "n" (nlev, cells) counted members, "kmin" / "kmax" their smallest / largest key, "t" (nq, nlev, cells) LINEAR's t."""
    assert all(m in MISTAKES for m in mistakes), mistakes
    x = np.asarray(members, dtype=np.float32)
    if "flushed" in mistakes:
        x = _flush(x)
    if "zeros equal" in mistakes:
        x = np.where(x == 0, np.float32(0), x).astype(np.float32)
    one_level = x.ndim == 3
    if one_level:
        x = x[:, None]
    nmem, nlev, ny, nx = x.shape
    cells = ny * nx
    x = x.reshape(nmem, nlev, cells)
    undef = np.float32(undef)
    ps = np.asarray(percentiles, dtype=np.float32).ravel()
    out = np.empty((ps.size, nlev, cells), np.float32)
    if nmem == 0:
        out[...] = undef
        fd = [NONE_DEFINED] * nlev
    else:
        with np.errstate(invalid="ignore"):
            d = ~np.isnan(x) & (x != undef)  # is_defined(in, undef)
        if flags is not None:
            f = np.asarray(flags).reshape(nmem, -1)
            d |= (np.broadcast_to(f, (nmem, nlev)) == ALL_DEFINED)[:, :, None]  # ALL_DEFINED: taken at its word
        k = np.sort(np.where(d, keys(x), PAD), axis=0)
        n = d.sum(axis=0)  # (nlev, cells)
        kmin, kmax = k[0], np.take_along_axis(k, np.clip(n - 1, 0, nmem - 1)[None], axis=0)[0]
        short = (nmem > 64) & ((kmin ^ kmax) < 4) if "prefix one bit short" in mistakes else np.zeros(n.shape, bool)
        if ranks is not None:
            ranks.update(n=n, kmin=kmin, kmax=kmax, t=np.zeros((ps.size, nlev, cells)))

        def pick(r):
            r = np.clip(r, 0, nmem - 1).astype(np.int64)
            return unkeys(np.where(short, kmin, np.take_along_axis(k, r[None], axis=0)[0]))

        for q, p in enumerate(ps):
            if method == LOWER:
                ii = ((n.astype(np.float32) * np.float32(p)) / np.float32(100.0)).astype(np.int64)  # float, truncated
                v = pick(np.minimum(ii, n - 1))
            else:
                h = ((n - 1).astype(np.float64) * np.float64(p)) / np.float64(100.0)
                kk = h.astype(np.int64)
                t = h - kk.astype(np.float64)
                xk, xk1 = pick(kk).astype(np.float64), pick(kk + 1).astype(np.float64)
                if ranks is not None:
                    ranks["t"][q] = np.where(n > 0, t, 0)
                with np.errstate(all="ignore"):
                    if "linear in float" in mistakes:
                        a32, b32 = xk.astype(np.float32), xk1.astype(np.float32)
                        lin = a32 + t.astype(np.float32) * (b32 - a32)
                    elif "linear contracted" in mistakes:
                        lin = _fma(t, xk1 - xk, xk).astype(np.float32)
                    elif "lerp" in mistakes:
                        lin = ((np.float64(1.0) - t) * xk + t * xk1).astype(np.float32)
                    else:
                        lin = (xk + t * (xk1 - xk)).astype(np.float32)
                v = np.where(t == 0, pick(kk), lin)
            out[q] = np.where(n == 0, undef, _flush(v) if "flushed" in mistakes else v)
        fd = [classify(int(c), cells) for c in (n == 0).sum(axis=1)]
    out = out.reshape((ps.size, nlev, ny, nx))
    return (out[:, 0] if one_level else out), fd
