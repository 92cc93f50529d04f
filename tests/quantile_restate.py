"""Numpy restatement of mifc_ensembleQuantiles (include/mifc.h, "percentiles across ensemble members"): the oracle of
tests/test_gpu_ensemble_quantiles.py.  LOWER in float32 numpy, LINEAR step by step in float64 numpy (every ufunc
rounds once, so nothing is contracted)."""
import numpy as np

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
LOWER, LINEAR = 0, 1
UNDEF = np.float32(1.0e35)
PAD = np.uint32(0xFFFFFFFF)


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


def quantiles(members, percentiles, method, flags=None, undef=UNDEF):
    """members: float32 (nmem, nlev, ny, nx), or (nmem, ny, nx) for one level; flags: None (every member SOME_DEFINED),
    (nmem,) or (nmem, nlev).  Returns (out, fdefined): out (nq,) + the member shape, fdefined a list of nlev flags."""
    x = np.asarray(members, dtype=np.float32)
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

        def pick(r):
            r = np.clip(r, 0, nmem - 1).astype(np.int64)
            return unkeys(np.take_along_axis(k, r[None], axis=0)[0])

        for q, p in enumerate(ps):
            if method == LOWER:
                ii = ((n.astype(np.float32) * np.float32(p)) / np.float32(100.0)).astype(np.int64)  # float, truncated
                v = pick(np.minimum(ii, n - 1))
            else:
                h = ((n - 1).astype(np.float64) * np.float64(p)) / np.float64(100.0)
                kk = h.astype(np.int64)
                t = h - kk.astype(np.float64)
                xk, xk1 = pick(kk).astype(np.float64), pick(kk + 1).astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    lin = (xk + t * (xk1 - xk)).astype(np.float32)
                v = np.where(t == 0, pick(kk), lin)
            out[q] = np.where(n == 0, undef, v)
        fd = [classify(int(c), cells) for c in (n == 0).sum(axis=1)]
    out = out.reshape((ps.size, nlev, ny, nx))
    return (out[:, 0] if one_level else out), fd
