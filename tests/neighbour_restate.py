"""numpy restatement of the neighbourhood statistics (FieldCalculations.cc:2862-3061), the checker of
tests/test_neighbour_cpu.py and tests/test_gpu_neighbour.py.

Mean / max / min walk the window offsets in the reference's order (row outer, column inner), vectorised over the
centres, in float32: every centre's chain sees its values in the reference's order, so the results are the
reference's bits.  Percentiles sort (np.sort); counts are int64 sums, i.e. exact (the reference's float summed-area
table is exact only while nx * ny <= 2^24).  The border and the step x step blocks follow the reference loops.

Each function works on `fres` in place and returns (status, flag): status "ok", "false" (the reference's own
`return false`) or "refused" (a case where the reference is undefined and the library refuses, DESIGN.md
"Neighbourhood statistics"); nothing is written unless status is "ok".
"""
import numpy as np

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
F32 = np.float32


def to_int(c):
    """`int x = constants[k]` where it is defined (truncation), None where it is not."""
    c = F32(c)
    if not (c >= -2147483648.0 and c < 2147483648.0):
        return None
    return int(c)


def box_counts(hit, r):
    """Exact (2r+1)^2 box counts of the 0/1 field `hit` at the centres [r, ny-r) x [r, nx-r)."""
    ny, nx = hit.shape
    s = np.zeros((ny + 1, nx + 1), np.int64)
    s[1:, 1:] = hit.astype(np.int64).cumsum(0).cumsum(1)
    w = 2 * r + 1
    return s[w:, w:] - s[: ny + 1 - w, w:] - s[w:, : nx + 1 - w] + s[: ny + 1 - w, : nx + 1 - w]


def _hit(f, compute, limit):
    lim = F32(limit)
    return (f > lim) if compute == 5 else (f < lim)  # a NaN compares false


def neighbour_prob(nx, ny, field, constants, compute, fres, fdefined, undef):
    """neighbourProbFunctions :2862."""
    if fdefined != ALL_DEFINED:
        return "false", fdefined
    if len(constants) < 2:
        return "false", fdefined
    limit, rng = to_int(constants[0]), to_int(constants[1])
    if limit is None or rng is None:
        return "refused", fdefined
    if rng < 0 or rng > nx or rng > ny:
        return "refused", fdefined
    f = np.asarray(field, F32).reshape(ny, nx)
    out = fres.reshape(ny, nx)
    if rng == 0:
        if compute in (5, 6):
            out[...] = _hit(f, compute, limit).astype(F32)
        return "ok", fdefined
    if compute not in (5, 6):
        return "refused", fdefined
    hit = _hit(f, compute, limit)  # read before anything is written: field may be fres
    res = np.full((ny, nx), F32(undef), F32)
    if nx > 2 * rng and ny > 2 * rng:
        res[rng : ny - rng, rng : nx - rng] = box_counts(hit, rng).astype(F32) / F32((2 * rng + 1) ** 2)
    out[...] = res
    return "ok", SOME_DEFINED


def _centre_values(f, compute, rng, step, limit, ii, cy, cx):
    ngridp = F32((2 * rng + 1) ** 2)
    w = 2 * rng + 1
    shape = (len(cy), len(cx))
    if compute == 4:
        vals = np.empty(shape + (w * w,), F32)
        for k in range(w):
            for l in range(w):
                vals[..., k * w + l] = f[np.ix_(cy - rng + k, cx - rng + l)]
        return np.sort(vals, axis=-1)[..., ii]
    if compute not in (1, 2, 3, 5, 6):
        return np.zeros(shape, F32)  # 0.0 (compute > 4: 0.0 / ngridp, still +0)
    v = f[np.ix_(cy - rng, cx - rng)].copy() if compute in (2, 3) else np.zeros(shape, F32)
    cnt = np.zeros(shape, np.int64)
    lim = F32(limit)
    for k in range(w):
        rows = cy - rng + k
        for l in range(w):
            t = f[np.ix_(rows, cx - rng + l)]
            if compute == 1:
                v = v + t
            elif compute == 2:
                v = np.where(t > v, t, v)
            elif compute == 3:
                v = np.where(t < v, t, v)
            elif compute == 5:
                cnt += t > lim
            else:
                cnt += t < lim
    if compute in (5, 6):
        v = cnt.astype(F32)
    if compute in (1, 5, 6):
        v = (v / ngridp).astype(F32)
    return v.astype(F32)


def neighbour_functions(nx, ny, field, constants, compute, fres, fdefined, undef):
    """neighbourFunctions :2955."""
    if fdefined != ALL_DEFINED:
        return "false", fdefined
    n = len(constants)
    if n < 1 or (n < 2 and compute > 3):
        return "false", fdefined
    rng, step, limit = 3, 3, 0
    if compute < 4:
        rng = to_int(constants[0])
        if n == 2:
            step = to_int(constants[1])
    else:
        limit, rng = to_int(constants[0]), to_int(constants[1])
        if n == 3:
            step = to_int(constants[2])
    if rng is None or step is None or limit is None:
        return "refused", fdefined
    if rng > nx or rng > ny or rng < 1:
        return "false", fdefined
    if step < 1:
        return "false", fdefined
    if step // 2 > rng:
        return "refused", fdefined
    ngridp = F32((2 * rng + 1) ** 2)
    ii = 0
    if compute == 4:
        q = F32(F32(ngridp * F32(limit)) / F32(100))
        if not (q > -1 and q < ngridp):
            return "refused", fdefined
        ii = int(q)
    if np.shares_memory(field, fres):
        return "refused", fdefined
    f = np.asarray(field, F32).reshape(ny, nx)
    out = fres.reshape(ny, nx)
    # the border first (:2988-3005) ...
    u = F32(undef)
    out[:rng, :] = u
    out[rng : max(ny - rng, rng), :rng] = u
    out[rng : max(ny - rng, rng), nx - rng :] = u
    out[ny - rng :, :] = u
    # ... then the centres' blocks (:3009-3048), disjoint because step / 2 <= range
    cy = np.arange(rng, ny - rng, step)
    cx = np.arange(rng, nx - rng, step)
    if len(cy) and len(cx):
        chunk = max(1, (1 << 22) // max(1, len(cx) * (2 * rng + 1) ** 2)) if compute == 4 else len(cy)
        for a in range(0, len(cy), chunk):
            ys = cy[a : a + chunk]
            v = _centre_values(f, compute, rng, step, limit, ii, ys, cx)
            for dy in range(-((step - 1) // 2), step // 2 + 1):
                for dx in range(-((step - 1) // 2), step // 2 + 1):
                    out[np.ix_(ys + dy, cx + dx)] = v
    return "ok", SOME_DEFINED


def run(which, nx, ny, field, constants, compute, fres, fdefined, undef):
    fn = neighbour_prob if which == "prob" else neighbour_functions
    return fn(nx, ny, field, constants, compute, fres, fdefined, undef)
