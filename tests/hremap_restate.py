"""Numpy restatement of mifc_hremap_levels (include/mifc.h, "level batches regridded by a sparse weight table"): the
oracle of tests/test_gpu_hremap.py.  Trips over r up to the longest row with a mask, as the kernel walks a slice: trip r
adds entry r of every row that has one, so every row is summed sequentially in its own order; every sum in float64, every
ufunc rounds once (nothing is contracted), the result rounded to float32 once.  Also the seeded case makers."""
import numpy as np

from vinterp_restate import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF, classify, is_defined, sprinkle  # noqa: F401

STRICT, RENORM = 0, 1
MODES = {"strict": STRICT, "renorm": RENORM}


def row_sums(rowptr, w):
    """Wall per row: the sequential float64 sum of the row's weights from +0.0."""
    rowptr, w = np.asarray(rowptr, np.int64), np.asarray(w, np.float32)
    ndst = rowptr.size - 1
    length = np.diff(rowptr)
    wall = np.zeros(ndst, np.float64)
    for r in range(int(length.max()) if ndst else 0):
        active = r < length
        e = np.where(active, rowptr[:-1] + r, 0)
        we = w[e].astype(np.float64) if w.size else np.zeros(ndst)
        wall = np.where(active, wall + we, wall)
    return wall


def remap(fields, rowptr, col, w, mode=STRICT, min_frac=0.0, flags=None, undef=UNDEF):
    """fields float32 (nf, nlev, ny, nx) or (nf, nlev, nsrc); the table in CSR form; flags None (SOME_DEFINED) or
    (nf, nlev).  Returns (out float32 (nf, nlev, ndst), flags_out int32 (nf, nlev))."""
    f = np.asarray(fields, np.float32)
    nf, nlev = f.shape[:2]
    f = f.reshape(nf, nlev, -1)
    rowptr, col, w = np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, np.float32)
    ndst = rowptr.size - 1
    undef = np.float32(undef)
    mode = MODES.get(mode, mode)
    assert mode in (STRICT, RENORM)
    fl = np.full((nf, nlev), SOME_DEFINED) if flags is None else np.asarray(flags).reshape(nf, nlev)
    length = np.diff(rowptr)
    trips = int(length.max()) if ndst else 0
    wall = row_sums(rowptr, w)
    out = np.full((nf, nlev, ndst), undef, np.float32)
    fd = np.zeros((nf, nlev), np.int32)
    with np.errstate(all="ignore"):
        for g in range(nf):
            for k in range(nlev):
                lev = f[g, k]
                all_defined = fl[g, k] == ALL_DEFINED
                S, wdef, nbad = np.zeros(ndst, np.float64), np.zeros(ndst, np.float64), np.zeros(ndst, np.int64)
                for r in range(trips):
                    active = r < length
                    e = np.where(active, rowptr[:-1] + r, 0)
                    c = col[e] if col.size else np.zeros(ndst, np.int64)
                    we = (w[e] if w.size else np.zeros(ndst, np.float32)).astype(np.float64)
                    x = lev[c]
                    ok = is_defined(all_defined, x, undef)
                    use = active & ok
                    prod = we * x.astype(np.float64)
                    S = np.where(use, S + prod, S)
                    wdef = np.where(use, wdef + we, wdef)
                    nbad = nbad + (active & ~ok)
                plain = S.astype(np.float32)
                if mode == STRICT:
                    hole = (length == 0) | (nbad > 0)
                    res = plain
                else:
                    lost = (nbad == length) | (wdef == 0.0) | ~(np.abs(wdef) >= np.float64(min_frac) * np.abs(wall))
                    hole = (length == 0) | ((nbad > 0) & lost)
                    res = np.where(nbad > 0, ((S / wdef) * wall).astype(np.float32), plain)
                out[g, k] = np.where(hole, undef, res)
                fd[g, k] = classify(int(hole.sum()), ndst)
    return out, fd


# ---------------------------------------------------------------------------------------------- case generators
def table_from_lengths(lengths, nsrc, seed=1, negative=False):
    """A table whose row d has lengths[d] entries: columns drawn from [0, nsrc) (repeats happen), weights uniform in
    (0, 1] scaled so that a row sums to about 1 -- with `negative` a fifth of them negated."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    rowptr = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    nnz = int(rowptr[-1])
    col = rng.integers(0, nsrc, nnz)
    w = rng.uniform(0.05, 1.0, nnz) / np.maximum(np.repeat(lengths, lengths), 1) * 2.0
    if negative:
        w = np.where(rng.uniform(size=nnz) < 0.2, -w, w)
    return rowptr.astype(np.int32), col.astype(np.int32), w.astype(np.float32)


def main_lengths(ndst, seed=1):
    """Row lengths 0..9 at random, with an empty row and a row of 17 where there is room."""
    rng = np.random.default_rng(seed + 500)
    lengths = rng.integers(0, 10, ndst)
    if ndst >= 8:
        lengths[ndst // 3] = 0
        lengths[ndst // 2] = 17
    return lengths


def main_fields(nf=1, nlev=1, ny=9, nx=13, seed=1, undef=UNDEF, frac=0.06):
    """Fields N(280 - 5 f, 10) with 6 % undefined cells."""
    rng = np.random.default_rng(seed)
    return np.stack([sprinkle((rng.normal(0, 10, (nlev, ny, nx)) + 280 - 5 * f).astype(np.float32), rng, frac, undef) for f in range(nf)])


def main_case(nf=1, nlev=1, ny=9, nx=13, ndst=600, seed=1, undef=UNDEF, frac=0.06):
    return main_fields(nf, nlev, ny, nx, seed, undef, frac), table_from_lengths(main_lengths(ndst, seed), ny * nx, seed)
