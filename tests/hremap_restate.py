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


# Departures from the definition that a test may ask for by name (`mistakes`): what a kernel that is subtly wrong would
# compute.  tests/test_horizontal_range_cpu.py shows that the cases of tests/horizontal_range_cases.py tell each from the rules.
MISTAKES = ("padding added as zero", "greater in place of greater or equal", "undef after the fact")
SLICE = 64  # destinations of a slice of the plan's layout: its rows are padded to the longest of them


def padding_columns(rowptr, col):
    """The source cell that the padding entries of each row name in the plan's layout (mifc_hremap_plan.h): the row's first
    column, 0 for an empty row; and the width of each row's slice."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    length = np.diff(rowptr)
    first = np.where(length > 0, col[np.minimum(rowptr[:-1], max(col.size - 1, 0))] if col.size else 0, 0)
    width = np.concatenate([np.full(length[s:s + SLICE].size, length[s:s + SLICE].max()) for s in range(0, length.size, SLICE)])
    return first, width


def remap(fields, rowptr, col, w, mode=STRICT, min_frac=0.0, flags=None, undef=UNDEF, mistakes=()):
    """fields float32 (nf, nlev, ny, nx) or (nf, nlev, nsrc); the table in CSR form; flags None (SOME_DEFINED) or
    (nf, nlev).  Returns (out float32 (nf, nlev, ndst), flags_out int32 (nf, nlev)).  mistakes: not part of the
    definition -- names from MISTAKES: "padding added as zero" adds 0 * x of the padding cell for the trips between a row's
    end and the width of its slice; "greater in place of greater or equal" in the min_frac test; "undef after the fact"
    takes a result equal to undef for a hole."""
    assert all(m in MISTAKES for m in mistakes), mistakes
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
                    if "padding added as zero" in mistakes:
                        pad_col, width = padding_columns(rowptr, col)
                        padding = ~active & (r < width)
                        c, we = np.where(padding, pad_col, c), np.where(padding, 0.0, we)
                    x = lev[c]
                    ok = is_defined(all_defined, x, undef)
                    use = active & ok
                    if "padding added as zero" in mistakes:
                        use = use | padding  # (the sums only: such an entry is not counted as bad)
                    prod = we * x.astype(np.float64)
                    S = np.where(use, S + prod, S)
                    wdef = np.where(use, wdef + we, wdef)
                    nbad = nbad + (active & ~ok)
                plain = S.astype(np.float32)
                if mode == STRICT:
                    hole = (length == 0) | (nbad > 0)
                    res = plain
                else:
                    enough = np.greater if "greater in place of greater or equal" in mistakes else np.greater_equal
                    lost = (nbad == length) | (wdef == 0.0) | ~enough(np.abs(wdef), np.float64(min_frac) * np.abs(wall))
                    hole = (length == 0) | ((nbad > 0) & lost)
                    res = np.where(nbad > 0, ((S / wdef) * wall).astype(np.float32), plain)
                if "undef after the fact" in mistakes:
                    hole = hole | (res == undef)
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
