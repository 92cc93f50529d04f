"""CPU checks of the percentile semantics of mifc_ensembleQuantiles through its numpy restatement
(tests/quantile_restate.py, the oracle of the GPU tests): LOWER is the reference's neighbourFunctions percentile rule,
LINEAR is numpy's "linear" method, the result does not depend on member order, and -0 / +0 / NaN sort as specified."""
import numpy as np
import pytest

import neighbour_cases as nc
import quantile_restate as qr
from cases import same_bits


def window_members(field, r):
    """The (2r+1)^2 values of every centre cell's window as members, centres r .. n - r - 1."""
    ny, nx = field.shape
    return np.stack([field[r + dy:ny - r + dy, r + dx:nx - r + dx] for dy in range(-r, r + 1) for dx in range(-r, r + 1)])


def ulps(a, b):
    return np.abs(qr.keys(a).astype(np.int64) - qr.keys(b).astype(np.int64))


def test_lower_is_the_reference_percentile(tmp_path):
    if not nc.ref_available():
        pytest.skip("oracle/_ref/libmifc_ref.so not built (needs the reference sources at build time)")
    shim = nc.RefShim(tmp_path)
    nx, ny = 23, 17
    for r in (1, 2):
        for p in range(100):
            field = nc.make_field(nx, ny, 4000 + 100 * r + p, specials="zeros")  # no NaN: std::sort is undefined on it
            res = np.full((ny, nx), nc.SENTINEL, np.float32)
            ok, _ = shim.run("functions", nx, ny, field, [p, r, 1], 4, res, qr.ALL_DEFINED)
            assert ok, (r, p)
            got, _ = qr.quantiles(window_members(field, r), [p], qr.LOWER)
            # which zero the reference returns depends on std::sort's order of equal elements
            assert np.array_equal(nc.percentile_zero_equal(got[0]), nc.percentile_zero_equal(res[r:ny - r, r:nx - r])), (r, p)


def test_linear_is_numpy_linear_within_one_ulp():
    rng = np.random.default_rng(7)
    for nmem in (1, 2, 3, 7, 31, 51, 64, 65, 200):
        x = (rng.normal(0, 10, size=(nmem, 9, 11)) * rng.choice([1e-3, 1, 1e3], size=(nmem, 9, 11))).astype(np.float32)
        ps = [0, 2.5, 10, 33.3, 50, 90, 99.9, 100]
        got, fd = qr.quantiles(x, ps, qr.LINEAR)
        assert fd == [qr.ALL_DEFINED]
        exp = np.percentile(x.astype(np.float64), np.asarray(ps, np.float32).astype(np.float64), axis=0, method="linear").astype(np.float32)
        assert ulps(got, exp).max() <= 1, nmem


@pytest.mark.parametrize("method", [qr.LOWER, qr.LINEAR])
def test_member_order_does_not_matter(method):
    rng = np.random.default_rng(11)
    nmem, nlev = 40, 3
    x = np.round(rng.normal(0, 2, size=(nmem, nlev, 13, 10)) * 4).astype(np.float32) / 4
    m = rng.random(x.shape)
    x[m < 0.05] = -0.0
    x[(m >= 0.05) & (m < 0.1)] = 0.0
    x[(m >= 0.1) & (m < 0.2)] = qr.UNDEF
    x[(m >= 0.2) & (m < 0.22)] = np.nan
    x[(m >= 0.22) & (m < 0.24)] = np.inf
    flags = rng.choice([qr.ALL_DEFINED, qr.SOME_DEFINED, qr.NONE_DEFINED], size=(nmem, nlev))
    ps = [0, 10, 50, 90, 100]
    ref, fd = qr.quantiles(x, ps, method, flags)
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(nmem)
        got, fd2 = qr.quantiles(x[perm], ps, method, flags[perm])
        assert same_bits(got, ref) and fd2 == fd


def test_signed_zeros_nan_and_undefined_members():
    one = lambda vals, p, method, flags=None, undef=qr.UNDEF: qr.quantiles(  # noqa: E731
        np.asarray(vals, np.float32).reshape(-1, 1, 1), [p], method, flags, undef)[0][0, 0, 0]
    bits = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    for method in (qr.LOWER, qr.LINEAR):
        assert bits(one([0.0, -0.0], 0, method)) == 0x80000000  # -0 < +0
        assert bits(one([0.0, -0.0], 100, method)) == 0x00000000
        assert bits(one([-0.0, 0.0, -0.0], 50, method)) == 0x80000000
        assert one([np.inf, -np.inf, 1], 0, method) == -np.inf
        assert one([np.inf, -np.inf, 1], 100, method) == np.inf
    # NaN only through an ALL_DEFINED member, above +inf
    nan_all = [np.nan, np.inf, 1.0]
    assert one(nan_all, 0, qr.LOWER, [0, 0, 0]) == 1.0
    assert one(nan_all, 50, qr.LOWER, [0, 0, 0]) == np.inf  # ii = (int)(3 * 50 / 100) = 1
    assert np.isnan(one(nan_all, 100, qr.LOWER, [0, 0, 0]))
    assert np.isnan(one(nan_all, 75, qr.LINEAR, [0, 0, 0]))  # between +inf and NaN
    assert one(nan_all, 100, qr.LOWER, [2, 2, 2]) == np.inf  # not ALL_DEFINED: the NaN does not count
    # undefined members do not count; a cell without any is undef, and so is its flag
    assert one([qr.UNDEF, 3.0, 5.0], 0, qr.LOWER) == 3.0
    assert one([qr.UNDEF, 3.0, 5.0], 50, qr.LINEAR) == 4.0
    assert one([qr.UNDEF, 3.0], 100, qr.LOWER, [0, 2]) == qr.UNDEF  # taken at its word: the stored value
    out, fd = qr.quantiles(np.full((3, 2, 2), qr.UNDEF, np.float32), [50], qr.LINEAR)
    assert (out == qr.UNDEF).all() and fd == [qr.NONE_DEFINED]
    # NaN as undef: every NaN is undefined unless its member is ALL_DEFINED
    assert one([np.nan, 2.0, 4.0], 0, qr.LOWER, undef=np.nan) == 2.0
    # LOWER: truncation in float, clamped to n - 1; LINEAR: t == 0 takes the stored value
    assert one([1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 99.9, qr.LOWER) == 10.0
    assert one([1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 10, qr.LOWER) == 2.0
    assert one([1, 2, 3, 4, 5], 25, qr.LINEAR) == 2.0
    assert one([1, 2, 3, 4, 5], 10, qr.LINEAR) == np.float32(1.4)
    # no members at all: undef, NONE_DEFINED
    out, fd = qr.quantiles(np.zeros((0, 2, 3, 4), np.float32), [50], qr.LOWER)
    assert out.shape == (1, 2, 3, 4) and (out == qr.UNDEF).all() and fd == [qr.NONE_DEFINED] * 2
