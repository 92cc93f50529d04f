"""The numpy restatement of the neighbourhood statistics (tests/neighbour_restate.py) against the compiled reference,
bit for bit, and the reference gtest's known answers (test/FieldCalculationsTest.cc:307-451) restated.  No GPU."""
import numpy as np
import pytest

import neighbour_cases as nc
import neighbour_restate as nr


def same(a, b, percentile=False):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if percentile:
        a, b = nc.percentile_zero_equal(a), nc.percentile_zero_equal(b)
    an, bn = np.isnan(a), np.isnan(b)
    return np.array_equal(an, bn) and np.array_equal(a[~an].view(np.uint32), b[~bn].view(np.uint32))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    if not nc.ref_available():
        pytest.skip("oracle/_ref/libmifc_ref.so not built (needs the reference sources at build time)")
    return nc.RefShim(tmp_path_factory.mktemp("nbshim"))


@pytest.mark.parametrize("nx,ny", [(23, 17), (9, 12)])
def test_restatement_is_the_reference_bit_for_bit(shim, nx, ny):
    checked = 0
    for k, (which, compute, consts, specials) in enumerate(nc.sweep(nx, ny)):
        field = nc.make_field(nx, ny, 1000 + k, specials)
        mine = np.full((ny, nx), nc.SENTINEL, np.float32)  # cells nobody writes are compared too
        status, flag = nr.run(which, nx, ny, field, consts, compute, mine, nr.ALL_DEFINED, nc.UNDEF)
        if status == "refused":  # the reference is undefined there (its own test: tests/test_gpu_neighbour.py)
            continue
        theirs = np.full((ny, nx), nc.SENTINEL, np.float32)
        ok, rflag = shim.run(which, nx, ny, field, consts, compute, theirs, nr.ALL_DEFINED)
        label = (which, compute, consts, nx, ny)
        assert ok == (status == "ok") and rflag == flag, label
        assert same(mine, theirs, percentile=(which == "functions" and compute == 4)), label
        checked += 1
    assert checked > 100


def test_flags_and_too_few_constants(shim):
    nx, ny = 12, 10
    field = nc.make_field(nx, ny, 7)
    for which, consts, compute in (("prob", [1], 5), ("functions", [], 1), ("functions", [2], 4), ("functions", [2], 5)):
        for flag in (nr.ALL_DEFINED, nr.SOME_DEFINED):
            a = np.full((ny, nx), nc.SENTINEL, np.float32)
            b = a.copy()
            assert nr.run(which, nx, ny, field, consts, compute, a, flag, nc.UNDEF)[0] == "false"
            assert shim.run(which, nx, ny, field, consts, compute, b, flag)[0] is False
            assert (a == nc.SENTINEL).all() and (b == nc.SENTINEL).all()
    for which, consts, compute in (("prob", [1, 2], 5), ("functions", [1], 2)):  # SOME_DEFINED input: false
        a = np.full((ny, nx), nc.SENTINEL, np.float32)
        assert nr.run(which, nx, ny, field, consts, compute, a, nr.SOME_DEFINED, nc.UNDEF) == ("false", nr.SOME_DEFINED)
        assert shim.run(which, nx, ny, field, consts, compute, a.copy(), nr.SOME_DEFINED) == (False, nr.SOME_DEFINED)


def test_beyond_2_pow_24_cells_the_count_is_exact_and_the_reference_is_not(shim):
    """Deviation 7: the reference's float summed-area table rounds once nx * ny > 2^24; the restatement (and the GPU)
    count exactly.  Shown on a 4400 x 4400 field (19.4 M cells, 18.4 M of them counted)."""
    nx = ny = 4400
    rng = np.random.default_rng(24)
    field = (rng.random((ny, nx)) < 0.95).astype(np.float32)
    r = 2
    mine = np.empty((ny, nx), np.float32)
    assert nr.run("prob", nx, ny, field, [0, r], 5, mine, nr.ALL_DEFINED, nc.UNDEF) == ("ok", nr.SOME_DEFINED)
    # exact-integer restatement, independently: the count of ones in every box by direct shifts
    hit = field > 0
    cnt = np.zeros((ny - 2 * r, nx - 2 * r), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            cnt += hit[dy : ny - 2 * r + dy, dx : nx - 2 * r + dx]
    assert np.array_equal(mine[r:-r, r:-r], cnt.astype(np.float32) / np.float32(25))
    theirs = np.empty((ny, nx), np.float32)
    assert shim.run("prob", nx, ny, field, [0, r], 5, theirs, nr.ALL_DEFINED) == (True, nr.SOME_DEFINED)
    differ = mine[r:-r, r:-r] != theirs[r:-r, r:-r]
    assert differ.any()  # rounded sums
    assert not differ[: 2000, : 2000].any()  # where the table is still below 2^24 the two agree


# ---- the reference gtest (test/FieldCalculationsTest.cc:307-451), restated -------------------------------------------
GT_UNDEF = np.float32(123456)


def gtest_runs(run):
    """Runs the gtest's calls through run(which, field, constants, compute, out, flag) -> (ok, flag); returns a list of
    (label, ok, flag, out) for the assertions of gtest_expectations."""
    NX = NY = 10
    res = []
    infield = np.zeros(NX * NY, np.float32)
    out = np.full(NX * NY, GT_UNDEF / 2, np.float32)
    res.append(("range>nx",) + run("functions", infield, [NX + 1], 2, out.copy(), nr.ALL_DEFINED))
    res.append(("step0",) + run("functions", infield, [NX, 0], 2, out.copy(), nr.ALL_DEFINED))
    infield = np.zeros(NX * NY, np.float32)
    infield[16] = 6
    res.append(("max",) + run("functions", infield, [3, 3], 2, out.copy(), nr.ALL_DEFINED))
    infield = np.zeros(NX * NY, np.float32)
    infield[[25, 26, 35, 36]] = 6
    res.append(("pct",) + run("functions", infield, [90, 2, 1], 4, out.copy(), nr.ALL_DEFINED))
    res.append(("f5",) + run("functions", infield, [5, 2, 1], 5, out.copy(), nr.ALL_DEFINED))
    res.append(("p5",) + run("prob", infield, [5, 2, 1], 5, out.copy(), nr.ALL_DEFINED))
    res.append(("f6",) + run("functions", infield, [5, 3, 1], 6, out.copy(), nr.ALL_DEFINED))
    res.append(("p6",) + run("prob", infield, [5, 3, 1], 6, out.copy(), nr.ALL_DEFINED))
    return res


def gtest_expectations(res):
    NX = NY = 10
    r = {row[0]: row[1:] for row in res}
    assert r["range>nx"][0] is False and r["step0"][0] is False
    for key in ("max", "pct", "f5", "p5", "f6", "p6"):
        assert r[key][0] is True and r[key][1] == nr.SOME_DEFINED, key
    exp_max = np.empty((NY, NX), np.float32)
    exp_pct = np.empty((NY, NX), np.float32)
    exp_5 = np.empty((NY, NX), np.float32)
    exp_6 = np.empty((NY, NX), np.float32)
    for i in range(NX):
        for j in range(NY):
            border2 = i < 2 or i >= NX - 2 or j < 2 or j >= NY - 2
            exp_max[j, i] = GT_UNDEF if border2 else (6 if j < 5 else 0)
            exp_pct[j, i] = GT_UNDEF if border2 else (6 if (3 < i < 8 and 1 < j < 5) else 0)
            if border2:
                exp_5[j, i] = GT_UNDEF
            elif i > 3 and j < 5:
                exp_5[j, i] = np.float32(0.16)
            elif i == 3 and j == 5:
                exp_5[j, i] = np.float32(0.04)
            elif i > 2 and j < 6:
                exp_5[j, i] = np.float32(0.08)
            else:
                exp_5[j, i] = 0
            border3 = i < 3 or i >= NX - 3 or j < 3 or j >= NY - 3
            exp_6[j, i] = GT_UNDEF if border3 else np.float32(45.0 / 49.0 if j < 6 else 47.0 / 49.0)
    assert np.array_equal(np.asarray(r["max"][2]).reshape(NY, NX), exp_max)
    assert np.array_equal(np.asarray(r["pct"][2]).reshape(NY, NX), exp_pct)
    assert np.array_equal(np.asarray(r["f5"][2]).reshape(NY, NX), exp_5)  # EXPECT_EQ against float(0.16) etc.
    np.testing.assert_array_equal(np.asarray(r["f5"][2]), np.asarray(r["p5"][2]))
    np.testing.assert_allclose(np.asarray(r["f6"][2]).reshape(NY, NX), exp_6, rtol=4 * np.finfo(np.float32).eps)  # EXPECT_FLOAT_EQ
    np.testing.assert_array_equal(np.asarray(r["f6"][2]), np.asarray(r["p6"][2]))


def test_gtest_neighbour_known_answers_restated():
    def run(which, field, consts, compute, out, flag):
        status, f = nr.run(which, 10, 10, field, consts, compute, out, flag, GT_UNDEF)
        return status == "ok", f, out

    gtest_expectations(gtest_runs(run))


def test_gtest_neighbour_known_answers_reference(shim):
    def run(which, field, consts, compute, out, flag):
        ok, f = shim.run(which, 10, 10, field, consts, compute, out, flag, GT_UNDEF)
        return ok, f, out

    gtest_expectations(gtest_runs(run))


def test_restatement_refusals():
    """The cases where the reference is undefined are refused (status "refused", nothing written); the GPU library
    refuses the same cases with a message (tests/test_gpu_neighbour.py)."""
    nx, ny = 12, 10
    field = nc.make_field(nx, ny, 3)
    for which, consts, compute in nc.DEVIATIONS:
        out = np.full((ny, nx), nc.SENTINEL, np.float32)
        f = field if consts != "alias" else out
        c = [1, 1] if consts == "alias" else consts
        assert nr.run(which, nx, ny, f, c, compute, out, nr.ALL_DEFINED, nc.UNDEF) == ("refused", nr.ALL_DEFINED), (which, consts, compute)
        if consts != "alias":
            assert (out == nc.SENTINEL).all()
