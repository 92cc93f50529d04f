"""CPU checks of the semantics of mifc_vlayer_hlevels / mifc_vlayer_fields through their numpy restatement
(tests/vlayer_restate.py, the oracle of the GPU tests): hand-computed answers on short columns, the rules one by one, the
coverage of the main generator, and that the entries are declared, bound and configured where the others are."""
import os
import re

import numpy as np

import vlayer_restate as vl

U = vl.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = vl.ALL_PRODUCTS


def column(coord, values, lo=-vl.INF, hi=vl.INF, products=ALL, flags=None, fdef_coord=None, undef=U, bounds_as_fields=False):
    """One column (ny = nx = 1), one or several fields: returns (out[nf][nproducts], flags[nf][nproducts])."""
    v = np.atleast_2d(np.asarray(values, np.float32))
    c = np.asarray(coord, np.float32)
    if bounds_as_fields:
        lo, hi = np.full((1, 1), lo, np.float32), np.full((1, 1), hi, np.float32)
    out, fd = vl.coord_fields(v[:, :, None, None], c[:, None, None], products, lo, hi, flags, fdef_coord, undef)
    return out[:, :, 0, 0], fd


def f32(*xs):
    return [np.float32(x) for x in xs]


def test_layer_inside_a_three_level_column():
    # 600..700: values 15..20, 700..800: 20..30 -> 100 * 17.5 + 100 * 25 = 4250 over 200
    out, fd = column([500, 700, 900], [10, 20, 40], 600, 800)
    assert list(out[0]) == f32(4250, 21.25, 30, 15, 800, 600) and (fd == vl.ALL_DEFINED).all()


def test_the_same_column_given_bottom_up():
    out, fd = column([900, 700, 500], [40, 20, 10], 600, 800)
    assert list(out[0]) == f32(4250, 21.25, 30, 15, 800, 600) and (fd == vl.ALL_DEFINED).all()


def test_open_layer():
    out, _ = column([500, 700, 900], [10, 20, 40])
    assert list(out[0]) == f32(9000, 22.5, 40, 10, 900, 500)  # 200 * 15 + 200 * 30
    out, _ = column([500, 700, 900], [10, 20, 40], lo=600)  # open above only
    assert list(out[0]) == f32(100 * 17.5 + 6000, (1750 + 6000) / 300, 40, 15, 900, 600)


def test_only_the_products_asked_for_in_their_order():
    out, fd = column([500, 700, 900], [10, 20, 40], 600, 800, products=["coord_of_min", vl.INTEGRAL])
    assert list(out[0]) == f32(600, 4250) and fd.shape == (1, 2)


def test_non_monotone_column_counts_overlapping_pairs_twice():
    # 500 -> 900 -> 700: 700..900 is walked twice
    out, _ = column([500, 900, 700], [0, 40, 20])
    assert out[0, 0] == np.float32(400 * 20 + 200 * 30) and out[0, 1] == np.float32(14000 / 600)
    assert list(out[0, 2:]) == f32(40, 0, 900, 500)


def test_undefined_value_inside_and_outside_the_layer():
    out, fd = column([100, 200, 300, 400], [[1, U, 3, 4], [1, 2, 3, U]], 250, 350)
    # field 0: level 1 is an end of the pair (1, 2) that takes part; field 1: level 3 too (pair (2, 3): 300..350)
    assert (out == U).all() and (fd == vl.NONE_DEFINED).all()
    out, fd = column([100, 200, 300, 400], [[U, 2, 3, 4], [1, 2, 3, U]], 200, 300)
    assert list(out[0]) == f32(250, 2.5, 3, 2, 300, 200) and list(out[1]) == list(out[0]) and (fd == vl.ALL_DEFINED).all()
    # flagged ALL_DEFINED the stored undef is a value like any other
    flags = [[vl.SOME_DEFINED, vl.ALL_DEFINED, vl.SOME_DEFINED, vl.SOME_DEFINED]]
    out, _ = column([100, 200, 300, 400], [1, U, 3, 4], 100, 200, flags=flags)
    assert out[0, 2] == U and out[0, 4] == 200 and out[0, 0] == np.float32((1 + np.float64(U)) * 0.5 * 100)


def test_undefined_or_nan_coordinate_makes_the_cell_undefined_for_all_fields():
    for c, fc in (([100, U, 300, 400], None), ([100, 200, 300, np.nan], [vl.ALL_DEFINED] * 4), ([np.nan, 200, 300, 400], None)):
        out, fd = column(c, [[1, 2, 3, 4], [5, 6, 7, 8]], 100, 150, fdef_coord=fc)  # the layer is nowhere near the bad level
        assert (out == U).all() and (fd == vl.NONE_DEFINED).all()
    # an undefined ps: every level of the cell
    x = np.ones((1, 3, 1, 2), np.float32)
    al, bl = vl.hybrid_levels(3)
    out, fd = vl.hlevels(x, np.array([[1000, U]], np.float32), al, bl, [vl.MEAN])
    assert out[0, 0, 0, 0] == 1 and out[0, 0, 0, 1] == U and fd[0, 0] == vl.SOME_DEFINED


def test_per_cell_bounds_undefined_nan_and_crossing():
    c, x = [500, 700, 900], [10, 20, 40]
    good, _ = column(c, x, 600, 800, bounds_as_fields=True)
    assert list(good[0]) == f32(4250, 21.25, 30, 15, 800, 600)
    for lo, hi in ((U, 800), (600, U), (np.nan, 800), (600, np.nan), (800, 600), (700, 700)):
        out, fd = column(c, x, lo, hi, bounds_as_fields=True)
        assert (out == U).all() and (fd == vl.NONE_DEFINED).all(), (lo, hi)
    # as a scalar the undef value is a bound like any other (the host refuses what is not lo < hi)
    out, _ = column(c, x, 600, U)
    assert out[0, 0] == np.float32(1750 + 6000)


def test_layer_entirely_above_or_below_the_column():
    for lo, hi in ((100, 400), (100, 500), (900, 1000), (950, 1000)):  # touching an end is not taking part either
        out, fd = column([500, 700, 900], [10, 20, 40], lo, hi)
        assert (out == U).all() and (fd == vl.NONE_DEFINED).all(), (lo, hi)


def test_equal_neighbouring_coordinates_contribute_nothing_and_divide_nothing():
    out, fd = column([500, 700, 700, 900], [10, 20, 99, 40])
    # the pair (1, 2) has no extent: 99 is seen by the pair (2, 3) only
    assert list(out[0]) == f32(200 * 15 + 200 * 69.5, (3000 + 13900) / 400, 99, 10, 700, 500) and (fd == vl.ALL_DEFINED).all()
    out, _ = column([700, 700], [1, 2])
    assert (out == U).all()
    out, _ = column([-0.0, 0.0, 5], [1, 2, 4], products=[vl.INTEGRAL, vl.COORD_OF_MIN])
    assert out[0, 0] == 15 and out[0, 1].tobytes() == np.float32(0.0).tobytes()


def test_first_occurrence_wins_and_a_nan_that_comes_first_stays():
    out, _ = column([100, 200, 300, 400], [7, 3, 7, 3], products=[vl.COORD_OF_MAX, vl.COORD_OF_MIN])
    assert list(out[0]) == f32(100, 200)
    flags = [[vl.ALL_DEFINED] * 3]
    out, _ = column([100, 200, 300], [np.nan, 5, 9], flags=flags)
    assert np.isnan(out[0, 0]) and np.isnan(out[0, 2]) and np.isnan(out[0, 3]) and out[0, 4] == 100 and out[0, 5] == 100
    out, _ = column([100, 200, 300], [5, np.nan, 9], flags=flags)  # a later NaN never replaces
    assert list(out[0, 2:]) == f32(9, 5, 300, 100)


def test_flag_tri_state_and_nan_as_undef():
    x = np.zeros((1, 2, 1, 3), np.float32)
    x[0, 1] = 10
    c = np.zeros((2, 1, 3), np.float32)
    c[1] = 10
    out, fd = vl.coord_fields(x, c, [vl.MEAN, vl.MAX])
    assert list(fd[0]) == [vl.ALL_DEFINED] * 2 and (out[0, 0] == 5).all() and (out[0, 1] == 10).all()
    x[0, 0, 0, 1] = U
    out, fd = vl.coord_fields(x, c, [vl.MEAN, vl.MAX])
    assert list(fd[0]) == [vl.SOME_DEFINED] * 2 and out[0, 0, 0, 1] == U and out[0, 1, 0, 1] == U
    out, fd = vl.coord_fields(x, c, [vl.MEAN], lo=20, hi=30)
    assert fd[0, 0] == vl.NONE_DEFINED
    nan = np.float32(np.nan)
    x[0, 0, 0, 1] = nan
    out, fd = vl.coord_fields(x, c, [vl.MEAN], undef=nan)
    assert fd[0, 0] == vl.SOME_DEFINED and np.isnan(out[0, 0, 0, 1]) and out[0, 0, 0, 0] == 5


def test_main_generator_covers_defined_and_undefined_outputs():
    fields, ps, alevel, blevel = vl.main_case()
    assert fields.shape == (3, 12, 9, 13)
    shares = []
    for lo, hi in vl.MAIN_LAYERS:
        out, fd = vl.hlevels(fields, ps, alevel, blevel, ALL, lo, hi)
        shares.append(float((out != U).mean()))
    print("defined shares:", shares)
    assert shares[0] >= 0.5 and shares[1] >= 0.5 and shares[2] >= 0.5 and shares[3] == 0


def test_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_vlayer_hlevels", "mifc_vlayer_fields"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    for code, name in enumerate(("INTEGRAL", "MEAN", "MAX", "MIN", "COORD_OF_MAX", "COORD_OF_MIN"), 1):
        assert re.search(r"MIFC_VLAYER_%s = %d\b" % (name, code), header), name
    env = open(os.path.join(ROOT, "mi-fieldcalc_amd", "csrc", "mifc_env.hip")).read()
    assert '"MIFC_VLAYER_CHUNK_MIB"' in env
    host = open(os.path.join(ROOT, "mi-fieldcalc_amd", "csrc", "mifc_capi_vlayer.hip")).read()
    assert "getenv" not in host and re.search(r"vlayer_chunk_mib > 0 \? mifc::env\(\)\.vlayer_chunk_mib : 256", host)
