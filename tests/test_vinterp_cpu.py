"""CPU checks of the semantics of mifc_vinterp_hlevels / mifc_vinterp_fields through their numpy restatement
(tests/vinterp_restate.py, the oracle of the GPU tests): hand-computed answers on columns of 2 to 4 levels, and the
coverage of the main generator."""
import numpy as np

import vinterp_restate as vr

U = vr.UNDEF


def column(coord, values, targets, method=vr.LINEAR, flags=None, fdef_coord=None, undef=U):
    """One column (ny = nx = 1), one or several fields: returns (out[nf][nt], flags[nf][nt])."""
    v = np.atleast_2d(np.asarray(values, np.float32))
    c = np.asarray(coord, np.float32)
    out, fd = vr.coord_fields(v[:, :, None, None], c[:, None, None], targets, method, flags, fdef_coord, undef)
    return out[:, :, 0, 0], fd


def test_linear_between_two_levels():
    out, fd = column([500, 700], [10, 20], [600, 550])
    assert out[0, 0] == np.float32(15) and out[0, 1] == np.float32(12.5) and list(fd[0]) == [vr.ALL_DEFINED] * 2


def test_target_on_a_level_returns_the_level_bit_for_bit():
    x0 = np.float32(0.1) * np.float32(3)  # an awkward float
    out, _ = column([500, 700, 900], [x0, 7, 9], [500, 700, 900])
    assert out[0, 0].tobytes() == x0.tobytes()  # w = 0: x_k + 0 * (..)
    assert out[0, 1] == np.float32(7)  # first bracket (500, 700) with w = 1: 10 * .. exact here
    assert out[0, 2] == np.float32(9)


def test_equal_coordinates_give_the_first_value_without_a_division():
    out, fd = column([700, 700, 800], [3, 5, 9], [700])
    assert out[0, 0] == np.float32(3) and fd[0, 0] == vr.ALL_DEFINED  # 0 / 0 would have been NaN
    out, _ = column([700, 700], [np.float32(-0.0), 5], [700])
    assert out[0, 0].tobytes() == np.float32(-0.0).tobytes()


def test_first_bracket_on_a_non_monotone_column():
    # 300 -> 800 -> 400 -> 900: 600 lies in all three pairs, 850 only in the last
    out, _ = column([300, 800, 400, 900], [0, 10, 20, 30], [600, 850])
    assert out[0, 0] == np.float32(6)  # pair (0, 1): w = 0.6
    assert out[0, 1] == np.float32(29)  # pair (2, 3): w = 0.9


def test_levels_given_bottom_up():
    down, _ = column([200, 500, 1000], [1, 2, 3], [350, 750])
    up, _ = column([1000, 500, 200], [3, 2, 1], [350, 750])
    assert list(down[0]) == [np.float32(1.5), np.float32(2.5)] and list(up[0]) == list(down[0])


def test_undefined_value_at_the_bracket_and_elsewhere():
    out, fd = column([100, 200, 300, 400], [[1, U, 3, 4], [1, 2, 3, U]], [150, 250, 350])
    assert list(out[0]) == [U, U, np.float32(3.5)]  # field 0: undefined at level 1, an end of the first two brackets
    assert list(out[1]) == [np.float32(1.5), np.float32(2.5), U]
    assert list(fd[:, 0]) == [vr.NONE_DEFINED, vr.ALL_DEFINED]
    # flagged ALL_DEFINED the stored undef is a value like any other
    flags = [[vr.SOME_DEFINED, vr.ALL_DEFINED, vr.SOME_DEFINED, vr.SOME_DEFINED]] * 2
    out, _ = column([100, 200, 300, 400], [[1, U, 3, 4], [1, 2, 3, U]], [150], flags=flags)
    assert out[0, 0] == np.float32((1 + 0.5 * (np.float64(U) - 1)))
    # an undefined coordinate: its two pairs cannot bracket
    out, fd = column([100, U, 300, 400], [1, 2, 3, 4], [150, 350])
    assert list(out[0]) == [U, np.float32(3.5)] and list(fd[0]) == [vr.NONE_DEFINED, vr.ALL_DEFINED]
    # a NaN coordinate flagged ALL_DEFINED never brackets either
    out, _ = column([100, np.nan, 300, 400], [1, 2, 3, 4], [150, 350], fdef_coord=[vr.ALL_DEFINED] * 4)
    assert list(out[0]) == [U, np.float32(3.5)]


def test_targets_above_and_below_the_column():
    out, fd = column([200, 500, 1000], [1, 2, 3], [100, 1000.5, 199.99])
    assert list(out[0]) == [U, U, U] and list(fd[0]) == [vr.NONE_DEFINED] * 3


def test_log_weights_and_non_positive_coordinates():
    out, _ = column([100, 1000], [0, 2], [np.sqrt(np.float32(1e5))], method=vr.LOG)
    assert abs(out[0, 0] - 1) < 1e-6  # the geometric mean is half way in log p
    ct = np.float32(300)
    w = (np.log(np.float64(ct)) - np.log(100.0)) / (np.log(1000.0) - np.log(100.0))
    out, _ = column([100, 1000], [5, 7], [ct], method=vr.LOG)
    assert out[0, 0] == np.float32(5 + w * 2.0)
    out, fd = column([0, 1000], [5, 7], [300], method=vr.LOG)
    assert out[0, 0] == U and fd[0, 0] == vr.NONE_DEFINED
    out, _ = column([-5, 1000], [5, 7], [300], method=vr.LOG)
    assert out[0, 0] == U
    out, _ = column([-5, 1000], [5, 7], [300], method=vr.LINEAR)
    assert out[0, 0] != U


def test_flag_tri_state_and_nan_undef():
    x = np.zeros((1, 2, 1, 3), np.float32)
    x[0, 1] = 10
    c = np.zeros((2, 1, 3), np.float32)
    c[1] = [[10, 10, 10]]
    out, fd = vr.coord_fields(x, c, [5, 20], vr.LINEAR)
    assert list(fd[0]) == [vr.ALL_DEFINED, vr.NONE_DEFINED] and (out[0, 0] == 5).all()
    x[0, 0, 0, 1] = U
    out, fd = vr.coord_fields(x, c, [5], vr.LINEAR)
    assert fd[0, 0] == vr.SOME_DEFINED and out[0, 0, 0, 1] == U
    nan = np.float32(np.nan)
    x[0, 0, 0, 1] = nan
    out, fd = vr.coord_fields(x, c, [5], vr.LINEAR, undef=nan)
    assert fd[0, 0] == vr.SOME_DEFINED and np.isnan(out[0, 0, 0, 1]) and out[0, 0, 0, 0] == 5


def test_hybrid_coordinate_is_the_float_product_then_the_float_sum():
    a, b = np.float32(12.3456), np.float32(0.987654)
    ps = np.array([[1013.25, 987.6]], np.float32)
    c = vr.hybrid_coordinate(ps, [a], [b])
    assert c.dtype == np.float32
    for i in range(2):
        prod = np.float32(np.float64(b) * np.float64(ps[0, i]))  # one rounding: the double product of two floats is exact
        assert c[0, 0, i] == np.float32(np.float64(a) + np.float64(prod))
    # an undefined ps leaves every level of the cell undefined
    x = np.ones((1, 3, 1, 2), np.float32)
    al, bl = vr.hybrid_levels(3)
    out, fd = vr.hlevels(x, np.array([[1000, U]], np.float32), al, bl, [500], vr.LINEAR)
    assert out[0, 0, 0, 0] == 1 and out[0, 0, 0, 1] == U and fd[0, 0] == vr.SOME_DEFINED


def test_main_generator_covers_defined_and_undefined_outputs():
    fields, ps, alevel, blevel = vr.main_case()
    assert fields.shape == (3, 12, 9, 13) and ps.shape == (9, 13)
    out, fd = vr.hlevels(fields, ps, alevel, blevel, vr.MAIN_TARGETS, vr.LINEAR)
    defined = out != U
    assert defined.mean() >= 0.5, defined.mean()
    assert defined[:, 0].mean() < 0.5  # 1000 hPa: below the ground for most columns
    assert not defined[:, -1].any() and (fd[:, -1] == vr.NONE_DEFINED).all()  # 0.5 hPa: above the top everywhere
    assert (fd[:, 3:6] == vr.SOME_DEFINED).all()
