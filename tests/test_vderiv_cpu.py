"""CPU checks of the semantics of mifc_vderiv_hlevels / mifc_vderiv_fields / mifc_vderiv_levels through their numpy
restatement (tests/vderiv_restate.py, the oracle of the GPU tests): hand-computed answers on short columns, the rules one
by one, the coverage of the main generator, and that the entries are declared, bound and configured where the others
are."""
import glob
import os
import re

import numpy as np

import vderiv_restate as vd

U = vd.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH_METHODS = (vd.CENTRED, vd.WEIGHTED)


def column(coord, values, method=vd.CENTRED, flags=None, fdef_coord=None, undef=U, magnitude=False):
    """One column (ny = nx = 1), one or several fields: returns (out[nf][nlev], flags[nf][nlev]) and, with magnitude, also
    (mag[nf / 2][nlev], mag_flags)."""
    v = np.atleast_2d(np.asarray(values, np.float32))
    c = np.asarray(coord, np.float32)
    res = vd.coord_fields(v[:, :, None, None], c[:, None, None], method, flags, fdef_coord, undef, magnitude)
    return tuple(r[:, :, 0, 0] if r.ndim == 4 else r for r in res)


def f32(*xs):
    return [np.float32(x) for x in xs]


def test_centred_on_three_uneven_levels():
    out, fd = column([100, 200, 400], [1, 3, 9])
    assert list(out[0]) == f32(2 * (1.0 / 100), 8 * (1.0 / 300), 6 * (1.0 / 200)) and (fd == vd.ALL_DEFINED).all()
    # the same through the `levels` form: one coordinate value per level
    x = np.array([1, 3, 9], np.float32).reshape(1, 3, 1, 1)
    out2, fd2 = vd.levels(x, [100, 200, 400])
    assert out2.tobytes() == out.tobytes() and (fd2 == fd).all()


def test_weighted_is_exact_for_a_quadratic_on_uneven_spacing():
    c = np.array([1, 2, 4, 8, 11], np.float64)
    out, _ = column(c, c * c, vd.WEIGHTED)
    for k in (1, 2, 3):  # 2 c at the inner levels, to float rounding
        assert abs(out[0, k] - np.float32(2 * c[k])) <= np.spacing(np.float32(2 * c[k])), k
    centred, _ = column(c, c * c, vd.CENTRED)
    assert centred[0, 1] == np.float32(5) and centred[0, 1] != out[0, 1]  # (16 - 1) / 3: first order only
    assert out[0, 0] == centred[0, 0] == 3 and out[0, 4] == centred[0, 4] == np.float32(57 * (1.0 / 3))  # the ends are one-sided in both


def test_both_methods_agree_on_even_spacing():
    a, _ = column([0, 8, 16, 24], [1, 5, 2, 7], vd.CENTRED)
    b, _ = column([0, 8, 16, 24], [1, 5, 2, 7], vd.WEIGHTED)
    assert list(a[0]) == f32(0.5, 1 / 16, 2 / 16, 5 / 8) and a.tobytes() == b.tobytes()


def test_one_sided_ends_and_two_levels():
    for m in BOTH_METHODS:
        out, fd = column([100, 300], [1, 5], m)
        assert list(out[0]) == f32(4 * (1.0 / 200), 4 * (1.0 / 200)) and (fd == vd.ALL_DEFINED).all()
        out, _ = column([1000, 900, 700], [10, 20, 60], m)
        assert out[0, 0] == np.float32(10 * (1.0 / -100)) and out[0, 2] == np.float32(40 * (1.0 / -200))


def test_the_same_column_given_bottom_up():
    c, x = [100, 200, 400, 450, 700], [1, 3, 9, 4, 4.5]
    for m in BOTH_METHODS:
        down, _ = column(c, x, m)
        up, _ = column(c[::-1], x[::-1], m)
        assert up[0, ::-1].tobytes() == down[0].tobytes(), m


def test_a_hole_makes_its_neighbours_one_sided():
    c = [100, 200, 400, 500, 700]
    for m in BOTH_METHODS:
        out, fd = column(c, [1, 3, U, 4, 8], m)
        # hole at k = 2: undef there; level 1 has the lower side only, level 3 the upper side only
        assert out[0, 2] == U and out[0, 1] == np.float32(2 * (1.0 / 100)) and out[0, 3] == np.float32(4 * (1.0 / 200))
        assert list(fd[0]) == [vd.ALL_DEFINED] * 2 + [vd.NONE_DEFINED] + [vd.ALL_DEFINED] * 2
        out, _ = column(c, [U, 3, 9, 4, U], m)  # holes at the ends: levels 1 and 3 fall to their other side
        assert out[0, 0] == U and out[0, 4] == U and out[0, 1] == np.float32(6 * (1.0 / 200)) and out[0, 3] == np.float32(-5 * (1.0 / 100))
        out, _ = column(c, [1, U, 9, U, 8], m)  # holes on both sides of level 2: no side
        assert out[0, 2] == U and out[0, 0] == U and out[0, 4] == U


def test_equal_neighbours_fall_to_the_other_side_and_a_folded_column_is_undef():
    for m in BOTH_METHODS:
        out, _ = column([100, 100, 300, 400], [1, 2, 6, 7], m)
        # level 0: the upper side has c_1 == c_0 and there is no lower one; level 1: c_0 == c_1, the upper side only
        assert out[0, 0] == U and out[0, 1] == np.float32(4 * (1.0 / 200))
        out, _ = column([100, -0.0, 0.0, 400], [1, 2, 6, 7], m)  # -0 == +0
        assert out[0, 1] == np.float32(1 * (1.0 / -100)) and out[0, 2] == np.float32(1 * (1.0 / 400))
        out, fd = column([100, 200, 100], [1, 2, 6], m)  # c_2 == c_0: both sides take part at level 1, the denominator is zero
        assert out[0, 1] == U and out[0, 0] == np.float32(1 * (1.0 / 100)) and out[0, 2] == np.float32(4 * (1.0 / -100))
        assert list(fd[0]) == [vd.ALL_DEFINED, vd.NONE_DEFINED, vd.ALL_DEFINED]


def test_unusable_coordinate_touches_its_neighbours_only():
    for c, fc in (([100, U, 300, 400, 500], None), ([100, np.nan, 300, 400, 500], [vd.ALL_DEFINED] * 5), ([100, np.nan, 300, 400, 500], None)):
        out, fd = column(c, [[1, 2, 3, 5, 8], [1, 1, 1, 1, 1]], vd.CENTRED, fdef_coord=fc)
        assert out[0, 0] == U and out[0, 1] == U  # level 0 has lost its only side
        assert out[0, 2] == np.float32(2 * (1.0 / 100)) and out[0, 3] == np.float32(5 * (1.0 / 200)) and out[0, 4] == np.float32(3 * (1.0 / 100))
        assert list(out[1]) == f32(U, U, 0, 0, 0)
    # an undefined ps: every level of that cell, no other cell
    x = np.arange(6, dtype=np.float32).reshape(1, 3, 1, 2)
    al, bl = vd.hybrid_levels(3)
    out, fd = vd.hlevels(x, np.array([[1000, U]], np.float32), al, bl)
    assert (out[0, :, 0, 1] == U).all() and (out[0, :, 0, 0] != U).all() and (fd == vd.SOME_DEFINED).all()


def test_stored_undef_under_all_defined_is_a_value():
    flags = [[vd.SOME_DEFINED, vd.ALL_DEFINED, vd.SOME_DEFINED]]
    out, fd = column([100, 200, 400], [1, U, 9], flags=flags)
    assert out[0, 0] == np.float32((np.float64(U) - 1) * (1.0 / 100)) and out[0, 1] == np.float32(8 * (1.0 / 300)) and (fd == vd.ALL_DEFINED).all()
    # a result that happens to equal undef, or is not finite, is a value too: not counted
    out, fd = column([0, 1, 2], [0, 0, 2 * np.float64(U)], flags=[[vd.ALL_DEFINED] * 3])
    assert out[0, 1] == U and fd[0, 1] == vd.ALL_DEFINED
    out, fd = column([0, 1, 2], [0, np.inf, 1], flags=[[vd.ALL_DEFINED] * 3])
    assert np.isinf(out[0, 0]) and np.isinf(out[0, 2]) and (fd == vd.ALL_DEFINED).all()


def test_nan_as_undef():
    nan = np.float32(np.nan)
    out, fd = column([100, 200, 400, 500], [1, nan, 9, 11], undef=nan)
    assert out[0, 0].tobytes() == nan.tobytes() and np.isnan(out[0, 1]) and out[0, 2] == np.float32(2 * (1.0 / 100))
    assert list(fd[0]) == [vd.NONE_DEFINED, vd.NONE_DEFINED, vd.ALL_DEFINED, vd.ALL_DEFINED]


def test_flag_tri_state_per_level():
    x = np.zeros((1, 3, 1, 3), np.float32)
    x[0, 1] = 10
    x[0, 2] = 30
    c = np.zeros((3, 1, 3), np.float32)
    c[1], c[2] = 10, 20
    out, fd = vd.coord_fields(x, c)
    assert (fd == vd.ALL_DEFINED).all() and (out[0, 0] == 1).all() and (out[0, 1] == 1.5).all() and (out[0, 2] == 2).all()
    x[0, 0, 0, 1] = U  # one cell of level 0: levels 0 (no centre) and 1 (one-sided now) -- only level 0 has an undef cell
    out, fd = vd.coord_fields(x, c)
    assert list(fd[0]) == [vd.SOME_DEFINED, vd.ALL_DEFINED, vd.ALL_DEFINED] and out[0, 0, 0, 1] == U and out[0, 1, 0, 1] == 2
    x[0, 0] = U
    out, fd = vd.coord_fields(x, c)
    assert list(fd[0]) == [vd.NONE_DEFINED, vd.ALL_DEFINED, vd.ALL_DEFINED]


def test_magnitude_of_a_pair():
    # du/dc = 3, dv/dc = 4 everywhere
    c = [0, 1, 2, 4]
    out, fd, mag, mfd = column(c, [[0, 3, 6, 12], [1, 5, 9, 17]], magnitude=True)
    assert (out[0] == 3).all() and (out[1] == 4).all() and (mag[0] == 5).all() and mag.shape == (1, 4) and (mfd == vd.ALL_DEFINED).all()
    # undef where either component is
    out, fd, mag, mfd = column(c, [[0, 3, 6, 12], [1, 5, U, 17]], magnitude=True)
    # (v has a hole at level 2: no value there, and the last level has lost its only side)
    assert out[1, 2] == U and out[1, 3] == U and (out[0] == 3).all() and (mag[0, 2:] == U).all() and (mag[0, :2] == 5).all()
    assert list(mfd[0]) == [vd.ALL_DEFINED] * 2 + [vd.NONE_DEFINED] * 2
    # a derivative that happens to equal undef is a value: the magnitude is computed from it
    out, fd, mag, mfd = column([0, 1, 2], [[0, 0, 2 * np.float64(U)], [0, 0, 0]], flags=[[vd.ALL_DEFINED] * 3] * 2, magnitude=True)
    assert out[0, 1] == U and np.isinf(mag[0, 1]) and mfd[0, 1] == vd.ALL_DEFINED  # (U * U overflows in float)
    # two pairs out of four fields
    out, fd, mag, mfd = column(c, [[0, 3, 6, 12], [1, 5, 9, 17], [0, 6, 12, 24], [0, 8, 16, 32]], magnitude=True)
    assert mag.shape == (2, 4) and (mag[0] == 5).all() and (mag[1] == 10).all()


def test_main_generator_reaches_every_branch():
    fields, ps, ab, coord = vd.deriv_case()
    assert fields.shape == (3, 12, 9, 13)
    for method in BOTH_METHODS:
        br = np.zeros(fields.shape, np.int64)
        out, fd = vd.coord_fields(fields, coord, method, branches=br)
        shares = np.bincount(br.ravel(), minlength=6) / br.size
        print("method", method, {n: float(round(s, 4)) for n, s in zip(vd.BRANCH_NAMES, shares)}, "defined", float((out != U).mean()))
        assert (shares > 0).all(), dict(zip(vd.BRANCH_NAMES, shares))
        assert (out != U).mean() >= 0.5
        hyb, _ = vd.hlevels(fields, ps, ab[0], ab[1], method)
        lev, _ = vd.levels(fields, vd.main_levels(12), method)
        assert (hyb != U).mean() >= 0.5 and (lev != U).mean() >= 0.5


def test_entries_are_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_vderiv_hlevels", "mifc_vderiv_fields", "mifc_vderiv_levels"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert re.search(r"MIFC_VDERIV_CENTRED = 0\b", header) and re.search(r"MIFC_VDERIV_WEIGHTED = 1\b", header)
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(csrc, "*"))) if '"MIFC_VDERIV_CHUNK_MIB"' in open(p, errors="replace").read()]
    assert readers == ["mifc_env.hip"], readers
    host = open(os.path.join(csrc, "mifc_capi_vderiv.hip")).read()
    assert "getenv" not in host and re.search(r"vderiv_chunk_mib > 0 \? mifc::env\(\)\.vderiv_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert "mifc_vderiv.hip" in makefile and "mifc_capi_vderiv.hip" in makefile
