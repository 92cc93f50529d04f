"""CPU checks of rule R (include/mifc.h) through its numpy restatement (tests/vrotate_restate.py, the oracle of the GPU tests
of mifc_vrotate_levels and mifc_hinterp_vector_levels): the identity and the quarter turn, the arithmetic against a
one-line formula, every cause of a hole and the share of computed results in the generators, the flags, and that the
entries are declared, bound and built where the others are."""
import os
import re

import numpy as np

import hinterp_restate as hi
import vrotate_restate as vr

U = vr.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_floats(rng, n):
    """Finite floats of every size: ordinary, huge (their products leave the float range), tiny and denormal, zeros of both signs."""
    a = rng.normal(0, 10, n).astype(np.float32)
    a[::7] = (np.clip(rng.normal(0, 1, a[::7].size), -3, 3) * 1e38).astype(np.float32)
    a[1::7] = (rng.normal(0, 1, a[1::7].size) * 1e-41).astype(np.float32)  # denormal
    a[2::7] = (rng.normal(0, 1, a[2::7].size) * 1e-30).astype(np.float32)
    a[3::49] = 0.0
    a[10::49] = -0.0
    return a


def test_the_identity_returns_the_bits_except_the_sign_of_a_zero():
    rng = np.random.default_rng(1)
    u, v = random_floats(rng, 4000), random_floats(rng, 4000)[::-1].copy()
    one, zero = np.ones(4000, np.float32), np.zeros(4000, np.float32)
    out, fd = vr.rotate(np.stack([u, v])[:, None], one, zero, flags=[[vr.ALL_DEFINED], [vr.ALL_DEFINED]], fdef_rot=vr.ALL_DEFINED)
    for got, want in ((out[0, 0], u), (out[1, 0], v)):
        nonzero = want != 0
        assert nonzero.sum() > 3000 and (want == 0).sum() > 50
        assert np.array_equal(bits(got)[nonzero], bits(want)[nonzero])
        assert (got[~nonzero] == 0).all()
    assert (fd == vr.ALL_DEFINED).all()
    # the sign of a zero: 1 * -0.0 - 0 * -3 = -0.0 - -0.0 = +0.0
    out, _ = vr.rotate(np.array([-0.0, -3.0], np.float32).reshape(2, 1, 1), np.ones(1, np.float32), np.zeros(1, np.float32))
    assert bits(out[0, 0])[0] == 0 and out[1, 0, 0] == -3.0


def test_the_quarter_turn_swaps_the_components_exactly():
    rng = np.random.default_rng(2)
    u, v = random_floats(rng, 4000), random_floats(rng, 4000)[::-1].copy()
    out, _ = vr.rotate(np.stack([u, v])[:, None], np.zeros(4000, np.float32), np.ones(4000, np.float32), fdef_rot=vr.ALL_DEFINED,
                       flags=[[vr.ALL_DEFINED], [vr.ALL_DEFINED]])
    assert np.array_equal(out[0, 0], -v) and np.array_equal(out[1, 0], u)  # (-v, u), values: 0 * u - 1 * v and 1 * u + 0 * v
    nz = (u != 0) & (v != 0)
    assert np.array_equal(bits(out[0, 0])[nz], bits(-v)[nz]) and np.array_equal(bits(out[1, 0])[nz], bits(u)[nz])


def test_the_restatement_is_the_one_line_formula():
    rng = np.random.default_rng(3)
    n = 20000
    u, v, c, s = (random_floats(rng, n) for _ in range(4))
    rng.shuffle(v), rng.shuffle(c), rng.shuffle(s)
    every = [[vr.ALL_DEFINED], [vr.ALL_DEFINED]]
    out, fd = vr.rotate(np.stack([u, v])[:, None], c, s, flags=every, fdef_rot=vr.ALL_DEFINED)
    with np.errstate(all="ignore"):
        want_u = np.float32(np.float64(c) * u - np.float64(s) * v)
        want_v = np.float32(np.float64(s) * u + np.float64(c) * v)
    for got, want in ((out[0, 0], want_u), (out[1, 0], want_v)):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])
        assert np.isinf(want).sum() > 0 and ((want != 0) & (np.abs(want) < 1e-38)).sum() > 0  # overflow and denormal results are there
    assert (fd == vr.ALL_DEFINED).all()
    # the products are exact in double: field algebra, which rounds every product to float, gives other results
    with np.errstate(all="ignore"):
        algebra = (c * u).astype(np.float32) - (s * v).astype(np.float32)
    assert (algebra != want_u).sum() > 0


def test_every_cause_of_a_hole_is_reached_on_the_grid():
    fields, c, s = vr.grid_case(2, 5)
    causes = np.zeros((2, 5, 9, 13), np.int64)
    out, fd = vr.rotate(fields, c, s, causes=causes)
    shares = np.bincount(causes.ravel(), minlength=4) / causes.size
    print("on the grid:", dict(zip(("computed", "coefficients", "u", "v"), shares.round(4))))
    assert all(shares[b] > 0 for b in (vr.COEFFICIENTS, vr.U_HOLE, vr.V_HOLE)) and shares[vr.COMPUTED] >= 0.5
    # as undef and as NaN, in every input
    for a in (fields[0], fields[1], c, s):
        assert (a == U).sum() > 0 and np.isnan(a).sum() > 0
    assert (out[0] == U).sum() == (out[1] == U).sum() == (causes[0] != vr.COMPUTED).sum()
    assert np.array_equal(fd[0], fd[1]) and (fd == vr.SOME_DEFINED).all()
    # NaN alone makes a hole: a NaN coefficient with every other input defined
    one = np.ones((2, 1, 4), np.float32)
    out, fd = vr.rotate(one, np.array([1, np.nan, 1, 1], np.float32), np.array([0, 0, np.nan, U], np.float32))
    assert list(out[0, 0]) == [1, U, U, U] and list(out[1, 0]) == [1, U, U, U] and fd[0, 0] == vr.SOME_DEFINED


def test_every_cause_of_a_hole_is_reached_while_sampling():
    for npairs, npos in ((1, 600), (4, 600), (1, 1100)):
        fields, x, y, c, s = vr.point_case(npairs, 1, npos=npos)
        for method in (hi.NEAREST, hi.BILINEAR, hi.BICUBIC):
            causes = np.zeros((npairs, 1, npos), np.int64)
            out, fd = vr.sample_rotate(fields, x, y, c, s, method, causes=causes)
            br = np.zeros((2 * npairs, 1, npos), np.int64)
            hi.sample(fields, x, y, method, branches=br)
            unusable = (br[0, 0] == hi.POSITION_UNDEFINED) | (br[0, 0] == hi.OUTSIDE)
            shares = np.bincount(causes.ravel(), minlength=4) / causes.size
            print("sampled: npairs", npairs, "npos", npos, "method", method, dict(zip(("computed", "coefficients", "u", "v"), shares.round(4))),
                  "unusable", float(unusable.mean()))
            assert all(shares[b] > 0 for b in (vr.COEFFICIENTS, vr.U_HOLE, vr.V_HOLE)) and shares[vr.COMPUTED] >= 0.5
            assert unusable.sum() > 0 and (out[0, 0][unusable] == U).all()
            assert (c == U).sum() > 0 and (s == U).sum() > 0 and np.isnan(c).sum() == 1 and np.isnan(s).sum() == 1
            assert (fd == vr.SOME_DEFINED).all() and np.array_equal(fd[0::2], fd[1::2])


def test_all_defined_flags_turn_a_stored_undef_into_a_value():
    f = np.array([[[U, 2, U, 4]], [[1, U, 3, U]]], np.float32)  # (2, 1, 4)
    c, s = np.array([1, 1, U, 1], np.float32), np.array([0, 0, 0, 1], np.float32)
    out, fd = vr.rotate(f, c, s)
    assert (out == U).all() and (fd == vr.NONE_DEFINED).all()
    # u under ALL_DEFINED: its undef is a value, v's still a hole; the coefficients are tested by fdef_rot alone
    out, fd = vr.rotate(f, c, s, flags=[[vr.ALL_DEFINED], [vr.SOME_DEFINED]])
    assert out[0, 0, 0] == U and out[1, 0, 0] == 1 and (out[:, 0, 1:] == U).all() and (fd == vr.SOME_DEFINED).all()  # cell 0: (U * 1 - 0 * 1, 0 * U + 1)
    out, fd = vr.rotate(f, c, s, flags=[[vr.ALL_DEFINED], [vr.ALL_DEFINED]])
    assert list(out[0, 0, :2]) == [U, 2] and list(out[1, 0, :2]) == [1, U] and (out[:, 0, 2] == U).all() and (fd == vr.SOME_DEFINED).all()
    assert out[0, 0, 3] == np.float32(4.0 - np.float64(U)) and out[1, 0, 3] == np.float32(4.0 + np.float64(U))
    out, fd = vr.rotate(f, c, s, flags=[[vr.ALL_DEFINED], [vr.ALL_DEFINED]], fdef_rot=vr.ALL_DEFINED)
    assert (fd == vr.ALL_DEFINED).all()
    with np.errstate(over="ignore"):  # (undef squared leaves the float range)
        assert out[0, 0, 2] == np.float32(np.float64(U) * np.float64(U) - 0.0) and out[1, 0, 2] == np.float32(0.0 * np.float64(U) + np.float64(U) * 3.0)


def test_flags_are_per_pair_and_level():
    f = np.ones((4, 3, 2, 2), np.float32)
    f[0, 1, 0, 0] = U  # pair 0, level 1: one hole through u
    f[3, 2] = U  # pair 1, level 2: all holes through v
    c = s = np.full((2, 2), np.float32(0.5))
    out, fd = vr.rotate(f, c, s)
    assert fd.tolist() == [[vr.ALL_DEFINED, vr.SOME_DEFINED, vr.ALL_DEFINED]] * 2 + [[vr.ALL_DEFINED, vr.ALL_DEFINED, vr.NONE_DEFINED]] * 2
    assert out[1, 1, 0, 0] == U and (out[2:, 2] == U).all() and out[0, 0, 0, 0] == 0.0 and out[1, 0, 0, 0] == 1.0


def truthful(fields, flags, rng):
    """The fields with every plane that is flagged ALL_DEFINED made so: its holes filled with values."""
    f = fields.copy()
    for g, k in zip(*np.nonzero(np.asarray(flags) == vr.ALL_DEFINED)):
        bad = np.isnan(f[g, k]) | (f[g, k] == U)
        f[g, k][bad] = rng.normal(280, 10, int(bad.sum())).astype(np.float32)
    return f


def test_the_vector_sampling_is_the_two_steps():
    """hinterp_levels, then vrotate_levels on its (nlev, 1, npos) batches with its flags: the same bits and flags as the one
    call, for flags that tell the truth (the second call recognises a hole by its value; the one call carries it)."""
    fields, x, y, c, s = vr.point_case(2, 3)
    flags = np.array([[vr.ALL_DEFINED, vr.SOME_DEFINED, vr.SOME_DEFINED], [vr.SOME_DEFINED, vr.ALL_DEFINED, vr.SOME_DEFINED]] * 2, np.int32)
    honest = truthful(fields, flags, np.random.default_rng(4))
    for method in (hi.NEAREST, hi.BILINEAR, hi.BICUBIC):
        for f, fl in ((fields, None), (honest, flags)):
            out, fd = vr.sample_rotate(f, x, y, c, s, method, fl)
            sampled, sfd = hi.sample(f, x, y, method, fl)
            out2, fd2 = vr.rotate(sampled.reshape(4, 3, 1, 600), c.reshape(1, 600), s.reshape(1, 600), sfd)
            assert out.tobytes() == out2.reshape(out.shape).tobytes() and np.array_equal(fd, fd2), (method, fl is None)
        # a stored undef under ALL_DEFINED is a value for the sampling and stays one in the one call; two calls lose it
        out, fd = vr.sample_rotate(fields, x, y, c, s, method, flags)
        sampled, sfd = hi.sample(fields, x, y, method, flags)
        out2, _ = vr.rotate(sampled, c, s, sfd)
        assert ((out != U) & (out2 == U)).sum() > 0 and ((out == U) & (out2 != U)).sum() == 0
    # sampling a field at its own nodes with (1, 0) is the identity up to the sign of a zero
    f2 = fields[:2, :, :, :]
    yy, xx = np.meshgrid(np.arange(9, dtype=np.float32), np.arange(13, dtype=np.float32), indexing="ij")
    out, fd = vr.sample_rotate(f2, xx, yy, np.ones((9, 13), np.float32), np.zeros((9, 13), np.float32), hi.BICUBIC)
    holes = (f2[0] == U) | (f2[1] == U)
    assert np.array_equal(out[0][~holes], f2[0][~holes]) and np.array_equal(out[1][~holes], f2[1][~holes]) and (out[:, holes] == U).all()


def test_entries_are_declared_bound_and_built():
    import mi_fieldcalc_amd._capi as capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_vrotate_levels", "mifc_last_vrotate_form", "mifc_hinterp_vector_levels"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert len(capi.SIGNATURES["mifc_vrotate_levels"][1]) == 14 and len(capi.SIGNATURES["mifc_hinterp_vector_levels"][1]) == 18
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_vrotate.hip") == 1 and makefile.count("mifc_capi_vrotate.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    for f in ("mifc_vrotate.hip", "mifc_capi_vrotate.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert "getenv" not in text, f
    # rule R stands in the header
    full = open(os.path.join(ROOT, "include", "mifc.h")).read()
    for word in ("R1.", "R2.", "R3.", "R4.", "The library does not normalise them"):
        assert word in full, word
    import mi_fieldcalc_amd as fc

    for method in ("vrotate_levels", "hinterp_vector_levels", "last_vrotate_form"):
        assert callable(getattr(fc.Context, method)), method
