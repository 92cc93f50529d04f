"""CPU checks of the semantics of mifc_hinterp_levels through its numpy restatement (tests/hinterp_restate.py, the oracle of
the GPU tests): hand-computed answers on small grids, the rules one by one, the identity on the grid's own nodes, the
coverage of the main generator, and that the entry is declared, bound and configured where the others are."""
import glob
import os
import re

import numpy as np

import hinterp_restate as hi

U = hi.UNDEF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_METHODS = (hi.NEAREST, hi.BILINEAR, hi.BICUBIC)


def one(grid, x, y, method=hi.BILINEAR, flag=None, undef=U):
    """One field, one level: the values at the positions and the flag."""
    g = np.asarray(grid, np.float32)
    out, fd = hi.sample(g[None, None], np.atleast_1d(np.asarray(x, np.float32)), np.atleast_1d(np.asarray(y, np.float32)), method,
                        None if flag is None else [[flag]], undef)
    return out[0, 0], int(fd[0, 0])


def test_cell_centre_is_the_mean_of_four():
    out, fd = one([[1, 2], [4, 9]], 0.5, 0.5)
    assert out[0] == np.float32(4.0) and fd == hi.ALL_DEFINED
    out, _ = one([[1, 2], [4, 9]], [0.25, 0.5], [0.0, 0.75])
    assert out[0] == np.float32(1.25) and out[1] == np.float32(1.5 + 0.75 * (6.5 - 1.5))


def test_a_point_on_a_row_does_not_need_the_row_below():
    grid = [[1, 3, 5], [U, U, U], [7, 8, 9]]
    for m in (hi.BILINEAR, hi.BICUBIC):
        out, fd = one(grid, [0.5, 1.75], [0.0, 0.0], m)
        assert out[0] == np.float32(2) and out[1] == np.float32(4.5) and fd == hi.ALL_DEFINED
        out, fd = one(grid, [0.5], [0.25], m)  # off the row it does
        assert out[0] == U and fd == hi.NONE_DEFINED


def test_a_point_on_a_node_with_all_neighbours_undefined_returns_the_node():
    grid = np.full((5, 5), U, np.float32)
    grid[2, 2] = np.float32(287.123)
    for m in ALL_METHODS:
        out, fd = one(grid, [2.0], [2.0], m)
        assert out[0].tobytes() == np.float32(287.123).tobytes() and fd == hi.ALL_DEFINED, m


def test_the_last_column_and_row_are_legal_and_read_nothing_outside():
    grid = np.arange(12, dtype=np.float32).reshape(3, 4)
    for m in ALL_METHODS:
        out, fd = one(grid, [3.0, 3.0, 1.5, -0.0], [2.0, 0.5, 2.0, -0.0], m)
        assert list(out) == [np.float32(11), np.float32(5), np.float32(9.5), np.float32(0)] if m != hi.NEAREST else list(out) == [11, 7, 10, 0]
        assert fd == hi.ALL_DEFINED
        out, fd = one(grid, [np.nextafter(np.float32(3), np.float32(4)), -1e-6, 1.0, np.inf, 1.0], [1.0, 1.0, 2.0001, 1.0, -np.inf], m)
        assert (out == U).all() and fd == hi.NONE_DEFINED


def test_one_by_one_grid_and_degenerate_axes():
    for m in ALL_METHODS:
        out, fd = one([[42]], [0.0, -0.0, 0.5], [0.0, 0.0, 0.0], m)
        assert list(out) == [np.float32(42), np.float32(42), U] and fd == hi.SOME_DEFINED
        out, _ = one([[1, 2, 4]], [1.5, 2.0], [0.0, 0.0], m)  # ny == 1
        assert list(out) == ([4, 4] if m == hi.NEAREST else [3, 4])
        out, _ = one([[1], [2], [4]], [0.0, 0.0], [0.25, 0.5], m)  # nx == 1
        assert list(out) == ([1, 2] if m == hi.NEAREST else [np.float32(1.25), np.float32(1.5)])


def test_nearest_rounds_half_up_and_returns_the_bits():
    grid = np.arange(20, dtype=np.float32).reshape(4, 5) + np.float32(0.1)
    out, fd = one(grid, [0.49, 0.5, 1.5, 3.999, 4.0], [0.0, 0.5, 2.49, 2.5, 3.0], hi.NEAREST)
    assert out.tobytes() == grid[[0, 1, 2, 3, 3], [0, 1, 2, 4, 4]].tobytes() and fd == hi.ALL_DEFINED


def poly_grid(coeff, ny=7, nx=9):
    i = np.arange(nx, dtype=np.float64)
    return np.broadcast_to(np.polyval(coeff, i), (ny, nx)).astype(np.float32)


def test_the_cubic_rule_on_polynomials_in_x():
    """Catmull-Rom weights reproduce every polynomial up to degree two exactly; for a cubic c3 x^3 + ... the slopes they
    build from central differences are off by c3, which leaves the known residual c3 * t (1 - t) (1 - 2 t) -- zero at the
    nodes and halfway between them.  Both to 1 ulp of the float result, in the interior."""
    rng = np.random.default_rng(5)
    x = rng.uniform(1, 6.999, 200).astype(np.float32)  # 1 <= i0 <= nx - 3
    y = rng.uniform(1, 4.999, 200).astype(np.float32)
    br = np.zeros((1, 1, 200), np.int64)
    for coeff in ([0.25, -2.0, 3.0], [0.125, -1.0, 0.5, 2.0]):
        grid = poly_grid(coeff)  # (every node is exact in float32)
        out, fd = hi.sample(grid[None, None], x, y, hi.BICUBIC, branches=br)
        assert (br == hi.CUBIC).all() and fd[0, 0] == hi.ALL_DEFINED
        xd = x.astype(np.float64)
        t = xd - np.floor(xd)
        c3 = coeff[0] if len(coeff) == 4 else 0.0
        exact = np.polyval(coeff, xd) + c3 * t * (1 - t) * (1 - 2 * t)
        err = np.abs(out[0, 0].astype(np.float64) - exact)
        assert (err <= np.spacing(np.abs(exact).astype(np.float32))).all(), (coeff, float(err.max()))
        if c3:  # and halfway between two nodes the cubic itself
            xm = np.arange(1, 7, dtype=np.float32) + np.float32(0.5)
            mid, _ = hi.sample(grid[None, None], xm, np.full(6, 2.5, np.float32), hi.BICUBIC)
            want = np.polyval(coeff, xm.astype(np.float64))
            assert (np.abs(mid[0, 0] - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    bil, _ = hi.sample(poly_grid([0.25, -2.0, 3.0])[None, None], x, y, hi.BILINEAR)
    assert (bil != out).any()  # (bilinear does not)


def test_the_cubic_rule_falls_back_to_bilinear_next_to_a_hole_and_in_the_outer_ring():
    rng = np.random.default_rng(6)
    grid = rng.normal(280, 10, (7, 9)).astype(np.float32)
    holed = grid.copy()
    holed[3, 4] = U
    br = np.zeros((1, 1, 4), np.int64)
    # (2.5, 2.5): the block is rows 1..4 x columns 1..4 and contains the hole, the four corners do not
    x, y = np.array([2.5, 0.5, 7.5, 5.5], np.float32), np.array([2.5, 3.5, 3.5, 5.5], np.float32)
    cub, _ = hi.sample(holed[None, None], x, y, hi.BICUBIC, branches=br)
    bil, fd = hi.sample(holed[None, None], x, y, hi.BILINEAR)
    assert list(br[0, 0]) == [hi.FULL_BILINEAR] * 4 and cub.tobytes() == bil.tobytes() and fd[0, 0] == hi.ALL_DEFINED
    # without the hole the first point takes the cubic rule and differs; the ring (i0 = 0, i0 = nx - 2, j0 = ny - 2) stays bilinear
    cub2, _ = hi.sample(grid[None, None], x, y, hi.BICUBIC, branches=br)
    assert list(br[0, 0]) == [hi.CUBIC] + [hi.FULL_BILINEAR] * 3 and cub2[0, 0, 0] != bil[0, 0, 0] and cub2[0, 0, 1:].tobytes() == bil[0, 0, 1:].tobytes()
    # a hole at a needed corner: undef in both, counted
    cub3, fd3 = hi.sample(holed[None, None], np.array([3.5], np.float32), np.array([2.5], np.float32), hi.BICUBIC)
    assert cub3[0, 0, 0] == U and fd3[0, 0] == hi.NONE_DEFINED
    # a point on a node never takes the cubic rule
    hi.sample(grid[None, None], np.array([3.0], np.float32), np.array([3.0], np.float32), hi.BICUBIC, branches=br[:, :, :1])
    assert br[0, 0, 0] == hi.ON_ROW


def test_stored_undef_under_all_defined_is_a_value():
    grid = np.array([[1, U], [3, 5]], np.float32)
    out, fd = one(grid, [0.5, 1.0], [0.0, 0.0], hi.BILINEAR, flag=hi.ALL_DEFINED)
    assert out[0] == np.float32(1.0 + 0.5 * (np.float64(U) - 1.0)) and out[1] == U and fd == hi.ALL_DEFINED  # computed, not counted
    out, fd = one(grid, [0.5, 1.0], [0.0, 0.0], hi.BILINEAR, flag=hi.SOME_DEFINED)
    assert (out == U).all() and fd == hi.NONE_DEFINED
    out, fd = one(grid, [1.0], [0.25], hi.NEAREST, flag=hi.ALL_DEFINED)
    assert out[0] == U and fd == hi.ALL_DEFINED
    # an unusable position is counted under ALL_DEFINED too
    out, fd = one(grid, [1.0, 5.0], [0.25, 0.0], hi.NEAREST, flag=hi.ALL_DEFINED)
    assert fd == hi.SOME_DEFINED


def test_nan_as_undef():
    nan = np.float32(np.nan)
    grid = np.array([[1, nan, 3], [4, 5, 6]], np.float32)
    for m in (hi.BILINEAR, hi.BICUBIC):
        out, fd = one(grid, [0.5, 0.0, nan, 2.0], [0.0, 1.0, 0.0, 0.5], m, undef=nan)
        assert np.isnan(out[0]) and out[1] == 4 and np.isnan(out[2]) and out[3] == np.float32(4.5) and fd == hi.SOME_DEFINED
    out, fd = one(grid, [1.0], [0.0], hi.NEAREST, undef=nan)
    assert np.isnan(out[0]) and fd == hi.NONE_DEFINED
    # with the usual undef a NaN position is unusable all the same, and a NaN value is undefined
    out, fd = one(grid, [nan, 0.5], [0.0, 0.0])
    assert (out == U).all() and fd == hi.NONE_DEFINED


def test_flag_is_tri_state_per_level():
    f = np.ones((1, 3, 2, 2), np.float32)
    f[0, 1, 0, 0] = U
    f[0, 2] = U
    out, fd = hi.sample(f, np.array([0.0, 1.0], np.float32), np.array([0.0, 1.0], np.float32), hi.NEAREST)
    assert list(fd[0]) == [hi.ALL_DEFINED, hi.SOME_DEFINED, hi.NONE_DEFINED]
    out, fd = hi.sample(f, np.array([0.0, 7.0], np.float32), np.array([1.0, 1.0], np.float32), hi.BILINEAR)  # one point outside
    assert list(fd[0]) == [hi.SOME_DEFINED, hi.SOME_DEFINED, hi.NONE_DEFINED] and out[0, 0, 1] == U and out[0, 0, 0] == 1


def test_sampling_a_field_at_its_own_nodes_is_the_identity():
    fields, _, _ = hi.main_case(2, 3)
    flags = np.array([[hi.ALL_DEFINED, hi.SOME_DEFINED, hi.SOME_DEFINED], [hi.SOME_DEFINED, hi.NONE_DEFINED, hi.ALL_DEFINED]], np.int32)
    nf, nlev, ny, nx = fields.shape
    yy, xx = np.meshgrid(np.arange(ny, dtype=np.float32), np.arange(nx, dtype=np.float32), indexing="ij")
    for m in ALL_METHODS:
        out, fd = hi.sample(fields, xx, yy, m, flags)
        assert out.shape == fields.shape and out.tobytes() == fields.tobytes(), m
        for f in range(nf):
            for k in range(nlev):
                holes = 0 if flags[f, k] == hi.ALL_DEFINED else int((fields[f, k] == U).sum())
                assert fd[f, k] == hi.classify(holes, ny * nx), (m, f, k)
    assert (fd == hi.SOME_DEFINED).sum() >= 3  # (the generator's 3 % of holes are there)


def test_main_generator_reaches_every_branch():
    fields, x, y = hi.main_case()
    assert fields.shape == (1, 1, 9, 13) and x.shape == (600,)
    for method in ALL_METHODS:
        br = np.zeros((1, 1, 600), np.int64)
        out, fd = hi.sample(fields, x, y, method, branches=br)
        shares = np.bincount(br.ravel(), minlength=8) / br.size
        print("method", method, {n: float(round(s, 4)) for n, s in zip(hi.BRANCH_NAMES, shares)}, "defined", float((out != U).mean()))
        assert all(shares[b] > 0 for b in hi.REACHABLE[method]), dict(zip(hi.BRANCH_NAMES, shares))
        assert all(shares[b] == 0 for b in range(8) if b not in hi.REACHABLE[method])
        assert (out != U).mean() >= 0.5
        assert fd[0, 0] == hi.SOME_DEFINED
    assert x[599] == 12 and y[599] == 8 and (x == U).sum() == 1 and np.isnan(y).sum() == 1


def test_entry_is_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_hinterp_levels", "mifc_last_hinterp_form"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    for enum in (r"MIFC_HINTERP_NEAREST = 0\b", r"MIFC_HINTERP_BILINEAR = 1\b", r"MIFC_HINTERP_BICUBIC = 2\b"):
        assert re.search(enum, header), enum
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(csrc, "*"))) if '"MIFC_HINTERP_CHUNK_MIB"' in open(p, errors="replace").read()]
    assert readers == ["mifc_env.hip"], readers
    host = open(os.path.join(csrc, "mifc_capi_hinterp.hip")).read()
    assert "getenv" not in host and re.search(r"hinterp_chunk_mib > 0 \? mifc::env\(\)\.hinterp_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_hinterp.hip") == 1 and makefile.count("mifc_capi_hinterp.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
