"""CPU checks of mifc_hstats_levels' definition (include/mifc.h) through its numpy restatement (tests/hstats_restate.py, the
oracle of the GPU tests): the vectorised form against the literal cell-by-cell loop bit for bit, every sum against
math.fsum within the bound of its chain of additions, the guard that the restatement has not collapsed into a plain sum,
the extremes against numpy's argmin / argmax, and the plumbing of the entry."""
import glob
import math
import os
import re

import numpy as np
import pytest

import hstats_restate as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = [hs.ALL_DEFINED, hs.SOME_DEFINED, hs.NONE_DEFINED]


def both_forms(label, fields, **kw):
    stats, mean, fd = hs.hstats(fields, **kw)
    lstats, lmean, lfd = hs.hstats_literal(fields, **kw)
    assert hs.same_bits64(stats, lstats), (label, np.argwhere(~((stats == lstats) | (np.isnan(stats) & np.isnan(lstats))))[:4])
    assert hs.same_bits64(mean.astype(np.float64), lmean.astype(np.float64)) and np.array_equal(fd, lfd), label
    return stats, mean, fd


@pytest.mark.parametrize("nx", [1, 3, 4, 5, 255, 256, 257, 260])
def test_vectorised_restatement_equals_the_literal_loop(nx):
    nf, nlev, ny = 2, 2, 3
    fields, minus, weight, pivot, box = hs.main_case(nf, nlev, ny, nx, seed=nx)
    flags = np.random.default_rng(nx).choice(MIXED, size=(nf, nlev)).astype(np.int32)
    flags[0, 0], flags[1, 1] = hs.SOME_DEFINED, hs.ALL_DEFINED
    for mode in (hs.AREA, hs.ROWS):
        both_forms(("plain", nx, mode), fields, mode=mode)
        both_forms(("box", nx, mode), fields, box=box, mode=mode, flags=flags)
        both_forms(("weight", nx, mode), fields, weight=weight, mode=mode)
        both_forms(("minus, pivot", nx, mode), fields, minus=minus, pivot=pivot, mode=mode, flags_minus=flags[::-1])
        both_forms(("everything", nx, mode), fields, minus=minus, pivot=pivot, weight=weight, box=box, mode=mode, flags=flags)


@pytest.mark.parametrize("nx", [4095, 4096, 4097])
def test_vectorised_restatement_equals_the_literal_loop_at_the_segment_seam(nx):
    fields, minus, weight, pivot, _ = hs.main_case(1, 1, 2, nx, seed=nx)
    for mode in (hs.AREA, hs.ROWS):
        both_forms(("plain", nx, mode), fields, mode=mode)
        both_forms(("everything", nx, mode), fields, minus=minus, pivot=pivot, weight=weight, box=(3, nx - 1, 0, 2), mode=mode)
    both_forms(("a box inside the second segment", nx), np.concatenate([fields, fields[..., :8]], axis=-1), box=(4096, nx + 8, 1, 2), mode=hs.ROWS)


WIDE_SHAPES = [(4, 7, 13), (4, 5, 64), (3, 9, 257), (2, 16, 1023), (2, 3, 4097), (1, 40, 1440)]


def wide_sums():
    """Per shape, level, weighted or not and moment: (the restatement's AREA sum, the cells' q in row-major order, partials)."""
    out = []
    for n, (nlev, ny, nx) in enumerate(WIDE_SHAPES):
        fields = hs.wide_fields((1, nlev, ny, nx), 10 + n)
        for weight in (None, hs.wide_weight(ny, nx, 10 + n)):
            stats, _, _ = hs.hstats(fields, weight=weight, mode=hs.AREA, products=hs.MOMENTS)
            for k in range(nlev):
                q = hs.cell_quantities(fields[0, k], hs.SOME_DEFINED, None, None, 0.0, weight, hs.SOME_DEFINED, (0, nx, 0, ny))
                for slot, m in ((hs.S1, 3), (hs.S2, 4)):
                    out.append((stats[0, k, 0, slot], q[m][q[0]], ny * (-(-nx // hs.SEGMENT))))
    return out


def test_every_sum_is_within_the_bound_of_its_chain_of_fsum():
    """A partial is at most 64 sequential additions, the merge six more, the combination one per partial: the standard
    bound (n - 1) u sum |q| of a chain of depth n."""
    sums = wide_sums()
    assert len(sums) >= 64
    for got, q, partials in sums:
        exact = math.fsum(q)
        bound = (70 + partials) * 2.0 ** -53 * math.fsum(np.abs(q))
        assert abs(got - exact) <= bound, (got, exact, bound)
    # rows mode, a box, a weight with holes and a minus batch: the same bound per row
    fields, minus, weight, pivot, box = hs.main_case(1, 2, 9, 5000, seed=3)
    stats, _, _ = hs.hstats(fields, minus=minus, weight=weight, pivot=pivot, box=box, mode=hs.ROWS, products=hs.MOMENTS)
    i0, i1, j0, j1 = box
    for k in range(2):
        inc, _, w, q1, q2 = hs.cell_quantities(fields[0, k], hs.SOME_DEFINED, minus[0, k], hs.SOME_DEFINED, pivot[0, k], weight, hs.SOME_DEFINED, box)
        for r in range(j1 - j0):
            assert stats[0, k, r, hs.N] == inc[j0 + r].sum()
            for slot, q in ((hs.W, w), (hs.S1, q1), (hs.S2, q2)):
                row = q[j0 + r][inc[j0 + r]]
                assert abs(stats[0, k, r, slot] - math.fsum(row)) <= (70 + 2) * 2.0 ** -53 * math.fsum(np.abs(row))


def test_the_order_of_the_additions_matters_on_the_test_data():
    """The guard against a restatement (or a kernel) that adds in another order and still passes: on wide-range data at
    least three quarters of the sums differ in bits from the flat left-to-right sum."""
    sums = wide_sums()
    differ = sum(1 for got, q, _ in sums if np.float64(got).tobytes() != np.float64(np.cumsum(q)[-1]).tobytes())
    print("sums that differ from the flat sum: %d of %d" % (differ, len(sums)))
    assert differ >= 0.75 * len(sums), (differ, len(sums))


def masked_extremes(level, included, rows):
    """numpy's own answer: (min, max, imin, imax) per row of `rows` (one entry: the whole level), NaN never selected."""
    out = []
    nx = level.shape[1]
    for sel in rows:
        d = level[sel].astype(np.float64)
        ok = included[sel] & ~np.isnan(d)
        first = sel.start * nx
        lo, hi = np.where(ok & (d != np.inf), d, np.inf), np.where(ok & (d != -np.inf), d, -np.inf)
        imin = int(np.argmin(lo)) if (lo != np.inf).any() else None
        imax = int(np.argmax(hi)) if (hi != -np.inf).any() else None
        out.append((np.inf if imin is None else d.ravel()[imin], -np.inf if imax is None else d.ravel()[imax],
                    -1.0 if imin is None else float(first + imin), -1.0 if imax is None else float(first + imax)))
    return np.array(out)


def test_extremes_against_numpy_on_ties_zeros_infinities_and_an_empty_row():
    fields, flags = hs.extremes_case()
    _, nlev, ny, nx = fields.shape
    for mode, rows in ((hs.AREA, [slice(0, ny)]), (hs.ROWS, [slice(j, j + 1) for j in range(ny)])):
        stats, mean, fd = hs.hstats(fields, mode=mode, flags=flags)
        for k in range(nlev):
            included = hs.is_defined(flags[0, k] == hs.ALL_DEFINED, fields[0, k], hs.UNDEF)
            assert hs.same_bits64(stats[0, k, :, hs.MIN:], masked_extremes(fields[0, k], included, rows)), (mode, k)
    rows, _, _ = hs.hstats(fields, mode=hs.ROWS, flags=flags)
    area, mean, fd = hs.hstats(fields, mode=hs.AREA, flags=flags)
    # ties: the first flat index, across lanes, trips, segments and rows
    assert area[0, 0, 0, hs.IMIN] == 1 * nx + 9 and rows[0, 0, 2, hs.IMIN] == 2 * nx + 3 and area[0, 0, 0, hs.IMAX] == 255
    assert rows[0, 0, 3, hs.IMAX] == 3 * nx + hs.SEGMENT + 1
    # -0.0 against +0.0: equal, the first one wins and keeps its sign
    assert rows[0, 1, 1, hs.IMIN] == nx + 17 and np.signbit(rows[0, 1, 1, hs.MIN]) and rows[0, 1, 1, hs.MIN] == 0
    assert rows[0, 1, 2, hs.IMIN] == 2 * nx + 5 and not np.signbit(rows[0, 1, 2, hs.MIN])
    assert area[0, 1, 0, hs.IMIN] == hs.SEGMENT + 2 and not np.signbit(area[0, 1, 0, hs.MIN])
    # infinities: -inf is a minimum and +inf a maximum; the starting infinity is never selected
    assert rows[0, 2, 3, hs.MIN] == -np.inf and rows[0, 2, 3, hs.IMIN] == 3 * nx + nx - 1
    assert rows[0, 2, 3, hs.MAX] == np.inf and rows[0, 2, 3, hs.IMAX] == 3 * nx + 100
    only_inf = np.full((1, 1, 1, 5), np.inf, np.float32)
    s, _, _ = hs.hstats(only_inf)
    assert s[0, 0, 0, hs.MIN] == np.inf and s[0, 0, 0, hs.IMIN] == -1 and s[0, 0, 0, hs.MAX] == np.inf and s[0, 0, 0, hs.IMAX] == 0
    # an empty row
    assert list(rows[0, 2, 0]) == [0, 0, 0, 0, np.inf, -np.inf, -1, -1]
    _, rmean, rfd = hs.hstats(fields, mode=hs.ROWS, flags=flags)
    assert rmean[0, 2, 0] == hs.UNDEF and rfd[0, 2] == hs.SOME_DEFINED and rfd[0, 0] == hs.ALL_DEFINED
    # a NaN under ALL_DEFINED: the sums are NaN, the extremes are not; the stored undef is the maximum there
    assert np.isnan(area[0, 3, 0, hs.S1]) and area[0, 3, 0, hs.MAX] == np.float64(hs.UNDEF) and area[0, 3, 0, hs.IMAX] == nx + 2
    assert area[0, 3, 0, hs.N] == ny * nx and not np.isnan(area[0, 3, 0, hs.MIN])
    # and the literal loop agrees on a cut of it that it can walk
    cut = np.ascontiguousarray(fields[:, :, :, hs.SEGMENT - 40:])
    both_forms("extremes, cut", cut, flags=flags, mode=hs.ROWS)
    both_forms("extremes, cut", cut, flags=flags, mode=hs.AREA)


def test_entry_is_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    for name in ("mifc_hstats_levels", "mifc_last_hstats_form"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert len(capi.SIGNATURES["mifc_hstats_levels"][1]) == 20
    for enum in (r"MIFC_HSTATS_AREA = 0\b", r"MIFC_HSTATS_ROWS = 1\b", r"MIFC_HSTATS_MOMENTS = 1\b", r"MIFC_HSTATS_EXTREMES = 2\b", r"MIFC_HSTATS_IMAX = 7\b"):
        assert re.search(enum, header), enum
    assert re.search(r"mifc_abi_version", header)
    # the environment variable is named in mifc_env.hip and mifc_env.h only, and read in mifc_env.hip only
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    named = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(csrc, "*.h*"))) if "MIFC_HSTATS_CHUNK_MIB" in open(p, errors="replace").read()]
    assert named == ["mifc_env.h", "mifc_env.hip"], named
    for f in ("mifc_hstats.hip", "mifc_capi_hstats.hip"):
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f
    host = open(os.path.join(csrc, "mifc_capi_hstats.hip")).read()
    assert re.search(r"hstats_chunk_mib > 0 \? mifc::env\(\)\.hstats_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_hstats.hip") == 1 and makefile.count("mifc_capi_hstats.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    # the definition is in the header, rule by rule
    full = open(os.path.join(ROOT, "include", "mifc.h")).read()
    for phrase in ("(i / 4) mod 64", "P[t] = P[t] + P[t + s]", "row-major order", "tests/hstats_restate.py", "S2 / W - (S1 / W)^2"):
        assert phrase in full, phrase
