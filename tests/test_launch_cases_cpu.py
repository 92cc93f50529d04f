"""The launch-seam cases of tests/launch_cases.py on the CPU, before any GPU is involved: every generator against the
restatement -- the output flag is the one the case is named for and the undefined output cells lie exactly where its label
says -- and, where the compiled reference is built, the restatement against it on every case, bit for bit for every
operator (both run glibc's powf on the CPU; the bar of tests/test_oracle_vs_ref.py).  Also the arithmetic of the positions
themselves: the shapes reach the trips, grids and tails they claim."""
import numpy as np
import pytest

import cases
import gpu_util
import launch_cases as lc

F = np.float32
UNDEF = cases.UNDEF


def _run(lib, case):
    with np.errstate(all="ignore"):
        return cases.run_cpu(lib, case, prefill=case.get("prefill"))


def check_expectation(case, ok, out, flag):
    """The result of a CPU checker is what the case is named for."""
    if case["op"].startswith("momentum") and (case["nx"] < 3 or case["ny"] < 3):
        assert not ok, case["label"]  # FieldCalculations.cc:2363, :2397
        return
    assert ok, case["label"]
    assert flag == case["expect_flag"], "%s: flag %d, named for %d" % (case["label"], flag, case["expect_flag"])
    got = np.nonzero(np.asarray(out).ravel() == UNDEF)[0]
    assert np.array_equal(got, case["expect_undef"]), "%s: undefined cells %s, named for %s" % (case["label"], got[:8], case["expect_undef"][:8])
    if "prefill" in case:  # every defined cell is left as it was
        keep = np.ones(out.size, bool)
        keep[case["expect_undef"]] = False
        assert cases.same_bits(out.ravel()[keep], case["prefill"].ravel()[keep]), case["label"]


def agree(case, res_o, res_r):
    (ok_o, out_o, flag_o), (ok_r, out_r, flag_r) = res_o, res_r
    assert ok_o == ok_r, case["label"]
    if not ok_r:
        return
    assert flag_o == flag_r, case["label"]
    gpu_util.compare(case, np.asarray(out_o), np.asarray(out_r), True)


def small_cases():
    for key in lc.TRIP_OPS:
        for blocks in (1, 2):
            yield from lc.trip_cases(key, blocks)
    for key in lc.KEEP_OPS:
        yield from lc.keep_cases(key, 1)
        yield from lc.keep_cases(key, 2)
        yield from lc.keep_cases(key, per_lane=1)
    for key in lc.SCALAR_OPS:
        yield from lc.scalar_cases(key, lc.SCALAR_SMALL)


def test_positions_reach_the_seams_they_name():
    for blocks, depths in ((1, {1, 2, 3, 5}), (2, {2, 3})):
        seen = set()
        for n4, tail, nx, ny in lc.trip_shapes(blocks):
            n = nx * ny
            assert n == 4 * n4 + tail
            cells = lc.seam_cells(n, blocks)
            nt = lc.trips(n4, blocks)
            seen.add(nt)
            assert cells["tail"] == list(range(4 * n4, n)) and cells["first"] == [0]
            assert cells["end_of_first_trip"] == [4 * min(n4, blocks * 256) - 1]
            if nt > 1:
                lo, hi = cells["last_trip"]
                assert lo == 4 * (nt - 1) * blocks * 256 and hi == 4 * n4 - 1 and lo <= hi
            assert all(0 <= c < n for c in lc.flat_cells(cells))
        assert seen == depths, seen
    # ny > 1 and nx no multiple of 4 wherever the cell count has such factors (7 x 147 = 1029: n4 257, tail 1)
    assert lc.shape_for(1029) == (7, 147)
    good = [(nx, ny) for _, _, nx, ny in lc.trip_shapes(1) + lc.trip_shapes(2) if ny > 1]
    assert len(good) >= 24 and all(nx % 4 and nx >= 3 and ny >= 3 for nx, ny in good)
    # the partials threshold from both sides, and the tail next to the partials
    grids = {k: lc.vector_grid(nx * ny) for k, (nx, ny) in lc.PARTIALS_SHAPES.items()}
    assert grids == {"at": 2048, "below": 2046, "above": 2049}
    assert [nx * ny % 4 for nx, ny in lc.PARTIALS_SHAPES.values()] == [0, 0, 3]
    # the scalar form: one trip, and 257 lanes with a second one
    n = lc.SCALAR_LOOP[0] * lc.SCALAR_LOOP[1]
    assert n == 4096 * 256 + 257 and lc.scalar_grid(n) == 4096 and lc.trips(n, 4096) == 2
    assert lc.seam_cells(n, 4096, 1)["last_trip"] == [4096 * 256, n - 1]
    assert lc.scalar_grid(1029) == 5 and lc.trips(1029, 5) == 1
    # nothing larger than 4100 x 1024
    assert max(c["nx"] * c["ny"] for c in lc.sequence_cases()) == 4100 * 1024


def test_every_small_case_is_what_it_is_named_for(oracle):
    n_cases, modes, momentum_ok = 0, set(), 0
    for case in small_cases():
        ok, out, flag = _run(oracle, case)
        check_expectation(case, ok, out, flag)
        n_cases += 1
        modes.add((case["key"], case["mode"]))
        momentum_ok += int(ok and case["op"].startswith("momentum"))
    assert n_cases > 800 and momentum_ok >= 2 * 24
    for key in lc.TRIP_OPS:
        assert {(key, m) for m in ("some", "all", "none", "clean")} <= modes, key
    # a hot cell under ALL_DEFINED is counted for every operator that reads the saturation table
    for key in lc.TRIP_OPS:
        case = [c for c in lc.trip_cases(key, 1) if c["mode"] == "all"][0]
        assert (case["expect_flag"] == cases.SOME_DEFINED) == (lc.OPS[key].hot is not None), key


@pytest.mark.parametrize("key", lc.PARTIALS_OPS)
def test_partials_cases_are_what_they_are_named_for(oracle, key):
    for where in lc.PARTIALS_SHAPES:
        for case in lc.partials_cases(key, where):
            ok, out, flag = _run(oracle, case)
            check_expectation(case, ok, out, flag)
            n = case["nx"] * case["ny"]
            if case["mode"] == "some":  # the first and the last workgroup and every tail cell hold an undefined cell
                und = case["expect_undef"]
                assert und[0] == 0 and np.any((und >= (case["grid"] - 1) * 1024) & (und < n - n % 4))
                assert set(range(n - n % 4, n)) <= set(und.tolist())


def test_sequence_and_looping_scalar_cases_are_what_they_are_named_for(oracle):
    flags = []
    for case in lc.sequence_cases():
        ok, out, flag = _run(oracle, case)
        check_expectation(case, ok, out, flag)
        flags.append(flag)
    assert flags == [cases.NONE_DEFINED, cases.ALL_DEFINED, cases.SOME_DEFINED]
    for key in lc.SCALAR_OPS:
        for case in lc.scalar_cases(key, lc.SCALAR_LOOP):
            ok, out, flag = _run(oracle, case)
            check_expectation(case, ok, out, flag)
            if case["mode"] == "some" or lc.OPS[key].hot is not None:  # undefined cells in the second trip
                assert case["expect_undef"][-1] == case["nx"] * case["ny"] - 1 and 4096 * 256 in case["expect_undef"]


def test_restatement_equals_compiled_reference_on_the_small_cases(oracle, ref):
    for case in small_cases():
        agree(case, _run(oracle, case), _run(ref, case))


@pytest.mark.parametrize("key", lc.PARTIALS_OPS)
def test_restatement_equals_compiled_reference_on_the_large_cases(oracle, ref, key):
    big = [c for where in lc.PARTIALS_SHAPES for c in lc.partials_cases(key, where)]
    if key in lc.SCALAR_OPS:
        big += lc.scalar_cases(key, lc.SCALAR_LOOP)
    if key == "vectorabs":
        big += lc.sequence_cases() + lc.scalar_cases("hlevelhum5", lc.SCALAR_LOOP)
    for case in big:
        agree(case, _run(oracle, case), _run(ref, case))
