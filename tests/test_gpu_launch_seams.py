"""The elementwise (mifc_ewise.hip) and catalogue (mifc_pointwise.hip) kernels at their launch seams: the cases of
tests/launch_cases.py on the GPU, each forced onto -- or sized for -- the launch shape it is named for:

  * several trips of the grid-stride loop of every ewise_kernel instantiation, with every tail length (MIFC_EWISE_MAX_BLOCKS
    1 and 2), host arrays and device tensors;
  * cells the operator leaves unwritten (hleveltemp, compute 0 and 6) across trips, in the tail and in the scalar form;
  * the one-cell-per-lane form (device pointers one float past the 16-byte grid), one trip and looping;
  * the counts by partials at, below and above the threshold, next to a tail, and the partials buffer kept in the context
    across a smaller and a larger call.

Every case: results and flag against the CPU restatement under the bars the project applies everywhere (bit for bit unless
gpu_util.uses_device_powf, else gpu_util.compare's 1e-5 bound with its floors and slack), AND bit for bit equal to the same
call in its default launch shape -- the launch shape must not change a bit, whatever the operator.  What shape a call took
is asserted from mifc_last_pointwise_form (gpu_util.check_pointwise_form), so a later change of a cap or of the threshold
cannot quietly turn these into ordinary small-field tests."""
import numpy as np
import pytest

import cases
import gpu_util
import launch_cases as lc

pytestmark = pytest.mark.gpu

UNDEF = cases.UNDEF
_EXPECTED = {}  # label -> the restatement's result of a small case, computed once


def _expected(oracle, case, keep=True):
    if case["label"] not in _EXPECTED or not keep:
        with np.errstate(all="ignore"):
            res = cases.run_cpu(oracle, case, prefill=case.get("prefill"))
        if not keep:
            return res
        _EXPECTED[case["label"]] = res
    return _EXPECTED[case["label"]]


def _check(case, got, flag, out_e, flag_e):
    got, out_e = np.asarray(got), np.asarray(out_e)
    gpu_util.compare(case, got, out_e, not gpu_util.uses_device_powf(case))
    assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)
    assert flag == case["expect_flag"], case["label"]
    assert np.array_equal(np.nonzero(got.ravel() == UNDEF)[0], case["expect_undef"]), case["label"]


def _same_bits(case, a, b, what):
    assert cases.same_bits(np.asarray(a), np.asarray(b)), "%s: %s changes the result" % (case["label"], what)


def _family(case):
    return "pointwise" if case["key"] in lc.CATALOGUE else "ewise"


def run_offset(ctx, case, prefill=None):
    """Like gpu_util.run_gpu with device tensors, every field a view that starts one float past the 16-byte grid."""
    import torch

    n = case["nx"] * case["ny"]

    def off(a):
        buf = torch.empty(n + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).cuda()
        view = buf[1:].view(case["ny"], case["nx"])
        assert view.data_ptr() % 16 == 4
        return view

    args = [off(a) if isinstance(a, np.ndarray) else a for a in case["args"]]
    fill = np.float32(-7777.0) if prefill is None else prefill
    out = off(np.full((case["ny"], case["nx"]), fill, np.float32))
    res = getattr(ctx, case["op"])(*args, fdefined=case["fdefined"], undef=case["undef"], out=out)
    if res is None:
        return False, None, None
    return True, res[0].cpu().numpy(), res[1]


# ---------------------------------------------------------------- trips of the vector form
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("key", lc.TRIP_OPS)
def test_trips_and_tails_of_every_ewise_instantiation(gpu_ctx, oracle, mifc_env, key, device):
    trips_seen = set()
    mifc_env("MIFC_EWISE_MAX_BLOCKS", None)
    plain = {}
    for blocks in (1, 2):
        for case in lc.trip_cases(key, blocks):
            plain[case["label"]] = gpu_util.run_gpu(gpu_ctx, case, device=device)
            if plain[case["label"]][0]:
                form = gpu_util.check_pointwise_form(gpu_ctx, case["label"], family="ewise", form="vector", tail=case["tail"], n=case["nx"] * case["ny"])
                assert form is None or lc.trips(case["n4"], form["grid"]) == 1  # the default shape of a small field: one trip
    for blocks in (1, 2):
        mifc_env("MIFC_EWISE_MAX_BLOCKS", blocks)
        for case in lc.trip_cases(key, blocks):
            ok_e, out_e, flag_e = _expected(oracle, case)
            ok, got, flag = gpu_util.run_gpu(gpu_ctx, case, device=device)
            assert ok == ok_e == plain[case["label"]][0], case["label"]
            if not ok:
                continue
            form = gpu_util.check_pointwise_form(gpu_ctx, case["label"], family="ewise", form="vector", grid=min(blocks, lc.vector_grid(4 * case["n4"])),
                                                 tail=case["tail"], partials=0, n=case["nx"] * case["ny"])
            if form is not None:
                assert lc.trips(form["n"] // 4, form["grid"]) == case["trips"], (case["label"], form)
                trips_seen.add(case["trips"])
            _check(case, got, flag, out_e, flag_e)
            _same_bits(case, got, plain[case["label"]][1], "MIFC_EWISE_MAX_BLOCKS=%d" % blocks)
            assert flag == plain[case["label"]][2], case["label"]
    assert not trips_seen or trips_seen == {1, 2, 3, 5}, trips_seen


# ---------------------------------------------------------------- kept cells
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("key", lc.KEEP_OPS)
def test_kept_cells_across_trips_and_in_the_tail(gpu_ctx, oracle, mifc_env, key, device):
    """hleveltemp with a compute outside 1..5 writes the undefined cells only: every other cell keeps what the output held
    (host arrays: the staging buffer is preloaded), here a pattern that differs from cell to cell."""
    for blocks in (1, 2):
        mifc_env("MIFC_EWISE_MAX_BLOCKS", blocks)
        for case in lc.keep_cases(key, blocks):
            ok_e, out_e, flag_e = _expected(oracle, case)
            ok, got, flag = gpu_util.run_gpu(gpu_ctx, case, device=device, prefill=case["prefill"])
            assert ok and ok_e, case["label"]
            form = gpu_util.check_pointwise_form(gpu_ctx, case["label"], family="ewise", form="vector", grid=blocks, tail=case["tail"], partials=0)
            assert form is None or (lc.trips(form["n"] // 4, form["grid"]) == case["trips"] >= 2 and form["tail"] > 0)
            _check(case, got, flag, out_e, flag_e)
            _same_bits(case, got, out_e, "the GPU")
            kept = np.ones(got.size, bool)
            kept[case["expect_undef"]] = False
            _same_bits(case, got.ravel()[kept], case["prefill"].ravel()[kept], "a kept cell: the call")


@pytest.mark.parametrize("key", lc.KEEP_OPS)
def test_kept_cells_in_the_scalar_form(gpu_ctx, oracle, key):
    for case in lc.keep_cases(key, per_lane=1):
        ok_e, out_e, flag_e = _expected(oracle, case)
        ok, got, flag = run_offset(gpu_ctx, case, prefill=case["prefill"])
        assert ok and ok_e, case["label"]
        gpu_util.check_pointwise_form(gpu_ctx, case["label"], family="ewise", form="scalar", grid=lc.scalar_grid(got.size), tail=0, partials=0)
        _check(case, got, flag, out_e, flag_e)
        _same_bits(case, got, out_e, "the GPU")


# ---------------------------------------------------------------- the scalar form
@pytest.mark.parametrize("shape", [lc.SCALAR_SMALL, lc.SCALAR_LOOP], ids=["one-trip", "looping"])
@pytest.mark.parametrize("key", lc.SCALAR_OPS)
def test_scalar_form_off_the_16_byte_grid(gpu_ctx, oracle, key, shape):
    n = shape[0] * shape[1]
    for case in lc.scalar_cases(key, shape):
        ok_e, out_e, flag_e = _expected(oracle, case, keep=shape == lc.SCALAR_SMALL)
        ok, got, flag = run_offset(gpu_ctx, case)
        assert ok and ok_e, case["label"]
        form = gpu_util.check_pointwise_form(gpu_ctx, case["label"], family=_family(case), form="scalar", grid=lc.scalar_grid(n), tail=0, partials=0, n=n)
        if form is not None:
            assert lc.trips(form["n"], form["grid"]) == (2 if shape == lc.SCALAR_LOOP else 1), form
        _check(case, got, flag, out_e, flag_e)
        ok_v, got_v, flag_v = gpu_util.run_gpu(gpu_ctx, case, device=True)  # the same fields on the grid: four cells per lane
        gpu_util.check_pointwise_form(gpu_ctx, case["label"], family=_family(case), form="vector", tail=n % 4)
        _same_bits(case, got, got_v, "the scalar form")
        assert flag == flag_v, case["label"]


# ---------------------------------------------------------------- counting by partials
@pytest.mark.parametrize("where", sorted(lc.PARTIALS_SHAPES))
@pytest.mark.parametrize("key", lc.PARTIALS_OPS)
def test_counts_by_partials_at_below_and_above_the_threshold(gpu_ctx, oracle, key, where):
    for case in lc.partials_cases(key, where):
        ok_e, out_e, flag_e = _expected(oracle, case, keep=False)
        assert ok_e
        for device in (False, True):
            ok, got, flag = gpu_util.run_gpu(gpu_ctx, case, device=device)
            assert ok, case["label"]
            gpu_util.check_pointwise_form(gpu_ctx, case["label"], family=_family(case), form="vector", grid=case["grid"],
                                          partials=1 if case["partials"] else 0, tail=case["tail"])
            _check(case, got, flag, out_e, flag_e)
    assert {"at": (True, 0), "below": (False, 0), "above": (True, 3)}[where] == (case["partials"], case["tail"])


def test_partials_buffer_kept_across_a_smaller_and_a_larger_call(oracle):
    """One context of its own, so that the buffer starts empty: 4096 partials of 1024 each (NONE_DEFINED); then 2048 workgroups
    with nothing undefined under a SOME_DEFINED flag, which comes back ALL_DEFINED only if the 2048 stale partials beyond
    the grid are not added; then more workgroups than the buffer has held, which reallocates it."""
    import mi_fieldcalc_amd as fc

    first, second, third = lc.sequence_cases()
    with fc.Context(0) as ctx:
        for case, grid in ((first, 4096), (second, 2048), (third, 4100)):
            ok_e, out_e, flag_e = _expected(oracle, case, keep=False)
            ok, got, flag = gpu_util.run_gpu(ctx, case, device=True)
            assert ok and ok_e, case["label"]
            gpu_util.check_pointwise_form(ctx, case["label"], family="ewise", form="vector", grid=grid, partials=1, tail=0)
            _check(case, got, flag, out_e, flag_e)
    assert (first["expect_flag"], second["expect_flag"], third["expect_flag"]) == (cases.NONE_DEFINED, cases.ALL_DEFINED, cases.SOME_DEFINED)
