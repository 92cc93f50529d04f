"""Pins the CPU restatement (oracle/mifc_oracle.cc) against the REAL reference
-- bit for bit, on the seeded sweep of tests/cases.py (every hot-path operator
x grid shape x undefined-value mode x compute/unit variant, plus the argument
validation cases).  Runs on the CPU, everywhere: the reference's answer to
every case is recorded in tests/golden/reference_sweep_digests.npz (return
value, flag, SHA-256 of each output; tests/golden/make_golden.py).  Where
oracle/Makefile has compiled the reference into oracle/_ref/, each case is
also run through it: the recording must still be what it computes, and a
difference from the restatement is reported cell by cell."""
import numpy as np
import pytest

import cases
import golden_util


@pytest.fixture(scope="module")
def recorded():
    return golden_util.RecordedSweep()


@pytest.fixture(scope="module")
def live_ref():
    from cpulib import CpuLib, available

    return CpuLib("ref") if available("ref") else None


def _outs(out):
    return out if isinstance(out, tuple) else (out,)


def _check(oracle, live_ref, case, expect):
    ok_r, flag_r, digests_r = expect
    ok_o, out_o, flag_o = cases.run_cpu(oracle, case)
    if live_ref is not None:
        ok_l, out_l, flag_l = cases.run_cpu(live_ref, case)
        assert (ok_l, flag_l if ok_l else None) == (ok_r, flag_r if ok_r else None), "stale recording: %s" % case["label"]
        if ok_l:
            assert [golden_util.output_digest(o) for o in _outs(out_l)] == digests_r, "stale recording: %s" % case["label"]
            for a, b in zip(_outs(out_o), _outs(out_l)):
                if not cases.same_bits(a, b, nan_payload=False):  # NaN sign/payload of an arithmetic NaN depends on instruction selection
                    bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))
                    raise AssertionError("%s: %d cells differ, first at %s: oracle %r ref %r" % (
                        case["label"], len(bad[0]), (bad[0][0], bad[1][0]), a[bad][0], b[bad][0]))
    assert ok_o == ok_r, case["label"]
    if not ok_r:
        return
    assert flag_o == flag_r, case["label"]
    assert [golden_util.output_digest(o) for o in _outs(out_o)] == digests_r, case["label"]


def _sweep(oracle, recorded, live_ref, family):
    cs = recorded.cases(family)
    for case, expect in cs:
        _check(oracle, live_ref, case, expect)
    return len(cs)


def test_kinds(oracle, recorded, live_ref):
    assert oracle.kind == "restatement"
    assert recorded.kind.startswith("reference 0.1.")
    if live_ref is not None:
        assert live_ref.kind == recorded.kind


def test_stencils_bit_exact(oracle, recorded, live_ref):
    assert _sweep(oracle, recorded, live_ref, "stencil") > 300


def test_two_pass_stencils_bit_exact(oracle, recorded, live_ref):
    """thermalFrontParameter / plevelqvector where the flag handed from pass to pass matters
    (clean first pass, zero-gradient plateaus, a NaN gradient from defined inputs)."""
    assert _sweep(oracle, recorded, live_ref, "fused2") > 250


def test_elementwise_bit_exact(oracle, recorded, live_ref):
    assert _sweep(oracle, recorded, live_ref, "ewise") > 1500


def test_catalogue_bit_exact(oracle, recorded, live_ref):
    """theta-e, ducting, indices, conversions, field algebra."""
    assert _sweep(oracle, recorded, live_ref, "catalogue") > 1500


def test_ensemble_reductions_bit_exact(oracle, recorded, live_ref):
    """SURVEY.md 8f-4."""
    assert _sweep(oracle, recorded, live_ref, "ensemble") > 400


def test_headline_level_bit_exact(oracle, recorded, live_ref):
    """One full 1440x720 level of the headline configuration, all-defined and with undefined cells."""
    assert _sweep(oracle, recorded, live_ref, "headline") == 4
