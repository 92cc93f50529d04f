"""mifc_vparcel_* on the GPU at scaled pressures and with the ends of the float range among its inputs: the cases of
tests/vparcel_range_cases.py through the library against the numpy restatement, by the rule of tests/test_gpu_vparcel.py
unchanged -- undef cells and flags exact on the stable cells, values within 2 * max_j |R_j - R0| + 2 ulp of the restatement's
nudge family.  One addition for the special cases: where R0 is NaN or infinite on a stable cell (every member of the family
then has the same bits there: vparcel_range_cases.Reference), the bound says nothing, and the kernel must give the same bits
(a NaN is a NaN).  What the cases reach and which mistakes they would show is asserted on the CPU in
tests/test_vparcel_range_cpu.py.

Per case and coordinate form: host memory, device memory on the 16-byte grid and one float past it give the same bits, the
launch form is read back, the result is compared with the reference.  Subsets of the outputs equal the full set; one scaled
case goes through the host path in several bands."""
import numpy as np
import pytest

import test_gpu_vparcel as tvp
import vparcel_cases as vc
import vparcel_range_cases as vr
import vparcel_restate as vp

pytestmark = pytest.mark.gpu

U = vp.UNDEF
ALL = vp.OUTPUTS


def against_reference(got, ref, label):
    """tests/test_gpu_vparcel.py::against_reference on the values of R0 that are finite; the others bit for bit."""
    r0 = ref.r0
    whole = ref.stable.all()
    for n in ALL:
        g, e = got[n], r0[n]
        assert g.shape == e.shape and g.dtype == np.float32, (label, n)
        st = ref.stable if e.ndim == 2 else np.broadcast_to(ref.stable, e.shape)
        gu, eu = g.view(np.uint32) == U.view(np.uint32), e == U
        assert np.array_equal(gu[st], eu[st]), (label, n, "undef cells differ", int((gu != eu)[st].sum()))
        if whole:
            assert np.array_equal(got["flags"][n], r0["flags"][n]), (label, n, got["flags"][n], r0["flags"][n])
        odd = st & ~np.isfinite(e)
        same = (g.view(np.uint32) == e.view(np.uint32)) | (np.isnan(g) & np.isnan(e))
        assert same[odd].all(), (label, n, "a NaN or infinity of the restatement is something else", g[odd & ~same][:4], e[odd & ~same][:4])
        m = st & ~eu & np.isfinite(e)
        with np.errstate(all="ignore"):
            err = np.abs(g.astype(np.float64) - e.astype(np.float64))[m]
            bound = ref.bound(n)[m]
        if not (err <= bound).all():
            bad = np.nonzero(~(err <= bound))[0]
            raise AssertionError("%s %s: %d stable values beyond the bound; worst |got - R0| / bound = %.3g (got %r, R0 %r, bound %r)" % (
                label, n, bad.size, float((err / bound)[bad].max()), g[m][bad[0]], e[m][bad[0]], bound[bad[0]]))


@pytest.mark.parametrize("name", vr.case_names())
def test_every_case_three_forms_and_three_placements(gpu_ctx, name):
    c = vr.by_name(name)
    v4 = 4 if (c["ny"] * c["nx"]) % 4 == 0 else 1
    for form in vc.FORMS:
        want = {"form": tvp.FORM_NAMES[form], "from": c["from"], "src": -1 if c["src_level"] is None else c["src_level"], "outputs": 6, "launches": 1}
        host = tvp.run(gpu_ctx, c, form, False)
        assert tvp.front().last_vparcel_form(gpu_ctx) == dict(want, v=4), (name, form)  # a staged band always takes four cells per lane
        on_grid = tvp.run(gpu_ctx, c, form, True)
        assert tvp.front().last_vparcel_form(gpu_ctx) == dict(want, v=v4), (name, form)
        off_grid = tvp.run(gpu_ctx, c, form, True, offset=True)
        assert tvp.front().last_vparcel_form(gpu_ctx) == dict(want, v=1), (name, form)
        tvp.same(on_grid, off_grid, (name, form, "on the grid / one float past it"))
        tvp.same(on_grid, host, (name, form, "device / host"))
        against_reference(on_grid, vr.reference(name, form), (name, form))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_any_subset_of_the_outputs_equals_all_of_them(gpu_ctx, device):
    names = vr.case_names()
    picks = [n for n in names if n.endswith("_s-49")][:1] + [n for n in names if n.endswith("_s116")][1:2] + [n for n in names if n.endswith("_special")][1:2]
    assert len(picks) == 3
    for name, form in zip(picks, vc.FORMS):
        c = vr.by_name(name)
        every = tvp.run(gpu_ctx, c, form, device)
        for subset in (("cape",), ("tparcel",), ("pel", "plcl"), ("cin", "plfc", "tparcel"), "plcl"):
            chosen = (subset,) if isinstance(subset, str) else subset
            got = tvp.run(gpu_ctx, c, form, device, outputs=subset)
            assert tvp.front().last_vparcel_form(gpu_ctx)["outputs"] == len(chosen)
            tvp.same(got, {**{n: every[n] for n in chosen}, "flags": {n: every["flags"][n] for n in chosen}}, (name, form, subset))


def test_a_scaled_case_in_several_bands(gpu_ctx, mifc_env):
    """p_b around 2^-40 through the host path with MIFC_VPARCEL_CHUNK_MIB = 1: several bands, the bits of one band and of
    the device call, and the banded result against the restatement by the rule of the file.  The grid is larger than the
    10 x 206 of the cases: the smallest budget is one MiB, which the 21 staged planes of 2 060 cells (170 KiB) do not
    exceed; it is the grid tests/test_gpu_vparcel.py takes its bands from."""
    c = vc.make(7, 41, 651, "last", "first", factor=vr.SCALES["s-49"])  # 26 691 cells, 21 planes staged: more than two MiB
    for form in ("hyb", "fld"):
        mifc_env("MIFC_VPARCEL_CHUNK_MIB", None)
        whole = tvp.run(gpu_ctx, c, form, False)
        assert tvp.front().last_vparcel_form(gpu_ctx)["launches"] == 1
        mifc_env("MIFC_VPARCEL_CHUNK_MIB", 1)
        banded = tvp.run(gpu_ctx, c, form, False)
        assert tvp.front().last_vparcel_form(gpu_ctx)["launches"] >= 3, tvp.front().last_vparcel_form(gpu_ctx)
        tvp.same(whole, banded, (c["name"], form, "one band / several"))
        dev = tvp.run(gpu_ctx, c, form, True)
        tvp.same(whole, dev, (c["name"], form, "host / device"))
        ref = vr.Reference(c, form)
        assert (~ref.stable).mean() <= 0.02 and (ref.r0["cape"] != U).mean() > 0.8
        against_reference(banded, ref, (c["name"], form, "bands"))
