"""The host build of the per-cell vessel-icing models (mi-fieldcalc_amd/csrc/mifc_icing_cell.h, the text the GPU
kernels compile) against the compiled reference, bit for bit.  No GPU."""
import numpy as np
import pytest

import icing_cases as ic


@pytest.fixture(scope="module")
def cell(tmp_path_factory):
    return ic.CellShim(tmp_path_factory.mktemp("iccell"))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    if not ic.ref_available():
        pytest.skip("oracle/_ref/libmifc_ref.so not built (needs the reference sources at build time)")
    return ic.RefShim(tmp_path_factory.mktemp("icref"))


MODELS = [(ic.MODSTALL, 1), (ic.MINCOG, 1), (ic.MINCOG, 2), (ic.MINCOG, 0)]


def test_bisection_trip_count(cell):
    """MINCOG's bisection runs min((int)log2((1.3f - -0.5f) / 1e-5f), 100) trips (FieldCalculationsVesselIcing.cc:391):
    17, derived on the host the way the reference derives it."""
    assert cell.lib.iccell_bisect_iterations() == 17
    assert int(np.log2(np.float32(np.float32(1.3) - np.float32(-0.5)) / np.float32(1e-5))) == 17


def test_sinhf_restatement_is_glibc(cell):
    """MINCOG "adj" calls sinhf, and glibc's is not the double sinh rounded once; the device restates glibc's float
    algorithm (sinhf_fdlibm).  Below 22 in magnitude (the expm1f branch) it is glibc's on every 3rd float; above, its
    expf is the double exp rounded once, which differs from glibc's expf on a few arguments in ten thousand."""
    assert cell.lib.iccell_sinhf_mismatches(0, 0x41B00000, 3) == 0
    big = cell.lib.iccell_sinhf_mismatches(0x41B00000, 0x42B20000, 1)
    assert big <= 2 * (0x42B20000 - 0x41B00000) * 1e-3


@pytest.mark.parametrize("model,alt", MODELS, ids=["modstall", "mincog-org", "mincog-adj2", "mincog-adj0"])
@pytest.mark.parametrize("flag", [ic.ALL_DEFINED, ic.SOME_DEFINED], ids=["all", "some"])
@pytest.mark.parametrize("specials", [False, True], ids=["plain", "specials"])
def test_cell_header_is_the_reference_bit_for_bit(cell, ref, model, alt, flag, specials):
    for seed, (nx, ny) in enumerate([(61, 37), (1, 1), (7, 130)]):
        fields = ic.make_inputs(nx, ny, 100 * model + 10 * alt + seed, specials=specials)
        if flag == ic.ALL_DEFINED and specials:  # undefined values only matter to the tested path; NaNs go through
            fields = [np.where(f == ic.UNDEF, np.float32(1.0), f) for f in fields]
        st, fl, mine = cell.run(model, fields, alt=alt, fdefined=flag, **ic.SCALARS)
        ok, rfl, theirs = ref.run(model, fields, alt=alt, fdefined=flag, **ic.SCALARS)
        label = (model, alt, flag, specials, nx, ny)
        assert st == 1 and ok and fl == rfl, label
        assert ic.same_bits(mine, theirs), label


@pytest.mark.parametrize("model", [ic.MODSTALL, ic.MINCOG])
@pytest.mark.parametrize("zmin,zmax", [(0.0, 0.0), (0.0, 60.0), (2.5, 7.5), (0.0, 0.5)])
@pytest.mark.parametrize("vs,alpha", [(5.0, 0.7), (0.0, 0.0), (12.0, 3.0), (3.0, 2.0)])
def test_scalars_bit_for_bit(cell, ref, model, zmin, zmax, vs, alpha):
    """One level, 121 levels, a fractional zmin, a half-integral span (the reference's false), and angles that take
    MINCOG's three beta_r branches."""
    fields = ic.make_inputs(23, 11, 7, specials=True)
    st, fl, mine = cell.run(model, fields, vs, alpha, zmin, zmax, alt=2)
    ok, rfl, theirs = ref.run(model, fields, vs, alpha, zmin, zmax, alt=2)
    assert (st == 1) == ok and fl == rfl
    assert ic.same_bits(mine, theirs)


def test_defined_cells_and_edge_cases_are_exercised(cell):
    """The sweep above reaches what it claims: undefined cells, early returns, both sides of the cuts, and the
    shallow-water fixed point giving up (10 000 trips for ModStall, 1000 for MINCOG) on negative depth."""
    fields = ic.make_inputs(61, 37, 3, specials=True)
    st, fl, out, (dh, lh) = cell.run(ic.MODSTALL, fields, trips=True, **ic.SCALARS)
    assert st == 1 and fl == ic.SOME_DEFINED
    assert dh[10001] > 0 and dh[1:100].sum() > 0  # gave up, and converged
    assert lh[1:1001].sum() > 0
    st, fl, out2, (dh2, lh2) = cell.run(ic.MINCOG, fields, alt=1, trips=True, **ic.SCALARS)
    assert dh2[1000] > 0 and (lh2[17] > 0) and lh2[:17].sum() == 0 and lh2[18:].sum() == 0
    assert (out2 == 0).any() and (out2 == ic.UNDEF).any() and ((out2 > 0) & (out2 != ic.UNDEF)).any()
    aice = fields[9]
    assert (out[aice == np.float32(0.4)] == ic.UNDEF).all()  # float 0.4 is not < double 0.4
    assert (out[aice == np.float32(0.39999998)] != ic.UNDEF).any()


@pytest.mark.parametrize("model", [ic.MODSTALL, ic.MINCOG])
def test_false_and_refusals(cell, ref, model):
    fields = ic.make_inputs(5, 4, 1)
    for vs, alpha, zmin, zmax in [(-1, 0.7, 0, 10), (5, -0.1, 0, 10), (5, 0.7, -1, 10), (5, 0.7, 3, 2), (5, 0.7, 0, 10.5),
                                  (5, 0.7, float("nan"), 10), (5, 0.7, 0, float("inf"))]:
        st, fl, mine = cell.run(model, fields, vs, alpha, zmin, zmax)
        ok, rfl, theirs = ref.run(model, fields, vs, alpha, zmin, zmax)
        assert st == 0 and not ok and fl == rfl == ic.SOME_DEFINED
        assert (mine == ic.SENTINEL).all() and (theirs == ic.SENTINEL).all()
    st, _, mine = cell.run(model, fields, 5, 0.7, 0, 2.0e9)  # 4e9 + 1 levels: not an int
    assert st == -1 and (mine == ic.SENTINEL).all()
