"""mifc_ensemble_levels without a GPU: the product-spec normalisation of Context.ensembleStatistics, and the entry's
declaration, export and binding."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc.so")


def test_product_specs_are_normalised():
    import mi_fieldcalc_amd as fc

    SUM, MEAN, STDDEV, EXTREME, PROB = 0, 1, 2, 3, 4
    flags = np.array([fc.ALL_DEFINED, fc.SOME_DEFINED], np.int32)
    got = fc.ensemble_products(["mean", ("stddev",), "sum", ("max", fc.ALL_DEFINED), ("min", flags), "argmax", ("argmin", 1), ("probability", 1, [2.5]), ("probability", 3, (1.0, 2.0)), ("probability", 6, [0, 1]),
                                ("probability", 5, 0.5)])
    assert [g[:3] for g in got] == [(MEAN, 0, ()), (STDDEV, 0, ()), (SUM, 0, ()), (EXTREME, 1, ()), (EXTREME, 2, ()), (EXTREME, 3, ()),
                                    (EXTREME, 4, ()), (PROB, 1, (2.5,)), (PROB, 3, (1.0, 2.0)), (PROB, 6, (0.0, 1.0)), (PROB, 5, (0.5,))]
    assert got[0][3] is None and got[1][3] is None and got[7][3] is None  # no input flag of their own
    assert got[2][3] == fc.SOME_DEFINED and got[3][3] == fc.ALL_DEFINED and got[4][3] is flags and got[5][3] == fc.SOME_DEFINED and got[6][3] == 1
    assert fc.ensemble_products([("extreme", 3, fc.ALL_DEFINED)]) == [(EXTREME, 3, (), fc.ALL_DEFINED)]
    assert fc.ensemble_products(["MEAN"]) == [(MEAN, 0, (), None)]
    # the most one list holds: fifteen
    full = ["sum", "mean", "stddev", "max", "min", "argmax", "argmin"] + [("probability", 1, [float(k)]) for k in range(8)]
    assert len(fc.ensemble_products(full)) == 15


@pytest.mark.parametrize("bad", [
    [],
    ["mean", "mean"],
    ["sum", ("sum", 0)],
    ["max", ("extreme", 1)],
    [("argmin", 0), "mean", "argmin"],
    [("probability", 1, [float(k)]) for k in range(9)],
    [("probability", 0, [1.0])],
    [("probability", 7, [1.0])],
    [("extreme", 5)],
    [("extreme", 0, 2)],
    [("probability", 3, [1.0])],
    [("probability", 6, 1.0)],
    [("probability", 1, [])],
    [("probability", 1, [1.0, 2.0, 3.0])],
    [("probability", 1)],
    ["median"],
    [("mean", 0)],
    [3],
], ids=lambda b: repr(b)[:40])
def test_bad_product_lists_are_rejected(bad):
    import mi_fieldcalc_amd as fc

    with pytest.raises(ValueError):
        fc.ensemble_products(bad)


def test_entry_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mifc.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+mifc_ensemble_levels\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, "include/mifc.h does not declare mifc_ensemble_levels"
    assert m.group(1).count(",") + 1 == 11
    assert re.search(r"typedef\s+struct\s+mifc_ens_product\s*\{[^}]*\}\s*mifc_ens_product\s*;", code, flags=re.S)
    for k, name in enumerate(("SUM", "MEAN", "STDDEV", "EXTREME", "PROBABILITY")):
        assert re.search(r"MIFC_ENS_%s\s*=\s*%d\b" % (name, k), code), name
    assert hasattr(ctypes.CDLL(LIB), "mifc_ensemble_levels"), "libmifc.so does not export mifc_ensemble_levels"
    import mi_fieldcalc_amd as fc
    import mi_fieldcalc_amd._capi as capi

    assert len(capi.SIGNATURES["mifc_ensemble_levels"][1]) == 11
    assert callable(fc.Context.ensembleStatistics)
    # the ctypes mirror of mifc_ens_product has the C layout: int, int, float[2], int, (padding,) two pointers
    p = capi.EnsProduct
    assert (p.stat.offset, p.compute.offset, p.limits.offset, p.nlimits.offset, p.out.offset, p.fdefined.offset) == (0, 4, 8, 16, 24, 32)
    assert ctypes.sizeof(p) == 40


def test_chunk_budget_is_read_with_the_rest_of_the_environment():
    env = open(os.path.join(ROOT, "mi-fieldcalc_amd", "csrc", "mifc_env.hip")).read()
    assert '"MIFC_ENSEMBLE_CHUNK_MIB"' in env
    host = open(os.path.join(ROOT, "mi-fieldcalc_amd", "csrc", "mifc_capi_ensemble.hip")).read()
    assert "ensemble_chunk_mib" in host and "getenv" not in host


def test_launch_shape_read_back_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "mifc.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.search(r"\bconst\s+char\s*\*\s*mifc_last_ensemble_form\s*\(\s*void\s*\)\s*;", code), "include/mifc.h does not declare it"
    doc = re.search(r"/\*\s*mifc_last_ensemble_form:.*?\*/", text, flags=re.S)
    assert doc, "include/mifc.h does not document it"
    for key in ("entry=single", "entry=levels", "entry=quantiles", "c=", "tail=", "welford=", "flagged=", "np=", "tier=", "inline=", "launches=",
                "lev_chunk=", "cell_chunk=", "partials="):
        assert key in doc.group(0), key
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "mifc_last_ensemble_form"), "libmifc.so does not export mifc_last_ensemble_form"
    import mi_fieldcalc_amd as fc
    import mi_fieldcalc_amd._capi as capi

    assert capi.SIGNATURES["mifc_last_ensemble_form"] == ("s", [])
    assert callable(fc.Context.last_ensemble_form)
    # "" before the first call of a thread: read on a fresh one (no GPU is touched)
    import threading

    lib.mifc_last_ensemble_form.restype = ctypes.c_char_p
    seen = []
    t = threading.Thread(target=lambda: seen.append(lib.mifc_last_ensemble_form()))
    t.start()
    t.join()
    assert seen == [b""]
    # every entry notes its shape through the one function of the member-batch driver
    csrc = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
    for name in ("mifc_capi_catalogue.hip", "mifc_capi_ensemble.hip", "mifc_capi_quantile.hip"):
        assert "note_ensemble_form(" in open(os.path.join(csrc, name)).read(), name
