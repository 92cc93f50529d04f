"""The two drop-in layers an existing caller of the reference links or imports, operator by operator:

* the C++ API (mi-fieldcalc_amd/src/FieldCalculations.cc), reached through oracle/libmifc_dropin.so -- the reference
  shim's flat wrappers compiled against the product's headers -- and
* the Python module mi_fieldcalc.py,

against the CPU restatement on the seeded cases of tests/cases.py, judged like test_gpu_parity._check_case (equal
return value and flag; values bit-identical, or 1e-5 relative for the operators with a per-cell device powf).

Every forwarder reorders arguments by hand, so the cases have to notice a transposed pair: the CPU part of this module
checks, with the restatement alone, that swapping any two field arguments (or two scalars) of an operator changes its
result, and checks that without a device every wrapper refuses and writes nothing."""
import itertools

import numpy as np
import pytest

import cases
import cpulib
import gpu_util
import icing_cases as ic

ALL, NONE, SOME = cases.ALL_DEFINED, cases.NONE_DEFINED, cases.SOME_DEFINED

FAMILIES = {
    "stencil": lambda: cases.stencil_cases(grids=[(3, 3), (5, 4), (64, 48), (260, 11)]),
    "fused2": cases.fused2_cases,
    "ewise": lambda: cases.ewise_cases(grids=[(1, 1), (17, 9), (129, 3)]),
    "catalogue": lambda: cases.catalogue_cases(grids=[(1, 1), (17, 9), (129, 3)]) + cases.order_cases(),
    "ensemble": lambda: cases.ensemble_cases(grids=((5, 4), (17, 9))),
}
# the same generators on the one grid of the argument-order check
ORDER_GRID = (17, 9)
ORDER_FAMILIES = {
    "stencil": lambda modes: cases.stencil_cases(grids=[ORDER_GRID], modes=modes),
    "ewise": lambda modes: cases.ewise_cases(grids=[ORDER_GRID], modes=modes),
    "catalogue": lambda modes: cases.catalogue_cases(grids=[ORDER_GRID], modes=modes) + cases.order_cases(grids=(ORDER_GRID,), modes=modes),
    "ensemble": lambda modes: cases.ensemble_cases(grids=(ORDER_GRID,), modes=modes),
}

# Operators that are symmetric in their fields by definition: no generator can make a swap show.
SYMMETRIC_OPS = {"minvalueFields", "maxvalueFields", "sumFields", "meanValue", "stddevValue", "extremeValue", "probability"}
ORDERED_COMPUTES = {"fieldOPERfield": (2, 4)}  # + and x are symmetric; every - and / case must notice
# Single pairs of an otherwise order-sensitive operator that enter it only through an expression that commutes bit for
# bit in IEEE arithmetic (argument positions in reference order).  A transposition of such a pair in a forwarder is no
# error: the result is the same for every input.  The check below also fails when a pair listed here does change a
# result, so the list cannot hide a pair that matters.
COMMUTING_PAIRS = {
    ("vectorabs", 0, 1): "sqrt(u*u + v*v)",
    ("windCooling", 1, 2): "u, v only as the speed sqrt(u*u + v*v)",
    ("vesselIcingOverland", 2, 3): "u, v only as the speed sqrt(u*u + v*v)",
    ("vesselIcingMertins", 2, 3): "u, v only as the speed sqrt(u*u + v*v)",
    ("snow_in_cm", 1, 2): "tk2m, td2m only as the mean (tk2m + td2m) / 2",
}


def _positions(op, kind):
    """Indices into case["args"] of the operator's arguments of one SIGS kind ('p' fields, 'f' float scalars)."""
    sig = cpulib.SIGS[op]
    k = 1 if sig.startswith("C") else 0
    pos = []
    for c in sig.lstrip("C"):
        if c in "on":
            continue
        if c == kind:
            pos.append(k)
        k += 1
    return pos


def _result(lib, case):
    ok, out, flag = cases.run_cpu(lib, case)
    outs = out if isinstance(out, tuple) else (out,)
    return ok, flag, tuple(o.tobytes() for o in outs)


def _swapped(case, a, b):
    args = list(case["args"])
    args[a], args[b] = args[b], args[a]
    return dict(case, args=args)


def _order_failures(oracle):
    """-> list of messages: pairs of arguments whose transposition the seeded cases would not notice."""
    def by_op(modes):
        d = {}
        for fam in ORDER_FAMILIES.values():
            for case in fam(modes):
                if (case["nx"], case["ny"]) == ORDER_GRID:  # the generators append their argument-validation cases on other grids
                    d.setdefault(case["op"], []).append(case)
        return d

    some_of, all_of = by_op(("some",)), by_op(cases.MODES)
    failures = []
    for op in sorted(cpulib.SIGS):
        some, mine = some_of.get(op, []), all_of.get(op, [])
        if not some:
            failures.append("%s: no %dx%d 'some' case" % ((op,) + ORDER_GRID))
            continue
        for kind in "pf":
            for a, b in itertools.combinations(_positions(op, kind), 2):
                if kind == "p" and op in SYMMETRIC_OPS:
                    continue
                pool = some
                if kind == "p" and op in ORDERED_COMPUTES:
                    pool = [c for c in some if c["args"][0] in ORDERED_COMPUTES[op]]
                base = {id(c): _result(oracle, c) for c in pool}
                if (op, a, b) in COMMUTING_PAIRS:
                    moved = [c["label"] for c in mine if _result(oracle, _swapped(c, a, b)) != _result(oracle, c)]
                    if moved:
                        failures.append("%s args %d/%d are listed as commuting but change %s" % (op, a, b, moved[:3]))
                    continue
                if op in ORDERED_COMPUTES and kind == "p":
                    blind = [c["label"] for c in pool if _result(oracle, _swapped(c, a, b)) == base[id(c)]]
                    if blind or not pool:
                        failures.append("%s args %d/%d: swap unnoticed by %s" % (op, a, b, blind[:3]))
                    continue
                if not any(_result(oracle, _swapped(c, a, b)) != base[id(c)] for c in pool):
                    failures.append("%s args %d/%d (%s): no 'some' case notices the swap" % (op, a, b, "fields" if kind == "p" else "scalars"))
    return failures


@pytest.fixture(scope="module")
def order_checked(oracle):
    return _order_failures(oracle)


def test_seeded_cases_notice_transposed_arguments(order_checked):
    """CPU, restatement only: for every operator, swapping any two field arguments -- and any two float scalars
    (p500 / p700 / p850, alevel / blevel, p1 / p2, precipMin / snowRateMax / tcMax ...) -- of its 17x9 'some' cases
    changes the return value, the flag or the output bits of at least one of them."""
    assert not order_checked, "\n".join(order_checked)


def _one_case_per_operator():
    grid = [(5, 4)]
    pool = (cases.stencil_cases(grids=grid, modes=("some",)) + cases.ewise_cases(grids=grid, modes=("some",)) +
            cases.catalogue_cases(grids=grid, modes=("some",)) + cases.ensemble_cases(grids=(grid[0],), modes=("some",)))
    picked = {}
    for case in pool:
        if (case["nx"], case["ny"]) == grid[0] and "-some" in case["label"]:
            picked.setdefault(case["op"], case)
    return picked


def test_no_silent_cpu_fallback_through_the_cxx_layer():
    """Without a usable device every wrapper over the C++ API returns 0, leaves the outputs as they were bit for bit
    and the flag as passed: the layer callers link refuses, it does not compute on the CPU."""
    import mi_fieldcalc_amd._capi as capi

    if capi.lib().mifc_device_count() > 0:
        pytest.skip("GPU present")
    dropin = cpulib.CpuLib("dropin")
    assert dropin.kind.startswith("dropin ")
    picked = _one_case_per_operator()
    assert set(picked) == set(cpulib.SIGS)
    fill = np.float32(-7777.0)
    for op, case in sorted(picked.items()):
        ok, out, flag = cases.run_cpu(dropin, case, prefill=fill)
        assert not ok, op
        assert flag == case["fdefined"], op
        for o in (out if isinstance(out, tuple) else (out,)):
            assert cases.same_bits(o, np.full_like(o, fill)), op
    assert "no context" in dropin.last_error()


# ------------------------------------------------------------------ the C++ API on the GPU
def _judge(lib, oracle, case, expected=None):
    """test_gpu_parity._check_case with the C++ layer in the place of the C ABI."""
    ok_e, out_e, flag_e = expected if expected is not None else cases.run_cpu(oracle, case)
    ok, out, flag = cases.run_cpu(lib, case)
    assert ok == ok_e, case["label"]
    if not ok_e:
        return
    exact = not gpu_util.uses_device_powf(case)
    outs = list(out) if isinstance(out, tuple) else [out]
    outs_e = list(out_e) if isinstance(out_e, tuple) else [out_e]
    for a, b in zip(outs, outs_e):
        gpu_util.compare(case, np.asarray(a), np.asarray(b), exact)
    assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)


class _Runs:
    """Each family through the drop-in once per module; the operator names that ran are kept for the coverage check."""

    def __init__(self, dropin, oracle):
        self.dropin, self.oracle, self.ops = dropin, oracle, {}

    def run(self, family):
        if family not in self.ops:
            ran = set()
            for case in FAMILIES[family]():
                _judge(self.dropin, self.oracle, case)
                ran.add(case["op"])
            self.ops[family] = ran
        return self.ops[family]


@pytest.fixture(scope="module")
def dropin(gpu_ctx):
    lib = cpulib.CpuLib("dropin")
    assert lib.kind.startswith("dropin "), lib.kind
    return lib


@pytest.fixture(scope="module")
def runs(dropin, oracle):
    return _Runs(dropin, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_cxx_api_matches_the_restatement(runs, order_checked, family):
    assert not order_checked, "the cases would not notice a transposed pair:\n" + "\n".join(order_checked)
    assert runs.run(family)


@pytest.mark.gpu
def test_every_wrapper_was_exercised(runs):
    """All of cpulib.SIGS, over the families: a wrapper added to the shim cannot go untested unnoticed."""
    ran = set()
    for family in FAMILIES:
        ran |= runs.run(family)
    assert ran == set(cpulib.SIGS), (sorted(set(cpulib.SIGS) - ran), sorted(ran - set(cpulib.SIGS)))


def _in_place(lib, case):
    """The case with the output aliasing its first field argument (member 0 of a table); the array is a copy."""
    op = case["op"]
    args = list(case["args"])
    sig = cpulib.SIGS[op]
    if "T" in sig:
        k = 1 if sig.startswith("C") else 0
        target = np.array(args[k][0], dtype=np.float32, order="C")
        args[k] = [target] + list(args[k][1:])
    else:
        k = _positions(op, "p")[0]
        target = np.array(args[k], dtype=np.float32, order="C")
        args[k] = target
    ok, out, flag = lib.call(op, case["nx"], case["ny"], *args, fdefined=case["fdefined"], undef=case["undef"], outs=[target])
    assert out is target
    return ok, out, flag


REDUCTIONS = ("sumFields", "meanValue", "stddevValue", "extremeValue", "probability")


@pytest.mark.gpu
@pytest.mark.parametrize("family", ("ewise", "catalogue") + REDUCTIONS)
def test_cxx_api_in_place(dropin, oracle, family):
    """Callers run the reference's pointwise operators with the output aliasing an input: out = the first field here,
    against the restatement run in place the same way.  For the reductions over members, out = member 0.

    The reference accumulates in the output, cell by cell (fres[i] = 0, then += every member; extremeValue starts from
    undef), so with out = member 0 it reads its own running result where member 0 was: sumFields then returns the sum of
    members 1..n-1, and the compiled reference and the restatement agree on that bit for bit.  The product has to as well
    (mifc_ensemble.hip, ens_aliased).  stddevValue reads every member before it writes."""
    grids = [(17, 9), (129, 3)]
    modes = ("all", "some")
    if family == "ewise":
        cs = cases.ewise_cases(grids=grids, modes=modes)
    elif family == "catalogue":
        cs = cases.catalogue_cases(grids=grids, modes=modes)
    else:
        cs = [c for c in cases.ensemble_cases(grids=tuple(grids), modes=modes) if c["op"] == family]
    ran = set()
    for case in cs:
        assert cases.N_OUT.get(case["op"], 1) == 1
        _judge_in_place(dropin, oracle, case)
        ran.add(case["op"])
    assert len(ran) >= {"ewise": 8, "catalogue": 38}.get(family, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("op", REDUCTIONS)
def test_reductions_in_place_device_resident(gpu_ctx, oracle, op):
    """The same with the members resident on the device and out = member 0's tensor, through the C ABI."""
    import torch

    for case in cases.ensemble_cases(grids=((17, 9), (129, 3)), modes=("all", "some")):
        if case["op"] != op:
            continue
        ok_e, out_e, flag_e = _in_place(oracle, case)
        args = list(case["args"])
        k = 1 if cpulib.SIGS[op].startswith("C") else 0
        members = [torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)).cuda() for m in args[k]]
        args[k] = members
        res = getattr(gpu_ctx, op)(*args, fdefined=case["fdefined"], undef=case["undef"], out=members[0])
        assert (res is not None) == ok_e, case["label"]
        if not ok_e:
            continue
        out, flag = res
        assert out.data_ptr() == members[0].data_ptr()
        gpu_util.compare(case, out.cpu().numpy(), out_e, True)
        assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)


def _judge_in_place(lib, oracle, case):
    ok_e, out_e, flag_e = _in_place(oracle, case)
    ok, out, flag = _in_place(lib, case)
    assert ok == ok_e, case["label"]
    if not ok_e:
        return
    gpu_util.compare(case, out, out_e, not gpu_util.uses_device_powf(case))
    assert flag == flag_e, "%s: flag %d vs %d" % (case["label"], flag, flag_e)


@pytest.mark.gpu
def test_last_error_after_a_refused_call(dropin):
    """Empty after an argument refusal, names the function after one that is not built (as
    test_capi_and_host.test_cxx_header_is_source_compatible pins for a compiled caller)."""
    import mi_fieldcalc_amd.synth as synth

    xm, ym, _ = synth.grid_maps(5, 4)
    z = synth.scalar_field(5, 4, 3)
    ok, out, flag = dropin.neighbourFunctions(5, 4, z, [1.0, 2.0], 1)
    assert not ok and "neighbourFunctions: not built on the GPU" in dropin.last_error()
    assert cases.same_bits(out, np.full_like(out, np.float32(-7777.0))) and flag == SOME
    ok, _, _ = dropin.call("gradient", 5, 4, z, xm, ym, 5)  # bad compute
    assert not ok and dropin.last_error() == ""
    ok, _, _ = dropin.neighbourFunctions(5, 4, z, [1.0, 2.0], 1)
    assert not ok and dropin.last_error() != ""
    ok, _, _ = dropin.call("gradient", 5, 4, z, xm, ym, 1)  # a call that succeeds clears it, too
    assert ok and dropin.last_error() == ""


@pytest.mark.gpu
def test_cxx_api_matches_the_compiled_reference(dropin, ref):
    """Stencil and ensemble families once more with the real reference in the place of the restatement."""
    n = 0
    for case in cases.stencil_cases(grids=[ORDER_GRID]) + cases.ensemble_cases(grids=(ORDER_GRID,)):
        _judge(dropin, None, case, expected=cases.run_cpu(ref, case))
        n += 1
    assert n > 200


# ------------------------------------------------------------------ the Python module
PY_FUNCTIONS = ("kIndex", "ductingIndex", "showalterIndex", "boydenIndex", "sweatIndex", "seaSoundSpeed", "cvtemp", "cvhum", "abshum", "windCooling",
                "underCooledRain", "vesselIcingOverland", "vesselIcingMertins")


def _python_cases():
    modes = ("all", "some")
    pool = cases.catalogue_cases(grids=[ORDER_GRID], modes=modes) + cases.order_cases(grids=(ORDER_GRID,), modes=modes)
    pool += [c for c in cases.ewise_cases(grids=[ORDER_GRID], modes=modes) if c["op"] == "cvhum"]  # cvhum's generator is the elementwise one
    return [c for c in pool if c["op"] in PY_FUNCTIONS]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_python_module_matches_the_restatement(gpu_ctx, oracle, order_checked, dtype):
    """mi_fieldcalc.<name>(*args, undef) in the reference module's positional order, every compute variant the
    generators have: float32 (ny, nx) result, None exactly where the operator returns false.  The module runs every
    operator with SOME_DEFINED (py_mi_fieldcalc.cc:89), so does the restatement here."""
    import mi_fieldcalc as pyfc

    assert not order_checked, "\n".join(order_checked)
    ran = set()
    for case in _python_cases():
        case = dict(case, fdefined=SOME)
        ok_e, out_e, _ = cases.run_cpu(oracle, case)
        # cells the operator never writes (showalterIndex outside its table, ...) hold whatever the fresh result array
        # held, in the reference module as well: found with a second prefill, and left out of the comparison
        _, other, _ = cases.run_cpu(oracle, case, prefill=np.float32(12345.5))
        unwritten = (out_e.view(np.uint32) != other.view(np.uint32)) if ok_e else None
        args = [np.asarray(a, dtype=dtype).reshape(case["ny"], case["nx"]) if isinstance(a, np.ndarray) else a for a in case["args"]]
        got = getattr(pyfc, case["op"])(*args, float(case["undef"]))
        if not ok_e:
            assert got is None, case["label"]
            continue
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (case["ny"], case["nx"]), case["label"]
        gpu_util.compare(case, np.where(unwritten, out_e, got), out_e, not gpu_util.uses_device_powf(case))
        ran.add(case["op"])
    assert ran == set(PY_FUNCTIONS), sorted(set(PY_FUNCTIONS) - ran)


@pytest.mark.gpu
def test_python_module_vessel_icing(gpu_ctx, tmp_path_factory):
    """vesselIcingModStall through the module: eleven distinct fields and four scalars in the reference's order, against
    the host build of the per-cell model (the reference bit for bit, test_vessel_icing_cpu.py), under the accuracy contract
    of icing_cases.  vesselIcingMincog stays unwired."""
    import mi_fieldcalc as pyfc

    cell = ic.CellShim(tmp_path_factory.mktemp("iccell_dropin"))
    fields = ic.make_inputs(129, 40, 12, specials=True)
    vs, alpha, zmin, zmax = 4.0, 0.6, 1.0, 9.0  # four different numbers
    st, _, expect = cell.run(ic.MODSTALL, fields, vs, alpha, zmin, zmax, fdefined=ic.SOME_DEFINED)
    assert st == 1
    for dtype in (np.float32, np.float64):
        got = pyfc.vesselIcingModStall(*[f.astype(dtype) for f in fields], vs, alpha, zmin, zmax, float(ic.UNDEF))
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (40, 129)
        placed, frac, excess, ndef = ic.contract(got, expect)
        assert placed and frac >= 0.999 and excess <= 0 and ndef > 3000, (placed, frac, excess, ndef)
    with pytest.raises(NotImplementedError):
        pyfc.vesselIcingMincog(*fields, vs, alpha, zmin, zmax, 1, float(ic.UNDEF))
