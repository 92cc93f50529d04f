"""Loads the committed golden vectors (tests/golden/*.npz, produced from the real
reference by tests/golden/make_golden.py) and pairs them with the seeded cases."""
import hashlib
import os

import numpy as np

import cases

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

GOLDEN_STENCIL_GRIDS = [(3, 3), (5, 4), (17, 9), (64, 48), (260, 11)]
GOLDEN_EWISE_GRIDS = [(1, 1), (5, 4), (17, 9)]
GOLDEN_CATALOGUE_GRIDS = [(5, 4), (17, 9)]
GOLDEN_ENSEMBLE_GRIDS = [(5, 4), (17, 9)]


def input_digest(case):
    h = hashlib.sha256()
    def feed(a):
        if isinstance(a, np.ndarray):
            h.update(np.ascontiguousarray(a, dtype=np.float32).tobytes())
        elif isinstance(a, (list, tuple)):  # table of member fields, per-member flags, limits
            h.update(b"[%d]" % len(a))
            for x in a:
                feed(x)
        else:
            h.update(repr(a).encode())

    for a in case["args"]:
        feed(a)
    h.update(repr((case["nx"], case["ny"], case["fdefined"], float(case["undef"]))).encode())
    return h.hexdigest()


class Golden:
    def __init__(self, fname):
        self.z = np.load(os.path.join(GOLDEN, fname), allow_pickle=False)
        self.labels = set(str(x) for x in self.z["labels"])

    def expect(self, case):
        """-> (ok, flag, [outputs]) recorded from the reference for this case."""
        lab = case["label"]
        ok, flag, n_out = (int(x) for x in self.z[lab + "/meta"])
        digest = bytes(self.z[lab + "/digest"]).hex()
        assert digest == input_digest(case), "input generator drifted for %s: regenerate tests/golden" % lab
        outs = [self.z["%s/out%d" % (lab, k)] for k in range(n_out)] if ok else []
        return bool(ok), flag, outs


def output_digest(a):
    """SHA-256 of an output field with every NaN made the same NaN: equal digests = cases.same_bits(nan_payload=False)."""
    a = np.array(a, dtype=np.float32)
    a[np.isnan(a)] = np.float32("nan")
    return hashlib.sha256(a.tobytes()).digest()


def headline_level_cases():
    """One full 1440x720 level of the headline configuration, all-defined and with undefined cells."""
    import mi_fieldcalc_amd.synth as synth

    nx, ny = 1440, 720
    xm, ym, fc = synth.grid_maps(nx, ny)
    u, v = synth.wind(nx, ny, 0x5EED0000 + 3000)
    out = []
    for mode in ("all", "some"):
        (u_, v_), flag = cases._apply_mode([u, v], mode, 99, 0.01)
        for op in ("relvort", "divergence"):
            out.append(dict(op=op, nx=nx, ny=ny, args=[u_, v_, xm, ym], fdefined=flag, undef=cases.UNDEF, label="%s-1440x720-%s" % (op, mode)))
    return out


# The whole seeded sweep of tests/cases.py as the compiled reference answers it, recorded by make_golden.py as digests
# (reference_sweep_digests.npz): what test_oracle_vs_ref.py compares the restatement with where oracle/_ref is not built.
SWEEP_FAMILIES = {
    "stencil": cases.stencil_cases,
    "fused2": cases.fused2_cases,
    "ewise": cases.ewise_cases,
    "catalogue": cases.catalogue_cases,
    "ensemble": cases.ensemble_cases,
    "headline": headline_level_cases,
}


def sweep_cases(family):
    cs = SWEEP_FAMILIES[family]()
    if family == "stencil":  # the reference has no guard there (UB); the restatement returns false
        cs = [c for c in cs if not (c["op"] == "plevelgwind_ycomp" and (c["nx"] < 3 or c["ny"] < 3))]
    return cs


class RecordedSweep:
    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "reference_sweep_digests.npz"), allow_pickle=False)
        self.kind = str(self.z["kind"])

    def cases(self, family):
        """-> [(case, (ok, flag, [output digests]))] recorded from the reference for every case of the family."""
        cs = sweep_cases(family)
        labels, meta, din, dout = (self.z["%s/%s" % (family, k)] for k in ("labels", "meta", "in", "out"))
        assert [c["label"] for c in cs] == [str(x) for x in labels], "case list of %s drifted: regenerate tests/golden" % family
        out = []
        for k, case in enumerate(cs):
            assert bytes(din[k]).hex() == input_digest(case), "input generator drifted for %s: regenerate tests/golden" % case["label"]
            ok, flag, n_out = (int(x) for x in meta[k])
            out.append((case, (bool(ok), flag, [bytes(d) for d in dout[k][:n_out]] if ok else [])))
        return out


def reference_symbols():
    """The miutil:: functions the compiled reference exports (mangled), recorded by make_golden.py."""
    with open(os.path.join(GOLDEN, "reference_symbols.txt")) as f:
        return [ln.strip() for ln in f if ln.strip()]


def stencil_golden_cases():
    g = Golden("stencil_golden.npz")
    return g, [c for c in cases.stencil_cases(grids=GOLDEN_STENCIL_GRIDS) if c["label"] in g.labels]


def ewise_golden_cases():
    g = Golden("ewise_golden.npz")
    return g, [c for c in cases.ewise_cases(grids=GOLDEN_EWISE_GRIDS) if c["label"] in g.labels]


def catalogue_golden_cases():
    g = Golden("catalogue_golden.npz")
    return g, [c for c in cases.catalogue_cases(grids=GOLDEN_CATALOGUE_GRIDS) if c["label"] in g.labels]


def ensemble_golden_cases():
    g = Golden("ensemble_golden.npz")
    return g, [c for c in cases.ensemble_cases(grids=GOLDEN_ENSEMBLE_GRIDS) if c["label"] in g.labels]
