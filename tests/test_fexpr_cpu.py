"""CPU checks of mifc_fexpr_levels: that the entry, its enum and its configuration are declared, bound and mirrored where
the others are; the program check (csrc/mifc_fexpr_prog.h) compiled with the host compiler -- through a shim and, under
the address and undefined-behaviour sanitizers, as a stand-alone program --; the expression compiler of the front; the
undefined rule of every operation on hand-worked cells of the numpy restatement (tests/fexpr_restate.py, the oracle of the
GPU tests); the front's marshalling against a recording stub library; that the fuzz cases the GPU tests run are fit for
purpose; and that no kernel of csrc/mifc_fexpr.hip uses scratch."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fexpr_restate as fr
import test_python_front_cpu as front
from mi_fieldcalc_amd import fexpr as fexpr_module  # (without the feature the file fails here)
from test_python_front_cpu import _data, _stub_context

F = np.float32
U = fr.UNDEF
NAN, INF = F(np.nan), F(np.inf)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mi-fieldcalc_amd", "csrc")
A, S_, N = fr.ALL_DEFINED, fr.SOME_DEFINED, fr.NONE_DEFINED
L, C = fr.LEVEL, fr.CONST
# the host tables of mifc_fexpr_levels for the recording stub: positions after the context
front.SPEC.setdefault("mifc_fexpr_levels", [(3, "ptr", front._at(4)), (5, "ptr", front._at(6)), (15, "ptr", front._at(14))])


def bits(x):
    return np.asarray(x, F).view(np.uint32).tolist()


# ------------------------------------------------------------------------------- declared, bound and configured
def test_entry_is_declared_bound_and_configured():
    import mi_fieldcalc_amd._capi as capi
    import mi_fieldcalc_amd._consts as consts

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mifc.h")).read(), flags=re.S)
    names = ("mifc_fexpr_levels", "mifc_last_fexpr_form")
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
    assert [len(capi.SIGNATURES[n][1]) for n in names] == [20, 0]
    assert capi.SIGNATURES["mifc_fexpr_levels"][1][14] == "pi" and capi.SIGNATURES["mifc_fexpr_levels"][1][18] == "f"
    # the enum, mirrored by name and value, in order and without holes
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"MIFC_FEXPR_([A-Z0-9_]+) = (\d+)", header))
    nops = enum.pop("nops")
    limits = {k: enum.pop(k) for k in ("nregs", "max_fields", "max_planes", "max_inputs", "max_scalars", "max_consts", "max_code", "max_out")}
    assert enum == consts.FEXPR_OPS and sorted(enum.values()) == list(range(nops)) and tuple(sorted(enum, key=enum.get)) == fr.OPS
    assert limits == {"nregs": 16, "max_fields": 8, "max_planes": 4, "max_inputs": 12, "max_scalars": 4, "max_consts": 16, "max_code": 64, "max_out": 4}
    assert consts.FEXPR_LIMITS == {"nregs": 16, "fields": 8, "planes": 4, "inputs": 12, "scalars": 4, "consts": 16, "code": 64, "out": 4}
    assert re.search(r"#define MIFC_FEXPR_LEVEL\(s\) \(16 \+ \(s\)\)", header) and re.search(r"#define MIFC_FEXPR_CONST\(j\) \(32 \+ \(j\)\)", header)
    assert (consts.FEXPR_LEVEL0, consts.FEXPR_CONST0) == (16, 32) == (fr.LEVEL0, fr.CONST0)
    assert re.search(r"typedef struct \{ unsigned char op, dst, a, b, c, pad\[3\]; \} mifc_fexpr_ins;", header)
    # the chunk variable is read in one place, the host file takes it from the snapshot
    readers = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if '"MIFC_FEXPR_CHUNK_MIB"' in open(p, errors="replace").read()]
    assert readers == ["mifc_env.hip"], readers
    host = open(os.path.join(CSRC, "mifc_capi_fexpr.hip")).read()
    assert "getenv" not in host and re.search(r"fexpr_chunk_mib > 0 \? mifc::env\(\)\.fexpr_chunk_mib : 256", host)
    makefile = open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read()
    assert makefile.count("mifc_fexpr.hip") == 1 and makefile.count("mifc_capi_fexpr.hip") == 2  # KERNELS; KERNELS and MEASURE_SRC
    assert makefile.count("mifc_fexpr_prog.h") == 1  # HDRS
    prog_header = open(os.path.join(CSRC, "mifc_fexpr_prog.h")).read()
    assert "hip" not in re.sub(r"//.*", "", prog_header).lower()  # free of device code: the host compiler builds it


# ------------------------------------------------------------------------ the program check through the host compiler
def _cxx():
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    return cxx


BASE = dict(nfields=2, nplanes=1, nscalars=1, nconsts=1, code=[("add", 3, 0, 1)], out_regs=[3])


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fexpr") / "libfexpr_prog_shim.so")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "fexpr_prog_shim.cc"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.mifc_test_fexpr_check.restype = ctypes.c_int

    def run(ncode=None, nout=None, null_code=False, null_out=False, **over):
        k = dict(BASE, **over)
        rows = np.zeros((max(len(k["code"]), 1), 8), np.uint8)
        for i, ins in enumerate(k["code"]):
            ins = list(ins)
            rows[i, : len(ins)] = [fr.OP[ins[0]] if isinstance(ins[0], str) else ins[0]] + ins[1:]
        regs = np.array(k["out_regs"] or [0], np.int32)
        info, norm, why = np.zeros(2, np.int32), np.zeros_like(rows), ctypes.create_string_buffer(128)
        ok = lib.mifc_test_fexpr_check(k["nfields"], k["nplanes"], k["nscalars"], k["nconsts"], None if null_code else rows.ctypes.data_as(ctypes.c_void_p),
                                       len(k["code"]) if ncode is None else ncode, None if null_out else regs.ctypes.data_as(ctypes.c_void_p),
                                       len(k["out_regs"]) if nout is None else nout, info.ctypes.data_as(ctypes.c_void_p),
                                       norm.ctypes.data_as(ctypes.c_void_p), why, 128)
        return ok, why.value.decode(), int(info[0]), int(info[1]), norm

    return run


REFUSALS = [
    (dict(nfields=9), "nfields 9 outside"), (dict(nfields=-1), "nfields -1 outside"), (dict(nplanes=5), "nplanes 5 outside"),
    (dict(nfields=0, nplanes=0), "nfields + nplanes 0 outside"), (dict(nscalars=5), "nscalars 5 outside"), (dict(nconsts=17), "nconsts 17 outside"),
    (dict(ncode=0), "ncode 0 outside"), (dict(ncode=65), "ncode 65 outside"), (dict(nout=0), "nout 0 outside"), (dict(nout=5), "nout 5 outside"),
    (dict(null_code=True), "null pointer"), (dict(null_out=True), "null pointer"),
    (dict(code=[(22, 3, 0, 1)]), "unknown op 22"), (dict(code=[("add", 16, 0, 1)]), "dst 16 is no register"),
    (dict(code=[("add", 3, 0, 20)]), "operand byte 20"), (dict(code=[("add", 3, 0, 200)]), "operand byte 200"),
    (dict(code=[("add", 3, 0, L(1))]), "level scalar 1 out of range"), (dict(code=[("add", 3, C(1), 1)]), "constant 1 out of range"),
    (dict(code=[("add", 3, 0, 5)]), "register 5 is read before"), (dict(code=[("select", 3, 0, 1, 9)]), "register 9 is read before"),
    (dict(code=[("mask", 3, 0, 200, 9)]), "register 9 is read before"),
    (dict(out_regs=[7]), "out_regs[0]: register 7 is read before"), (dict(out_regs=[16]), "out_regs[0] = 16 is no register"),
    (dict(out_regs=[-1]), "out_regs[0] = -1 is no register"),
]


@pytest.mark.parametrize("over,reason", REFUSALS, ids=[r for _, r in REFUSALS])
def test_program_check_refuses(check, over, reason):
    ok, why, _, _, _ = check(**over)
    assert ok == 0 and reason in why, why


def test_program_check_accepts_and_normalises(check):
    assert check()[:4] == (1, "", 4, 0)
    # the bytes an operation does not read are ignored, and come back as `a`
    ok, why, nregs, tables, norm = check(code=[("abs", 3, 1, 200, 77), ("mask", 4, 3, 201, L(0)), ("pow", 5, 4, C(0), 99)], out_regs=[5])
    assert (ok, why, nregs, tables) == (1, "", 6, 1)
    assert norm[:, :5].tolist() == [[fr.OP["abs"], 3, 1, 1, 1], [fr.OP["mask"], 4, 3, 3, L(0)], [fr.OP["pow"], 5, 4, C(0), 4]]
    # the limits: 12 inputs, 16 registers, 64 instructions, 4 outputs, every operand kind at its last index
    code = [(i % len(fr.OPS), 12 + i % 4, i % 12, L(3) if i % 2 else C(15), 11) for i in range(64)]
    assert check(nfields=8, nplanes=4, nscalars=4, nconsts=16, code=code, out_regs=[12, 13, 14, 15])[:4] == (1, "", 16, 1)
    assert check(nfields=8, nplanes=4, code=code[:1] + [("mov", 15, 12)], out_regs=[15], nscalars=0, nconsts=16)[0] == 1
    # a register set by an earlier instruction may be read; an input may be overwritten and read again
    assert check(code=[("add", 0, 0, 1), ("mul", 9, 0, 0), ("mov", 1, 9)], out_regs=[1, 0, 9])[:3] == (1, "", 10)


def test_program_check_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "fexpr_prog_asan")
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-static-libubsan", "-I", CSRC, os.path.join(ROOT, "tests", "host", "fexpr_prog_main.cc"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)  # (the environment as it is: the runtimes are linked in)
    assert run.returncode == 0 and "28 cases, 0 failures" in run.stdout, run.stdout + run.stderr


# ----------------------------------------------------------------------------------------------------- the compiler
def test_compiler_counts_shares_and_maps():
    fx = fexpr_module
    p = fx.compile("t*(1+0.608*q)", fields=("t", "q"))
    assert p.ncode == 3 and bits(p.consts) == bits([1.0, 0.608]) and p.nout == 1 and (p.nfields, p.nplanes, p.nscalars) == (2, 0, 0)
    assert [i[0] for i in p.instructions()] == ["mul", "add", "mul"] and p.nregs == 2  # the inputs' registers are reused
    # a repeated subexpression appears once, whatever the spelling of its blanks; constants are deduplicated, never folded
    p = fx.compile("(t+q)*(t + q) + 2*3 + 2", fields=("t", "q"))
    assert [i[0] for i in p.instructions()].count("add") == 3 and p.ncode == 5 and bits(p.consts) == bits([2.0, 3.0])
    # > is < with the sides swapped, >= is <=, != is ne; where(c, a, b) puts c last
    ins = fx.compile("t > q", fields=("t", "q")).instructions()
    assert ins == [("lt", ins[0][1], 1, 0, None)]
    ins = fx.compile("t >= q", fields=("t", "q")).instructions()
    assert ins == [("le", ins[0][1], 1, 0, None)]
    assert fx.compile("t != q", fields=("t", "q")).instructions()[0][:1] == ("ne",) and fx.compile("t == 1", fields=("t",)).instructions()[0][0] == "eq"
    ins = fx.compile("where(c < 0, t, -t)", fields=("t",), planes=("c",)).instructions()
    assert [i[0] for i in ins] == ["neg", "lt", "select"] and ins[2][2:] == (0, ins[0][1], ins[1][1])
    ins = fx.compile("mask(t, p - 100), ifdef(t, 0) ** 2, -1.5", fields=("t",), level_scalars=("p",))
    assert [i[0] for i in ins.instructions()] == ["sub", "mask", "ifdef", "pow", "mov"] and ins.nout == 3 and bits(ins.consts) == bits([100, 0, 2, -1.5])
    assert ins.instructions()[0][2:4] == (fr.LEVEL(0), fr.CONST(0)) and len(set(ins.out_regs.tolist())) == 3
    # a tuple of strings is several outputs; an output that is a bare input is moved, so that there is an instruction
    p = fx.compile(("t", "min(t, q)"), fields=("t", "q"))
    assert [i[0] for i in p.instructions()] == ["min", "mov"] and p.nout == 2
    # every function
    p = fx.compile("max(abs(t), sqrt(q)) + log(t) + log10(t) + exp(t) + pow10(t)", fields=("t", "q"))
    assert sorted(i[0] for i in p.instructions()) == sorted(["max", "abs", "sqrt", "log", "log10", "exp", "pow10"] + ["add"] * 4)
    # Program.from_code takes names or numbers, and short rows
    q = fx.Program.from_code([("mul", 2, 0, 1), (fr.OP["mov"], 3, 2)], consts=[1.5], out_regs=[3], nfields=2)
    assert q.code.tolist() == [[2, 2, 0, 1, 0, 0, 0, 0], [21, 3, 2, 0, 0, 0, 0, 0]] and q.nregs == 4 and q.nfields == 2 and q.nout == 1


@pytest.mark.parametrize("expr,kw,reason", [
    ("t + zz", dict(fields=("t",)), "unknown name 'zz'"),
    ("sin(t)", dict(fields=("t",)), "unknown function 'sin'"),
    ("min(t)", dict(fields=("t",)), "min takes 2 arguments"),
    ("t if t else 1", dict(fields=("t",)), "not accepted"),
    ("t < 1 < 2", dict(fields=("t",)), "a comparison has two sides"),
    ("t +", dict(fields=("t",)), "not an expression"),
    ("t % 2", dict(fields=("t",)), "not accepted"),
    ("t, t, t, t, t", dict(fields=("t",)), "1..4 outputs"),
    ("t", dict(fields=()), "1..12 of both"),
    ("t", dict(fields=("t", "t")), "the name 't' is taken"),
    ("+".join("%d.5*t" % i for i in range(17)), dict(fields=("t",)), "more than 16 constants"),
    ("+".join("a%d*(a%d+%d)" % (i % 8, (i + 1) % 8, i % 9) for i in range(30)), dict(fields=tuple("a%d" % i for i in range(8))), "more than 64 instructions"),
], ids=lambda x: x if isinstance(x, str) and len(x) < 30 else None)
def test_compiler_errors(expr, kw, reason):
    with pytest.raises(ValueError, match=re.escape(reason)):
        fexpr_module.compile(expr, **kw)


def test_compiler_reuses_registers_and_runs_out_of_them():
    names = tuple("a%d" % i for i in range(8)) + tuple("p%d" % i for i in range(4))
    # twelve inputs, each read once: a product of twelve sums needs no register beyond the sixteen
    wide = " * ".join("(%s + %d.5)" % (n, i) for i, n in enumerate(names))
    assert fexpr_module.compile(wide, fields=names[:8], planes=names[8:]).nregs <= 16
    # three outputs stay alive, all twelve inputs are still to be read, and the fourth output holds two more values
    with pytest.raises(ValueError, match="more than 16 live registers"):
        fexpr_module.compile("(a0+1)*(a1+2), (a2+3)*(a3+4), (a4+5)*(a5+6), " + " + ".join("%s*%s" % (names[i], names[(i + 5) % 12]) for i in range(12)),
                             fields=names[:8], planes=names[8:])


def _special_fields(rng, n, shape=(2, 3, 7)):
    pool = np.array([U, NAN, 0.0, -0.0, INF, -INF, 1e-40, -3e-39, 1.5, -2.25, 3e30, 1e-3], F)
    return [rng.choice(pool, shape).astype(F) for _ in range(n)]


def test_compiled_programs_equal_the_expression_in_numpy():
    """A program compiled from a string and interpreted by the restatement equals the same expression written directly in
    numpy float32, operation by operation, on data with undef, NaN, +-0, +-inf and denormals."""
    rng = np.random.default_rng(7)
    t, q, s = _special_fields(rng, 3)
    u = F(U)

    def D(x):
        return fr.is_def(x, u)

    def op(f, *xs):  # the default rule: undef where an operand is undefined
        with np.errstate(all="ignore"):
            return np.where(np.logical_and.reduce([D(x) for x in xs]), f(*xs), u).astype(F)

    c1, c608, c2 = np.full(t.shape, F(1)), np.full(t.shape, F(0.608)), np.full(t.shape, F(2))
    # t * (1 + 0.608 * q)
    want = op(np.multiply, t, op(np.add, c1, op(np.multiply, c608, q)))
    p = fexpr_module.compile("t*(1+0.608*q)", fields=("t", "q"))
    got, fd = fr.interpret(p.code[:, :5], p.consts, p.out_regs, [t, q])
    assert bits(got[0]) == bits(want) and 0 < int((got[0] == u).sum()) < got[0].size and fd.tolist() == [[S_, S_]]
    # (t - s) / q, min and max, a comparison, where, ifdef
    p = fexpr_module.compile("(t - s) / q, max(min(t, q), s), where(t <= q, s, 2), ifdef(t, q)", fields=("t", "q", "s"))
    got, _ = fr.interpret(p.code[:, :5], p.consts, p.out_regs, [t, q, s])
    diff = op(np.subtract, t, s)
    with np.errstate(all="ignore"):
        want0 = np.where(D(diff) & D(q) & (q != 0), diff / q, u).astype(F)
        want1 = op(lambda a, b: np.where(a < b, b, a), op(lambda a, b: np.where(b < a, b, a), t, q), s)
        le = op(lambda a, b: (a <= b).astype(F), t, q)
        pick = np.where(le != 0, s, c2)
        want2 = np.where(D(le) & D(pick), pick, u).astype(F)
        want3 = np.where(D(t), t, q)
    for o, want in enumerate((want0, want1, want2, want3)):
        assert bits(got[o]) == bits(want), o


# ------------------------------------------------------------------------------------------------- hand-worked cells
def cell(code, values, consts=(), scalars=(), out=15, undef=U):
    """One cell, one level: the fields are the numbers `values`; (the value of register `out`, the flag)."""
    fields = [np.full((1, 1, 1), v, F) for v in values]
    got, fd = fr.interpret(code, consts, [out], fields, (), np.asarray(scalars, F).reshape(-1, 1), undef)
    return got[0, 0, 0, 0], int(fd[0, 0])


def same(got, value, flag):
    return bits(got[0]) == bits(value) and got[1] == flag


def test_hand_worked_undefined_rules():
    assert same(cell([("add", 15, 0, 1)], [1.5, 2.25]), 3.75, A)
    for name in ("add", "sub", "mul", "div", "min", "max", "pow", "lt", "le", "eq", "ne"):
        for values in ([U, 1.0], [1.0, U], [NAN, 1.0], [1.0, NAN]):
            assert same(cell([(name, 15, 0, 1)], values), U, N), (name, values)
    for name in ("abs", "neg", "sqrt", "log", "log10", "exp", "pow10", "mov"):
        assert same(cell([(name, 15, 0)], [U]), U, N) and same(cell([(name, 15, 0)], [NAN]), U, N), name
    # DIV by zero of either sign is undef; zero divided is zero
    assert same(cell([("div", 15, 0, 1)], [1.0, 0.0]), U, N) and same(cell([("div", 15, 0, 1)], [1.0, -0.0]), U, N)
    assert same(cell([("div", 15, 0, 1)], [0.0, 2.0]), 0.0, A) and same(cell([("div", 15, 0, 1)], [1.0, INF]), 0.0, A)
    # MIN and MAX in the operand order of the reference: equal operands give a, and so do zeros of either sign
    assert same(cell([("min", 15, 0, 1)], [0.0, -0.0]), 0.0, A) and same(cell([("min", 15, 0, 1)], [-0.0, 0.0]), -0.0, A)
    assert same(cell([("max", 15, 0, 1)], [-0.0, 0.0]), -0.0, A) and same(cell([("max", 15, 0, 1)], [1.0, 2.0]), 2.0, A)
    # the comparisons give 1.0 or 0.0; infinities are values
    assert same(cell([("lt", 15, 0, 1)], [1.0, INF]), 1.0, A) and same(cell([("le", 15, 0, 1)], [2.0, 1.0]), 0.0, A)
    assert same(cell([("eq", 15, 0, 1)], [0.0, -0.0]), 1.0, A) and same(cell([("ne", 15, 0, 1)], [0.0, -0.0]), 0.0, A)
    # SELECT reads the condition and the chosen operand only: the unchosen NaN or undef does not matter
    sel = [("select", 15, 0, 1, 2)]
    assert same(cell(sel, [7.0, NAN, 1.0]), 7.0, A) and same(cell(sel, [NAN, 8.0, 0.0]), 8.0, A) and same(cell(sel, [U, 8.0, -0.0]), 8.0, A)
    assert same(cell(sel, [NAN, 8.0, 1.0]), U, N) and same(cell(sel, [7.0, U, 0.0]), U, N)
    assert same(cell(sel, [7.0, 8.0, U]), U, N) and same(cell(sel, [7.0, 8.0, NAN]), U, N)
    # IFDEF: a where a is defined, else b as it is -- both undefined gives b, whichever kind of undefined that is
    ifd = [("ifdef", 15, 0, 1)]
    assert same(cell(ifd, [3.0, U]), 3.0, A) and same(cell(ifd, [U, 4.0]), 4.0, A) and same(cell(ifd, [NAN, 4.0]), 4.0, A)
    assert same(cell(ifd, [U, U]), U, N) and same(cell(ifd, [NAN, U]), U, N)
    got = cell(ifd, [U, NAN])
    assert np.isnan(got[0]) and got[1] == A  # a NaN is not counted
    # MASK: a as it is where c is defined and not zero
    msk = [("mask", 15, 0, 0, 1)]
    assert same(cell(msk, [5.0, 1.0]), 5.0, A) and same(cell(msk, [5.0, 0.0]), U, N) and same(cell(msk, [5.0, -0.0]), U, N)
    assert same(cell(msk, [5.0, U]), U, N) and same(cell(msk, [5.0, NAN]), U, N) and same(cell(msk, [U, 1.0]), U, N)
    assert np.isnan(cell(msk, [NAN, 2.0])[0])
    # a constant or a level scalar equal to undef is undefined like a cell
    assert same(cell([("add", 15, 0, C(0))], [1.0], consts=[U]), U, N) and same(cell([("mul", 15, 0, L(0))], [1.0], scalars=[U]), U, N)
    assert same(cell([("add", 15, 0, C(1))], [1.0], consts=[U, 2.0]), 3.0, A) and same(cell([("mov", 15, L(0))], [1.0], scalars=[-4.0]), -4.0, A)
    # an intermediate that computes to exactly undef is undefined for the next operation, as in a chain of calls
    assert same(cell([("mul", 3, 0, 1), ("add", 15, 3, 1)], [5.0e34, 2.0]), U, N)
    assert same(cell([("mul", 15, 0, 1)], [5.0e34, 2.0]), U, N)  # ... and counted where it is an output
    assert same(cell([("mul", 3, 0, 1), ("ifdef", 15, 3, 1)], [5.0e34, 2.0]), 2.0, A)
    # a NaN result is kept, and not counted; the next operation finds it undefined
    for code, values in (([("sub", 15, 0, 1)], [INF, INF]), ([("mul", 15, 0, 1)], [0.0, INF]), ([("sqrt", 15, 0)], [-1.0]), ([("log", 15, 0)], [-1.0])):
        got = cell(code, values)
        assert np.isnan(got[0]) and got[1] == A, code
    assert same(cell([("sqrt", 3, 0), ("add", 15, 3, 1)], [-1.0, 1.0]), U, N)
    # infinite results are values; a register may be overwritten, its input included, and read again
    assert same(cell([("div", 15, 0, 1)], [1.0, 1e-40]), INF, A) and same(cell([("exp", 15, 0)], [1000.0]), INF, A)
    assert same(cell([("add", 0, 0, 0), ("mul", 0, 0, 0), ("mov", 15, 0)], [1.5]), 9.0, A)
    # another undef value
    assert same(cell([("add", 15, 0, 1)], [-999.0, 1.0], undef=-999.0), -999.0, N) and same(cell([("add", 15, 0, 1)], [U, 1.0], undef=-999.0), U + F(1), A)
    # the transcendental functions are the float64 function rounded once
    assert same(cell([("pow", 15, 0, 1)], [2.0, 0.5]), F(np.sqrt(2.0)), A) and same(cell([("pow10", 15, 0)], [2.0]), 100.0, A)
    assert same(cell([("log10", 15, 0)], [1000.0]), 3.0, A) and same(cell([("log", 15, 0)], [0.0]), -INF, A)


def test_flags_per_output_and_level():
    f = np.array([[[1.0, U, 3.0]], [[U, U, U]], [[1.0, 2.0, NAN]]], F)  # (nlev 3, ny 1, nx 3)
    out, fd = fr.interpret([("mov", 4, 0), ("ifdef", 5, 0, C(0))], [0.0], [4, 5], [f])
    assert fd.tolist() == [[S_, N, S_], [A, A, A]] and bits(out[1][2]) == bits([[1.0, 2.0, 0.0]])  # MOV of a NaN is undef: the default rule
    # planes are shared by the levels, level scalars differ per level
    pl = np.array([[10.0, 20.0, U]], F)
    out, fd = fr.interpret([("add", 4, 0, 1), ("mul", 4, 4, L(0))], [], [4], [f], [pl], [[1.0, U, 2.0]])
    assert bits(out[0]) == bits([[[11.0, U, U]], [[U, U, U]], [[22.0, 44.0, U]]]) and fd.tolist() == [[S_, N, S_]]


# ------------------------------------------------------------------------------- the front against a recording stub
def _entry_calls(lib, name):
    return [a for n, a in lib.calls if n == name]


def test_front_marshals_tables_counts_and_outputs_in_header_order():
    fx = fexpr_module
    d = _data()
    ctx, lib = _stub_context(d)
    nlev, ny, nx = d["B"].shape
    level = nlev * ny * nx * 4
    prog = fx.compile("t*(1+0.608*q)", fields=("t", "q"))
    out, fd = fx.evaluate(ctx, prog, [d["T"], d["Q"]], undef=-5.0)
    a = _entry_calls(lib, "mifc_fexpr_levels")[-1]
    assert len(a) == 19 and a[:3] == [nx, ny, nlev] and a[3] == [["T", 0], ["Q", 0]] and a[4] == 2 and a[5] is None and a[6] == 0
    assert a[7] is None and a[8] == 0 and a[9]["numpy"] == "float32" and bits(a[9]["values"]) == bits([1.0, 0.608]) and a[10] == 2
    assert a[11]["numpy"] == "uint8" and a[11]["shape"] == [3, 8] and a[11]["values"] == prog.code.ravel().tolist() and a[12] == 3
    assert a[13]["numpy"] == "int32" and a[13]["values"] == prog.out_regs.tolist() and a[14] == 1 and a[15] == ["<other>"]
    assert a[16]["numpy"] == "int32" and a[16]["shape"] == [1, nlev] and a[17] == -5.0 and a[18] == 0
    assert out.shape == (nlev, ny, nx) and out.dtype == np.float32 and fd.shape == (nlev,)  # the leading axis dropped for one output
    # several outputs into out=, planes and level scalars by name, an expression instead of a program
    res = front._o(d, 2, nlev, ny, nx)
    scal = np.arange(2 * nlev, dtype=np.float32).reshape(2, nlev)
    out, fd = fx.evaluate(ctx, "u*c - v*s + p0, u*s + v*c + p1", {"u": d["B"], "v": d["V"]}, planes={"c": d["COSA"], "s": d["SINA"]},
                          level_scalars={"p0": scal[0], "p1": scal[1]}, out=res)
    a = _entry_calls(lib, "mifc_fexpr_levels")[-1]
    assert a[3] == [["B", 0], ["V", 0]] and a[4] == 2 and a[5] == [["COSA", 0], ["SINA", 0]] and a[6] == 2
    assert a[7]["numpy"] == "float32" and a[7]["shape"] == [2, nlev] and a[7]["values"] == scal.ravel().tolist() and a[8] == 2
    assert a[9] is None and a[10] == 0 and a[12] == 8 and a[14] == 2 and a[15] == [["OUT", 0], ["OUT", level]] and a[17] == float(np.float32(1e35))
    assert out is res and fd.shape == (2, nlev)
    # a stacked batch, one batch, a dict for a program with names
    fx.evaluate(ctx, fx.compile("a + b", fields=("a", "b")), d["F2"])
    assert _entry_calls(lib, "mifc_fexpr_levels")[-1][3] == [["F2", 0], ["F2", level]]
    fx.evaluate(ctx, fx.compile("abs(a)", fields=("a",)), d["B"])
    assert _entry_calls(lib, "mifc_fexpr_levels")[-1][3] == [["B", 0]]
    fx.evaluate(ctx, fx.compile("a - b", fields=("a", "b")), {"b": d["V"], "a": d["B"]})
    assert _entry_calls(lib, "mifc_fexpr_levels")[-1][3] == [["B", 0], ["V", 0]]
    # planes only: the levels come from the level scalars
    out, fd = fx.evaluate(ctx, "c * p", {}, planes={"c": d["COSA"]}, level_scalars={"p": scal[0]})
    a = _entry_calls(lib, "mifc_fexpr_levels")[-1]
    assert a[:3] == [nx, ny, nlev] and a[3] is None and a[4] == 0 and a[5] == [["COSA", 0]] and out.shape == (nlev, ny, nx)
    # what the front itself refuses
    with pytest.raises(ValueError, match="out must have shape"):
        fx.evaluate(ctx, prog, [d["T"], d["Q"]], out=res)
    with pytest.raises(ValueError, match="takes 2 fields and 0 planes"):
        fx.evaluate(ctx, prog, [d["T"]])
    with pytest.raises(ValueError, match="the program's fields are t, q"):
        fx.evaluate(ctx, prog, {"t": d["T"], "x": d["Q"]})
    with pytest.raises(ValueError, match="dicts by name"):
        fx.evaluate(ctx, "t + 1", [d["T"]])
    with pytest.raises(ValueError, match="a plane must have the shape"):
        fx.evaluate(ctx, "t * c", {"t": d["T"]}, planes={"c": d["B"]})
    with pytest.raises(ValueError, match="takes 1 level scalars"):
        fx.evaluate(ctx, "t * p", {"t": d["T"]}, level_scalars={"p": scal[0][:-1]})


def test_a_refused_call_raises_refused_with_the_librarys_message():
    fx = fexpr_module
    d = _data()
    ctx, lib = _stub_context(d, rc=0)
    lib.__dict__["mifc_last_error"] = lambda c: b"mifc_fexpr_levels: instruction 0: register 9 is read before anything set it"
    with pytest.raises(fx.Refused, match=r"register 9 is read before anything set it") as info:
        fx.evaluate(ctx, fx.Program.from_code([("add", 3, 0, 9)], out_regs=[3]), d["B"])
    assert isinstance(info.value, ValueError) and isinstance(info.value, RuntimeError)
    lib.__dict__["mifc_last_fexpr_form"] = lambda: b"family=fexpr form=vector grid=1 nlev=3 ncode=3 nregs=2 nout=1 tail=1 partials=0 tables=0 bands=1"
    form = fx.last_fexpr_form(ctx)
    assert form["family"] == "fexpr" and form["form"] == "vector" and form["tail"] == 1 and form["bands"] == 1 and form["partials"] == 0


# ------------------------------------------------------------------------------------------- the fuzz cases of the GPU
@pytest.mark.parametrize("seed", fr.FUZZ_SEEDS)
def test_fuzz_inputs_are_fit_for_purpose(seed):
    case = fr.fuzz_case(seed)
    names = {fr.OPS[op] for op in case["code"][:, 0]}
    assert names <= set(fr.IEEE_OPS) and 8 <= len(case["code"]) <= 64  # IEEE-only: bit for bit on the GPU
    defined, stats, nan_out = fr.fuzz_is_fit(case)  # (interpret() raises where a register is read before it is set)
    assert 0.10 <= defined <= 0.90, defined
    assert stats["operand"] >= 1 and stats["zero_div"] >= 1 and stats["nan"] >= 1 and nan_out >= 1, (stats, nan_out)
    pool = np.concatenate([f.ravel() for f in case["fields"] + case["planes"]])
    kinds = (pool == case["undef"], np.isnan(pool), (pool == 0) & ~np.signbit(pool), (pool == 0) & np.signbit(pool), np.isinf(pool),
             (pool != 0) & (np.abs(pool) < F(1.17549435e-38)))
    assert all(k.any() for k in kinds)  # undef, NaN, +0, -0, infinities and denormals all occur
    assert bits(fr.fuzz_case(seed)["fields"][0]) == bits(case["fields"][0])  # seeded: the GPU file gets the same case


MID_CHECKSUM = 776216049  # crc32 of the fields and the code of fuzz_case(FUZZ_SEEDS[0]) before the classes were added
RANGE_FUZZ = [(klass, seed) for klass in ("huge", "tiny") for seed in fr.FUZZ_RANGE_SEEDS[klass]]


@pytest.mark.parametrize("klass,seed", RANGE_FUZZ)
def test_fuzz_inputs_of_the_range_classes_are_fit_for_purpose(klass, seed):
    """The `huge` and `tiny` fuzz cases: 10 .. 90 % of the output cells defined; arithmetic makes an infinity from finite
    operands, a NaN and a nonzero subnormal, and an infinity, a NaN and a subnormal are each kept in an output; an
    intermediate equals 1e35 by arithmetic (5e34 + 5e34) and the next operation's operand test turns it away."""
    case = fr.fuzz_case(seed, klass=klass)
    names = [fr.OPS[op] for op in case["code"][:, 0]]
    assert set(names) <= set(fr.IEEE_OPS) and 8 <= len(names) <= 64
    defined, stats, kept = fr.fuzz_range_is_fit(case)
    assert 0.10 <= defined <= 0.90, defined
    assert min(stats[k] for k in ("operand", "zero_div", "nan", "inf", "subnormal", "made_undef")) >= 1, stats
    assert min(kept.values()) >= 1, kept
    # the sum of the constants is undef bit for bit, and what reads it is undefined everywhere
    assert F(case["consts"][0]) + F(case["consts"][0]) == fr.UNDEF and names[2:4] == ["add", "max"]
    first4 = fr.interpret(case["code"][:4], case["consts"], [11, 10], case["fields"], case["planes"], case["level_scalars"], case["undef"])[0]
    assert (first4 == fr.UNDEF).all()
    pool = np.concatenate([f.ravel() for f in case["fields"] + case["planes"]])
    for v in (fr.FLT_MAX, -fr.FLT_MAX, fr.DENORM_MIN, -fr.DENORM_MIN, np.nextafter(fr.UNDEF, F(0)), np.nextafter(fr.UNDEF, F(np.inf)), fr.UNDEF):
        assert (pool == F(v)).any(), v
    lo, hi = fr.FUZZ_DECADES[klass]
    with np.errstate(invalid="ignore", divide="ignore"):
        inside = (np.log10(np.abs(pool.astype(np.float64))) >= lo - 0.01) & (np.log10(np.abs(pool.astype(np.float64))) <= hi + 0.01)
    assert inside.mean() > 0.6
    for k in range(len(case["level_scalars"])):
        d = np.log10(np.abs(case["level_scalars"][k].astype(np.float64)))
        assert (d >= lo - 0.5).all() and (d <= hi + 0.01).all()
    assert bits(fr.fuzz_case(seed, klass=klass)["fields"][0]) == bits(case["fields"][0])


def test_the_mid_class_is_the_generator_as_it_was():
    """`mid` is the default: the existing seeds keep their cases (the first one pinned by a checksum of its bits)."""
    import zlib

    case = fr.fuzz_case(fr.FUZZ_SEEDS[0])
    same = fr.fuzz_case(fr.FUZZ_SEEDS[0], klass="mid")
    assert all(bits(a) == bits(b) for a, b in zip(case["fields"], same["fields"])) and np.array_equal(case["code"], same["code"])
    assert zlib.crc32(b"".join(f.tobytes() for f in case["fields"]) + case["code"].tobytes()) == MID_CHECKSUM


@pytest.mark.parametrize("name", fr.RANGE_TABLE_OPS)
def test_one_operation_table_is_the_ieee_operation_on_defined_operands(name):
    """The restatement of one operation over every pair of range operands, against numpy said once more, cell by cell in
    plain Python floats: where the rules leave the result to IEEE arithmetic it is that arithmetic's float32 result."""
    a, b, c = fr.range_operand_fields()
    prog = fr.range_table_program(name)
    out, _ = fr.interpret(prog["code"], prog["consts"], prog["out_regs"], [a, b, c])
    U = fr.UNDEF
    isdef = lambda v: not np.isnan(v) and v != U  # noqa: E731
    n = fr.RANGE_OPERANDS.size
    with np.errstate(all="ignore"):
        for k in range(n):
            for j in range(n):
                for i in range(n):
                    x, y, z, got = a[k, j, i], b[k, j, i], c[k, j, i], out[0, k, j, i]
                    if name == "ifdef":
                        want = x if isdef(x) else y
                    elif name == "mask":
                        want = x if (isdef(z) and z != 0) else U
                    elif name == "select":
                        r = x if z != 0 else y
                        want = r if (isdef(z) and isdef(r)) else U
                    elif name == "sqrt":
                        want = np.sqrt(x) if isdef(x) else U
                    elif not (isdef(x) and isdef(y)) or (name == "div" and y == 0):
                        want = U
                    else:
                        want = {"div": lambda: x / y, "min": lambda: y if y < x else x, "max": lambda: y if x < y else x, "lt": lambda: F(x < y),
                                "le": lambda: F(x <= y), "eq": lambda: F(x == y), "ne": lambda: F(x != y)}[name]()
                    want = F(want)
                    assert (np.isnan(got) and np.isnan(want)) or bits(np.array([got], F)) == bits(np.array([want], F)), (name, x, y, z, got, want)


def test_fuzz_cases_cover_the_operations_between_them():
    seen = set()
    for seed in fr.FUZZ_SEEDS:
        seen |= {fr.OPS[op] for op in fr.fuzz_case(seed)["code"][:, 0]}
    assert seen == set(fr.IEEE_OPS), set(fr.IEEE_OPS) - seen


# ------------------------------------------------------------------------------------------------------- no scratch
def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if not hipcc:
        pytest.skip("hipcc is not installed")
    flags = re.search(r"^HIPFLAGS := (.*)$", open(os.path.join(ROOT, "mi-fieldcalc_amd", "Makefile")).read(), flags=re.M).group(1).replace("$(ARCH)", "gfx950")
    run = subprocess.run([hipcc] + flags.split() + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "mifc_fexpr.hip"), "-o",
                                                    str(tmp_path / "mifc_fexpr.o")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    kernels = re.findall(r"Function Name: (\S*fexpr_kernel\S*)", run.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", run.stderr)]
    assert len(set(kernels)) == 4 and len(scratch) >= 4 and all(s == 0 for s in scratch), (kernels, scratch)
