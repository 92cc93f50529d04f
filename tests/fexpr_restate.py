"""mifc_fexpr_levels restated in numpy (include/mifc.h, rules 1-5): an instruction list interpreted operation by operation
in float32, the oracle of the GPU tests.  LOG, LOG10, EXP, POW10 and POW are the float64 function rounded once to float32
(the device functions are within 1 ulp of that); everything else is IEEE arithmetic and compared bit for bit.

Also the seeded random programs and fields of the fuzz tests (fuzz_case): the CPU file asserts that they are fit for
purpose, the GPU file runs them."""
import numpy as np

F = np.float32
UNDEF = F(1.0e35)
OPS = ("add", "sub", "mul", "div", "min", "max", "abs", "neg", "sqrt", "log", "log10", "exp", "pow10", "pow", "lt", "le", "eq", "ne", "select", "ifdef",
       "mask", "mov")
OP = {n: i for i, n in enumerate(OPS)}
ONE_OPERAND = ("abs", "neg", "sqrt", "log", "log10", "exp", "pow10", "mov")
LEVEL0, CONST0 = 16, 32
ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2


def LEVEL(s):
    return LEVEL0 + s


def CONST(j):
    return CONST0 + j


def is_def(x, undef):
    return ~np.isnan(x) & (x != F(undef))


def classify(n_undefined, n):
    return ALL_DEFINED if n_undefined == 0 else (NONE_DEFINED if n_undefined == n else SOME_DEFINED)


def interpret(code, consts, out_regs, fields, planes=(), level_scalars=(), undef=UNDEF, stats=None):
    """code: rows of (op, dst, a[, b[, c]]), op a number or a name; fields: (nlev, ny, nx) arrays, planes: (ny, nx),
    level_scalars: (nscalars, nlev).  Returns (out float32 (nout, nlev, ny, nx), flags int32 (nout, nlev)).  stats: a dict
    that receives how many cells an instruction left undef because an operand was undefined ("operand") or the divisor
    zero ("zero_div"), and how many arithmetic results were NaN and kept ("nan")."""
    undef = F(undef)
    fields = [np.asarray(f, F) for f in fields]
    planes = [np.asarray(p, F) for p in planes]
    ls = np.asarray(level_scalars, F)
    shape = fields[0].shape if fields else ((ls.shape[-1] if ls.size else 1),) + planes[0].shape
    nlev = shape[0]
    regs = {}
    for i, f in enumerate(fields):
        regs[i] = f.copy()
    for i, p in enumerate(planes):
        regs[len(fields) + i] = np.broadcast_to(p, shape).copy()
    consts = np.asarray(consts, F).ravel()
    count = {"operand": 0, "zero_div": 0, "nan": 0}

    def src(s):
        if s < 16:
            return regs[s]  # KeyError: read before anything set it
        if s < 32:
            return np.broadcast_to(ls.reshape(-1, nlev)[s - LEVEL0].reshape(nlev, 1, 1), shape)
        return np.broadcast_to(consts[s - CONST0], shape)

    with np.errstate(all="ignore"):
        for ins in code:
            ins = list(ins) + [0] * (5 - len(ins))
            name = ins[0] if isinstance(ins[0], str) else OPS[int(ins[0])]
            dst = int(ins[1])
            a = src(int(ins[2]))
            b = a if name in ONE_OPERAND or name == "mask" else src(int(ins[3]))
            ok = is_def(a, undef) & is_def(b, undef)
            by_operand = ~ok
            zero = np.zeros(shape, bool)
            if name == "add":
                r = a + b
            elif name == "sub":
                r = a - b
            elif name == "mul":
                r = a * b
            elif name == "div":
                r = a / b
                zero = ok & (b == 0)
                ok = ok & (b != 0)
            elif name == "min":
                r = np.where(b < a, b, a)
            elif name == "max":
                r = np.where(a < b, b, a)
            elif name == "abs":
                r = np.abs(a)
            elif name == "neg":
                r = -a
            elif name == "sqrt":
                r = np.sqrt(a)
            elif name == "log":
                r = np.log(a.astype(np.float64)).astype(F)
            elif name == "log10":
                r = np.log10(a.astype(np.float64)).astype(F)
            elif name == "exp":
                r = np.exp(a.astype(np.float64)).astype(F)
            elif name == "pow10":
                r = np.power(10.0, a.astype(np.float64)).astype(F)
            elif name == "pow":
                r = np.power(a.astype(np.float64), b.astype(np.float64)).astype(F)
            elif name in ("lt", "le", "eq", "ne"):
                r = {"lt": a < b, "le": a <= b, "eq": a == b, "ne": a != b}[name].astype(F)
            elif name == "mov":
                r = a
            elif name == "select":
                c = src(int(ins[4]))
                r = np.where(c != 0, a, b)
                ok = is_def(c, undef) & is_def(r, undef)
                by_operand = ~ok
            elif name == "ifdef":
                r = np.where(is_def(a, undef), a, b)
                ok = np.ones(shape, bool)
                by_operand = ~ok
            elif name == "mask":
                c = src(int(ins[4]))
                r = a
                ok = is_def(c, undef) & (c != 0)
                by_operand = ~is_def(c, undef)
            else:
                raise ValueError("unknown op %r" % (ins[0],))
            r = np.asarray(r, F)
            count["operand"] += int(by_operand.sum())
            count["zero_div"] += int(zero.sum())
            if name not in ("ifdef", "mask", "mov", "select"):
                count["nan"] += int((ok & np.isnan(r)).sum())
            regs[dst] = np.where(ok, r, undef).astype(F)
    out = np.stack([regs[int(o)] for o in out_regs]).astype(F)
    flags = np.array([[classify(int((out[o, k] == undef).sum()), out[o, k].size) for k in range(nlev)] for o in range(out.shape[0])], np.int32)
    if stats is not None:
        stats.update(count)
    return out, flags


# ------------------------------------------------------------------------------------------------- the fuzz cases
IEEE_OPS = ("add", "sub", "mul", "div", "min", "max", "abs", "neg", "sqrt", "lt", "le", "eq", "ne", "select", "ifdef", "mask", "mov")
# every seed gives a case that the CPU test accepts: 10 .. 90 % of its output cells defined, a cell left undef by an
# operand, one by a zero divisor, and a NaN that is kept in an output (test_fuzz_inputs_are_fit_for_purpose)
FUZZ_SEEDS = (0, 20, 24, 42, 46, 56)
FUZZ_SHAPE = (3, 5, 37)  # nlev, ny, nx: 185 cells, 46 quads and a tail of one


def fuzz_field(rng, shape, undef=UNDEF):
    """Values around one with everything the rules speak of sprinkled in: undef, NaN, zeros of both signs, infinities,
    denormals and huge numbers."""
    x = rng.uniform(-4.0, 4.0, shape).astype(F)
    kind = rng.random(shape)
    specials = ((0.05, undef), (0.07, np.nan), (0.13, 0.0), (0.15, -0.0), (0.16, np.inf), (0.17, -np.inf), (0.19, 1e-40), (0.20, -3e-39), (0.21, 3e30))
    lo = 0.0
    for hi, v in specials:
        x[(kind >= lo) & (kind < hi)] = F(v)
        lo = hi
    return x


def fuzz_case(seed, shape=FUZZ_SHAPE, undef=UNDEF):
    """A random valid program of IEEE-only operations and its inputs: a dict with code (rows of 5 bytes), consts, out_regs,
    fields, planes, level_scalars, undef."""
    rng = np.random.default_rng(1000 + seed)
    nlev, ny, nx = shape
    nfields, nplanes, nscalars = int(rng.integers(1, 5)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
    consts = rng.choice(np.array([0.5, 2.0, -1.0, 0.0, 3.25, 1e-3, -7.5], F), int(rng.integers(1, 5)), replace=False).astype(F)
    fields = [fuzz_field(rng, shape, undef) for _ in range(nfields)]
    planes = [fuzz_field(rng, (ny, nx), undef) for _ in range(nplanes)]
    level_scalars = rng.uniform(-2.0, 2.0, (nscalars, nlev)).astype(F)
    written = list(range(nfields + nplanes))

    def source(register_only=False):
        kinds = ["reg"] * 6 + (["lev"] if nscalars else []) + ["const"]
        kind = "reg" if register_only else kinds[int(rng.integers(len(kinds)))]
        if kind == "reg":
            return int(written[int(rng.integers(len(written)))])
        if kind == "lev":
            return LEVEL(int(rng.integers(nscalars)))
        return CONST(int(rng.integers(len(consts))))

    code = [[OP["div"], 12, 0, source(True), 0], [OP["sqrt"], 13, source(True), 0, 0]]  # a divisor with zeros, negative arguments
    written += [12, 13]
    for _ in range(int(rng.integers(6, 18))):
        name = IEEE_OPS[int(rng.integers(len(IEEE_OPS)))]
        dst = int(rng.integers(0, 16))  # inputs are overwritten too
        code.append([OP[name], dst, source(), source(), source()])
        if dst not in written:
            written.append(dst)
    # the outputs: what the repair operations leave of the last results, so that a fair share of the cells stays defined
    nout = int(rng.integers(1, 4))
    last = [c[1] for c in code[-nout:]]
    out_regs = []
    for o in range(nout):
        dst = 15 - o
        code.append([OP["ifdef"], dst, last[o], source(True), 0])
        out_regs.append(dst)
    return {"code": np.array(code, np.uint8), "consts": consts, "out_regs": np.array(out_regs, np.int32), "fields": fields, "planes": planes,
            "level_scalars": level_scalars, "undef": F(undef)}


def fuzz_is_fit(case):
    """(defined fraction of the output cells, the stats of interpret, NaNs kept in the outputs)."""
    stats = {}
    out, _ = interpret(case["code"], case["consts"], case["out_regs"], case["fields"], case["planes"], case["level_scalars"], case["undef"], stats)
    return float(is_def(out, case["undef"]).mean()), stats, int(np.isnan(out).sum())
