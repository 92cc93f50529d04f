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
FLT_MAX, FLT_MIN, DENORM_MIN = np.finfo(F).max, np.finfo(F).tiny, F(2.0) ** F(-149)


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
    zero ("zero_div"), and how many arithmetic results were NaN and kept ("nan"); of the results of operations that compute
    (not ifdef, mask, mov, select) also how many were infinite from finite operands ("inf"), nonzero subnormal
    ("subnormal") or equal to undef from defined operands ("made_undef": stored, they are undefined to the next operation);
    and under "kept" how many output cells hold an infinity, a NaN or a nonzero subnormal that such an operation MADE (an
    infinity from finite operands, a NaN from operands that are none, any subnormal result) and that the operations which
    only hand a value on (mov, ifdef, select, mask, min, max, abs, neg) carried there -- not one copied from an input."""
    undef = F(undef)
    fields = [np.asarray(f, F) for f in fields]
    planes = [np.asarray(p, F) for p in planes]
    ls = np.asarray(level_scalars, F)
    shape = fields[0].shape if fields else ((ls.shape[-1] if ls.size else 1),) + planes[0].shape
    nlev = shape[0]
    regs, made = {}, {}  # made: the cell's value is an inf, NaN or subnormal that a computing operation produced
    none = np.zeros(shape, bool)
    for i, f in enumerate(fields):
        regs[i] = f.copy()
    for i, p in enumerate(planes):
        regs[len(fields) + i] = np.broadcast_to(p, shape).copy()
    consts = np.asarray(consts, F).ravel()
    count = {"operand": 0, "zero_div": 0, "nan": 0, "inf": 0, "subnormal": 0, "made_undef": 0}

    def made_of(s):
        return made.get(s, none) if s < 16 else none

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
            ma, mb = made_of(int(ins[2])), made_of(int(ins[2]) if name in ONE_OPERAND or name == "mask" else int(ins[3]))
            if name in ("mov", "mask", "abs", "neg"):
                m = ma
            elif name == "ifdef":
                m = np.where(is_def(a, undef), ma, mb)
            elif name == "select":
                m = np.where(c != 0, ma, mb)
            elif name == "min":
                m = np.where(b < a, mb, ma)
            elif name == "max":
                m = np.where(a < b, mb, ma)
            elif name in ("lt", "le", "eq", "ne"):
                m = none
            else:
                m = (np.isinf(r) & np.isfinite(a) & np.isfinite(b)) | (np.isnan(r) & ~np.isnan(a) & ~np.isnan(b)) | ((r != 0) & (np.abs(r) < FLT_MIN))
            made[dst] = ok & m
            count["operand"] += int(by_operand.sum())
            count["zero_div"] += int(zero.sum())
            if name not in ("ifdef", "mask", "mov", "select"):
                count["nan"] += int((ok & np.isnan(r)).sum())
                count["inf"] += int((ok & np.isinf(r) & np.isfinite(a) & np.isfinite(b)).sum())
                count["subnormal"] += int((ok & (r != 0) & (np.abs(r) < FLT_MIN)).sum())
                count["made_undef"] += int((ok & (r == undef)).sum())
            regs[dst] = np.where(ok, r, undef).astype(F)
    out = np.stack([regs[int(o)] for o in out_regs]).astype(F)
    flags = np.array([[classify(int((out[o, k] == undef).sum()), out[o, k].size) for k in range(nlev)] for o in range(out.shape[0])], np.int32)
    if stats is not None:
        om = np.stack([made.get(int(o), none) for o in out_regs])
        count["kept"] = {"inf": int((om & np.isinf(out)).sum()), "nan": int((om & np.isnan(out)).sum()),
                         "subnormal": int((om & (out != 0) & (np.abs(out) < FLT_MIN)).sum())}
        stats.update(count)
    return out, flags


# ------------------------------------------------------------------------------------------------- the fuzz cases
IEEE_OPS = ("add", "sub", "mul", "div", "min", "max", "abs", "neg", "sqrt", "lt", "le", "eq", "ne", "select", "ifdef", "mask", "mov")
# every seed gives a case that the CPU test accepts: 10 .. 90 % of its output cells defined, a cell left undef by an
# operand, one by a zero divisor, and a NaN that is kept in an output (test_fuzz_inputs_are_fit_for_purpose)
FUZZ_SEEDS = (0, 20, 24, 42, 46, 56)
FUZZ_SHAPE = (3, 5, 37)  # nlev, ny, nx: 185 cells, 46 quads and a tail of one


# The magnitude classes of the fuzz cases.  `mid` is the generator as it always was, bit for bit.  `huge`: decades 1e18 ..
# 3e38, so that products and sums straddle FLT_MAX; `tiny`: subnormal .. 1e-19, so that products, quotients and roots
# straddle FLT_MIN.  Both also sprinkle the two neighbours of 1e35, +-FLT_MAX and +-2^-149.
FUZZ_CLASSES = ("mid", "huge", "tiny")
FUZZ_DECADES = {"huge": (18.0, 38.5), "tiny": (-45.0, -19.0)}
RANGE_SPECIALS = ((0.22, np.nextafter(UNDEF, F(0))), (0.23, np.nextafter(UNDEF, F(np.inf))), (0.24, FLT_MAX), (0.25, -FLT_MAX), (0.26, DENORM_MIN), (0.27, -DENORM_MIN))


def fuzz_magnitudes(rng, shape, klass):
    lo, hi = FUZZ_DECADES[klass]
    x = 10.0 ** rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], size=shape)
    return np.clip(x, -float(FLT_MAX), float(FLT_MAX)).astype(F)


def fuzz_field(rng, shape, undef=UNDEF, klass="mid"):
    """Values around one (klass "mid"; or of the decades of "huge" / "tiny") with everything the rules speak of sprinkled in:
    undef, NaN, zeros of both signs, infinities, denormals and huge numbers."""
    x = rng.uniform(-4.0, 4.0, shape).astype(F) if klass == "mid" else fuzz_magnitudes(rng, shape, klass)
    kind = rng.random(shape)
    specials = ((0.05, undef), (0.07, np.nan), (0.13, 0.0), (0.15, -0.0), (0.16, np.inf), (0.17, -np.inf), (0.19, 1e-40), (0.20, -3e-39), (0.21, 3e30))
    if klass != "mid":
        specials += RANGE_SPECIALS
    lo = 0.0
    for hi, v in specials:
        x[(kind >= lo) & (kind < hi)] = F(v)
        lo = hi
    return x


def fuzz_case(seed, shape=FUZZ_SHAPE, undef=UNDEF, klass="mid"):
    """A random valid program of IEEE-only operations and its inputs: a dict with code (rows of 5 bytes), consts, out_regs,
    fields, planes, level_scalars, undef.  klass "huge" / "tiny": fields, planes, level scalars and half of the constants
    of that class's decades, and a program that begins with 5e34 + 5e34 from constants -- a result that equals 1e35 by
    arithmetic -- and an operation that reads it."""
    mid = klass == "mid"
    rng = np.random.default_rng(1000 + seed if mid else [1000 + seed, FUZZ_CLASSES.index(klass)])
    nlev, ny, nx = shape
    nfields, nplanes, nscalars = int(rng.integers(1, 5)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
    if mid:
        consts = rng.choice(np.array([0.5, 2.0, -1.0, 0.0, 3.25, 1e-3, -7.5], F), int(rng.integers(1, 5)), replace=False).astype(F)
    else:
        consts = np.concatenate([[F(5e34)], rng.choice(np.array([0.5, 2.0, -1.0, 0.0], F), 2, replace=False), fuzz_magnitudes(rng, 2, klass)]).astype(F)
    fields = [fuzz_field(rng, shape, undef, klass) for _ in range(nfields)]
    planes = [fuzz_field(rng, (ny, nx), undef, klass) for _ in range(nplanes)]
    level_scalars = rng.uniform(-2.0, 2.0, (nscalars, nlev)).astype(F) if mid else fuzz_magnitudes(rng, (nscalars, nlev), klass)
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
    if not mid:  # 1e35 by arithmetic, and an operand test that sees it
        code += [[OP["add"], 11, CONST(0), CONST(0), 0], [OP["max"], 10, 11, source(True), 0]]
        written += [11, 10]
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


# seeds of the `huge` and `tiny` classes that tests/test_fexpr_cpu.py accepts: 10 .. 90 % of the output cells defined; an
# infinity that arithmetic made from finite operands, a NaN that arithmetic made and a nonzero subnormal result each
# occur and each reaches an output (as interpret's "kept" counts it: made by a computing operation, not copied from an
# input; about one seed in two hundred does); an intermediate equals 1e35 by arithmetic
FUZZ_RANGE_SEEDS = {"huge": (85, 482, 932, 1080), "tiny": (323, 378, 539, 826)}


def fuzz_range_is_fit(case):
    """(defined fraction, stats, what the outputs keep of what arithmetic made: counts of inf, NaN and nonzero subnormal
    cells whose value a computing operation produced -- interpret's "kept")."""
    stats = {}
    out, _ = interpret(case["code"], case["consts"], case["out_regs"], case["fields"], case["planes"], case["level_scalars"], case["undef"], stats)
    return float(is_def(out, case["undef"]).mean()), stats, stats.pop("kept")


# ------------------------------------------------------------------------------------- one operation, range operands
# Every pair (a, b) and, for select and mask, every condition c of these values: the zeros, a subnormal against FLT_MAX,
# FLT_MAX against FLT_MAX, undef and both its neighbours, NaN, the infinities.  a runs along x, b along y, c along the levels.
RANGE_OPERANDS = np.array([0.0, -0.0, DENORM_MIN, -DENORM_MIN, FLT_MIN, FLT_MAX, -FLT_MAX, np.nextafter(UNDEF, F(0)), UNDEF, np.nextafter(UNDEF, F(np.inf)),
                           np.nan, np.inf, -np.inf, 1.0, 2.0], F)
RANGE_TABLE_OPS = ("div", "sqrt", "min", "max", "lt", "le", "eq", "ne", "select", "ifdef", "mask")


def range_operand_fields():
    """(a, b, c), each (n, n, n) with n = len(RANGE_OPERANDS)."""
    n = RANGE_OPERANDS.size
    shape = (n, n, n)
    a = np.broadcast_to(RANGE_OPERANDS.reshape(1, 1, n), shape).copy()
    b = np.broadcast_to(RANGE_OPERANDS.reshape(1, n, 1), shape).copy()
    c = np.broadcast_to(RANGE_OPERANDS.reshape(n, 1, 1), shape).copy()
    return a, b, c


def range_table_program(name):
    """The program of one operation on the registers 0, 1, 2 = a, b, c into register 3."""
    return dict(code=np.array([[OP[name], 3, 0, 1, 2]], np.uint8), consts=np.zeros(1, F), out_regs=np.array([3], np.int32))
