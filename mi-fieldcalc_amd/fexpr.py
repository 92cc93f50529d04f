"""Field expressions over level batches (include/mifc.h, mifc_fexpr_levels; EXTENSION): a small register program
evaluated per cell in one launch, every operation rounded as the single-field call rounds it.  Free functions that take a
Context, like vcumul.

    from mi_fieldcalc_amd import fexpr
    prog = fexpr.compile("t * (1 + 0.608 * q)", fields=("t", "q"))
    tv, flags = fexpr.evaluate(ctx, prog, [t, q])
    th, flags = fexpr.evaluate(ctx, "t * (1000 / p) ** 0.2857", {"t": t}, level_scalars={"p": plevels})

Fields are numpy arrays (host memory) or CUDA tensors (device); the result lives where the fields live."""
import ast
import builtins
import ctypes

import numpy as np

from ._args import _Arg, _level_batches, _output, _parse_form, _pointer_table, _stacked_table
from ._consts import FEXPR_CONST0, FEXPR_LEVEL0, FEXPR_LIMITS, FEXPR_OPS, UNDEF

__all__ = ["FEXPR_OPS", "Refused", "Program", "compile", "evaluate", "last_fexpr_form"]

_ONE_OPERAND = ("abs", "neg", "sqrt", "log", "log10", "exp", "pow10", "mov")
_NAMES = {v: k for k, v in FEXPR_OPS.items()}
_BINOPS = {ast.Add: "add", ast.Sub: "sub", ast.Mult: "mul", ast.Div: "div", ast.Pow: "pow"}
# a > b is b < a, a >= b is b <= a: (operation, operands swapped)
_COMPARES = {ast.Lt: ("lt", False), ast.LtE: ("le", False), ast.Gt: ("lt", True), ast.GtE: ("le", True), ast.Eq: ("eq", False), ast.NotEq: ("ne", False)}
# name -> (operation, number of arguments); where(c, a, b), ifdef(a, b), mask(a, c)
_FUNCTIONS = {"min": ("min", 2), "max": ("max", 2), "abs": ("abs", 1), "sqrt": ("sqrt", 1), "log": ("log", 1), "log10": ("log10", 1), "exp": ("exp", 1),
              "pow10": ("pow10", 1), "where": ("select", 3), "ifdef": ("ifdef", 2), "mask": ("mask", 2)}


class Refused(ValueError, RuntimeError):
    """A call the library refused, with its reason: a ValueError (the arguments were wrong) that the handlers of the
    Context methods' RuntimeError catch too."""


def _reads(op):
    """The source bytes an operation reads, as positions in (a, b, c)."""
    name = _NAMES[op]
    if name in _ONE_OPERAND:
        return (0,)
    if name == "select":
        return (0, 1, 2)
    if name == "mask":
        return (0, 2)
    return (0, 1)


class Program:
    """A program of mifc_fexpr_levels: `code` uint8 (ncode, 8) rows of (op, dst, a, b, c, 0, 0, 0), `consts` float32,
    `out_regs` int32, `nregs` the registers in use, and the numbers (and, from compile(), the names) of the inputs the
    register file starts with: fields, then planes; level_scalars are operands."""

    def __init__(self, code, consts, out_regs, nregs, fields, planes, level_scalars):
        self.code = np.ascontiguousarray(code, dtype=np.uint8).reshape(-1, 8)
        self.consts = np.ascontiguousarray(consts, dtype=np.float32).ravel()
        self.out_regs = np.ascontiguousarray(out_regs, dtype=np.int32).ravel()
        self.nregs = int(nregs)
        self.fields, self.planes, self.level_scalars = tuple(fields), tuple(planes), tuple(level_scalars)

    nfields = property(lambda self: len(self.fields))
    nplanes = property(lambda self: len(self.planes))
    nscalars = property(lambda self: len(self.level_scalars))
    ncode = property(lambda self: int(self.code.shape[0]))
    nout = property(lambda self: int(self.out_regs.size))

    def instructions(self):
        """The code as a list of (name, dst, a, b, c) with the bytes the operation does not read as None."""
        out = []
        for op, dst, a, b, c in self.code[:, :5].tolist():
            src = [a, b, c]
            out.append((_NAMES[op], dst) + tuple(src[i] if i in _reads(op) else None for i in range(3)))
        return out

    @classmethod
    def from_code(cls, code, consts=(), out_regs=(0,), nfields=1, nplanes=0, nscalars=0):
        """A program from a raw instruction list: rows of (op, dst, a[, b[, c]]) with op a number or a name of FEXPR_OPS and
        the source bytes as the header defines them (a register, FEXPR_LEVEL0 + s, FEXPR_CONST0 + j).  Nothing is checked
        here but the shape of a row: the library refuses a bad program with its reason."""
        rows, top = [], int(nfields) + int(nplanes)
        for ins in code:
            ins = list(ins)
            if not 3 <= len(ins) <= 5:
                raise ValueError("an instruction is (op, dst, a[, b[, c]]): %r" % (ins,))
            op = FEXPR_OPS.get(ins[0], -1) if isinstance(ins[0], str) else int(ins[0])
            if not 0 <= op <= 255:
                raise ValueError("unknown operation %r" % (ins[0],))
            row = [op] + [int(x) for x in ins[1:]] + [0] * (8 - len(ins))
            if builtins.min(row) < 0 or builtins.max(row) > 255:
                raise ValueError("an instruction is made of bytes: %r" % (ins,))
            rows.append(row)
            top = builtins.max([top] + [x + 1 for x in row[1:5] if x < FEXPR_LIMITS["nregs"]])
        return cls(np.array(rows, dtype=np.uint8).reshape(-1, 8), consts, out_regs, top, range(int(nfields)), range(int(nplanes)), range(int(nscalars)))


# ------------------------------------------------------------------------------------------------------- the compiler
class _Graph:
    """The expression as a graph whose structurally equal nodes are one node: leaves ("reg", i), ("lev", s), ("const", bits),
    operations (name, a, b, c) over node numbers."""

    def __init__(self, fields, planes, scalars):
        self.nodes, self.index, self.consts = [], {}, []
        self.names = {}
        for i, n in enumerate(tuple(fields) + tuple(planes)):
            self._name(n, ("reg", i))
        for s, n in enumerate(scalars):
            self._name(n, ("lev", s))

    def _name(self, n, leaf):
        if not isinstance(n, str) or not n.isidentifier():
            raise ValueError("%r is no name" % (n,))
        if n in self.names or n in _FUNCTIONS:
            raise ValueError("the name %r is taken" % n)
        self.names[n] = self.node(leaf)

    def node(self, key):
        if key not in self.index:
            self.index[key] = len(self.nodes)
            self.nodes.append(key)
        return self.index[key]

    def const(self, value):
        bits = int(np.float32(value).view(np.uint32))  # deduplicated by bits, never folded
        if bits not in self.consts:
            self.consts.append(bits)
        return self.node(("const", bits))

    def build(self, e):
        if isinstance(e, ast.Constant) and isinstance(e.value, (int, float)) and not isinstance(e.value, bool):
            return self.const(e.value)
        if isinstance(e, ast.Name):
            if e.id not in self.names:
                raise ValueError("unknown name %r" % e.id)
            return self.names[e.id]
        if isinstance(e, ast.UnaryOp) and isinstance(e.op, (ast.USub, ast.UAdd)):
            if isinstance(e.operand, ast.Constant) and isinstance(e.operand.value, (int, float)) and not isinstance(e.operand.value, bool):
                return self.const(-e.operand.value if isinstance(e.op, ast.USub) else e.operand.value)  # a signed literal
            x = self.build(e.operand)
            return self.node(("neg", x, None, None)) if isinstance(e.op, ast.USub) else x
        if isinstance(e, ast.BinOp) and type(e.op) in _BINOPS:
            return self.node((_BINOPS[type(e.op)], self.build(e.left), self.build(e.right), None))
        if isinstance(e, ast.Compare):
            if len(e.ops) != 1 or type(e.ops[0]) not in _COMPARES:
                raise ValueError("a comparison has two sides and is one of < <= > >= == !=")
            name, swap = _COMPARES[type(e.ops[0])]
            a, b = self.build(e.left), self.build(e.comparators[0])
            return self.node((name, b, a, None) if swap else (name, a, b, None))
        if isinstance(e, ast.Call):
            if not isinstance(e.func, ast.Name) or e.func.id not in _FUNCTIONS:
                raise ValueError("unknown function %r" % (getattr(e.func, "id", None) or ast.dump(e.func),))
            name, nargs = _FUNCTIONS[e.func.id]
            if e.keywords or len(e.args) != nargs:
                raise ValueError("%s takes %d argument%s" % (e.func.id, nargs, "" if nargs == 1 else "s"))
            x = [self.build(a) for a in e.args]
            if name == "select":  # where(c, a, b)
                return self.node((name, x[1], x[2], x[0]))
            if name == "mask":  # mask(a, c)
                return self.node((name, x[0], None, x[1]))
            return self.node((name, x[0], x[1] if nargs == 2 else None, None))
        raise ValueError("not accepted in a field expression: %s" % type(e).__name__)


def compile(expr, fields=(), planes=(), level_scalars=()):
    """The program of an infix expression over the names `fields` (level batches), `planes` (one plane for every level) and
    `level_scalars` (one number per level).  expr: a string, several outputs separated by commas, or a tuple of strings.
    Accepted: names, numbers, + - * / **, unary minus, < <= > >= == != (1.0 or 0.0), and min(a, b) max(a, b) abs sqrt log
    log10 exp pow10 where(c, a, b) ifdef(a, b) mask(a, c).  a > b is computed as b < a, a >= b as b <= a.  Structurally
    equal subexpressions are computed once, registers are reused after their last read, constants are deduplicated and never
    folded (folding would change the rounding; a signed number is one constant).  Raises ValueError with the reason."""
    L = FEXPR_LIMITS
    if isinstance(fields, str) or isinstance(planes, str) or isinstance(level_scalars, str):
        raise ValueError("fields, planes and level_scalars are sequences of names")
    if len(fields) > L["fields"] or len(planes) > L["planes"] or not 1 <= len(fields) + len(planes) <= L["inputs"] or len(level_scalars) > L["scalars"]:
        raise ValueError("0..%d fields, 0..%d planes, 1..%d of both, 0..%d level scalars" % (L["fields"], L["planes"], L["inputs"], L["scalars"]))
    g = _Graph(fields, planes, level_scalars)
    text = expr if isinstance(expr, str) else ", ".join("(%s)" % e for e in expr)
    try:
        tree = ast.parse(text.strip(), mode="eval").body
    except SyntaxError as e:
        raise ValueError("not an expression: %s" % e) from None
    outs = [g.build(e) for e in (tree.elts if isinstance(tree, ast.Tuple) else [tree])]
    if not 1 <= len(outs) <= L["out"]:
        raise ValueError("1..%d outputs" % L["out"])
    if len(g.consts) > L["consts"]:
        raise ValueError("more than %d constants" % L["consts"])

    # the operations in an order that computes operands first, each once
    order, seen = [], set()

    def visit(n):
        if n in seen:
            return
        seen.add(n)
        key = g.nodes[n]
        if key[0] not in ("reg", "lev", "const"):
            for x in key[1:]:
                if x is not None:
                    visit(x)
            order.append(n)

    for o in outs:
        visit(o)
    # an output that is a bare input, level scalar or constant is moved into a register of its own
    moved = {}
    for o in outs:
        if g.nodes[o][0] in ("reg", "lev", "const") and o not in moved:
            moved[o] = g.node(("mov", o, None, None))
            order.append(moved[o])
    outs = [moved.get(o, o) for o in outs]
    if len(order) > L["code"]:
        raise ValueError("more than %d instructions" % L["code"])

    last = {}  # node -> the position of its last read; an output is read at the end
    for pos, n in enumerate(order):
        for x in g.nodes[n][1:]:
            if x is not None:
                last[x] = pos
    for o in outs:
        last[o] = len(order)
    nin = len(fields) + len(planes)
    reg = {g.node(("reg", i)): i for i in range(nin)}
    free = [r for r in range(nin, L["nregs"])] + [i for i in range(nin) if g.node(("reg", i)) not in last]
    free.sort()
    top, code = nin, []

    def operand(x):
        if x is None:
            return 0
        key = g.nodes[x]
        if key[0] == "lev":
            return FEXPR_LEVEL0 + key[1]
        if key[0] == "const":
            return FEXPR_CONST0 + g.consts.index(key[1])
        return reg[x]

    for pos, n in enumerate(order):
        key = g.nodes[n]
        src = [operand(x) for x in key[1:]]
        for x in set(key[1:]):  # a register read here for the last time may be this instruction's own destination
            if x in reg and last.get(x) == pos:
                free.append(reg[x])
        free.sort()
        if not free:
            raise ValueError("more than %d live registers" % L["nregs"])
        reg[n] = free.pop(0)
        top = builtins.max(top, reg[n] + 1)
        code.append([FEXPR_OPS[key[0]], reg[n]] + src + [0, 0, 0])
    return Program(np.array(code, dtype=np.uint8).reshape(-1, 8), np.array(g.consts, dtype=np.uint32).view(np.float32), [reg[o] for o in outs], top,
                   fields, planes, level_scalars)


# ------------------------------------------------------------------------------------------------------- evaluation
def _named(prog, given, names, what):
    """`given` -- a dict by name, a sequence, a stacked array or None -- as a list in the program's order."""
    if given is None:
        given = []
    if isinstance(given, dict):
        if sorted(given) != sorted(str(n) for n in names):
            raise ValueError("the program's %s are %s" % (what, ", ".join(str(n) for n in names) or "none"))
        return [given[n] for n in names]
    if hasattr(given, "shape"):
        return given
    return list(given)


def evaluate(ctx, prog_or_expr, fields, planes=None, level_scalars=None, out=None, undef=UNDEF):
    """EXTENSION (include/mifc.h, mifc_fexpr_levels): the program in every cell of the level batches, in one launch.
    prog_or_expr: a Program, or an expression for compile() -- `fields`, `planes` and `level_scalars` are then dicts by name,
    in the order the register file takes them.  With a Program, fields is a list of (nlev, ny, nx) numpy arrays (host
    memory) or CUDA tensors (device), one batch, one stacked (nf, nlev, ny, nx), or a dict by the program's names; planes: a
    list (or dict) of (ny, nx); level_scalars: (nscalars, nlev) numbers, a list of rows or a dict.  out: (nlev, ny, nx) for one
    output, (nout, nlev, ny, nx) for several.  Returns (out, flags int32 (nout, nlev)), the leading axis dropped from both
    for one output.  A refused call raises Refused (a ValueError) with the library's reason."""
    if not isinstance(prog_or_expr, Program):
        if not (isinstance(fields, dict) and isinstance(planes or {}, dict) and isinstance(level_scalars or {}, dict)):
            raise ValueError("with an expression, fields, planes and level_scalars are dicts by name")
        prog = compile(prog_or_expr, tuple(fields), tuple(planes or {}), tuple(level_scalars or {}))
    else:
        prog = prog_or_expr
    fields = _named(prog, fields, prog.fields, "fields")
    planes = _named(prog, planes, prog.planes, "planes")
    level_scalars = _named(prog, level_scalars, prog.level_scalars, "level scalars")
    pa = [_Arg(p) for p in (planes if not hasattr(planes, "shape") else [planes[i] for i in range(planes.shape[0])])]
    if hasattr(fields, "shape") or len(fields):
        _, batches, fa, shape = _level_batches(fields)
        ref = batches[0]
    else:  # planes only: the levels are the level scalars', or the output's, or one
        if not pa:
            raise ValueError("no fields and no planes")
        fa, ref = [], pa[0].keep
        nlev = np.shape(level_scalars)[-1] if np.size(level_scalars) else (1 if out is None else int(out.shape[-3]))
        shape = (int(nlev),) + tuple(pa[0].shape)
    nlev, ny, nx = shape
    if len(fa) != prog.nfields or len(pa) != prog.nplanes:
        raise ValueError("the program takes %d fields and %d planes" % (prog.nfields, prog.nplanes))
    if any(tuple(a.shape) != (ny, nx) for a in pa):
        raise ValueError("a plane must have the shape %s" % ((ny, nx),))
    ls = np.asarray(level_scalars, dtype=np.float32)
    if ls.size != prog.nscalars * nlev:
        raise ValueError("the program takes %d level scalars of %d levels each" % (prog.nscalars, nlev))
    ls = np.ascontiguousarray(ls.reshape(prog.nscalars, nlev))
    nout = prog.nout
    res, oa = _output(out, ref, shape if nout == 1 else (nout,) + shape)
    ftab, ptab = _pointer_table([a.addr for a in fa]), _pointer_table([a.addr for a in pa])
    otab = _stacked_table(oa.addr, nout, nlev * ny * nx * 4)
    fd = np.zeros((nout, nlev), np.int32)
    try:
        ctx._launch("mifc_fexpr_levels", fa + pa + [oa],
                    [nx, ny, nlev, ctypes.addressof(ftab) if fa else None, len(fa), ctypes.addressof(ptab) if pa else None, len(pa),
                     ls if ls.size else None, ls.shape[0], prog.consts if prog.consts.size else None, int(prog.consts.size), prog.code, prog.ncode,
                     prog.out_regs, nout, ctypes.addressof(otab), fd, float(undef)])
    except RuntimeError as e:
        raise Refused(str(e)) from None
    return (res, fd[0]) if nout == 1 else (res, fd)


def last_fexpr_form(ctx):
    """The launch shape of this thread's last fexpr call as a dict (mifc_last_fexpr_form; a diagnostic for tests): family
    and form as strings, the other keys as ints."""
    return _parse_form(ctx._lib.mifc_last_fexpr_form(), ("family", "form"))
