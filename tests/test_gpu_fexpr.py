"""GPU tests of mifc_fexpr_levels against the library's own single-field entries (a program made of their operations is
the chain of calls, bit for bit) and against the numpy restatement (tests/fexpr_restate.py): every launch shape, host
memory in bands, the fuzz cases of the CPU file, the transcendental operations on their seam inputs, every operand kind,
and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

import fexpr_restate as fr
import seam_cases
from cases import same_bits
from mi_fieldcalc_amd import fexpr

pytestmark = pytest.mark.gpu

F = np.float32
U = fr.UNDEF
L, C = fr.LEVEL, fr.CONST


def dev(a, off=0):
    """A device tensor with the array's values, its first float `off` floats behind the 16-byte grid."""
    import torch

    a = np.ascontiguousarray(a, F)
    room = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
    assert room.data_ptr() % 16 == 0
    t = room[off:off + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def dev_out(shape, off=0, fill=-4242.5):
    import torch

    n = int(np.prod(shape))
    room = torch.full((n + 8,), fill, dtype=torch.float32, device="cuda")
    return room[off:off + n].view(*shape)


def restated(prog, fields, planes=(), scalars=(), undef=U):
    return fr.interpret(prog.code[:, :5], prog.consts, prog.out_regs, fields, planes, scalars, undef)


def agree(got, fd, want, wfd, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert same_bits(got.reshape(want.shape), want, nan_payload=False), what
    assert np.array_equal(np.asarray(fd).reshape(wfd.shape), wfd), (what, fd, wfd)


@functools.lru_cache(maxsize=None)
def shape_inputs(nlev, ny, nx):
    rng = np.random.default_rng(nlev * 1000 + ny * 37 + nx)
    t, q = fr.fuzz_field(rng, (nlev, ny, nx)), fr.fuzz_field(rng, (nlev, ny, nx))
    w = fr.fuzz_field(rng, (ny, nx))
    p = rng.uniform(0.5, 2.0, (1, nlev)).astype(F)
    return t, q, w, p


SHAPE_PROGRAMS = {1: "mask(ifdef(t, 1.5) * w + q / p, w)",  # two fields, a plane, a level scalar
                  2: "ifdef(t, 1.5) * w + q / p, mask(t - q, w)"}


def shape_program(nout):
    return fexpr.compile(SHAPE_PROGRAMS[nout], fields=("t", "q"), planes=("w",), level_scalars=("p",))


# ----------------------------------------------------------------------------------------------- the launch shapes
# (a stacked output of two batches keeps the second one on the 16-byte grid where a batch has a multiple of four cells)
@pytest.mark.parametrize("nlev,ny,nx,off,nout,form", [
    (3, 5, 37, 0, 1, dict(form="vector", grid=1, tail=1)),   # 185 cells: 46 quads and a tail of one; levels 1, 2 at dword alignment
    (3, 5, 37, 1, 1, dict(form="scalar", grid=1, tail=0)),   # the same fields one float off the 16-byte grid
    (3, 5, 37, 0, 2, dict(form="scalar", grid=1, tail=0)),   # ... and the second output of a stacked pair, 555 floats behind the first
    (1, 4, 16, 0, 2, dict(form="vector", grid=1, tail=0)),   # one level
    (2, 1, 3, 0, 1, dict(form="scalar", grid=1, tail=0)),    # fewer than four cells
    (2, 17, 64, 0, 2, dict(form="vector", grid=2, tail=0)),  # 272 quads: two workgroups, the second one partly outside
    (4, 17, 63, 0, 2, dict(form="vector", grid=2, tail=3)),  # 1071 cells: 267 quads, a tail of three
    (2, 17, 64, 3, 2, dict(form="scalar", grid=5, tail=0)),  # five workgroups of the scalar form, the last one partly outside
], ids=lambda v: "-".join("%s" % x for x in v.values()) if isinstance(v, dict) else str(v))
def test_launch_shapes(gpu_ctx, nlev, ny, nx, off, nout, form):
    t, q, w, p = shape_inputs(nlev, ny, nx)
    prog = shape_program(nout)
    want, wfd = restated(prog, [t, q], [w], p)
    out = dev_out((nout, nlev, ny, nx) if nout > 1 else (nlev, ny, nx), off)
    got, fd = fexpr.evaluate(gpu_ctx, prog, [dev(t, off), dev(q, off)], [dev(w, off)], p, out=out)
    agree(got, fd, want, wfd, form)
    report = fexpr.last_fexpr_form(gpu_ctx)
    assert report["family"] == "fexpr" and {k: report[k] for k in form} == form, report
    assert (report["nlev"], report["ncode"], report["nregs"], report["nout"], report["partials"], report["tables"], report["bands"]) == \
        (nlev, prog.ncode, prog.nregs, nout, 0, 0, 1), report
    # one misplaced pointer is enough for the scalar form: the plane alone
    if form["form"] == "vector":
        fexpr.evaluate(gpu_ctx, prog, [dev(t), dev(q)], [dev(w, 2)], p)
        assert fexpr.last_fexpr_form(gpu_ctx)["form"] == "scalar"


def test_nothing_is_written_beside_the_outputs(gpu_ctx):
    nlev, ny, nx = 3, 5, 37
    t, q, w, p = shape_inputs(nlev, ny, nx)
    prog = shape_program(2)
    for off in (0, 1):
        import torch

        n = 2 * nlev * ny * nx
        room = torch.full((n + 16,), -4242.5, dtype=torch.float32, device="cuda")
        out = room[4 + off:4 + off + n].view(2, nlev, ny, nx)
        fexpr.evaluate(gpu_ctx, prog, [dev(t, off), dev(q, off)], [dev(w, off)], p, out=out)
        assert (room[:4 + off] == -4242.5).all().item() and (room[4 + off + n:] == -4242.5).all().item(), off


# ------------------------------------------------------------------------------------------------------ host memory
def test_host_memory_goes_in_bands(gpu_ctx, mifc_env):
    nlev, ny, nx = 16, 50, 256  # 2 * 16 + 1 + 16 planes of a row: 20 rows fit one MiB -- bands of 20, 20 and 10 rows
    rng = np.random.default_rng(5)
    t, q, w = fr.fuzz_field(rng, (nlev, ny, nx)), fr.fuzz_field(rng, (nlev, ny, nx)), fr.fuzz_field(rng, (ny, nx))
    p = rng.uniform(0.5, 2.0, (1, nlev)).astype(F)
    prog = fexpr.compile("t * (1 + 0.608 * q) / p + w", fields=("t", "q"), planes=("w",), level_scalars=("p",))
    whole, wfd = fexpr.evaluate(gpu_ctx, prog, [dev(t), dev(q)], [dev(w)], p)
    assert fexpr.last_fexpr_form(gpu_ctx)["bands"] == 1
    mifc_env("MIFC_FEXPR_CHUNK_MIB", 1)
    got, fd = fexpr.evaluate(gpu_ctx, prog, [t, q], [w], p)
    report = fexpr.last_fexpr_form(gpu_ctx)
    assert report["bands"] == 3 and report["form"] == "vector" and report["grid"] == 3 and report["tail"] == 0, report  # (the last band: 10 rows, 640 quads)
    assert same_bits(got, whole.cpu().numpy()) and np.array_equal(fd, wfd)
    agree(got, fd, *restated(prog, [t, q], [w], p), "host bands")
    # a width that is no multiple of four: every band has its own tail
    t3, q3, w3 = t[:, :, :255], q[:, :, :255], w[:, :255]
    got, fd = fexpr.evaluate(gpu_ctx, prog, [t3, q3], [w3], p)
    assert fexpr.last_fexpr_form(gpu_ctx)["bands"] == 3
    agree(got, fd, *restated(prog, [t3, q3], [w3], p), "host bands, ragged")


# -------------------------------------------------------------------------------- the chain of single-field calls
def chain_fields(n=3, shape=(3, 6, 29), seed=11):
    """Fields with undef, NaN, zeros, negatives and denormals."""
    rng = np.random.default_rng(seed)
    return [fr.fuzz_field(rng, shape) for _ in range(n)]


def levelwise(gpu_ctx, call, *batches):
    """A single-field call level by level on device tensors, SOME_DEFINED: the stacked result."""
    import torch

    out = []
    for k in range(batches[0].shape[0]):
        res = call(*[b[k] for b in batches])
        assert res is not None, gpu_ctx.last_error()
        out.append(res[0])
    return torch.stack(out)


def test_tv_program_is_the_chain_of_calls(gpu_ctx):
    t, q = chain_fields(2)
    dt, dq = dev(t), dev(q)
    prog = fexpr.compile("t*(1+0.608*q)", fields=("t", "q"))
    got, fd = fexpr.evaluate(gpu_ctx, prog, [dt, dq])
    a = levelwise(gpu_ctx, lambda x: gpu_ctx.constantOPERfield(3, 0.608, x), dq)
    b = levelwise(gpu_ctx, lambda x: gpu_ctx.constantOPERfield(1, 1.0, x), a)
    tv = levelwise(gpu_ctx, lambda x, y: gpu_ctx.fieldOPERfield(3, x, y), dt, b)
    assert same_bits(got.cpu().numpy(), tv.cpu().numpy()), "Tv"
    want, wfd = restated(prog, [t, q])
    agree(got, fd, want, wfd, "Tv against the restatement")
    assert 0 < int((want == U).sum()) < want.size


def test_rotation_pair_is_the_chain_of_calls(gpu_ctx):
    u, v = chain_fields(2, seed=12)
    rng = np.random.default_rng(13)
    ang = rng.uniform(0, 2 * np.pi, u.shape[1:])
    c, s = np.cos(ang).astype(F), np.sin(ang).astype(F)
    c[0, :3], s[1, :3] = U, np.nan
    du, dv, dc, ds = dev(u), dev(v), dev(c), dev(s)
    prog = fexpr.compile("u*c - v*s, u*s + v*c", fields=("u", "v"), planes=("c", "s"))
    got, fd = fexpr.evaluate(gpu_ctx, prog, [du, dv], [dc, ds])
    mul = lambda x, y: levelwise(gpu_ctx, lambda a, b: gpu_ctx.fieldOPERfield(3, a, b), x, y)  # noqa: E731
    cc, ss = dc.expand(u.shape[0], -1, -1).contiguous(), ds.expand(u.shape[0], -1, -1).contiguous()
    ur = levelwise(gpu_ctx, lambda a, b: gpu_ctx.fieldOPERfield(2, a, b), mul(du, cc), mul(dv, ss))
    vr = levelwise(gpu_ctx, lambda a, b: gpu_ctx.fieldOPERfield(1, a, b), mul(du, ss), mul(dv, cc))
    assert same_bits(got[0].cpu().numpy(), ur.cpu().numpy()) and same_bits(got[1].cpu().numpy(), vr.cpu().numpy())
    agree(got, fd, *restated(prog, [u, v], [c, s]), "rotation against the restatement")


def test_catalogue_functions_in_one_program_are_the_chain_of_calls(gpu_ctx):
    a, b = chain_fields(2, seed=14)
    da, db = dev(a), dev(b)
    prog = fexpr.compile("min(max(abs(a), 0.5), 3.0), log(a) + log10(a), pow10(exp(b) ** 0.37), (min(a, b) - max(a, b)) / b",
                         fields=("a", "b"))
    got, fd = fexpr.evaluate(gpu_ctx, prog, [da, db])
    assert fexpr.last_fexpr_form(gpu_ctx)["tables"] == 1
    g = gpu_ctx
    one = lambda f, x: levelwise(g, f, x)  # noqa: E731
    two = lambda f, x, y: levelwise(g, f, x, y)  # noqa: E731
    o0 = one(lambda x: g.minvalueFieldConst(x, 3.0), one(lambda x: g.maxvalueFieldConst(x, 0.5), one(g.absvalueField, da)))
    o1 = two(lambda x, y: g.fieldOPERfield(1, x, y), one(g.logField, da), one(g.log10Field, da))
    o2 = one(g.pow10Field, one(lambda x: g.powerField(x, float(F(0.37))), one(g.expField, db)))
    o3 = two(lambda x, y: g.fieldOPERfield(4, x, y), two(lambda x, y: g.fieldOPERfield(2, x, y), two(g.minvalueFields, da, db), two(g.maxvalueFields, da, db)), db)
    for o, chain in enumerate((o0, o1, o2, o3)):
        assert same_bits(got[o].cpu().numpy(), chain.cpu().numpy()), o
    # the flags against the restatement (the reference's own flags for these calls are not all updated); its transcendental
    # values are within an ulp of the device's, the places of its undefined cells are the device's
    want, wfd = restated(prog, [a, b])
    assert np.array_equal(fd, wfd) and np.array_equal(got.cpu().numpy() == U, want == U)


def test_field_and_constant_forms_are_the_chain_of_calls(gpu_ctx):
    (a,) = chain_fields(1, seed=15)
    da = dev(a)
    prog = fexpr.compile("a / 4, 4 / a, a - 2.5, 2.5 - a", fields=("a",))
    got, fd = fexpr.evaluate(gpu_ctx, prog, da)
    g = gpu_ctx
    chains = (levelwise(g, lambda x: g.fieldOPERconstant(4, x, 4.0), da), levelwise(g, lambda x: g.constantOPERfield(4, 4.0, x), da),
              levelwise(g, lambda x: g.fieldOPERconstant(2, x, 2.5), da), levelwise(g, lambda x: g.constantOPERfield(2, 2.5, x), da))
    for o, chain in enumerate(chains):
        assert same_bits(got[o].cpu().numpy(), chain.cpu().numpy()), o
    agree(got, fd, *restated(prog, [a]), "constants against the restatement")


# ----------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("seed", fr.FUZZ_SEEDS)
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_fuzz_programs_equal_the_restatement(gpu_ctx, seed, device):
    case = fr.fuzz_case(seed)
    prog = fexpr.Program.from_code(case["code"].tolist(), case["consts"], case["out_regs"], len(case["fields"]), len(case["planes"]),
                                   len(case["level_scalars"]))
    put = dev if device else np.ascontiguousarray
    got, fd = fexpr.evaluate(gpu_ctx, prog, [put(f) for f in case["fields"]], [put(p) for p in case["planes"]], case["level_scalars"], undef=case["undef"])
    want, wfd = restated(prog, case["fields"], case["planes"], case["level_scalars"], case["undef"])
    agree(got, fd, want, wfd.reshape(np.asarray(fd).shape), seed)  # every cell, bit for bit (a NaN matches a NaN), every flag


RANGE_FUZZ = [(klass, seed) for klass in ("huge", "tiny") for seed in fr.FUZZ_RANGE_SEEDS[klass]]


@pytest.mark.parametrize("klass,seed", RANGE_FUZZ)
def test_fuzz_programs_of_the_range_classes_equal_the_restatement(gpu_ctx, klass, seed):
    """The `huge` and `tiny` fuzz cases (tests/test_fexpr_cpu.py holds what they reach: overflow, underflow, NaN, an
    intermediate that equals 1e35 by arithmetic): device memory on the 16-byte grid, one float off it (the scalar form) and
    host memory; every cell bit for bit, every flag."""
    case = fr.fuzz_case(seed, klass=klass)
    prog = fexpr.Program.from_code(case["code"].tolist(), case["consts"], case["out_regs"], len(case["fields"]), len(case["planes"]),
                                   len(case["level_scalars"]))
    want, wfd = restated(prog, case["fields"], case["planes"], case["level_scalars"], case["undef"])
    for where, put in (("device", dev), ("off the grid", lambda a: dev(a, 1)), ("host", np.ascontiguousarray)):
        got, fd = fexpr.evaluate(gpu_ctx, prog, [put(f) for f in case["fields"]], [put(p) for p in case["planes"]], case["level_scalars"], undef=case["undef"])
        agree(got, fd, want, wfd.reshape(np.asarray(fd).shape), (klass, seed, where))
        form = fexpr.last_fexpr_form(gpu_ctx)["form"]
        if where == "off the grid" or (where == "device" and len(case["out_regs"]) == 1):  # (a stacked second output is off the grid by itself)
            assert form == ("scalar" if where == "off the grid" else "vector"), (klass, seed, where, form)


@pytest.mark.parametrize("name", fr.RANGE_TABLE_OPS)
def test_one_operation_over_the_range_operands(gpu_ctx, name):
    """One operation per program over every pair (for select and mask: triple) of the range operands: zeros of both signs,
    +-2^-149, FLT_MIN, +-FLT_MAX, 1e35 and both its neighbours, NaN, the infinities.  The interpreter computes and selects
    undef afterwards; the restatement tests first.  Bit for bit, in the vector and the scalar form and from host memory."""
    a, b, c = fr.range_operand_fields()
    table = fr.range_table_program(name)
    prog = fexpr.Program.from_code(table["code"].tolist(), table["consts"], table["out_regs"], 3, 0, 0)
    want, wfd = restated(prog, [a, b, c])
    for where, put in (("device", dev), ("off the grid", lambda x: dev(x, 1)), ("host", np.ascontiguousarray)):
        got, fd = fexpr.evaluate(gpu_ctx, prog, [put(a), put(b), put(c)])
        agree(got, fd, want, wfd.reshape(np.asarray(fd).shape), (name, where))


def ulps(a, b):
    """The distance of two float32 arrays in units in the last place (zeros of both signs are one number, infinity is the
    number after the largest finite one); NaN against NaN is 0, NaN against a number is huge."""
    def ordered(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(ordered(a) - ordered(b))
    an, bn = np.isnan(a), np.isnan(b)
    return np.where(an & bn, 0, np.where(an | bn, 1 << 40, d))


TRANSCENDENTAL = [("log(x)", seam_cases.log_arguments, None), ("log10(x)", seam_cases.log_arguments, None),
                  ("exp(x)", lambda: seam_cases.exp_arguments(False), None), ("pow10(x)", lambda: seam_cases.exp_arguments(True), None)]
TRANSCENDENTAL += [("x ** y", seam_cases.log_arguments, e) for e in seam_cases.POWER_EXPONENTS]
TRANSCENDENTAL += [("x ** y", lambda bases=bases: bases, e) for e, bases in seam_cases.power_pairs_near_switch()]


@pytest.mark.parametrize("expr,arguments,exponent", TRANSCENDENTAL, ids=["%s-%s" % (e, "" if x is None else x) for e, _, x in TRANSCENDENTAL])
def test_transcendental_operations_on_their_seams(gpu_ctx, expr, arguments, exponent):
    x = np.ascontiguousarray(arguments(), F)
    x = np.concatenate([x, [U]]).astype(F).reshape(1, 1, -1)
    scalars = {} if exponent is None else {"y": [F(exponent)]}
    prog = fexpr.compile(expr, fields=("x",), level_scalars=tuple(scalars))
    got, fd = fexpr.evaluate(gpu_ctx, prog, {"x": dev(x)}, level_scalars=scalars)
    want, wfd = restated(prog, [x], (), np.asarray(list(scalars.values()), F).reshape(len(scalars), 1))
    got, want = got.cpu().numpy(), want[0]
    assert np.array_equal(got == U, want == U) and np.array_equal(np.asarray(fd).ravel(), wfd.ravel())  # undefined cells and flags: exactly
    worst = int(ulps(got, want).max())
    assert worst <= 1, (expr, exponent, worst)


# ------------------------------------------------------------------------------------------------------- operands
def test_level_scalars_planes_four_outputs_and_an_overwritten_input(gpu_ctx):
    nlev, ny, nx = 4, 3, 10
    rng = np.random.default_rng(21)
    f = rng.uniform(1.0, 2.0, (nlev, ny, nx)).astype(F)
    pl = rng.uniform(1.0, 2.0, (ny, nx)).astype(F)
    scal = np.array([[1.0, 2.0, U, 4.0], [0.5, 0.25, 0.125, -1.0]], F)  # level 2 of the first scalar is undefined
    code = [("mul", 2, 0, L(0)),        # f * s0: level 2 all undef
            ("add", 3, 1, L(1)),        # the plane plus s1: shared by the levels, defined everywhere
            ("add", 0, 0, C(0)),        # the input register overwritten ...
            ("mul", 0, 0, 0),           # ... and read again
            ("select", 4, 2, 3, L(1)),  # s1 is never zero: register 2
            ("mov", 1, C(1))]           # a plane register overwritten with a constant
    prog = fexpr.Program.from_code(code, consts=[10.0, -3.5], out_regs=[2, 3, 0, 1], nfields=1, nplanes=1, nscalars=2)
    got, fd = fexpr.evaluate(gpu_ctx, prog, dev(f), [dev(pl)], scal)
    want, wfd = restated(prog, [f], [pl], scal)
    agree(got, fd, want, wfd, "operands")
    assert fd.tolist() == [[0, 0, 1, 0], [0] * 4, [0] * 4, [0] * 4] and (want[0, 2] == U).all()  # NONE_DEFINED at the level of the undefined scalar
    assert same_bits(want[1], np.broadcast_to(pl, f.shape) + scal[1].reshape(-1, 1, 1)) and same_bits(want[2], (f + F(10)) * (f + F(10)))
    assert (want[3] == F(-3.5)).all() and fexpr.last_fexpr_form(gpu_ctx)["nregs"] == 5
    # the out_regs order is the order of the outputs, and a register may be given twice
    prog2 = fexpr.Program.from_code(code, consts=[10.0, -3.5], out_regs=[0, 2, 0], nfields=1, nplanes=1, nscalars=2)
    got2, fd2 = fexpr.evaluate(gpu_ctx, prog2, dev(f), [dev(pl)], scal)
    agree(got2, fd2, want[[2, 0, 2]], wfd[[2, 0, 2]], "out_regs")
    # planes only, with the levels of the level scalars
    prog3 = fexpr.compile("c * p", planes=("c",), level_scalars=("p",))
    got3, fd3 = fexpr.evaluate(gpu_ctx, prog3, {}, {"c": dev(pl)}, {"p": scal[1]})
    agree(got3, fd3, *restated(prog3, [], [pl], scal[1:]), "planes only")


def test_the_limits_run(gpu_ctx):
    """12 inputs, 16 registers, 64 instructions, 16 constants, 4 level scalars, 4 outputs."""
    nlev, ny, nx = 2, 3, 9
    rng = np.random.default_rng(31)
    fields = [rng.uniform(0.5, 1.5, (nlev, ny, nx)).astype(F) for _ in range(8)]
    planes = [rng.uniform(0.5, 1.5, (ny, nx)).astype(F) for _ in range(4)]
    scal = rng.uniform(0.5, 1.5, (4, nlev)).astype(F)
    consts = rng.uniform(0.5, 1.5, 16).astype(F)
    names = ("add", "mul", "sub", "max")
    code = [(names[i % 4], 12 + i % 4, i % 12, (C(i % 16) if i % 3 else L(i % 4)) if i < 4 else 12 + (i + 1) % 4) for i in range(64)]
    prog = fexpr.Program.from_code(code, consts, [12, 13, 14, 15], 8, 4, 4)
    got, fd = fexpr.evaluate(gpu_ctx, prog, [dev(f) for f in fields], [dev(p) for p in planes], scal)
    agree(got, fd, *restated(prog, fields, planes, scal), "limits")
    report = fexpr.last_fexpr_form(gpu_ctx)
    assert (report["ncode"], report["nregs"], report["nout"]) == (64, 16, 4)


# ------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    import torch

    lib, c = gpu_ctx._lib, gpu_ctx._ctx
    nlev, ny, nx = 3, 5, 8
    cells, batch = ny * nx, nlev * ny * nx
    rng = np.random.default_rng(41)
    x = dev(fr.fuzz_field(rng, (2, nlev, ny, nx)))
    room = torch.zeros(batch + cells + batch, dtype=torch.float32, device="cuda")  # room of the test's own around the plane
    plane = room[batch:batch + cells].copy_(torch.from_numpy(fr.fuzz_field(rng, (cells,))))
    sentinel = -4242.5
    outs = torch.full((2, nlev, ny, nx), sentinel, dtype=torch.float32, device="cuda")
    good = np.array([[fr.OP["add"], 3, 0, 1, 0, 0, 0, 0], [fr.OP["mul"], 4, 3, 2, 0, 0, 0, 0]], np.uint8)

    def call(nx_=nx, ny_=ny, nlev_=nlev, code=good, out_ptrs=None, out_regs=(3, 4), plane_=0, memkind=1, sync=True, nconsts=0):
        ftab = (ctypes.c_void_p * 2)(x[0].data_ptr(), x[1].data_ptr())
        ptab = (ctypes.c_void_p * 1)(plane.data_ptr() if plane_ == 0 else plane_)
        o = (ctypes.c_void_p * 2)(*(out_ptrs or [outs[0].data_ptr(), outs[1].data_ptr()]))
        regs = np.array(out_regs, np.int32)
        fd = np.full(2 * max(nlev_, 1), 7, np.int32)
        rc = lib.mifc_fexpr_levels(c, nx_, ny_, nlev_, ctypes.addressof(ftab), 2, ctypes.addressof(ptab), 1, None, 0, None, nconsts, code.ctypes.data, len(code),
                                   regs.ctypes.data, 2, ctypes.addressof(o), fd.ctypes.data, float(U), memkind)
        if sync:
            torch.cuda.synchronize()
        return rc, gpu_ctx.last_error(), fd

    own = [outs[0].data_ptr(), outs[1].data_ptr()]
    bad_op, unset = good.copy(), good.copy()
    bad_op[1, 0], unset[1, 3] = 22, 9
    refusals = {
        "nlev 0": (dict(nlev_=0), "nlev < 1"),
        "negative nx": (dict(nx_=-1), "a negative nx or ny"),
        "2^31 cells": (dict(nx_=65536, ny_=32768), "more than 2^31 - 1 cells per level"),
        "bad memkind": (dict(memkind=7), "unknown memkind 7"),
        "unknown op": (dict(code=bad_op), "instruction 1: unknown op 22"),
        "unset register": (dict(code=unset), "instruction 1: register 9 is read before anything set it"),
        "unset output": (dict(out_regs=(3, 7)), "out_regs[1]: register 7 is read before anything set it"),
        "nconsts 17": (dict(nconsts=17), "nconsts 17 outside 0..16"),
        "null consts": (dict(nconsts=1), "a null pointer (fields, planes, level_scalars, consts, fres or fdefined_out)"),
        "null plane": (dict(plane_=None), "a null pointer (planes[0])"),
        "output is an input": (dict(out_ptrs=[own[0], x[1].data_ptr()]), "fres[1] overlaps fields[1]"),
        "output ends in an input": (dict(out_ptrs=[x[0].data_ptr() - 4 * (batch - 1), own[1]]), "fres[0] overlaps fields[0]"),
        "output begins in the plane": (dict(out_ptrs=[plane.data_ptr() + 4 * (cells - 1), own[1]]), "fres[0] overlaps planes[0]"),
        "output ends in the plane": (dict(out_ptrs=[plane.data_ptr() - 4 * (batch - 1), own[1]]), "fres[0] overlaps planes[0]"),
        "same output twice": (dict(out_ptrs=[own[0], own[0]]), "fres[0] overlaps fres[1]"),
        "outputs overlap": (dict(out_ptrs=[own[0], own[0] + 4 * (batch - 1)]), "fres[0] overlaps fres[1]"),
    }
    before = {"x": x.clone(), "room": room.clone()}
    for what, (kw, tail) in refusals.items():
        rc, err, fd = call(**kw)
        assert rc == 0 and err == "mifc_fexpr_levels: " + tail, (what, err)
        assert (outs == sentinel).all().item() and (fd == 7).all(), what
    assert torch.equal(x.view(torch.int32), before["x"].view(torch.int32)) and torch.equal(room.view(torch.int32), before["room"].view(torch.int32))
    # while a graph capture is open (nothing may synchronise inside it)
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with gpu_ctx.graph_capture() as g:
        gpu_ctx.zero_counts_enqueue(counts)
        rc, err, fd = call(sync=False)
    g.close()
    assert rc == 0 and err.startswith("mifc_fexpr_levels: ") and "capture" in err and (fd == 7).all() and (outs == sentinel).all().item()
    # an empty grid succeeds and writes flags only
    rc, err, fd = call(nx_=0)
    assert rc == 1 and (fd == fr.ALL_DEFINED).all() and (outs == sentinel).all().item(), err
    # afterwards the same call runs
    rc, err, fd = call()
    assert rc == 1 and err == "" and (fd != 7).all(), err
    xh = x.cpu().numpy()
    want, wfd = fr.interpret(good[:, :5].tolist(), [], [3, 4], [xh[0], xh[1]], [plane.cpu().numpy().reshape(ny, nx)])
    agree(outs, fd.reshape(2, nlev), want, wfd, "after the refusals")
