"""Cases for the launch seams of the elementwise (mifc_ewise.hip), catalogue (mifc_pointwise.hip) and fused derived
(mifc_derived.hip) kernels: what depends on HOW a field is cut into workgroups, trips of a grid-stride loop, a tail
launch and partial counts, not on what a cell computes (tests/seam_cases.py has that).

A case is a dict in the form of tests/cases.py (op, args, nx, ny, fdefined, undef, label), so cases.run_cpu and
gpu_util.run_gpu take it as it is, plus what the case is named for:

  expect_flag    the output flag (ALL / SOME / NONE_DEFINED)
  expect_undef   sorted cell indices of the undefined output cells
  prefill        (kept-cell cases only) the per-cell pattern the output holds before the call

The undefined cells sit at stated positions of the launch shape the case is meant for (seam_cells): the first cell, the
last cell of the first trip, the first and the last cell of the last trip, every cell of the tail launch and the two ends
of the first and of the last workgroup.  Modes:

  some   input flag SOME_DEFINED, an undefined input value at every such position, spread over the inputs the operator
         tests -> SOME_DEFINED
  all    input flag ALL_DEFINED and, for the operators that read the saturation-pressure table, a temperature beyond the
         table (400 K; 700 K where the input is a potential temperature) at every such position: the only way a cell is
         counted without an input test -> SOME_DEFINED; the table-free operators -> ALL_DEFINED, nothing undefined
  none   every tested input undefined everywhere -> NONE_DEFINED, which holds only if the count equals n exactly
  clean  input flag SOME_DEFINED but no undefined value -> ALL_DEFINED, which holds only if the count is exactly 0

The constants below restate the launchers' (mifc_ewise.hip launch_ewise_op, mifc_pointwise.hip launch_pw, mifc_ctx.hip
partials_for); the GPU tests assert through mifc_last_pointwise_form that a case took the shape it was built for.
"""
import functools

import numpy as np

import mi_fieldcalc_amd.synth as synth
from cases import ALL_DEFINED, NONE_DEFINED, SOME_DEFINED, UNDEF

F = np.float32
LANES = 256                  # lanes of a workgroup
PARTIALS_MIN_BLOCKS = 2048   # from this many workgroups on the counts go through the partials buffer
SCALAR_MAX_BLOCKS = 4096     # grid cap of the one-cell-per-lane form
HOT_T, HOT_THETA = F(400.0), F(700.0)  # beyond the saturation table (tC >= 100) at every pressure the cases use


def trips(units, grid):
    """Trips of the busiest lane: units = float4 groups (vector form) or cells (scalar form)."""
    return -(-units // (grid * LANES))


def vector_grid(n, cap=None):
    g = max(1, -(-(n // 4) // LANES))
    return g if cap is None else min(g, cap)


def scalar_grid(n):
    return min(max(1, -(-n // LANES)), SCALAR_MAX_BLOCKS)


def seam_cells(n, grid, per_lane=4):
    """name -> cells, for a field of n cells on `grid` workgroups whose lanes take per_lane cells a trip (4: the vector
    form with its tail launch, 1: the scalar form)."""
    units = n // per_lane
    step = grid * LANES
    nt = trips(units, grid)
    main = units * per_lane
    cells = {"first": [0], "end_of_first_trip": [min(step, units) * per_lane - 1] if units else []}
    if nt > 1:
        cells["last_trip"] = [(nt - 1) * step * per_lane, main - 1]
    cells["tail"] = list(range(main, n)) if per_lane > 1 else []
    if units:
        wg = LANES * per_lane  # cells of one workgroup's trip
        cells["first_workgroup"] = [0, min(wg, main) - 1]
        last = min(grid, -(-units // LANES)) - 1
        cells["last_workgroup"] = [last * wg, min((last + 1) * wg, main) - 1]
    return cells


def flat_cells(cells):
    return sorted({c for group in cells.values() for c in group})


def shape_for(n):
    """(nx, ny) with nx * ny == n, ny > 1 and nx no multiple of 4 (cell % nx then changes inside a lane's four cells) and
    both >= 3 (the momentum coordinates want that); (n, 1) where n has no such factors."""
    for nx in (7, 3, 5, 9, 13, 11, 6, 257):
        if n % nx == 0 and n // nx >= 3:
            return nx, n // nx
    return n, 1


class _Fields:
    """The inputs of one grid, made when first asked for and then shared by every case on that grid: a case copies a field
    before it changes a cell (make_case), nobody writes to these."""

    def __init__(self, nx, ny):
        self.nx, self.ny, self.seed = nx, ny, 7001 * nx + ny
        self._made = {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        if name not in self._made:
            for key, a in self._make(name).items():
                self._made[key] = np.ascontiguousarray(a, F)
        return self._made[name]

    def _make(self, name):
        nx, ny, seed, shape = self.nx, self.ny, self.seed, (self.ny, self.nx)
        if name in ("u", "v"):
            u, v = synth.wind(nx, ny, seed)
            return dict(u=u, v=v)
        if name in ("t", "q", "ps"):
            t, q, ps = synth.thermo(nx, ny, seed)
            return dict(t=t, q=q, ps=ps)
        if name.startswith("theta_"):  # the potential temperature that gives t back at the pressure the operator uses
            p = {"theta_850": 850.0, "theta_700": 700.0, "theta_h": A + B * self.ps.astype(np.float64), "theta_a": self.p3.astype(np.float64)}[name]
            return {name: self.t * np.power(1000.0 / p, 287.0 / 1004.0)}
        if name == "rh":
            return dict(rh=synth.uniform(shape, seed + 9, 0.5, 110.0))
        if name == "td":
            return dict(td=(self.t - synth.uniform(shape, seed + 10, 0.0, 25.0).astype(F)).astype(F))
        if name == "p3":
            return dict(p3=synth.uniform(shape, seed + 11, 150.0, 1040.0))
        if name in ("xm", "ym", "fc"):
            xm, ym, fc = synth.grid_maps(nx, ny)
            return dict(xm=xm, ym=ym, fc=fc)
        raise AttributeError(name)


@functools.lru_cache(maxsize=4)
def fields(nx, ny):
    return _Fields(nx, ny)


A, B = 12.5, 0.73  # the hybrid level of tests/cases.py


class Spec:
    """op: the operator; build: fields -> args; tested: indices of the args whose cells the operator tests against undef;
    hot: (index of the temperature argument, the value beyond the table) or None for a table-free operator;
    counts: False where the operator leaves the flag alone."""

    def __init__(self, op, build, tested, hot=None, counts=True):
        self.op, self.build, self.tested, self.hot, self.counts = op, build, tested, hot, counts


# plevelhum numbering: 1,2 q->RH; 7,8 q->Td.  hlevelhum / alevelhum: 1,2 q->RH; 3,4 RH->q; 5,6 q->Td; 7,8 RH->Td.
# Odd computes start from T, even ones from theta.  alevelhum tests its pressure field only for compute 7 (:1429).
OPS = {
    "vectorabs": Spec("vectorabs", lambda f: [f.u, f.v], (0, 1)),
    "pleveltemp2": Spec("pleveltemp", lambda f: [f.theta_850, 850.0, "", 2], (0,), counts=False),
    "pleveltemp4": Spec("pleveltemp", lambda f: [f.t, 850.0, "", 4], (0,), hot=(0, HOT_T)),
    "hleveltemp3": Spec("hleveltemp", lambda f: [f.t, f.ps, A, B, "", 3], (0, 1)),
    "hleveltemp5": Spec("hleveltemp", lambda f: [f.theta_h, f.ps, A, B, "", 5], (0, 1), hot=(0, HOT_THETA)),
    "aleveltemp4": Spec("aleveltemp", lambda f: [f.t, f.p3, "", 4], (0, 1), hot=(0, HOT_T)),
    "plevelhum1": Spec("plevelhum", lambda f: [f.t, f.q, 700.0, "", 1], (0, 1), hot=(0, HOT_T)),
    "plevelhum2": Spec("plevelhum", lambda f: [f.theta_700, f.q, 700.0, "", 2], (0, 1), hot=(0, HOT_THETA)),
    "plevelhum7": Spec("plevelhum", lambda f: [f.t, f.q, 700.0, "", 7], (0, 1), hot=(0, HOT_T)),
    "plevelhum8": Spec("plevelhum", lambda f: [f.theta_700, f.q, 700.0, "", 8], (0, 1), hot=(0, HOT_THETA)),
    "hlevelhum1": Spec("hlevelhum", lambda f: [f.t, f.q, f.ps, A, B, "", 1], (0, 1, 2), hot=(0, HOT_T)),
    "hlevelhum3": Spec("hlevelhum", lambda f: [f.t, f.rh, f.ps, A, B, "", 3], (0, 1, 2), hot=(0, HOT_T)),
    "hlevelhum4": Spec("hlevelhum", lambda f: [f.theta_h, f.rh, f.ps, A, B, "", 4], (0, 1, 2), hot=(0, HOT_THETA)),
    "hlevelhum5": Spec("hlevelhum", lambda f: [f.t, f.q, f.ps, A, B, "", 5], (0, 1, 2), hot=(0, HOT_T)),
    "hlevelhum6": Spec("hlevelhum", lambda f: [f.theta_h, f.q, f.ps, A, B, "", 6], (0, 1, 2), hot=(0, HOT_THETA)),
    "alevelhum1": Spec("alevelhum", lambda f: [f.t, f.q, f.p3, "", 1], (0, 1), hot=(0, HOT_T)),
    "alevelhum2": Spec("alevelhum", lambda f: [f.theta_a, f.q, f.p3, "", 2], (0, 1), hot=(0, HOT_THETA)),
    "alevelhum7": Spec("alevelhum", lambda f: [f.t, f.rh, f.p3, "", 7], (0, 1, 2), hot=(0, HOT_T)),
    "alevelhum8": Spec("alevelhum", lambda f: [f.theta_a, f.rh, f.p3, "", 8], (0, 1), hot=(0, HOT_THETA)),
    "cvhum1": Spec("cvhum", lambda f: [f.t, f.rh, "kelvin", 1], (0, 1), hot=(0, HOT_T)),  # T, RH -> Td
    "cvhum4": Spec("cvhum", lambda f: [f.t, f.td, "", 4], (0, 1), hot=(0, HOT_T)),        # T, Td -> RH
    "momentumX": Spec("momentumXcoordinate", lambda f: [f.v, f.xm, f.fc, 2.0e-5], (0,)),
    "momentumY": Spec("momentumYcoordinate", lambda f: [f.u, f.ym, f.fc, -3.0e-5], (0,)),
    # hleveltemp with a compute outside 1..5: defined cells are left unwritten (FieldCalculations.cc:1080-1090)
    "hleveltemp0": Spec("hleveltemp", lambda f: [f.t, f.ps, A, B, "", 0], (0, 1)),
    "hleveltemp6": Spec("hleveltemp", lambda f: [f.t, f.ps, A, B, "", 6], (0, 1)),
    # the catalogue (mifc_pointwise.hip): one operator with the saturation table, one without any table
    "plevelthe1": Spec("plevelthe", lambda f: [f.t, f.rh, 850.0, 1], (0, 1), hot=(0, HOT_T)),
    "hlevelpressure": Spec("hlevelpressure", lambda f: [f.ps, A, B], (0,)),
}
# one operator per ewise_kernel instantiation and pressure source
TRIP_OPS = [k for k in OPS if k not in ("hleveltemp0", "hleveltemp6", "plevelthe1", "hlevelpressure", "hlevelhum1")]
KEEP_OPS = ["hleveltemp0", "hleveltemp6"]
SCALAR_OPS = ["hlevelhum5", "plevelthe1", "hlevelpressure"]
PARTIALS_OPS = ["vectorabs", "hlevelhum1", "plevelthe1", "hlevelpressure"]
CATALOGUE = ("plevelthe1", "hlevelpressure")


def make_case(key, nx, ny, mode, cells, tag):
    spec = OPS[key]
    f = fields(nx, ny)
    args = spec.build(f)
    n = nx * ny
    cells = np.asarray(sorted(set(cells)), np.int64)
    flag, undef_out = SOME_DEFINED, cells

    own = set()

    def writable(k):  # the fields are shared between cases: copy before the first write
        if k not in own:
            args[k] = args[k].copy()
            own.add(k)
        return args[k].reshape(-1)

    if mode == "some":
        for j, c in enumerate(cells):
            writable(spec.tested[j % len(spec.tested)])[c] = UNDEF
    elif mode == "none":
        for k in spec.tested:
            args[k] = np.full((ny, nx), UNDEF, F)
        undef_out = np.arange(n, dtype=np.int64)
    elif mode == "all":
        flag = ALL_DEFINED
        if spec.hot is None:
            undef_out = cells[:0]
        else:
            writable(spec.hot[0])[cells] = spec.hot[1]
    else:
        assert mode == "clean", mode
        undef_out = cells[:0]
    expect = ALL_DEFINED if undef_out.size == 0 else (NONE_DEFINED if undef_out.size == n else SOME_DEFINED)
    if not spec.counts:
        expect = flag  # the operator does not touch the flag
    return dict(op=spec.op, args=args, nx=nx, ny=ny, fdefined=flag, undef=UNDEF, label="launch-%s-%dx%d-%s-%s" % (key, nx, ny, tag, mode), key=key,
                mode=mode, expect_flag=expect, expect_undef=undef_out)


# ---- trips of the vector form under MIFC_EWISE_MAX_BLOCKS = 1 and 2
TRIP_N4 = {1: (1, 255, 256, 257, 512, 513, 1025), 2: (513, 1025)}  # with 2 workgroups: workgroup 0 takes one more trip than workgroup 1
TAILS = (0, 1, 2, 3)


def trip_shapes(blocks):
    return [(n4, tail) + shape_for(4 * n4 + tail) for n4 in TRIP_N4[blocks] for tail in TAILS]


def trip_cases(key, blocks):
    """Every n4 and tail with undefined inputs at the seams and with none; at two deep shapes with a tail (13 x 158 and 11 x 373
    cells) also the other modes."""
    out = []
    for n4, tail, nx, ny in trip_shapes(blocks):
        n = nx * ny
        cells = flat_cells(seam_cells(n, blocks))
        # `some` makes every tail cell undefined, which hides what a tail launch computes: `clean` runs at every shape too
        modes = ("some", "all", "none", "clean") if (n4, tail) in ((513, 2), (1025, 3)) else ("some", "clean")
        for mode in modes:
            case = make_case(key, nx, ny, mode, cells, "b%d-n4_%d+%d" % (blocks, n4, tail))
            case.update(n4=n4, tail=tail, blocks=blocks, trips=trips(n4, blocks))
            out.append(case)
    return out


# ---- kept cells: hleveltemp with compute 0 and 6
def keep_prefill(nx, ny):
    """Differs in every cell, and from undef and from anything hleveltemp computes."""
    return (F(-1000.0) - F(0.25) * np.arange(nx * ny, dtype=F)).reshape(ny, nx)


def keep_cases(key, blocks=1, per_lane=4):
    """Several trips with a tail under MIFC_EWISE_MAX_BLOCKS = blocks (per_lane 4), or the shape of the scalar form (1)."""
    out = []
    for nx, ny in ((7, 147), (5, 411)):  # n4 = 257 tail 1 (two trips on one workgroup); n4 = 513 tail 3 (three, or two on two)
        n = nx * ny
        if per_lane == 4 and trips(n // 4, blocks) < 2:
            continue
        grid = blocks if per_lane == 4 else scalar_grid(n)
        cells = flat_cells(seam_cells(n, grid, per_lane))
        for mode in ("some", "none", "clean"):
            case = make_case(key, nx, ny, mode, cells, "keep-%s" % ("b%d" % blocks if per_lane == 4 else "scalar"))
            case.update(prefill=keep_prefill(nx, ny), n4=n // 4, tail=n % 4, blocks=blocks, trips=trips(n // 4, blocks))
            out.append(case)
    return out


# ---- the scalar form (device pointers off the 16-byte grid)
SCALAR_SMALL = (7, 147)            # 1029 cells: 5 workgroups, one trip
SCALAR_LOOP = (9, 116537)          # 4096 * 256 + 257 = 1 048 833 cells: 257 lanes take a second trip


def scalar_cases(key, shape):
    nx, ny = shape
    n = nx * ny
    cells = flat_cells(seam_cells(n, scalar_grid(n), 1))
    return [make_case(key, nx, ny, mode, cells, "scalar") for mode in (("some", "all") if shape == SCALAR_LOOP else ("some", "all", "none", "clean"))]


# ---- counting by partials
PARTIALS_SHAPES = {
    "at": (2048, 1024),     # 2048 workgroups exactly: partials
    "below": (2048, 1023),  # 2046 workgroups: one atomic per workgroup
    "above": (2047, 1025),  # 2049 workgroups by partials and a 3-cell tail that counts by atomic next to them
}


def partials_cases(key, where):
    nx, ny = PARTIALS_SHAPES[where]
    n = nx * ny
    cells = flat_cells(seam_cells(n, vector_grid(n)))
    out = [make_case(key, nx, ny, mode, cells, "partials-" + where) for mode in ("some", "none")]
    for case in out:
        case.update(grid=vector_grid(n), partials=vector_grid(n) >= PARTIALS_MIN_BLOCKS, tail=n % 4)
    return out


def sequence_cases():
    """On one context, in this order: 4096 partials of 1024 each; then half as many workgroups with nothing undefined (a
    stale partial beyond the grid would show in the flag); then more workgroups than the buffer has held so far."""
    first = make_case("vectorabs", 4096, 1024, "none", [], "sequence1")
    second = make_case("vectorabs", 2048, 1024, "clean", [], "sequence2")
    n = 4100 * 1024
    third = make_case("vectorabs", 4100, 1024, "some", flat_cells(seam_cells(n, vector_grid(n))), "sequence3")
    return [first, second, third]
