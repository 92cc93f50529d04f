"""Host-memory calls get the device homes of their fields from the context's scratch slots in call order
(csrc/mifc_ctx.h, mifc_host::Staging): a slot holds a map field in one entry point and a level batch, a bit table or
intermediates in the next, and only ever grows.  One long-lived Context therefore runs a mixed sequence of entry points
on numpy arrays, forwards and then backwards, and every result and flag must equal -- bit for bit -- what the same call
gives on a fresh Context with the same arguments as CUDA tensors.  GPU against GPU on purpose: it isolates staging from
arithmetic and needs no tolerance."""
import numpy as np
import pytest

import icing_cases as ic

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-4242.5)


class Host:
    """arguments as numpy arrays (inputs as they are: a held field is found by its address)"""

    host = True

    @staticmethod
    def inp(a):
        return a

    @staticmethod
    def io(a):
        return a.copy()


class Device:
    host = False

    @staticmethod
    def inp(a):
        import torch

        return torch.from_numpy(a).cuda()

    io = inp


def bits(x):
    x = x if isinstance(x, np.ndarray) else x.cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def results(*pairs):
    """[(field, flag or flags), ...] -> [(uint32 view, int32 array), ...]"""
    out = []
    for p in pairs:
        assert p is not None, "the call was refused"
        out.append((bits(p[0]), np.atleast_1d(np.asarray(p[1], dtype=np.int32))))
    return out


def make_steps():
    import mi_fieldcalc_amd as fc
    import mi_fieldcalc_amd.synth as synth

    # a small single field and a larger one (its width a multiple of 4: the one-launch kernels take it)
    sx, sy = 64, 48
    sxm, sym, _ = synth.grid_maps(sx, sy)
    su, sv = synth.wind(sx, sy, 11)
    su = synth.sprinkle_undef(su, 12, 0.02)
    bx, by = 360, 180
    xm, ym, fcor = synth.grid_maps(bx, by)
    z = synth.sprinkle_undef(synth.scalar_field(bx, by, 21), 22, 0.01)
    t = synth.thermo(bx, by, 23)[0]
    tx = synth.sprinkle_undef(t, 24, 0.01)
    rough = synth.scalar_field(bx, by, 25, noise=40.0)
    # vessel icing: 3 levels, one bathymetry for all of them
    icing = ic.make_inputs(97, 33, 51, nlev=3, specials=True)
    icing[10] = icing[10][0].copy()
    # ensembles
    members = [synth.sprinkle_undef(synth.scalar_field(120, 90, 100 + j), 200 + j, 0.01 if j % 5 == 0 else 0.0) for j in range(70)]
    member_flags = [fc.SOME_DEFINED if j % 5 == 0 else fc.ALL_DEFINED for j in range(70)]
    qmem = np.stack([np.stack([synth.scalar_field(80, 60, 1000 + 10 * j + l) for l in range(6)]) for j in range(20)])
    qmem[3, 2] = synth.sprinkle_undef(qmem[3, 2], 31, 0.05)

    def relvort_small(ctx, a):
        return results(ctx.relvort(a.inp(su), a.inp(sv), a.inp(sxm), a.inp(sym)))

    def qvector(ctx, a):
        return results(ctx.plevelqvector(a.inp(z), a.inp(t), a.inp(xm), a.inp(ym), a.inp(fcor), 500.0, 2),
                       ctx.plevelqvector(a.inp(z), a.inp(t), a.inp(xm), a.inp(ym), a.inp(fcor), 850.0, 3, fdefined=fc.ALL_DEFINED))

    def tfp(ctx, a):
        return results(ctx.thermalFrontParameter(a.inp(tx), a.inp(xm), a.inp(ym)))

    def qvector_held_xmapr(ctx, a):
        """the map ratio resident (it takes no slot), then released (it takes one again)"""
        if a.host:
            ctx.hold_field(xm)
        held = ctx.plevelqvector(a.inp(z), a.inp(t), a.inp(xm), a.inp(ym), a.inp(fcor), 700.0, 4)
        if a.host:
            ctx.release_field(xm)
        return results(held, ctx.plevelqvector(a.inp(z), a.inp(t), a.inp(xm), a.inp(ym), a.inp(fcor), 700.0, 4))

    def shapiro_in_place(ctx, a):
        f = a.io(rough)
        return results(ctx.shapiro2_filter(f, fdefined=fc.ALL_DEFINED, out=f))

    def neighbour_preloaded(ctx, a):
        """step 4: the interior cells that no block covers (here column nx - 3 and row ny - 3) keep what the caller's output held"""
        out = a.io(np.full((by, bx), SENTINEL, np.float32))
        r = results(ctx.neighbourFunctions(a.inp(rough), [2, 4], 1, out=out))
        assert (r[0][0] == bits(np.array([SENTINEL]))[0]).any()
        return r

    def icing_levels(ctx, a):
        return results(ctx.vesselIcing_levels("modstall", [a.inp(f) for f in icing], undef=ic.UNDEF, **ic.SCALARS))

    def mean_of_70(ctx, a):
        return results(ctx.meanValue([a.inp(m) for m in members], member_flags))

    def quantiles_in_chunks(ctx, a):
        # host memory: (20 + 3) * 4 bytes per cell, 4800 cells per level, 1 MiB at a time = 2 of the 6 levels per chunk
        return results(ctx.ensembleQuantiles(a.inp(qmem), [10, 50, 90], method="linear"))

    fused, passes = {"MIFC_FUSED2": None}, {"MIFC_FUSED2": "0"}
    chunks = {"MIFC_QUANTILE_CHUNK_MIB": "1"}
    return [
        ("relvort 64x48", {}, relvort_small),
        ("plevelqvector", fused, qvector),
        ("plevelqvector, pass by pass", passes, qvector),
        ("thermalFrontParameter", fused, tfp),
        ("plevelqvector, xmapr held", passes, qvector_held_xmapr),
        ("thermalFrontParameter, pass by pass", passes, tfp),
        ("shapiro2_filter in place", {}, shapiro_in_place),
        ("neighbourFunctions step 4", {}, neighbour_preloaded),
        ("vesselIcing_levels", {}, icing_levels),
        ("meanValue of 70", {}, mean_of_70),
        ("ensembleQuantiles in chunks", chunks, quantiles_in_chunks),
        ("relvort 64x48 again", {}, relvort_small),
    ]


def test_one_context_many_entry_points_both_orders(mifc_env):
    import mi_fieldcalc_amd as fc

    steps = make_steps()

    def run(ctx, step, args):
        name, env, fn = step
        for k, v in env.items():
            mifc_env(k, v)
        try:
            return fn(ctx, args)
        finally:
            for k in env:
                mifc_env(k, None)

    expected = {}
    for step in steps:
        with fc.Context(0) as fresh:
            expected[step[0]] = run(fresh, step, Device)

    with fc.Context(0) as ctx:
        for order, seq in (("forwards", steps), ("backwards", steps[::-1])):
            for step in seq:
                got = run(ctx, step, Host)
                want = expected[step[0]]
                assert len(got) == len(want)
                for k, ((gb, gf), (wb, wf)) in enumerate(zip(got, want)):
                    assert np.array_equal(gf, wf), (order, step[0], k, gf, wf)
                    assert gb.shape == wb.shape and np.array_equal(gb, wb), (order, step[0], k, int((gb != wb).sum()))
