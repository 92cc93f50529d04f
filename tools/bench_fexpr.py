#!/usr/bin/env python3
"""Field expressions over level batches: mifc_fexpr_levels on device-resident batches next to what it replaces -- the chain
of single-operation calls per level, the library's way before this entry -- and next to torch on the same tensors, which
is what vcumul.geopotential_height_hlevels does for its virtual temperature.  All in one process on the same arrays.
  tv        Tv = t * (1 + 0.608 * q): 3 operations, 2 fields in, 1 out
  rotate    the wind rotation of DESIGN.md 4.21 as field algebra: 6 operations, 2 fields and 2 planes in, 2 out; also
            mifc_vrotate_levels, the hand-written kernel for the same arrays (it rounds once per result, in double)
  theta     t * (1000 / p) ** 0.2857 with p one number per level: 3 operations, two of them per level only in the chain
  poly16    one 16-operation program over 2 fields: where instruction issue takes over from bandwidth
Per call: the wall time from a synchronised start to the synchronised end of each of ROUNDS calls after a warm-up call, the
calls alternating; median, minimum and spread (max - min).  The kernel time of the fused call is one timing section
(measurement build); of the chain, the sum of one timing section per level (two for poly16); of torch, two events around the expression.
The algorithmic bytes are 4 B per cell, level and batch read or written (planes once), and the rate they give as a share
of 8 TB/s; for the chain, what its calls move: 12 B per cell and two-field operation, 8 B per operation with a constant.

    python tools/bench_fexpr.py [--small]   -> one JSON line per call, one summary line per case
"""
import json
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch

import mi_fieldcalc_amd as fc
from mi_fieldcalc_amd import fexpr

ROUNDS = 7
ADD, SUB, MUL, DIV = 1, 2, 3, 4
UNDEF = float(fc.UNDEF)


def report(case, name, wall, kernel, nbytes, **more):
    r = {"case": case, "call": name, **more}
    if wall:
        r.update(bk.stats(wall, "wall_ms"))
    if kernel:
        r.update(bk.stats(kernel))
    gbps, share = bk.rate(nbytes, r.get("kernel_ms", r.get("wall_ms")))
    r.update(algorithmic_bytes=nbytes, TBps=round(gbps / 1e3, 3), share_of_peak=share)
    print(json.dumps(r), flush=True)
    return r


def faster(new, old, key):
    """Faster by more than the two spreads."""
    return bool(new[key + "_min"] + new[key + "_spread"] + old[key + "_spread"] < old[key + "_min"])


def run_case(ctx, case, fused, chain, torch_expr, fused_bytes, chain_bytes, check, extra=None, **shape):
    """fused(): the one call; chain(section): the single-operation calls, one section(part) per level; torch_expr(): torch."""
    calls = {
        "fexpr": (fused, bk.WALL_KERNEL),
        "chain of single-operation calls, wall": (lambda: chain(lambda part: part()), bk.WALL),
        "chain of single-operation calls, kernels": (chain, bk.SECTIONS),
        "torch, wall": (torch_expr, bk.WALL),
        "torch, events": (torch_expr, bk.EVENTS),
    }
    for name, entry in (extra or {}).items():
        calls[name] = entry[0]
    wall, kernel = bk.alternate(ctx, calls, ROUNDS)
    res = {}
    for name in calls:
        nbytes = fused_bytes if name.startswith(("fexpr", "torch")) else (chain_bytes if name.startswith("chain") else extra[name][1])
        res[name] = report(case, name, wall[name], kernel[name], nbytes, **shape)
    one, cw, ck = res["fexpr"], res["chain of single-operation calls, wall"], res["chain of single-operation calls, kernels"]
    fused()
    line = {"case": case, "launch": ctx._lib.mifc_last_fexpr_form().decode()}
    line.update(chain_kernel_over_fexpr_kernel=round(ck["kernel_ms"] / one["kernel_ms"], 2), chain_wall_over_fexpr_wall=round(cw["wall_ms"] / one["wall_ms"], 2),
                faster_in_kernel_time=faster(one, ck, "kernel_ms"), faster_in_call_time=faster(one, cw, "wall_ms"),
                torch_events_over_fexpr_kernel=round(res["torch, events"]["kernel_ms"] / one["kernel_ms"], 2),
                torch_wall_over_fexpr_wall=round(res["torch, wall"]["wall_ms"] / one["wall_ms"], 2), same_bits_as_chain=check())
    for name in extra or {}:
        line[name.split(",")[0] + "_kernel_over_fexpr_kernel"] = round(res[name]["kernel_ms"] / one["kernel_ms"], 3)
        line[name.split(",")[0] + "_share_of_peak"] = res[name]["share_of_peak"]
    line["fexpr_share_of_peak"] = one["share_of_peak"]
    print(json.dumps(line), flush=True)


def same(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2027)
    cells, batch = ny * nx, nlev * ny * nx
    shape = dict(nx=nx, ny=ny, nlev=nlev)
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        t = (torch.randn((nlev, ny, nx), generator=gen, device=dev) * 15 + 260).contiguous()
        q = (torch.rand((nlev, ny, nx), generator=gen, device=dev) * 0.02).contiguous()
        u, v = (torch.randn((2, nlev, ny, nx), generator=gen, device=dev) * 10).contiguous()
        angle = torch.rand((ny, nx), generator=gen, device=dev) * 6.2831853
        c, s = torch.cos(angle).contiguous(), torch.sin(angle).contiguous()
        out, ref = torch.empty((2, nlev, ny, nx), device=dev), torch.empty((2, nlev, ny, nx), device=dev)
        tmp = torch.empty((3, ny, nx), device=dev)
        undef = torch.tensor(UNDEF, device=dev)

        # ---- Tv
        prog = fexpr.compile("t*(1+0.608*q)", fields=("t", "q"))

        def tv_chain(section):
            for k in range(nlev):
                def level(k=k):
                    ctx.constantOPERfield(MUL, 0.608, q[k], out=tmp[0])
                    ctx.constantOPERfield(ADD, 1.0, tmp[0], out=tmp[1])
                    ctx.fieldOPERfield(MUL, t[k], tmp[1], out=ref[0, k])
                section(level)

        def tv_torch():
            bad = (t == UNDEF) | (q == UNDEF) | torch.isnan(t) | torch.isnan(q)
            return torch.where(bad, undef, t * (1 + 0.608 * q))

        run_case(ctx, "tv", lambda: fexpr.evaluate(ctx, prog, [t, q], out=out[0]), tv_chain, tv_torch, 12 * batch, (8 + 8 + 12) * batch,
                 lambda: same(out[0], ref[0]), **shape)

        # ---- the rotation pair
        prog_r = fexpr.compile("u*c - v*s, u*s + v*c", fields=("u", "v"), planes=("c", "s"))

        def rot_chain(section):
            for k in range(nlev):
                def level(k=k):
                    ctx.fieldOPERfield(MUL, u[k], c, out=tmp[0])
                    ctx.fieldOPERfield(MUL, v[k], s, out=tmp[1])
                    ctx.fieldOPERfield(SUB, tmp[0], tmp[1], out=ref[0, k])
                    ctx.fieldOPERfield(MUL, u[k], s, out=tmp[0])
                    ctx.fieldOPERfield(MUL, v[k], c, out=tmp[1])
                    ctx.fieldOPERfield(ADD, tmp[0], tmp[1], out=ref[1, k])
                section(level)

        def rot_torch():
            bad = (u == UNDEF) | (v == UNDEF) | torch.isnan(u) | torch.isnan(v) | ((c == UNDEF) | (s == UNDEF) | torch.isnan(c) | torch.isnan(s))[None]
            return torch.where(bad, undef, u * c - v * s), torch.where(bad, undef, u * s + v * c)

        pair, rotated = torch.stack([u, v]), torch.empty((2, nlev, ny, nx), device=dev)
        rot_bytes = 16 * batch + 8 * cells
        run_case(ctx, "rotate", lambda: fexpr.evaluate(ctx, prog_r, [u, v], [c, s], out=out), rot_chain, rot_torch, rot_bytes, 72 * batch,
                 lambda: same(out, ref), extra={"vrotate_levels, the hand-written kernel": ((lambda: ctx.vrotate_levels(pair, c, s, out=rotated), bk.WALL_KERNEL), rot_bytes)},
                 **shape)
        del pair, rotated

        # ---- potential temperature on pressure levels
        p = np.linspace(10.0, 1000.0, nlev).astype(np.float32)
        prog_t = fexpr.compile("t * (1000/p)**0.2857", fields=("t",), level_scalars=("p",))
        factor = (np.float32(1000.0) / p).astype(np.float64) ** float(np.float32(0.2857))  # per level on the host, as a caller does today
        dp = torch.from_numpy(p).to(dev)[:, None, None]

        def th_chain(section):
            for k in range(nlev):
                section(lambda k=k: ctx.fieldOPERconstant(MUL, t[k], float(np.float32(factor[k])), out=ref[0, k]))

        def th_torch():
            return torch.where((t == UNDEF) | torch.isnan(t), undef, t * (1000.0 / dp) ** 0.2857)

        run_case(ctx, "theta", lambda: fexpr.evaluate(ctx, prog_t, [t], level_scalars=[p], out=out[0]), th_chain, th_torch, 8 * batch, 8 * batch,
                 lambda: bool(((out[0] - ref[0]).abs() <= 1e-6 * ref[0].abs()).all().item()), **shape)

        # ---- sixteen operations: Horner steps over two fields
        steps = 8
        expr = "q"
        for i in range(steps):
            expr = "(%s) * %s + %d.5" % (expr, "q" if i % 2 else "u", i)
        prog_p = fexpr.compile(expr, fields=("u", "q"))
        assert prog_p.ncode == 2 * steps

        def poly_chain(section):
            for k in range(nlev):
                for half in (0, 1):  # (a timing section holds eight launches)
                    def part(k=k, half=half):
                        for i in range(half * steps // 2, (half + 1) * steps // 2):
                            ctx.fieldOPERfield(MUL, tmp[2] if i else q[k], q[k] if i % 2 else u[k], out=tmp[i % 2])
                            ctx.fieldOPERconstant(ADD, tmp[i % 2], i + 0.5, out=ref[0, k] if i == steps - 1 else tmp[2])
                    section(part)

        def poly_torch():
            cur = q
            for i in range(steps):
                cur = cur * (q if i % 2 else u) + (i + 0.5)
            return torch.where((u == UNDEF) | (q == UNDEF) | torch.isnan(u) | torch.isnan(q), undef, cur)

        run_case(ctx, "poly16", lambda: fexpr.evaluate(ctx, prog_p, [u, q], out=out[0]), poly_chain, poly_torch, 12 * batch, steps * (12 + 8) * batch,
                 lambda: same(out[0], ref[0]), **shape)


if __name__ == "__main__":
    main()
