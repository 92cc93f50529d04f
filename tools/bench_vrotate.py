#!/usr/bin/env python3
"""Vector pairs of level batches rotated: mifc_vrotate_levels and mifc_hinterp_vector_levels on device-resident batches,
next to what they replace and to a same-bytes yardstick, all in one process on the same data.
  rotate    one pair 1440x720x137 (then 2 and 4 pairs): vrotate_levels, fields flagged SOME_DEFINED (every value tested) and
            ALL_DEFINED; the field-algebra route it replaces, six fieldOPERfield calls per level; the fused derived batch
            writing ff and dd from u and v, the library's level-batch kernel with the same 16 B per cell and level.
  chunks    vrotate_levels with the levels per workgroup forced (MIFC_HINTERP_LEVEL_CHUNK) on a small and on the large grid,
            next to the rule of vrotate_plan.
  regrid    one pair to a 2000x1000 grid of rotated positions, section: 2000 points -- hinterp_vector_levels against the two
            calls it fuses, hinterp_levels of both components and then vrotate_levels; bilinear and bicubic.
Per call: the wall time from a synchronised start to the synchronised end of each of ROUNDS calls after a warm-up call, the
calls alternating; its median, minimum and spread (max - min); for the library's single calls also the kernel time (HIP
events around the launches, measurement build); the algorithmic bytes -- 16 B per cell, level and pair plus the two
coefficient planes once -- and the rate they give, as a share of 8 TB/s.

    python tools/bench_vrotate.py [--small]   -> one JSON line per call
"""
import json
import os
import sys

import benchkit as bk  # first: the path and the measurement build (mifc_timing_*)
import numpy as np
import torch
from bench_hinterp import rotated_grid

import mi_fieldcalc_amd as fc

ROUNDS = 9
ADD, SUB, MUL = 1, 2, 3
SINGLE, SEVERAL = bk.WALL_KERNEL, bk.WALL  # one timing section holds the call's launches, or the wall time alone


def report(case, name, wall, kernel, nbytes, **more):
    r = {"case": case, "call": name, **bk.stats(wall, "wall_ms"), **more}
    if kernel:
        r.update(bk.stats(kernel))
    if nbytes:
        gbps, share = bk.rate(nbytes, r.get("kernel_ms", r["wall_ms"]))
        r.update(algorithmic_bytes=nbytes, TBps=round(gbps / 1e3, 3), share_of_peak=share)
    print(json.dumps(r), flush=True)
    return r


def rotate_bytes(npairs, nlev, cells):
    return 16 * npairs * nlev * cells + 8 * cells


def algebra(ctx, u, v, c, s, out_u, out_v, tmp):
    """The route the entry replaces: per level c*u, s*v, their difference, s*u, c*v, their sum -- every product rounded to float."""
    for k in range(u.shape[0]):
        ctx.fieldOPERfield(MUL, c, u[k], out=tmp[0])
        ctx.fieldOPERfield(MUL, s, v[k], out=tmp[1])
        ctx.fieldOPERfield(SUB, tmp[0], tmp[1], out=out_u[k])
        ctx.fieldOPERfield(MUL, s, u[k], out=tmp[0])
        ctx.fieldOPERfield(MUL, c, v[k], out=tmp[1])
        ctx.fieldOPERfield(ADD, tmp[0], tmp[1], out=out_v[k])


def case_rotate(ctx, pairs, c, s, out):
    npairs, _, nlev, ny, nx = pairs.shape
    cells = ny * nx
    every = np.zeros((npairs, 2, nlev), np.int32)  # ALL_DEFINED
    for np_ in (1, 2, 4):
        if np_ > npairs:
            break
        calls = {
            "vrotate_levels": (lambda n=np_: ctx.vrotate_levels(pairs[:n], c, s, out=out[:n]), SINGLE),
            "vrotate_levels, ALL_DEFINED": (lambda n=np_: ctx.vrotate_levels(pairs[:n], c, s, fdefined_in=every[:n], fdef_rot=fc.ALL_DEFINED, out=out[:n]), SINGLE),
        }
        if np_ == 1:
            u, v = pairs[0, 0], pairs[0, 1]
            tmp = torch.empty((2, ny, nx), device=u.device, dtype=torch.float32)
            ps = torch.full((ny, nx), 1000.0, device=u.device, dtype=torch.float32)
            yard = {"ff": out[0, 0], "dd": out[0, 1]}
            calls["derived batch ff + dd (16 B per cell)"] = (lambda: ctx.hlevel_derived_batch(u, v, None, None, ps, None, None, ff=True, dd=True, out=yard), SINGLE)
            calls["derived batch ff (12 B per cell)"] = (lambda: ctx.hlevel_derived_batch(u, v, None, None, ps, None, None, ff=True, out={"ff": out[0, 0]}), SINGLE)
            calls["field algebra, 6 calls per level"] = (lambda: algebra(ctx, u, v, c, s, out[0, 0], out[0, 1], tmp), SEVERAL)
        wall, kernel = bk.alternate(ctx, calls, ROUNDS)
        res = {}
        for name in calls:
            nbytes = (12 if "12 B" in name else 16) * nlev * cells if name.startswith("derived") else (
                72 * nlev * cells if name.startswith("field") else rotate_bytes(np_, nlev, cells))
            res[name] = report("rotate", name, wall[name], kernel[name], nbytes, npairs=np_, nx=nx, ny=ny, nlev=nlev)
        print(json.dumps({"case": "rotate", "npairs": np_, "launch": ctx.last_vrotate_form()}), flush=True)
        if np_ == 1:
            mine = res["vrotate_levels"]
            print(json.dumps({"case": "rotate", "algebra_wall_over_vrotate_wall": round(res["field algebra, 6 calls per level"]["wall_ms"] / mine["wall_ms"], 1),
                              "vrotate_kernel_over_yardstick_kernel": round(mine["kernel_ms"] / res["derived batch ff + dd (16 B per cell)"]["kernel_ms"], 3)}),
                  flush=True)


def case_chunks(ctx, pairs, c, s, out, label):
    _, _, nlev, ny, nx = pairs.shape
    calls, order = {}, ["rule"] + [ch for ch in (1, 2, 4, 8, 16, 32, 64, nlev) if ch <= nlev]

    def forced(chunk):
        if chunk == "rule":
            os.environ.pop("MIFC_HINTERP_LEVEL_CHUNK", None)
        else:
            os.environ["MIFC_HINTERP_LEVEL_CHUNK"] = str(chunk)
        ctx.reload_env()
        ctx.vrotate_levels(pairs[:1], c, s, out=out[:1])

    for chunk in order:
        calls["chunk %s" % chunk] = (lambda chunk=chunk: forced(chunk), SINGLE)
    wall, kernel = bk.alternate(ctx, calls, ROUNDS)
    for chunk in order:
        forced(chunk)
        report("chunks " + label, "chunk %s" % chunk, wall["chunk %s" % chunk], kernel["chunk %s" % chunk], rotate_bytes(1, nlev, ny * nx), nx=nx, ny=ny,
               nlev=nlev, launch=ctx.last_vrotate_form())
    forced("rule")


def case_sample(ctx, case, pair, x, y, c, s):
    _, nlev, ny, nx = pair.shape
    where = tuple(x.shape)
    fused = torch.empty((2, nlev) + where, device=pair.device, dtype=torch.float32)
    sampled, rotated = torch.empty_like(fused), torch.empty_like(fused)
    npos = x.numel()

    def two_calls(method):
        _, fd = ctx.hinterp_levels(pair, x, y, method, out=sampled)
        ctx.vrotate_levels(sampled.view(2, nlev, 1, npos), c.view(1, npos), s.view(1, npos), fdefined_in=fd, out=rotated.view(2, nlev, 1, npos))

    calls = {}
    for method in ("bilinear", "bicubic"):
        calls["hinterp_vector_levels %s" % method] = (lambda m=method: ctx.hinterp_vector_levels(pair, x, y, c, s, m, out=fused), SINGLE)
        calls["hinterp_levels + vrotate_levels %s" % method] = (lambda m=method: two_calls(m), SINGLE)
    wall, kernel = bk.alternate(ctx, calls, ROUNDS)
    res = {name: report(case, name, wall[name], kernel[name], 0, nx=nx, ny=ny, nlev=nlev, npos=npos) for name in calls}
    for method in ("bilinear", "bicubic"):
        one, two = res["hinterp_vector_levels %s" % method], res["hinterp_levels + vrotate_levels %s" % method]
        print(json.dumps({"case": case, "method": method, "two_calls_kernel_over_fused_kernel": round(two["kernel_ms"] / one["kernel_ms"], 3),
                          "two_calls_wall_over_fused_wall": round(two["wall_ms"] / one["wall_ms"], 3)}), flush=True)
    assert torch.equal(fused.view(torch.int32), rotated.view(torch.int32))  # (the last method's results: the same bits)


def main():
    nx, ny, nlev = bk.shape(sys.argv)
    gx, gy, npts, npairs, q = bk.shape(sys.argv, (2000, 1000, 2000, 4, 4), (500, 250, 500, 2, 2))
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(2026)
    with fc.Context(0) as ctx:
        ctx.use_torch_stream()
        pairs = torch.randn((npairs, 2, nlev, ny, nx), generator=gen, device=dev, dtype=torch.float32) * 10
        out = torch.empty_like(pairs)
        angle = torch.rand((ny, nx), generator=gen, device=dev) * 6.2831853
        c, s = torch.cos(angle).contiguous(), torch.sin(angle).contiguous()
        case_rotate(ctx, pairs, c, s, out)
        case_chunks(ctx, pairs, c, s, out, "%dx%d" % (nx, ny))
        case_chunks(ctx, pairs[:, :, :, :ny // q, :nx // q].contiguous(), c[:ny // q, :nx // q].contiguous(), s[:ny // q, :nx // q].contiguous(),
                    out[:, :, :, :ny // q, :nx // q].contiguous(), "%dx%d" % (nx // q, ny // q))
        case_chunks(ctx, pairs[:, :, :, :ny // (4 * q), :nx // (4 * q)].contiguous(), c[:ny // (4 * q), :nx // (4 * q)].contiguous(),
                    s[:ny // (4 * q), :nx // (4 * q)].contiguous(), out[:, :, :, :ny // (4 * q), :nx // (4 * q)].contiguous(),
                    "%dx%d" % (nx // (4 * q), ny // (4 * q)))
        del out
        x, y = rotated_grid(nx, ny, gx, gy, dev)
        angle = torch.rand(tuple(x.shape), generator=gen, device=dev) * 6.2831853
        case_sample(ctx, "regrid", pairs[0], x, y, torch.cos(angle).contiguous(), torch.sin(angle).contiguous())
        print(json.dumps({"case": "regrid", "launch": ctx.last_hinterp_form()}), flush=True)
        t = torch.linspace(0, 1, npts, device=dev)
        xs = ((0.02 + 0.96 * t) * (nx - 1) + torch.randn(npts, generator=gen, device=dev)).clamp(0, nx - 1).contiguous()
        ys = ((0.5 + 0.4 * torch.sin(6.28 * t)) * (ny - 1) + torch.randn(npts, generator=gen, device=dev)).clamp(0, ny - 1).contiguous()
        angle = torch.rand(npts, generator=gen, device=dev) * 6.2831853
        case_sample(ctx, "section", pairs[0], xs, ys, torch.cos(angle).contiguous(), torch.sin(angle).contiguous())
        print(json.dumps({"case": "section", "launch": ctx.last_hinterp_form()}), flush=True)


if __name__ == "__main__":
    main()
