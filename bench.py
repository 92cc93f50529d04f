#!/usr/bin/env python3
"""Headline benchmark: Mcells/s of fused relative vorticity + divergence on a
1440x720x137 float32 grid (BASELINE.json), one process per GPU.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full --dump-outputs DIR
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one pass of the fused kernel over one batch of 137 levels (one
ensemble member) that is already resident in HBM.  With N GPUs every rank owns
one such member (members are independent: no data-path collective, weak
scaling); `value` = cells processed by all ranks / max-over-ranks wall time.

A plain run does only what `value` needs: it sets the batch up (placement
search included), warms up, times the K steps and prints the JSON line, whose
roofline comes from the HIP events around those K steps.  --dump-outputs DIR
writes what the last timed step computed, as float32 .npy files (rank 0's
member): rvort_levels / diverg_levels hold whole levels DUMP_LEVELS, and
rvort_sample / diverg_sample a fixed, seeded sample of DUMP_SAMPLE cells of
the whole batch (flat [level][row][column] indices from DUMP_SEED), 42 MB in
all.  The inputs are generated from a fixed seed, so two builds can be
compared file for file.

--full adds the checks and side measurements below (each can still be
switched off on its own with the matching --no-* option):
  verified     : before anything is timed, sampled levels of the GPU's rvort and
                 diverg are compared bit for bit with the reference CPU path (the
                 same calls cpu_baseline times) -- both the ALL_DEFINED fast path
                 and the tested SOME_DEFINED variant; a mismatch aborts the run;
  roofline.per_launch_event_pairs_ms: every launch between its own pair of
                 HIP events, in a run of its own after the timed steps;
  roofline_as_allocated: the same launch on four plain allocations;
  check_variant: the same launch with per-cell undefined tests and per-level
                 counts (SOME_DEFINED inputs), timed right after the headline;
  cpu_baseline : the reference CPU path (oracle/_ref, compiled from the
                 reference's own sources; or the bit-exact restatement if that
                 library is not present) calling relvort then divergence per
                 level on this host, on a bounded sample.
Both kinds of run report `roofline`: algorithmic bytes (16 B/cell + map
factors once per batch) over the kernel's average duration measured with HIP
events on the launch stream, against the 8 TB/s HBM3E peak.
The CPU library is only ever the checker / the reported baseline: nothing inside a
timed region touches it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

NX, NY, NLEV = 1440, 720, 137
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md
SEED = 0x5EED0000 + 3000
DUMP_LEVELS = (0, NLEV // 2, NLEV - 1)
DUMP_SAMPLE = 1 << 21
DUMP_SEED = 0x5EED0000 + 3001


def algorithmic_bytes(nx, ny, nlev):
    # read u,v + write rvort,diverg = 16 B/cell, xmapr+ymapr once per batch
    return nx * ny * nlev * 16 + 2 * nx * ny * 4


def _cpu_library():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cpulib

    which = "ref" if cpulib.available("ref") else "oracle"
    return cpulib, which, cpulib.CpuLib(which)


def verify_against_cpu(levels, u_levels, v_levels, xm, ym, rv_levels, dg_levels, flag, counts=None):
    """Checker leg (never timed): the reference CPU path on the sampled levels, relvort then
    divergence like cpu_baseline(); the GPU's results must equal it bit for bit (a NaN matches a
    NaN: its payload is an ISA property).  Returns the name of the CPU library used."""
    import numpy as np

    cpulib, which, lib = _cpu_library()

    def same(a, b):
        an, bn = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn]))

    for k, l in enumerate(levels):
        for name, got in (("relvort", rv_levels[k]), ("divergence", dg_levels[k])):
            ok, expect, f = lib.call(name, NX, NY, u_levels[k], v_levels[k], xm, ym, fdefined=flag)
            if not (ok and same(got, expect)):
                raise SystemExit("bench.py: GPU %s of level %d differs from the CPU reference path (%s) -- nothing is timed" % (name, l, which))
            if counts is not None:
                import mi_fieldcalc_amd as fc

                if fc.classify(int(counts[k]), NX * NY - 2 * NX) != f:
                    raise SystemExit("bench.py: flag of level %d differs from the CPU reference path" % l)
    return "reference" if which == "ref" else "port"


def cpu_baseline(seconds_target=10.0):
    """Reference CPU path timed on this host.  The oracle / reference build is used
    here ONLY as the reported baseline, never on the product path."""
    import concurrent.futures as cf

    import numpy as np

    import mi_fieldcalc_amd.synth as synth

    cpulib, which, lib = _cpu_library()
    kind = "reference" if which == "ref" else "port"
    nlev = NLEV
    xm, ym, _ = synth.grid_maps(NX, NY)
    u, v = synth.wind(NX, NY, SEED, nlev=nlev)
    n = NX * NY
    relvort, diverg = lib.raw("relvort"), lib.raw("divergence")
    import ctypes

    def one_level(l, out):
        fd = ctypes.c_int(0)  # ALL_DEFINED, like the GPU run
        relvort(NX, NY, u[l].ctypes.data, v[l].ctypes.data, xm.ctypes.data, ym.ctypes.data, out.ctypes.data, ctypes.addressof(fd), 1e35)
        fd = ctypes.c_int(0)
        diverg(NX, NY, u[l].ctypes.data, v[l].ctypes.data, xm.ctypes.data, ym.ctypes.data, out.ctypes.data, ctypes.addressof(fd), 1e35)

    out = np.empty((NY, NX), np.float32)
    for l in range(3):  # warm-up
        one_level(l, out)
    t0 = time.perf_counter()
    passes = 0
    while True:
        for l in range(nlev):
            one_level(l, out)
        passes += 1
        if time.perf_counter() - t0 >= seconds_target:
            break
    dt = time.perf_counter() - t0
    res = {
        "value": round(n * nlev * passes / dt / 1e6, 1),
        "unit": "Mcells/s",
        "cores": 1,
        "kind": kind,
        "sample": "%d passes over %d levels of 1440x720 (relvort then divergence per level, ALL_DEFINED, default build: OpenMP off), %.1f s" % (passes, nlev, dt),
    }
    extras = {"host_cpus": os.cpu_count()}
    try:
        with open("/proc/cpuinfo") as f:
            extras["cpu_model"] = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "unknown")
    except OSError:
        pass
    # whole host: every hardware thread busy -- the levels are cut into row pieces (serial reference calls on
    # sub-fields that overlap by the two rows a stencil needs; ctypes releases the GIL), 2 pieces per level on a
    # 256-thread host = 274 tasks
    workers = os.cpu_count() or 1
    pieces = max(1, -(-workers // nlev))
    rows = -(-(NY - 2) // pieces)
    tasks = []
    for l in range(nlev):
        for k in range(pieces):
            j0 = k * rows  # piece = computed rows j0+1 .. j0+rows, handed to the reference as a field of rows j0 .. j0+rows+1
            nyp = min(rows + 2, NY - j0)
            if nyp >= 3:
                tasks.append((l, j0, nyp))
    outs = [np.empty((rows + 2, NX), np.float32) for _ in range(workers)]

    def piece(w):
        for l, j0, nyp in tasks[w::workers]:
            fd = ctypes.c_int(0)
            relvort(NX, nyp, u[l, j0:].ctypes.data, v[l, j0:].ctypes.data, xm[j0:].ctypes.data, ym[j0:].ctypes.data, outs[w].ctypes.data,
                    ctypes.addressof(fd), 1e35)
            fd = ctypes.c_int(0)
            diverg(NX, nyp, u[l, j0:].ctypes.data, v[l, j0:].ctypes.data, xm[j0:].ctypes.data, ym[j0:].ctypes.data, outs[w].ctypes.data,
                   ctypes.addressof(fd), 1e35)

    with cf.ThreadPoolExecutor(workers) as ex:
        list(ex.map(piece, range(workers)))  # warm-up
        t0 = time.perf_counter()
        passes = 0
        while time.perf_counter() - t0 < seconds_target / 2:
            list(ex.map(piece, range(workers)))
            passes += 1
        dt = time.perf_counter() - t0
    extras["all_cores"] = {"value": round(n * nlev * passes / dt / 1e6, 1), "unit": "Mcells/s", "cores": workers, "kind": kind,
                           "sample": "%d passes, %d tasks (%d row pieces per level) over %d threads" % (passes, len(tasks), pieces, min(workers, len(tasks)))}
    # the library's own OpenMP path (ENABLE_OPENMP=ON), capped at 8 threads by the reference (openmp_tools.cc:54,65)
    if which == "ref" and cpulib.available("ref_omp"):
        os.environ.setdefault("OMP_NUM_THREADS", "8")
        omp = cpulib.CpuLib("ref_omp")
        r2, d2 = omp.raw("relvort"), omp.raw("divergence")

        def one_level_omp(l):
            fd = ctypes.c_int(0)
            r2(NX, NY, u[l].ctypes.data, v[l].ctypes.data, xm.ctypes.data, ym.ctypes.data, out.ctypes.data, ctypes.addressof(fd), 1e35)
            fd = ctypes.c_int(0)
            d2(NX, NY, u[l].ctypes.data, v[l].ctypes.data, xm.ctypes.data, ym.ctypes.data, out.ctypes.data, ctypes.addressof(fd), 1e35)

        for l in range(3):
            one_level_omp(l)
        t0 = time.perf_counter()
        passes = 0
        while time.perf_counter() - t0 < seconds_target / 2:
            for l in range(nlev):
                one_level_omp(l)
            passes += 1
        dt = time.perf_counter() - t0
        extras["openmp8"] = {"value": round(n * nlev * passes / dt / 1e6, 1), "unit": "Mcells/s", "cores": min(8, workers), "kind": kind,
                             "sample": "%d passes, ENABLE_OPENMP=ON, OMP_NUM_THREADS=8" % passes}
    return res, extras


def pmc_traffic():
    """HBM bytes per launch from the committed rocprofv3 --pmc passes (profiles/),
    corrected as MI355X_MICROARCH.md prescribes; None if not collected."""
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if os.path.exists(p):
        try:
            with open(p) as f:
                return json.load(f).get("hbm_bytes_per_launch")
        except (OSError, ValueError):
            return None
    return None


def dump_index(device):
    """Device indices of what --dump-outputs writes: the levels DUMP_LEVELS, and (level, row, column) of a fixed sample of
    DUMP_SAMPLE cells.  Made during set-up, so that only device copies follow the steps they copy."""
    import numpy as np
    import torch

    flat = np.sort(np.random.default_rng(DUMP_SEED).choice(NLEV * NY * NX, DUMP_SAMPLE, replace=False))
    cells = tuple(torch.from_numpy(a).to(device) for a in (flat // (NY * NX), flat // NX % NY, flat % NX))
    return torch.tensor(DUMP_LEVELS, device=device), cells


def dump_snapshot(rv, dg, index):
    """Device copies of the dumped levels and cells of both outputs (stream order keeps later launches from overwriting
    them first)."""
    levels, (l, j, i) = index
    snap = {}
    for name, t in (("rvort", rv), ("diverg", dg)):
        snap[name + "_levels"] = t.index_select(0, levels)
        snap[name + "_sample"] = t[l, j, i]
    return snap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default 20 on one GPU, 100 on several: the max over ranks of a 7.7 ms region is thin)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also verify against the CPU reference path, time each launch on its own, the as-allocated batch, the tested variant and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (whole levels and a seeded sample of cells, float32) to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: do not time the CPU baseline")
    ap.add_argument("--no-verify", action="store_true", help="with --full: skip the comparison with the CPU reference path before timing (profiling runs)")
    ap.add_argument("--no-check-variant", action="store_true", help="with --full: do not time the SOME_DEFINED (per-cell tests + counts) variant")
    ap.add_argument("--check", action="store_true", help="(kept for compatibility: --full times the tested variant)")
    ap.add_argument("--settle-ms", type=float, default=40.0, help="untimed launches for this long before the W warm-up steps (clock ramp after idle); 0 = none")
    ap.add_argument("--placement-pool", type=int, default=48,
                    help="the four arrays of the batch are chosen from a pool of this many arrays allocated in one go (mi-fieldcalc_amd/placement.py: which "
                         "combination of arrays a kernel streams decides its time by up to 12 %%); 0 = four allocations as they come")
    ap.add_argument("--placement-rounds", type=int, default=3, help="pools searched one after the other (each of --placement-pool arrays, --placement-tries probes); the best set is kept")
    ap.add_argument("--placement-tries", type=int, default=240, help="probes (index sets of the pool timed with the kernel) the search may spend; the fastest set is kept")
    ap.add_argument("--no-as-allocated", action="store_true", help="with --full: do not time the same launch on four plain allocations (roofline_as_allocated)")
    ap.add_argument("--level-stride", type=int, default=None, help="floats between levels (default: the library's mifc_batch_level_stride)")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 20 if args.gpus <= 1 else 100

    import numpy as np
    import torch
    import torch.distributed as dist

    import mi_fieldcalc_amd as fc
    import mi_fieldcalc_amd.synth as synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node %d for --gpus %d" % (args.gpus, args.gpus))
    # MIFC_BENCH_BACKEND=gloo is a self-test aid only (rehearsing the N>1 control flow on a
    # one-GPU box, ranks sharing cuda:0); the driver's runs use nccl (= RCCL), one rank per GPU.
    backend = os.environ.get("MIFC_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if backend == "nccl" else local_rank % max(ndev, 1)
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    # ---- this rank's batch: one ensemble member = 137 levels, generated in HBM
    ctx = fc.Context(dev_index)
    ctx.use_torch_stream()
    xm, ym, _ = synth.grid_maps(NX, NY)
    dxm, dym = torch.from_numpy(xm).to(dev), torch.from_numpy(ym).to(dev)
    # the batch lives in the library's layout: [nlev][ny][nx] with the levels mifc_batch_level_stride() floats apart
    level_stride = args.level_stride or ctx.batch_level_stride(NX, NY)
    flags = np.full(NLEV, fc.ALL_DEFINED, np.int32)
    counts = torch.zeros(NLEV, dtype=torch.int64, device=dev)
    su, sv = synth.device_wind(NX, NY, NLEV, SEED + 17 * rank, dev)

    def probe_batch(arrays):  # median of 3 x 4 launches of the kernel the bench times
        a, b, c, d = arrays
        if not warmed:  # the first launches of a process run 2-3 % slower for ~15 ms (time_series.txt): not a property of the placement
            for _ in range(60):
                ctx.vortdiv_levels_enqueue(a, b, dxm, dym, c, d, fdefined=flags, n_undefined=None)
            torch.cuda.synchronize()
            warmed.append(True)
        ms = []
        for k in range(4):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(4):
                if not ctx.vortdiv_levels_enqueue(a, b, dxm, dym, c, d, fdefined=flags, n_undefined=None):
                    raise RuntimeError(ctx.last_error())
            e.record()
            torch.cuda.synchronize()
            if k:
                ms.append(s.elapsed_time(e) / 4)
        return float(np.median(ms))

    # Which physical pages the four arrays of the batch lie on changes a streaming kernel's time by up to 12 % (stable
    # once allocated, bimodal -- 0.40 / 0.435 ms -- and a property of the COMBINATION of arrays: DESIGN.md 4.1,
    # mi-fieldcalc_amd/placement.py).  A long-lived batch is therefore chosen from a pool of arrays allocated in one go:
    # structured and random index sets are probed with the kernel, then coordinate descent from the best; the rest of
    # the pool is freed.  The pool is 48 arrays (27 GB): about one stretch of 24 consecutive allocations in six holds NO fast
    # set at all (profiles/r02/experiments/placement_pools.txt), two stretches make that a 3 % event.  Outside every timed region; the report (incl. what the first four arrays of the pool --
    # "allocated in one go" -- would have given) goes into the JSON line.  --placement-pool 0: four allocations as they come.
    warmed = []
    from mi_fieldcalc_amd.placement import choose_search_rounds
    # the pools are sized to what is free on THIS device (ranks may share one in rehearsals; other tenants): at most a third
    # of the free memory per pool round, and four plain allocations when even a small pool does not fit or runs out of memory
    pool = args.placement_pool
    if pool >= 4:
        free_b, _ = torch.cuda.mem_get_info(dev)
        per_array = level_stride * NLEV * 4
        pool = min(pool, int(free_b * 0.9 / max(1, args.placement_rounds) / per_array))
    placement = None
    if pool >= 8:
        try:
            # ... and a pool of 48 can still hold none (two of five processes of one round-end run): up to three pools, the best set kept
            (du, dv, rv, dg), placement = choose_search_rounds(lambda: ctx.batch_empty(NLEV, NY, NX, level_stride=level_stride), 4, probe_batch,
                                                               rounds=args.placement_rounds, pool_size=pool, random_sets=48,
                                                               max_probes=max(1, args.placement_tries), device=dev)
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            placement = None
    if placement is None:
        du, dv, rv, dg = (ctx.batch_empty(NLEV, NY, NX, level_stride=level_stride) for _ in range(4))
        placement = {"method": "four allocations as they come"}
    du.copy_(su)
    dv.copy_(sv)
    del su, sv
    torch.cuda.empty_cache()

    def step(check=False):
        if check:
            ok = ctx.vortdiv_levels_enqueue(du, dv, dxm, dym, rv, dg, fdefined=None, n_undefined=counts)
        else:
            ok = ctx.vortdiv_levels_enqueue(du, dv, dxm, dym, rv, dg, fdefined=flags, n_undefined=None)
        if not ok:
            raise RuntimeError(ctx.last_error())

    def barrier():
        if world > 1:
            dist.barrier()

    def timed(nsteps, check=False):
        """-> wall seconds of the K steps (barrier + synchronize on both sides), and the GPU time of the same
        K launches from ONE pair of HIP events around the region, on the stream the kernel is launched on
        (the context is bound to torch's current stream): region / K is the average launch duration."""
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        for k in range(nsteps):
            step(check)
        ev1.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0  # this rank's K steps; the closing barrier (an RCCL kernel of ~0.1 ms) is not part of them
        barrier()
        return wall, ev0.elapsed_time(ev1) / nsteps

    def per_launch(nsteps, check=False):
        """Each launch between its own pair of events (not part of the timed region): spread of the launches.
        A pair of events around a single launch adds the event packets' own time, 1-2 % here."""
        starts = [torch.cuda.Event(enable_timing=True) for _ in range(nsteps)]
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(nsteps)]
        for k in range(nsteps):
            starts[k].record()
            step(check)
            ends[k].record()
        torch.cuda.synchronize()
        return [s.elapsed_time(e) for s, e in zip(starts, ends)]

    # ---- checker leg, before anything is timed: sampled levels against the reference CPU path
    verified, verified_kind = None, None
    sample = (0, NLEV // 2, NLEV - 1)
    if rank == 0 and args.full and not args.no_verify:
        def grab(t):
            return [t[l].cpu().numpy() for l in sample]

        step()
        torch.cuda.synchronize()
        verified_kind = verify_against_cpu(sample, grab(du), grab(dv), xm, ym, grab(rv), grab(dg), fc.ALL_DEFINED)
        # the tested variant on inputs that carry undefined values (restored afterwards)
        keep = [(l, du[l, 100:110, 200:260].clone()) for l in sample]
        for l in sample:
            du[l, 100:110, 200:260] = float(fc.UNDEF)
        step(True)
        torch.cuda.synchronize()
        cs = counts.cpu().numpy()
        verify_against_cpu(sample, grab(du), grab(dv), xm, ym, grab(rv), grab(dg), fc.SOME_DEFINED, counts=[cs[l] for l in sample])
        for l, blk in keep:
            du[l, 100:110, 200:260] = blk
        verified = True

    dump_at = dump_index(dev) if args.dump_outputs and rank == 0 else None

    # The first ~15 ms of GPU work after an idle stretch (the verification above copies levels to the host and
    # runs the CPU reference) run 2-3 % slower (profiles/r02/experiments/time_series.txt): W steps of 0.4 ms do
    # not cover that, so the W warm-up steps are preceded by untimed launches until --settle-ms have passed.
    t_settle = time.perf_counter()
    while (time.perf_counter() - t_settle) * 1e3 < args.settle_ms:
        for _ in range(10):
            step()
        torch.cuda.synchronize()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    wall, kernel_avg_ms = timed(args.steps)
    kern_ms = per_launch(max(10, args.steps)) if args.full else None
    # what the last timed step computed: the per-launch pairs of --full repeat that step on the same inputs, so the
    # copies come after them (the gathers slow the launches that follow them by ~9 %)
    snapshot = dump_snapshot(rv, dg, dump_at) if dump_at is not None else None
    # the same four-array batch "as allocated": four plain allocations made now, timed like the headline (what a caller who
    # allocates a batch and computes gets; 65-72 % of peak depending on the process)
    as_allocated = None
    if args.full and not args.no_as_allocated and world == 1:
        try:
            keep = (du, dv, rv, dg)
            du, dv, rv, dg = (ctx.batch_empty(NLEV, NY, NX, level_stride=level_stride) for _ in range(4))
            du.copy_(keep[0])
            dv.copy_(keep[1])
            for _ in range(max(3, args.warmup)):
                step()
            torch.cuda.synchronize()
            _, aa_ms = timed(args.steps)
            as_allocated = {"kernel_ms_avg": round(aa_ms, 4), "frac": round(algorithmic_bytes(NX, NY, NLEV) / (aa_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                            "note": "four plain allocations, no placement search; same launch, same K steps between one pair of events"}
            du, dv, rv, dg = keep
            del keep
            torch.cuda.empty_cache()
        except torch.cuda.OutOfMemoryError:
            du, dv, rv, dg = keep
            torch.cuda.empty_cache()
    per_rank_frac = None
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())
        mine = algorithmic_bytes(NX, NY, NLEV) / (kernel_avg_ms / 1e3) / 1e9 / HBM_PEAK_GBS
        f = torch.tensor([mine, -mine], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(f, op=dist.ReduceOp.MAX)
        per_rank_frac = {"min": round(-float(f[1]), 4), "max": round(float(f[0]), 4)}

    cells_per_step = NX * NY * NLEV
    value = cells_per_step * world * args.steps / wall / 1e6
    avg_kernel_s = kernel_avg_ms / 1e3
    alg = algorithmic_bytes(NX, NY, NLEV)
    achieved = alg / avg_kernel_s / 1e9
    out = {
        "metric": "Mcells/s fused vorticity+divergence, 1440x720x137 grid; % HBM roofline",
        "value": round(value, 1),
        "unit": "Mcells/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(wall / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32 in/out, f64 combine",
        "data": "synthetic",
        "config": {
            "workload": "1440x720x137 float32 fused relvort+divergence (BASELINE.json configs[2]), one 137-level ensemble member per GPU, inputs ALL_DEFINED and resident in HBM",
            "nx": NX, "ny": NY, "nlev": NLEV, "members_per_gpu": 1, "sharding": "members across GPUs, no collective",
            "tuning": os.environ.get("MIFC_VORTDIV_TUNE", "default"),
            "level_stride_floats": int(level_stride),
            "placement": placement,
        },
        "verified": verified,
        "verified_against": None if not verified else "%s CPU path, levels %s bit for bit, ALL_DEFINED and SOME_DEFINED (+ flags)" % (verified_kind, list(sample)),
        "roofline": {
            "bound": "hbm",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": pmc_traffic(),
            "algorithmic_bytes_per_launch": alg,
            "kernel_ms_avg": round(avg_kernel_s * 1e3, 4),
            "kernel_ms_avg_note": "one pair of HIP events around the K launches of the timed region, / K",
            "per_launch_event_pairs_ms": None if kern_ms is None else
            {"median": round(float(np.median(kern_ms)), 4), "min": round(float(np.min(kern_ms)), 4), "max": round(float(np.max(kern_ms)), 4)},
            "per_rank_frac": per_rank_frac,
        },
        "roofline_as_allocated": as_allocated,
    }
    if args.full and rank == 0 and world == 1 and not args.no_check_variant:
        du[:, 100:110, 200:260] = float(fc.UNDEF)  # some undefined cells so that the count path does real work
        for _ in range(2):
            step(True)
        torch.cuda.synchronize()

        nchk = max(10, args.steps)
        bursts = []
        for _ in range(5):  # five bursts of K steps each (the first follows freed memory and an idle device): the median is reported
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(nchk):
                step(True)
            ev1.record()
            torch.cuda.synchronize()
            bursts.append(ev0.elapsed_time(ev1) / nchk)
        chk_ms = float(np.median(bursts))
        out["check_variant"] = {"kernel_ms_avg": round(chk_ms, 4), "bursts_ms": [round(b, 4) for b in bursts],
                                "Mcells_per_s": round(cells_per_step / (chk_ms / 1e3) / 1e6, 1),
                                "roofline_frac": round(alg / (chk_ms / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                                "note": "SOME_DEFINED inputs: per-cell undefined tests + per-level counts (memset + kernel), the variant the parity tests cover"}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        base, extras = cpu_baseline()
        out["cpu_baseline"] = base
        out["cpu_baseline_extra"] = extras
    if snapshot is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, t in snapshot.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), t.cpu().numpy())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
