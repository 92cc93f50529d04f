#!/usr/bin/env python3
"""What the per-family tools/bench_<family>.py share: the preamble, the shapes, the synthetic hybrid atmosphere, the one
timing loop, the statistics of its times -- and the A/B comparison of two runs of the same tool.

Importing this module is the preamble: the repository root goes onto sys.path and MIFC_LIB_PATH defaults to the
measurement build (mifc_timing_*, mifc_bench_stream2), so import it before mi_fieldcalc_amd.

    python tools/benchkit.py compare PARENT.txt NEW.txt [PARENT2.txt NEW2.txt ...]

pairs the measurement rows of the two runs in order (a measurement row has a *_ms median and algorithmic_bytes; the other
lines need only carry the same keys), refuses pairs that do not describe the same case, prints per pair the ratio of the
medians and the verdict of not_slower(), then one summary line.  Exit status 1 when a row is slower beyond the two
spreads, 2 when the runs cannot be paired.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("MIFC_LIB_PATH", os.path.join(ROOT, "mi-fieldcalc_amd", "libmifc_measure.so"))

PEAK_GBPS = 8000.0
# how alternate() times a call
KERNEL = "kernel"  # a library call inside one timing section: the kernel ms of timing_begin / timing_end_ms
EVENTS = "events"  # a foreign call between two torch events (in the kernel times: it is what a yardstick has for them)
SECTIONS = "sections"  # call(section) runs its parts through section(part), one timing section each; their times are summed
WALL = "wall"  # the host clock around the call and a synchronise, from a synchronised start
WALL_KERNEL, WALL_SECTIONS = "wall+kernel", "wall+sections"  # both clocks


def tests_on_path():
    """For the tools that take their fields or their CPU baseline from the suite's case modules."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))


def shape(argv, full=(1440, 720, 137), small=(360, 180, 24)):
    """The --small switch."""
    return small if "--small" in argv else full


def hybrid_levels(eta):
    """alevel, blevel and the levels at ps = 1000 of a hybrid coordinate with the given eta."""
    import numpy as np

    alevel, blevel = (1000 * (eta - eta ** 2)).astype(np.float32), (eta ** 2).astype(np.float32)
    return alevel, blevel, (alevel + blevel * np.float32(1000)).astype(np.float32)


def coordinate_batch(alevel, blevel, ps, dev):
    """alevel + blevel * ps as a contiguous (nlev, ny, nx) batch on the device."""
    import torch

    return (torch.from_numpy(alevel).to(dev)[:, None, None] + torch.from_numpy(blevel).to(dev)[:, None, None] * ps[None]).contiguous()


def hybrid_atmosphere(nx, ny, nlev, dev, gen):
    """alevel, blevel, levels, ps, coord: the levels of a cubic eta distribution and a smooth surface pressure
    (orography-like, 520..1040 hPa) plus small noise, so the targets of a wave's cells sit at neighbouring levels as they
    do in model output.  Draws one randn of (ny, nx) from gen, nothing else.  coord() builds the coordinate batch when it
    is called: a tool allocates it where it always did, behind its fields."""
    import numpy as np
    import torch

    alevel, blevel, levels = hybrid_levels(np.linspace(0.01, 1, nlev) ** 3)
    yy, xx = torch.meshgrid(torch.linspace(0, 6.28, ny, device=dev), torch.linspace(0, 12.56, nx, device=dev), indexing="ij")
    ps = (780 + 260 * torch.sin(xx) * torch.cos(yy) + torch.randn((ny, nx), generator=gen, device=dev)).clamp(520, 1040).contiguous()
    return alevel, blevel, levels, ps, lambda: coordinate_batch(alevel, blevel, ps, dev)


def alternate(ctx, calls, rounds, sync=None):
    """The timing loop.  calls: name -> (call, how), how one of KERNEL, EVENTS, SECTIONS, WALL, WALL_KERNEL,
    WALL_SECTIONS; a bare callable is timed as KERNEL.  Every call is warmed up once (code object, scratch, the
    allocator's blocks), in dict order; one synchronise; then `rounds` rounds in which every call is timed once, in dict
    order, with a synchronise behind each call before its time is read.  Returns (wall, kernel): name -> the raw times in
    ms, an empty list where the kind does not measure that clock.

    Where the tools' own loops differed, the stricter behaviour holds for all: a host-clock timing starts from a
    synchronised device, and a timing section that returns a negative time (it held more launches than the context has
    event pairs for) raises instead of being reported as a time.

    sync defaults to torch.cuda.synchronize."""
    if sync is None:
        import torch

        sync = torch.cuda.synchronize

    def end_ms():
        ms = ctx.timing_end_ms()
        if ms < 0:
            raise RuntimeError("a timing section with too many launches")
        return ms

    def section(part):
        ctx.timing_begin()
        part()
        sync()
        return end_ms()

    calls = {name: entry if isinstance(entry, tuple) else (entry, KERNEL) for name, entry in calls.items()}
    for call, how in calls.values():
        if SECTIONS in how:
            call(lambda part: part())
        else:
            call()
    sync()
    wall, kernel = {name: [] for name in calls}, {name: [] for name in calls}
    for _ in range(rounds):
        for name, (call, how) in calls.items():
            if how == EVENTS:
                import torch

                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if WALL in how:
                sync()
            if KERNEL in how:
                ctx.timing_begin()
            t0 = time.perf_counter()
            if SECTIONS in how:
                parts = []
                call(lambda part: parts.append(section(part)))  # noqa: B023
            elif how == EVENTS:
                e0.record()
                call()
                e1.record()
            else:
                call()
            sync()
            t1 = time.perf_counter()
            if WALL in how:
                wall[name].append((t1 - t0) * 1e3)
            if KERNEL in how:
                kernel[name].append(end_ms())
            elif SECTIONS in how:
                kernel[name].append(sum(parts))
            elif how == EVENTS:
                kernel[name].append(e0.elapsed_time(e1))
    return wall, kernel


def stats(ts, key="kernel_ms"):
    """Median, minimum and spread (max - min) of the times of one call."""
    return {key: round(float(statistics.median(ts)), 4), key + "_min": round(min(ts), 4), key + "_spread": round(max(ts) - min(ts), 4)}


def rate(nbytes, ms):
    """GB/s of nbytes in ms, to 0.1, and its share of PEAK_GBPS, to 0.001."""
    gbps = round(nbytes / ms / 1e6, 1)
    return gbps, round(gbps / PEAK_GBPS, 3)


def not_slower(new, parent, key="kernel_ms"):
    """The project's criterion for two stats() of the same work: the new minimum is not above the parent's minimum plus
    the two spreads -- two runs of the same code differ by that much."""
    return bool(new[key + "_min"] <= parent[key + "_min"] + parent[key + "_spread"] + new[key + "_spread"])


# ---- compare -------------------------------------------------------------------------------------------------------------

def _measured(key):
    """A time, or a number derived from one."""
    return "ms" in key.split("_") or "Bps" in key or key == "share_of_peak"


def _median_key(row):
    """The key of a measurement row's median (the kernel time where the row has both clocks), or None for any other line."""
    if "algorithmic_bytes" not in row:
        return None
    if "kernel_ms" in row:
        return "kernel_ms"
    return next((k for k in row if k == "ms" or k.endswith("_ms")), None)


def _lines(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.startswith("{")]


def compare(paths, out=print):
    """Pairs the rows of (parent, new, parent, new, ...), prints one line per measurement row and the summary; returns the
    exit status.  Raises ValueError when two runs cannot be paired."""
    ratios, slower, unjudged = [], 0, 0
    for parent_path, new_path in zip(paths[0::2], paths[1::2]):
        parent, new = _lines(parent_path), _lines(new_path)
        if len(parent) != len(new):
            raise ValueError("different numbers of rows: %d in %s, %d in %s" % (len(parent), parent_path, len(new), new_path))
        for n, (p, r) in enumerate(zip(parent, new), 1):
            where = "row %d of %s and %s" % (n, parent_path, new_path)
            # the one key a new run may have and its parent not: bench_vinterp.py printed no spread
            if list(p) != [k for k in r if k != "kernel_ms_spread" or k in p]:
                raise ValueError("%s: different keys: %s and %s" % (where, list(p), list(r)))
            key = _median_key(p)
            if key is None:
                continue
            case = {k: v for k, v in p.items() if not _measured(k)}
            for k, v in case.items():
                if r[k] != v:
                    raise ValueError("%s: not the same case: %s is %r and %r" % (where, k, v, r[k]))
            ratios.append(r[key] / p[key])
            if key + "_spread" in p and key + "_spread" in r:
                verdict = not_slower(r, p, key)
                slower += not verdict
            else:
                verdict = "no spread"
                unjudged += 1
            out(json.dumps({**{k: v for k, v in case.items() if not isinstance(v, dict)}, "parent_" + key: p[key], "new_" + key: r[key],
                            "ratio": round(ratios[-1], 4), "not_slower_beyond_the_two_spreads": verdict}))
    out(json.dumps({"rows": len(ratios), "slower_beyond_the_two_spreads": slower, "without_spread": unjudged,
                    "median_ratio": round(statistics.median(ratios), 4) if ratios else None,
                    "largest_ratio": round(max(ratios), 4) if ratios else None, "smallest_ratio": round(min(ratios), 4) if ratios else None}))
    return 1 if slower else 0


def main(argv):
    if len(argv) < 3 or argv[0] != "compare" or len(argv) % 2 == 0:
        print(__doc__, file=sys.stderr)
        return 2
    try:
        return compare(argv[1:])
    except ValueError as e:
        print("compare: %s" % e, file=sys.stderr)
        return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
