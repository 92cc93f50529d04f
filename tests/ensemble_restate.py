"""Numpy restatement of the five reductions over ensemble members (include/mifc.h: mifc_sumFields, mifc_meanValue,
mifc_stddevValue, mifc_extremeValue, mifc_probability, and mifc_ensemble_levels, which is the five per level): ens_member /
ens_finish of csrc/mifc_ensemble.hip statement by statement (FieldCalculations.cc:2671-2860), the members walked in index
order, every accumulator a float32 array over the cells of a level and every ufunc rounding once.  The oracle of
tests/test_gpu_member_range.py; tests/test_member_range_cpu.py ties it to the CPU checkers first.

What the reference does and a tidier restatement would not:
  * extremeValue starts its running value at undef and takes a member whenever the running value EQUALS undef: member 0 is
    taken whatever it is (undefined, NaN), and a defined member that happens to store undef re-arms the walk; a NaN in
    the running value stays (every comparison with it is false); with undef = NaN nothing ever equals undef, so the
    running value stays NaN and no cell is counted as undefined.
  * sumFields stops a cell at its first undefined member; a sum that happens to equal undef is not counted as undefined.
  * probability tests `!= undef` only (a NaN fails the limits, a stored undef of an ALL_DEFINED member does not count) and
    leaves out the members flagged NONE_DEFINED; the percentage is formed in double.
  * the index variants store (float)j.
"""
import numpy as np

ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
UNDEF = np.float32(1.0e35)
EXTREME = {"max": 1, "min": 2, "argmax": 3, "argmin": 4}

# not part of the definition: what tests/test_member_range_cpu.py shows the range cases to tell from it
MISTAKES = ("double accumulators", "welford contracted", "reciprocal", "fmax", "first maximum lost", "flushed", "hole by magnitude",
            "probability tests is_def")

_TINY = np.float32(np.finfo(np.float32).tiny)


def classify(n_undefined, n):
    """miutil::checkDefined, FieldDefined.cc:62-70."""
    if n_undefined == 0:
        return ALL_DEFINED
    return NONE_DEFINED if n_undefined == n else SOME_DEFINED


def flush(x):
    """Subnormal float32 to zero of the same sign (the mistake "flushed")."""
    x = np.asarray(x, np.float32)
    return np.where((np.abs(x) < _TINY) & (x != 0), np.copysign(np.float32(0), x), x).astype(np.float32)


def name_of(product):
    return product if isinstance(product, str) else product[0]


def _flag_in(product, nlev):
    """The in/out flag of a sum / extreme product per level: ("max", flags) or "max" (SOME_DEFINED)."""
    if isinstance(product, str) or len(product) < 2:
        return np.full(nlev, SOME_DEFINED, np.int32)
    return np.broadcast_to(np.asarray(product[1], np.int32), (nlev,))


def _level(x, fl, product, in_all, undef, mistakes):
    """One product on one level: x float32 (nmem, cells), fl (nmem,) member flags -> (out float32 (cells,), n_undefined)."""
    nmem, cells = x.shape
    name = name_of(product)
    f32 = np.float32
    wide = "double accumulators" in mistakes
    acc = np.float64 if wide else np.float32
    with np.errstate(all="ignore"):
        if "hole by magnitude" in mistakes:
            defined = ~np.isnan(x) & (np.abs(x) < np.abs(undef))
        else:
            defined = ~np.isnan(x) & (x != undef)  # is_def
        m_all, m_none = fl == ALL_DEFINED, fl == NONE_DEFINED

        if name == "sum":  # :2682-2690
            r, live = np.zeros(cells, acc), np.ones(cells, bool)
            for j in range(nmem):
                ok = defined[j] | bool(in_all)
                r = np.where(live & ok, r + x[j].astype(acc), r)
                r = np.where(live & ~ok, acc(undef), r)
                live = live & ok
            return r.astype(f32), int((~live).sum())

        if name == "mean":  # :2709-2720
            r, n = np.zeros(cells, acc), np.zeros(cells, np.int32)
            for j in range(nmem):
                ok = defined[j] | m_all[j]
                n = n + ok
                r = np.where(ok, r + x[j].astype(acc), r)
            nf = np.maximum(n, 1).astype(acc)
            q = r * (acc(1) / nf) if "reciprocal" in mistakes else r / nf
            return np.where(n > 0, q.astype(f32), undef).astype(f32), int((n == 0).sum())

        if name == "stddev":  # :2739-2753, Welford in float, sqrt the double function
            m, m2, n = np.zeros(cells, acc), np.zeros(cells, acc), np.zeros(cells, np.int32)
            for j in range(nmem):
                ok = defined[j] | m_all[j]
                f = x[j].astype(acc)
                delta = f - m
                n1 = n + 1
                step = delta * (acc(1) / n1.astype(acc)) if "reciprocal" in mistakes else delta / n1.astype(acc)
                m1 = m + step
                if "welford contracted" in mistakes and not wide:  # one rounding: the product of two floats is exact in double
                    m21 = (m2.astype(np.float64) + delta.astype(np.float64) * (f - m1).astype(np.float64)).astype(f32)
                else:
                    m21 = m2 + delta * (f - m1)
                n, m, m2 = np.where(ok, n1, n), np.where(ok, m1, m), np.where(ok, m21, m2)
            nf = np.maximum(n, 1).astype(acc)
            q = (m2 * (acc(1) / nf) if "reciprocal" in mistakes else m2 / nf).astype(f32)
            return np.where(n > 0, np.sqrt(q.astype(np.float64)).astype(f32), undef).astype(f32), int((n == 0).sum())

        if name in EXTREME:  # :2776-2799
            compute = EXTREME[name]
            up = compute in (1, 3)
            run = np.full(cells, undef, f32)  # the running extreme (fres itself for compute 1 and 2)
            idx = np.full(cells, undef, f32)
            for j in range(nmem):
                ok = defined[j] | bool(in_all)
                f = x[j]
                if compute <= 2 and "fmax" in mistakes:
                    run = np.where(run == undef, f, np.where(ok, (np.fmax if up else np.fmin)(run, f), run)).astype(f32)
                    continue
                if compute >= 3 and "first maximum lost" in mistakes:
                    beats = (run <= f) if up else (run >= f)
                else:
                    beats = (run < f) if up else (run > f)
                take = (run == undef) | (ok & beats)
                run = np.where(take, f, run)
                idx = np.where(take, f32(j), idx)
            out = run if compute <= 2 else idx
            return out.astype(f32), int((out == undef).sum())

        if name == "probability":  # :2821-2856
            compute, limits = int(product[1]), [f32(v) for v in np.atleast_1d(product[2])]
            between = compute in (3, 6)
            above, below = compute in (1, 4) or between, compute in (2, 5) or between
            v_above, v_below = limits[0], (limits[1] if between else limits[0])
            r, ndef = np.zeros(cells, f32), 0
            for j in range(nmem):
                if m_none[j]:
                    continue
                ndef += 1
                f = x[j]
                counts = (defined[j] | m_all[j]) if "probability tests is_def" in mistakes else (f != undef)
                if above:
                    counts = counts & (f > v_above)
                if below:
                    counts = counts & (f < v_below)
                r = np.where(counts, r + f32(1), r)
            if ndef == 0:
                return np.full(cells, undef, f32), cells
            if compute < 4:
                r = (r.astype(np.float64) / (np.float64(ndef) / np.float64(100.0))).astype(f32)
            return r.astype(f32), 0
    raise ValueError("unknown product %r" % (product,))


def statistics(members, flags, products, undef=UNDEF, mistakes=()):
    """members float32 (nmem, nlev, ny, nx); flags None (SOME_DEFINED) or int (nmem, nlev); products in the spelling of
    Context.ensembleStatistics: "sum", "mean", "stddev", "max", "min", "argmax", "argmin", (name, flags_in[nlev]) for sum
    and the extremes, ("probability", compute, limits).  Returns [(out float32 (nlev, ny, nx), flags int32 (nlev,))] in
    product order.  mistakes: names from MISTAKES."""
    assert all(m in MISTAKES for m in mistakes), mistakes
    x = np.ascontiguousarray(members, np.float32)
    nmem, nlev, ny, nx = x.shape
    cells = ny * nx
    x = x.reshape(nmem, nlev, cells)
    undef = np.float32(undef)
    fl = np.full((nmem, nlev), SOME_DEFINED, np.int32) if flags is None else np.asarray(flags, np.int32).reshape(nmem, nlev)
    if "flushed" in mistakes:
        x = flush(x)
    res = []
    for p in products:
        out, fd = np.empty((nlev, cells), np.float32), np.empty(nlev, np.int32)
        fin = _flag_in(p, nlev) if name_of(p) == "sum" or name_of(p) in EXTREME else None
        for l in range(nlev):
            o, bad = _level(x[:, l], fl[:, l], p, fin is not None and fin[l] == ALL_DEFINED, undef, mistakes)
            out[l] = flush(o) if "flushed" in mistakes else o
            fd[l] = classify(bad, cells)
        res.append((out.reshape(nlev, ny, nx), fd))
    return res


def single(name, fields, flags=None, compute=0, limits=(), fdefined=SOME_DEFINED, undef=UNDEF, mistakes=()):
    """One of the five single-field functions on 2-D members: name in "sum", "mean", "stddev", "extreme", "probability";
    flags: the member flags (mean, stddev, probability); fdefined: the in/out flag (sum, extreme).  -> (out (ny, nx), flag)."""
    x = np.stack([np.asarray(f, np.float32) for f in fields])[:, None]
    if name == "extreme":
        product = ({v: k for k, v in EXTREME.items()}[int(compute)], [fdefined])
    elif name == "sum":
        product = ("sum", [fdefined])
    elif name == "probability":
        product = ("probability", int(compute), limits)
    else:
        product = name
    (out, fd), = statistics(x, None if flags is None else np.asarray(flags).reshape(-1, 1), [product], undef, mistakes)
    return out[0], int(fd[0])
