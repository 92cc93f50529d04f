"""Numpy restatement of mifc_vparcel_hlevels / mifc_vparcel_fields / mifc_vparcel_levels (include/mifc.h, "parcel ascent
over level batches"): the definition, rule by rule, in float32 and float64 operations in the stated order.  It is the
oracle of tests/test_gpu_vparcel.py.  pi comes from a float64 pow rounded to float32 (the standard tests/test_gpu_seams.py
holds pow_kappa to); `pi_nudge`, an int array in {-1, 0, +1} of shape (nlev + 1, ny, nx), moves the float32 power of every
(point, cell) to its neighbour before it is multiplied by cp -- row k belongs to level k, row nlev to a source given by
planes: the family of runs that bounds what a device power one ulp off can do to a result."""
import numpy as np

from seam_cases import EWT, ewt_value, ewt_x  # noqa: F401  (the float32 table lookups of MetConstants.h:56-80)

F, D = np.float32, np.float64
UNDEF = F(1.0e35)
ALL_DEFINED, NONE_DEFINED, SOME_DEFINED = 0, 1, 2
FROM_FIRST, FROM_LAST = 0, 1
FROM = {"first": 0, "last": 1}
OUTPUTS = ("cape", "cin", "plcl", "plfc", "pel", "tparcel")
R, CP, T0, EPS, XLH = F(287.0), F(1004.0), F(273.15), F(0.622), F(2.501e6)  # MetConstants.h:39-41
P0INV = F(1.0 / 1000.0)
KAPPA = R / CP
CPLR = XLH / (R / CP)  # :42
EXL = EPS * XLH


# Departures from the definition that a kernel could plausibly make where its arithmetic takes a branch keyed on magnitude
# (tests/test_vparcel_range_cpu.py holds which of them the scaled cases can see); `with mistaken(name):` makes one.
MISTAKES = ("qsat through a float reciprocal of p", "a1 through a float reciprocal of tcl", "power two ulp off beyond the fast domain", "qsat flushed to zero")
_mistakes = set()


class mistaken:
    def __init__(self, *names):
        assert all(n in MISTAKES for n in names), names
        self.names = set(names)

    def __enter__(self):
        _mistakes.update(self.names)

    def __exit__(self, *exc):
        _mistakes.difference_update(self.names)


def check_defined(n_undefined, n):
    return ALL_DEFINED if n_undefined == 0 else (NONE_DEFINED if n_undefined == n else SOME_DEFINED)


def pi_of(p, nudge=None):
    """rule 2: cp * powf(p * p0inv, kappa) with the power from float64, rounded once; nudge moves it to a neighbour."""
    with np.errstate(all="ignore"):
        x = (np.asarray(p, F) * P0INV).astype(D)
        w = np.power(x, D(KAPPA)).astype(F)
        if "power two ulp off beyond the fast domain" in _mistakes:  # the fast domain of pow_kappa: 2^-32 <= x < 2^32
            beyond = ~((x >= 2.0 ** -32) & (x < 2.0 ** 32)) & np.isfinite(w) & (w > 0)
            w = np.where(beyond, np.nextafter(np.nextafter(w, F(np.inf)), F(np.inf)), w).astype(F)
        if nudge is not None:
            w = np.where(nudge > 0, np.nextafter(w, F(np.inf)), np.where(nudge < 0, np.nextafter(w, F(-np.inf)), w)).astype(F)
        return (CP * w).astype(F)


def sat_test(tcl, p):
    """(in the table, qsat) of the state tcl at pressure p: FieldCalculations.cc:949-953."""
    with np.errstate(all="ignore"):
        x = ewt_x((tcl / CP).astype(F) - T0)
        ok = (x > F(-1.0)) & (x < F(40.0))
        num = (EPS * ewt_value(np.where(ok, x, F(0.0)))).astype(F)
        qsat = (num / p).astype(F)
        if "qsat through a float reciprocal of p" in _mistakes:
            qsat = (num * (F(1.0) / np.asarray(p, F)).astype(F)).astype(F)
        if "qsat flushed to zero" in _mistakes:
            qsat = np.where((qsat != 0) & (np.abs(qsat) < np.finfo(F).tiny), np.copysign(F(0.0), qsat), qsat).astype(F)
    return ok, qsat


def adjust_trip(tcl, qcl, p):
    """One trip of FieldCalculations.cc:949-959; ok False = its `break` (the caller keeps the state)."""
    with np.errstate(all="ignore"):
        ok, qsat = sat_test(tcl, p)
        dq = (qcl - qsat).astype(F)
        a1 = ((CPLR * qcl).astype(F) / tcl).astype(F)
        if "a1 through a float reciprocal of tcl" in _mistakes:
            a1 = ((CPLR * qcl).astype(F) * (F(1.0) / tcl).astype(F)).astype(F)
        a2 = (EXL / tcl).astype(F)
        dq = (dq.astype(D) / (1.0 + (a1 * a2).astype(F).astype(D))).astype(F)
        return ok, (tcl + (dq * XLH).astype(F)).astype(F), (qcl - dq).astype(F)


def adjust(tcl, qcl, p, run):
    """The seven trips where `run`; returns the new (tcl, qcl)."""
    tcl, qcl, run = tcl.copy(), qcl.copy(), run.copy()
    for _ in range(7):
        if not run.any():
            break
        ok, t2, q2 = adjust_trip(tcl, qcl, p)
        run &= ok
        tcl = np.where(run, t2, tcl)
        qcl = np.where(run, q2, qcl)
    return tcl, qcl


class _State:
    pass


def _piece(s, m, Ba, Bb, la, lb, sat, pos_at):
    """rule 6 on the cells m: one piece of B from (Ba, la) to (Bb, lb); sat: the piece lies at or above the LCL."""
    with np.errstate(all="ignore"):
        h = la - lb
        both = (Ba > 0) & (Bb > 0)
        up = ~(Ba > 0) & (Bb > 0)
        down = (Ba > 0) & ~(Bb > 0)
        cross = up | down
        w0 = Ba / (Ba - Bb)
        lx = la + w0 * (lb - la)
        h1 = w0 * h
        h2 = h - h1
        A1 = (Ba * 0.5) * h1
        A2 = (Bb * 0.5) * h2
        A = ((Ba + Bb) * 0.5) * h
        pos = np.where(cross, np.where(up, A2, A1), np.where(both, A, 0.0))
        neg = np.where(cross, np.where(up, A1, A2), np.where(both, 0.0, A))
        nolfc = m & ~s.lfc
        had = m & s.lfc
        s.cin = np.where(nolfc, s.cin + neg, s.cin)
        new = nolfc & sat & up
        s.plfc = np.where(new, np.exp(lx).astype(F), s.plfc)
        s.lfc_pos = np.where(new, pos_at, s.lfc_pos)
        s.cape = np.where(new | had, s.cape + pos, s.cape)
        s.lfc = s.lfc | new
        el = had & down
        s.pel = np.where(el, np.exp(lx).astype(F), s.pel)
        s.el_pos = np.where(el, pos_at, s.el_pos)
        s.el = s.el | el


def parcel(t, p, q_src, from_=FROM_FIRST, src_level=0, t_src=None, p_src=None, fdefined_in=None, fdef_tsrc=SOME_DEFINED, fdef_qsrc=SOME_DEFINED,
           fdef_psrc=SOME_DEFINED, undef=UNDEF, pi_nudge=None, pi_levels=None, diag=None):
    """The definition on a pressure batch p (nlev, ny, nx) that holds NaN where rule 1 leaves the pressure undefined.
    Returns a dict: the five planes, tparcel, "flags".  pi_levels: float32[nlev], pi per level from elsewhere (the `levels`
    form's host powf).  diag: a dict that receives lcl_pos / lfc_pos / el_pos (the walk position whose piece holds the
    level, -1: none; the source is position -1 + 1 = 0 of a source level's walk) and adjusted (nlev, ny, nx)."""
    from_ = FROM.get(from_, from_)
    t = np.asarray(t, F)
    nlev, ny, nx = t.shape
    N = ny * nx
    t = t.reshape(nlev, N)
    p = np.asarray(p, F).reshape(nlev, N)
    und = F(undef)
    fdin = None if fdefined_in is None else np.broadcast_to(np.asarray(fdefined_in).reshape(-1), (nlev,))
    nudge = None if pi_nudge is None else np.asarray(pi_nudge).reshape(nlev + 1, N)
    order = list(range(nlev)) if from_ == FROM_FIRST else list(range(nlev - 1, -1, -1))
    src = -1 if src_level is None else int(src_level)

    def t_ok(k):
        all_def = fdin is not None and fdin[k] == ALL_DEFINED
        return (np.ones(N, bool) if all_def else t[k] != und) & ~np.isnan(t[k])

    def pi_at(k):
        if pi_levels is not None:
            return np.full(N, F(pi_levels[k]), F)
        return pi_of(p[k], None if nudge is None else nudge[k])

    q = np.asarray(q_src, F).reshape(N)
    with np.errstate(all="ignore"):
        if src >= 0:
            js = order.index(src)
            T, ps_, ok = t[src], p[src], t_ok(src)
            pis = pi_at(src)
        else:
            js = -1
            T, ps_ = np.asarray(t_src, F).reshape(N), np.asarray(p_src, F).reshape(N)
            ok = ((T != und) | (fdef_tsrc == ALL_DEFINED)) & ~np.isnan(T) & ((ps_ != und) | (fdef_psrc == ALL_DEFINED))
            pis = pi_of(ps_, None if nudge is None else nudge[nlev])
        ok = ok & ((q != und) | (fdef_qsrc == ALL_DEFINED)) & ~np.isnan(q) & (ps_ > 0)
        s = _State()
        s.tcl = (CP * T).astype(F)
        s.qcl = q.copy()
        s.pi, s.p = pis, ps_.astype(F).copy()
        in_tab, qsat = sat_test(s.tcl, ps_)
        ok = ok & in_tab
        s.d = qsat.astype(D) - s.qcl.astype(D)
        s.lnp = np.log(ps_.astype(D))
        s.B = np.zeros(N, D)
        s.cape, s.cin = np.zeros(N, D), np.zeros(N, D)
        s.plcl, s.plfc, s.pel = ps_.astype(F).copy(), np.zeros(N, F), np.zeros(N, F)
        s.alive = ok.copy()
        s.started = np.full(N, js >= 0)
        s.sat = ~(s.qcl < qsat)
        s.lfc, s.el = np.zeros(N, bool), np.zeros(N, bool)
        s.lcl_pos = np.where(s.sat, js, -1)
        s.lfc_pos, s.el_pos = np.full(N, -1), np.full(N, -1)
        tparcel = np.full((nlev, N), und, F)
        adjusted = np.zeros((nlev, N), bool)
        if js >= 0:
            tparcel[src] = np.where(ok, (s.tcl / CP).astype(F), und)

        for j in range(js + 1, nlev):
            k = order[j]
            pk, tk = p[k], t[k]
            below = pk < s.p
            walk = s.alive & (s.started | below)
            usable = below & (pk > 0) & t_ok(k)
            pi = pi_at(k)
            ratio = (pi / s.pi).astype(F)
            tcl = (s.tcl * ratio).astype(F)
            in_tab, qsat = sat_test(tcl, pk)
            usable = usable & in_tab
            stepped = walk & usable
            adj = stepped & (s.qcl > qsat)
            db = qsat.astype(D) - s.qcl.astype(D)
            s.alive = s.alive & ~(walk & ~usable)
            s.started = s.started | walk
            s.tcl = np.where(stepped, tcl, s.tcl)
            s.pi = np.where(stepped, pi, s.pi)
            s.tcl, s.qcl = adjust(s.tcl, s.qcl, pk, adj)
            adjusted[k] = adj
            tp = (s.tcl / CP).astype(F)
            tparcel[k] = np.where(stepped, tp, und)
            lnp = np.log(pk.astype(D))
            B = tp.astype(D) - tk.astype(D)
            newlcl = adj & ~s.sat
            rest = stepped & ~newlcl
            # rule 5: the LCL cuts the piece in two
            w = s.d / (s.d - db)
            lm = s.lnp + w * (lnp - s.lnp)
            Bm = s.B + w * (B - s.B)
            _piece(s, newlcl, s.B, Bm, s.lnp, lm, np.zeros(N, bool), j)
            s.plcl = np.where(newlcl, np.exp(lm).astype(F), s.plcl)
            s.lcl_pos = np.where(newlcl, j, s.lcl_pos)
            at_lcl = newlcl & (Bm > 0)
            s.plfc = np.where(at_lcl, s.plcl, s.plfc)
            s.lfc_pos = np.where(at_lcl, j, s.lfc_pos)
            s.lfc = s.lfc | at_lcl
            s.sat = s.sat | newlcl
            _piece(s, newlcl, Bm, B, lm, lnp, np.ones(N, bool), j)
            _piece(s, rest, s.B, B, s.lnp, lnp, s.sat, j)
            s.lnp = np.where(stepped, lnp, s.lnp)
            s.B = np.where(stepped, B, s.B)
            s.d = np.where(stepped, db, s.d)
            s.p = np.where(stepped, pk, s.p)

        sat, lfc = s.alive & s.sat, s.alive & s.lfc
        el = lfc & s.el & ~(s.B > 0)
        out = {
            "cape": np.where(s.alive, np.where(lfc, (D(R) * s.cape).astype(F), F(0.0)), und),
            "cin": np.where(lfc, (D(R) * s.cin).astype(F), und),
            "plcl": np.where(sat, s.plcl, und),
            "plfc": np.where(lfc, s.plfc, und),
            "pel": np.where(el, s.pel, und),
        }
    flags = {n: check_defined(int((out[n] == und).sum()), N) for n in out}
    out = {n: a.astype(F).reshape(ny, nx) for n, a in out.items()}
    out["tparcel"] = tparcel.reshape(nlev, ny, nx)
    flags["tparcel"] = np.array([check_defined(int((tparcel[k] == und).sum()), N) for k in range(nlev)], np.int32)
    out["flags"] = flags
    if diag is not None:
        diag.update(lcl_pos=np.where(sat, s.lcl_pos, -1).reshape(ny, nx), lfc_pos=np.where(lfc, s.lfc_pos, -1).reshape(ny, nx),
                    el_pos=np.where(el, s.el_pos, -1).reshape(ny, nx), adjusted=adjusted.reshape(nlev, ny, nx))
    return out


def hybrid_pressure(ps, alevel, blevel, fdef_ps=SOME_DEFINED, undef=UNDEF):
    """rule 1 of mifc_vinterp_*: alevel + blevel * ps, the product rounded, then the sum; NaN where ps is undefined."""
    ps = np.asarray(ps, F)
    a, b = np.asarray(alevel, F), np.asarray(blevel, F)
    with np.errstate(all="ignore"):
        psn = ps if fdef_ps == ALL_DEFINED else np.where(ps == F(undef), F(np.nan), ps)
        return (a[:, None, None] + (b[:, None, None] * psn[None]).astype(F)).astype(F)


def field_pressure(p, fdef_coord=None, undef=UNDEF):
    p = np.asarray(p, F)
    if fdef_coord is None:
        return np.where(p == F(undef), F(np.nan), p)
    fc_ = np.asarray(fdef_coord).reshape(-1)
    return np.stack([p[k] if fc_[k] == ALL_DEFINED else np.where(p[k] == F(undef), F(np.nan), p[k]) for k in range(p.shape[0])])


def hlevels(t, ps, alevel, blevel, q_src, fdef_ps=SOME_DEFINED, undef=UNDEF, **kw):
    return parcel(t, hybrid_pressure(ps, alevel, blevel, fdef_ps, undef), q_src, undef=undef, **kw)


def fields(t, p, q_src, fdef_coord=None, undef=UNDEF, **kw):
    return parcel(t, field_pressure(p, fdef_coord, undef), q_src, undef=undef, **kw)


def levels(t, lev, q_src, host_pi=False, **kw):
    """The `levels` form; host_pi: pi per level as the host's powf gives it (one float32 power per level, no nudge)."""
    t = np.asarray(t, F)
    lv = np.asarray(lev, F)
    p = np.broadcast_to(lv[:, None, None], t.shape)
    return parcel(t, p, q_src, pi_levels=pi_of(lv) if host_pi else None, **kw)
