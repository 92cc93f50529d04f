"""The batched stencil and derived entries -- synchronous over host arrays or device tensors, and the asynchronous
*_enqueue forms on device tensors -- with what replays or decomposes them: PreparedCalls, Graph, SlabPlan and the
communicator calls."""
import ctypes

import numpy as np

from ._args import _Arg, _empty_like, _flag_table, _kept, _memkind, _same_shape
from ._consts import MEM_DEVICE, SOME_DEFINED, UNDEF


def _hybrid_or(levels, default, nlev):
    """alevel / blevel of the derived batches as float32[nlev]; None: `default` on every level."""
    return np.ascontiguousarray(levels if levels is not None else default(nlev), dtype=np.float32).reshape(nlev)


class _BatchedOps:
    """Mixin of Context: vortdiv / stencil / derived batches, their *_enqueue twins, graphs, slab plans, communicators."""

    def vortdiv_levels(self, u, v, xmapr, ymapr, fdefined=None, undef=UNDEF, rvort=None, diverg=None, want=("rvort", "diverg")):
        """Fused relvort + divergence over u, v of shape (nlev, ny, nx).
        fdefined: int sequence per level (default SOME_DEFINED).  Returns
        ((rvort, diverg), flags ndarray) or None."""
        au, av, ax, ay = _Arg(u), _Arg(v), _Arg(xmapr), _Arg(ymapr)
        if len(au.shape) != 3:
            raise ValueError("u, v must have shape (nlev, ny, nx)")
        nlev, ny, nx = au.shape
        if rvort is None and "rvort" in want:
            rvort = _empty_like(u)
        if diverg is None and "diverg" in want:
            diverg = _empty_like(u)
        ar, ad = _Arg(rvort, allow_none=True, output=True), _Arg(diverg, allow_none=True, output=True)
        if not _same_shape([av, ar, ad], au.shape) or not _same_shape([ax, ay], (ny, nx)):
            raise ValueError("u, v, rvort, diverg must be (nlev, ny, nx) and xmapr, ymapr (ny, nx)")
        flags = _flag_table(fdefined, nlev)
        if not self._launch("mifc_vortdiv_levels", [au, av, ax, ay, ar, ad],
                            [nx, ny, nlev, au.addr, av.addr, ax.addr, ay.addr, ar.addr, ad.addr, flags.ctypes.data, float(undef)], raises=False):
            return None
        outs = tuple(o if o is None else _kept(o, a) for o, a in ((rvort, ar), (diverg, ad)))
        return outs, flags

    OPS = {"relvort": 0, "absvort": 1, "divergence": 2, "vortdiv": 3, "gradient1": 4, "gradient2": 5, "gradient3": 6, "gradient4": 7,
           "plevelgwind_xcomp": 8, "plevelgwind_ycomp": 9, "plevelgvort": 10, "ilevelgwind": 11, "jacobian": 13}

    def stencil_levels(self, op, f0, f1, xmapr, ymapr, fcoriolis=None, fdefined=None, undef=UNDEF, out0=None, out1=None):
        """Any stencil operator (name from Context.OPS) over f0/f1 of shape (nlev, ny, nx).
        Returns ((out0, out1-or-None), flags) or None."""
        code = self.OPS[op]
        a0, a1 = _Arg(f0), _Arg(f1, allow_none=True)
        ax, ay, af = _Arg(xmapr, allow_none=True), _Arg(ymapr, allow_none=True), _Arg(fcoriolis, allow_none=True)
        nlev, ny, nx = a0.shape
        two = code in (3, 11)
        if out0 is None:
            out0 = _empty_like(f0)
        if two and out1 is None:
            out1 = _empty_like(f0)
        o0, o1 = _Arg(out0, output=True), _Arg(out1 if two else None, allow_none=True, output=True)
        if len(a0.shape) != 3 or not _same_shape([a1, o0, o1], a0.shape) or not _same_shape([ax, ay, af], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and the map / Coriolis fields (ny, nx)")
        flags = _flag_table(fdefined, nlev)
        if not self._launch("mifc_stencil_levels", [a0, a1, ax, ay, af, o0, o1],
                            [code, nx, ny, nlev, a0.addr, a1.addr, ax.addr, ay.addr, af.addr, o0.addr, o1.addr, flags.ctypes.data, float(undef)],
                            raises=False):
            return None
        return (_kept(out0, o0), _kept(out1, o1) if two else None), flags

    OPS_EX = {"advection": 12, "thermalFrontParameter": 14, "plevelqvector": 15, "shapiro2_filter": 17}

    def stencil_levels_ex(self, op, f0, f1=None, f2=None, xmapr=None, ymapr=None, fcoriolis=None, level_scalars=None, scalar=0.0, compute=0,
                          fdefined=None, undef=UNDEF, out0=None):
        """The f1 operators over a level batch (mifc_stencil_levels_ex): op in OPS_EX; fields (nlev, ny, nx),
        map / Coriolis fields (ny, nx) shared.  advection: f0 = f, f1 = u, f2 = v, scalar = hours;
        thermalFrontParameter: f0 = tx; plevelqvector: f0 = z, f1 = t, level_scalars = p per level, compute 1..4;
        shapiro2_filter: f0 = field.  Returns (out0, flags) or None."""
        code = self.OPS_EX[op]
        a0, a1, a2 = _Arg(f0), _Arg(f1, allow_none=True), _Arg(f2, allow_none=True)
        ax, ay, af = _Arg(xmapr, allow_none=True), _Arg(ymapr, allow_none=True), _Arg(fcoriolis, allow_none=True)
        if len(a0.shape) != 3:
            raise ValueError("level fields must be (nlev, ny, nx)")
        nlev, ny, nx = a0.shape
        if out0 is None:
            out0 = _empty_like(f0)
        o0 = _Arg(out0, output=True)
        if not _same_shape([a1, a2, o0], a0.shape) or not _same_shape([ax, ay, af], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and the map / Coriolis fields (ny, nx)")
        flags = _flag_table(fdefined, nlev)
        ls = None if level_scalars is None else np.ascontiguousarray(level_scalars, dtype=np.float32).reshape(nlev)
        if not self._launch("mifc_stencil_levels_ex", [a0, a1, a2, ax, ay, af, o0],
                            [code, nx, ny, nlev, a0.addr, a1.addr, a2.addr, ax.addr, ay.addr, af.addr, None if ls is None else ls.ctypes.data,
                             float(scalar), int(compute), o0.addr, None, flags.ctypes.data, float(undef)], raises=False):
            return None
        return _kept(out0, o0), flags

    # ---- the asynchronous forms: device tensors only, nothing read back.  They are on the benchmark's timed path, so each
    # makes its checks inline and goes to _call itself; without flags there is no flag table and no call for one.
    def vortdiv_levels_enqueue(self, u, v, xmapr, ymapr, rvort, diverg, fdefined=None, undef=UNDEF, n_undefined=None):
        """Asynchronous form on device tensors; n_undefined: int64 CUDA tensor[nlev] or None.
        u, v and rvort, diverg may be level-padded batches (see batch_empty)."""
        au, av, ax, ay = _Arg(u, levels=True), _Arg(v, levels=True), _Arg(xmapr), _Arg(ymapr)
        ar, ad = _Arg(rvort, allow_none=True, levels=True), _Arg(diverg, allow_none=True, levels=True)
        if len(au.shape) != 3:
            raise ValueError("u, v must have shape (nlev, ny, nx)")
        nlev, ny, nx = au.shape
        if not _same_shape([av, ar, ad], au.shape) or not _same_shape([ax, ay], (ny, nx)):
            raise ValueError("u, v, rvort, diverg must be (nlev, ny, nx) and xmapr, ymapr (ny, nx)")
        if _memkind([au, av, ax, ay, ar, ad], self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        outs = [a for a in (ar, ad) if a.addr is not None]
        if not outs:
            raise ValueError("at least one of rvort, diverg is required")
        if av.lstride != au.lstride or (len(outs) == 2 and outs[0].lstride != outs[1].lstride):
            raise ValueError("u and v (and rvort and diverg) must share one level stride")
        flags = None if fdefined is None else _flag_table(fdefined, nlev)
        self._bind_stream(MEM_DEVICE)
        rc = self._call(
            "mifc_vortdiv_levels_strided_enqueue",
            [
                nx, ny, nlev, au.addr, av.addr, ax.addr, ay.addr, ar.addr, ad.addr, au.lstride, outs[0].lstride,
                flags, float(undef),
                None if n_undefined is None else n_undefined.data_ptr(),
            ],
        )
        return bool(rc)

    def vortdiv_ff_levels_enqueue(self, u, v, xmapr, ymapr, rvort, diverg, ff, fdefined=None, undef=UNDEF, n_undefined=None, n_undefined_ff=None):
        """Vorticity, divergence and the wind speed of a level batch in one pass (mifc_vortdiv_ff_levels_enqueue); device tensors
        (nlev, ny, nx); n_undefined / n_undefined_ff: int64[nlev] (classify against nx*ny - 2*nx / nx*ny), None allowed when every
        level is ALL_DEFINED."""
        a = [_Arg(x) for x in (u, v, xmapr, ymapr, rvort, diverg, ff)]
        if len(a[0].shape) != 3:
            raise ValueError("u, v must have shape (nlev, ny, nx)")
        nlev, ny, nx = a[0].shape
        if not _same_shape([a[1], a[4], a[5], a[6]], a[0].shape) or not _same_shape(a[2:4], (ny, nx)):
            raise ValueError("u, v, rvort, diverg, ff must be (nlev, ny, nx) and xmapr, ymapr (ny, nx)")
        if _memkind(a, self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        flags = None if fdefined is None else _flag_table(fdefined, nlev)
        self._bind_stream(MEM_DEVICE)
        rc = self._call("mifc_vortdiv_ff_levels_enqueue", [nx, ny, nlev] + [x.addr for x in a] + [
            flags, float(undef), None if n_undefined is None else n_undefined.data_ptr(),
            None if n_undefined_ff is None else n_undefined_ff.data_ptr()])
        return bool(rc)

    def stencil_levels_enqueue(self, op, f0, f1, xmapr, ymapr, fcoriolis, out0, out1=None, fdefined=None, undef=UNDEF, n_undefined=None):
        """Asynchronous form of stencil_levels on device tensors (mifc_stencil_levels_enqueue): nothing is read back;
        n_undefined: int64 CUDA tensor[nlev] (None allowed when every level is ALL_DEFINED).  The flag of level l is
        classify(n_undefined[l], stencil_count_domain(op, nx, ny)) once the stream has drained."""
        code = self.OPS[op]
        a0, a1 = _Arg(f0), _Arg(f1, allow_none=True)
        ax, ay, af = _Arg(xmapr), _Arg(ymapr), _Arg(fcoriolis, allow_none=True)
        o0, o1 = _Arg(out0, allow_none=True, output=True), _Arg(out1, allow_none=True, output=True)
        if len(a0.shape) != 3:
            raise ValueError("level fields must be (nlev, ny, nx)")
        nlev, ny, nx = a0.shape
        if not _same_shape([a1, o0, o1], a0.shape) or not _same_shape([ax, ay, af], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and the map / Coriolis fields (ny, nx)")
        if _memkind([a0, a1, ax, ay, af, o0, o1], self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        flags = None if fdefined is None else _flag_table(fdefined, nlev)
        self._bind_stream(MEM_DEVICE)
        rc = self._call("mifc_stencil_levels_enqueue", [code, nx, ny, nlev, a0.addr, a1.addr, ax.addr, ay.addr, af.addr, o0.addr, o1.addr,
                                                        flags, float(undef),
                                                        None if n_undefined is None else n_undefined.data_ptr()])
        return bool(rc)

    def stencil_count_domain(self, op, nx, ny):
        return int(self._lib.mifc_stencil_count_domain(self.OPS[op], nx, ny))

    # ---- the fused derived batches on hybrid levels
    def hlevel_derived_levels(self, u, v, t, q, ps, alevel, blevel, fdef_wind=None, fdef_thermo=None, undef=UNDEF,
                              want=("ff", "rh", "theta"), out=None):
        """Fused ff / RH(%) / theta on hybrid levels; u, v, t, q: (nlev, ny, nx), ps: (ny, nx).
        Returns ({name: array}, {name: flags}) or None."""
        ref = next(x for x in (u, t) if x is not None)
        nlev, ny, nx = _Arg(ref).shape
        out = dict(out or {})
        for k in want:
            if out.get(k) is None:
                out[k] = _empty_like(ref)
        a = {k: _Arg(x, allow_none=True) for k, x in dict(u=u, v=v, t=t, q=q, ps=ps).items()}
        o = {k: _Arg(out.get(k), allow_none=True) for k in ("ff", "rh", "theta")}
        if not _same_shape([a[k] for k in ("u", "v", "t", "q")] + list(o.values()), (nlev, ny, nx)) or not _same_shape([a["ps"]], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and ps (ny, nx)")
        fo = {k: np.full(nlev, -1, np.int32) for k in ("ff", "rh", "theta")}
        if not self._launch("mifc_hlevel_derived_levels", list(a.values()) + list(o.values()), [
                nx, ny, nlev, a["u"].addr, a["v"].addr, a["t"].addr, a["q"].addr, a["ps"].addr, _hybrid_or(alevel, np.zeros, nlev),
                _hybrid_or(blevel, np.ones, nlev), o["ff"].addr, o["rh"].addr, o["theta"].addr, _flag_table(fdef_wind, nlev), _flag_table(fdef_thermo, nlev),
                fo["ff"].ctypes.data, fo["rh"].ctypes.data, fo["theta"].ctypes.data, float(undef)], raises=False):
            return None
        return {k: _kept(out[k], o[k]) for k in want}, {k: fo[k] for k in want}

    def hlevel_derived_batch(self, u, v, t, h, ps, alevel, blevel, temp=None, hum=None, hum2=None, ff=True, dd=False, fdef_wind=None,
                             fdef_thermo=None, undef=UNDEF, out=None, enqueue_counts=None):
        """The general fused derived batch (mifc_hlevel_derived_batch): per level any of
          ff   = vectorabs(u, v)                         (ff=True)
          temp = hleveltemp(t, ps, a, b, unit, compute)  (temp=(unit, compute))
          hum  = hlevelhum(t, h, ps, a, b, unit, compute)   (hum=(unit, compute))
          hum2 = a second hlevelhum variant of the same inputs (hum2=(unit, compute))
          dd   = wind direction from u, v (dd=True) -- EXTENSION, not a reference function
        u, v, t, h: (nlev, ny, nx); ps: (ny, nx).  out: optional dict of preallocated outputs.
        Returns ({name: array}, {name: flags}) or None.  With enqueue_counts (int64 CUDA tensor[5*nlev]) the call is
        asynchronous on device tensors and returns the outputs only (counts: ff | temp | hum | hum2 | dd)."""
        ref = next(x for x in (u, t) if x is not None)
        nlev, ny, nx = _Arg(ref).shape
        every = ("ff", "temp", "hum", "hum2", "dd")
        names = [k for k, w in zip(every, (ff, temp, hum, hum2, dd)) if w]
        out = dict(out or {})
        for k in names:
            if out.get(k) is None:
                out[k] = _empty_like(ref)
        a = {k: _Arg(x, allow_none=True) for k, x in dict(u=u, v=v, t=t, h=h, ps=ps).items()}
        o = {k: _Arg(out.get(k) if k in names else None, allow_none=True, output=True) for k in every}
        if not _same_shape([a[k] for k in ("u", "v", "t", "h")] + list(o.values()), (nlev, ny, nx)) or not _same_shape([a["ps"]], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and ps (ny, nx)")
        mk = _memkind(list(a.values()) + list(o.values()), self.device)
        self._bind_stream(mk)
        unit = lambda w: (w[0] if w else "").encode()
        comp = lambda w: int(w[1]) if w else 0
        common = [nx, ny, nlev, a["u"].addr, a["v"].addr, a["t"].addr, a["h"].addr, a["ps"].addr, _hybrid_or(alevel, np.zeros, nlev),
                  _hybrid_or(blevel, np.ones, nlev), o["ff"].addr, o["temp"].addr, unit(temp), comp(temp), o["hum"].addr, unit(hum), comp(hum),
                  o["hum2"].addr, unit(hum2), comp(hum2), o["dd"].addr, _flag_table(fdef_wind, nlev), _flag_table(fdef_thermo, nlev)]
        if enqueue_counts is not None:
            if mk != MEM_DEVICE:
                raise ValueError("the *_enqueue calls take device tensors only")
            rc = self._call("mifc_hlevel_derived_batch_enqueue", common + [float(undef), enqueue_counts.data_ptr()])
            return {k: out[k] for k in names} if rc else None
        fo = {k: np.full(nlev, -1, np.int32) for k in every}
        if not self._call("mifc_hlevel_derived_batch", common + [fo[k].ctypes.data for k in every] + [float(undef), mk]):
            return None
        return {k: _kept(out[k], o[k]) for k in names}, {k: fo[k] for k in names}

    def hlevel_derived_levels_enqueue(self, u, v, t, q, ps, alevel, blevel, ff, rh, theta, n_undefined, fdef_wind=None,
                                      fdef_thermo=None, undef=UNDEF):
        ref = next(x for x in (u, t) if x is not None)
        nlev, ny, nx = _Arg(ref).shape
        a = [_Arg(x, allow_none=True) for x in (u, v, t, q, ps)]
        o = [_Arg(x, allow_none=True) for x in (ff, rh, theta)]
        al = np.ascontiguousarray(alevel, dtype=np.float32).reshape(nlev)
        bl = np.ascontiguousarray(blevel, dtype=np.float32).reshape(nlev)
        fw = None if fdef_wind is None else _flag_table(fdef_wind, nlev)
        ft = None if fdef_thermo is None else _flag_table(fdef_thermo, nlev)
        if not _same_shape(a[:4] + o, (nlev, ny, nx)) or not _same_shape([a[4]], (ny, nx)):
            raise ValueError("level fields must be (nlev, ny, nx) and ps (ny, nx)")
        if _memkind(a + o, self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        self._bind_stream(MEM_DEVICE)
        rc = self._call(
            "mifc_hlevel_derived_levels_enqueue",
            [nx, ny, nlev] + [x.addr for x in a] + [al, bl] + [x.addr for x in o]
            + [fw, ft, float(undef), n_undefined.data_ptr()],
        )
        return bool(rc)

    def vortdiv_slab_enqueue(self, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in=SOME_DEFINED,
                             undef=UNDEF, n_undefined=None, rows=None, accumulate=False):
        """Row-slab form (see include/mifc.h); all tensors on the device.  rows=(begin, end) restricts the
        launch to those owned rows (halo overlap); accumulate=True adds to n_undefined instead of zeroing it."""
        a = [_Arg(x, allow_none=True) for x in (u_halo, v_halo, xmapr, ymapr, rvort, diverg)]
        if not _same_shape(a[:2], (ny_local + 2, nx)) or not _same_shape(a[2:], (ny_local, nx)):
            raise ValueError("u_halo, v_halo must be (ny_local + 2, nx); xmapr, ymapr, rvort, diverg (ny_local, nx)")
        if _memkind(a, self.device) != MEM_DEVICE:
            raise ValueError("the *_enqueue calls take device tensors only")
        self._bind_stream(MEM_DEVICE)
        r0, r1 = (0, int(ny_local)) if rows is None else (int(rows[0]), int(rows[1]))
        rc = self._call(
            "mifc_vortdiv_slab_rows_enqueue",
            [int(nx), int(ny_global), int(j0), int(ny_local), r0, r1] + [x.addr for x in a]
            + [int(fdefined_in), float(undef), None if n_undefined is None else n_undefined.data_ptr(), 1 if accumulate else 0],
        )
        return bool(rc)

    # ---- a sequence of *_enqueue calls as one launch (include/mifc.h: mifc_graph_*)
    def counts_accumulate(self, on=True):
        """The *_enqueue entries add to the counters they are given instead of zeroing them first (mifc_counts_accumulate)."""
        return bool(self._lib.mifc_counts_accumulate(self._ctx, 1 if on else 0))

    def zero_counts_enqueue(self, counts):
        """One asynchronous fill of an int64 CUDA tensor of counters (mifc_zero_counts_enqueue)."""
        self._bind_stream(MEM_DEVICE)
        return bool(self._call("mifc_zero_counts_enqueue", [counts.data_ptr(), counts.numel()]))

    def graph_capture(self, max_levels_per_call=0, lanes=1):
        """with ctx.graph_capture() as g: ... *_enqueue calls ...   ->  g.launch() replays them with one runtime call.
        lanes > 1: g.lane(k) before a call records it in lane k; calls in different lanes must be independent."""
        return Graph(self, max_levels_per_call, lanes)

    # ---- the decomposed step as one call (include/mifc.h: mifc_comm_*, mifc_slab_plan_*)
    def comm_unique_id(self):
        """mifc_comm_unique_id: the bytes rank 0 hands to every rank of a new communicator."""
        ident = ctypes.create_string_buffer(128)
        if not self._lib.mifc_comm_unique_id(ctypes.cast(ident, ctypes.c_void_p)):
            raise RuntimeError("mifc_comm_unique_id failed (RCCL not loadable?)")
        return ident.raw

    def comm_init(self, ident, rank, world):
        """mifc_comm_init: a communicator of the library's own for `world` processes, this one being `rank`."""
        buf = ctypes.create_string_buffer(bytes(ident), 128)
        if not self._call("mifc_comm_init", [ctypes.cast(buf, ctypes.c_void_p), int(rank), int(world)]):
            raise RuntimeError("mifc_comm_init: " + self.last_error())
        return True

    def comm_init_from_torch(self, group=None):
        """A communicator for the ranks of a torch.distributed group: rank 0's id is broadcast through the group."""
        import torch.distributed as dist

        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [self.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        return self.comm_init(box[0], rank, world)

    def comm_adopt(self, nccl_comm_ptr):
        """Use an ncclComm_t the caller owns (an integer address, e.g. ProcessGroupNCCL._comm_ptr())."""
        return bool(self._call("mifc_comm_adopt", [int(nccl_comm_ptr)]))

    def comm_release(self):
        return bool(self._lib.mifc_comm_release(self._ctx))

    def comm_info(self):
        """(has a communicator, rank, world)"""
        r, w = ctypes.c_int(0), ctypes.c_int(1)
        has = self._lib.mifc_comm_info(self._ctx, ctypes.cast(ctypes.pointer(r), ctypes.c_void_p), ctypes.cast(ctypes.pointer(w), ctypes.c_void_p))
        return bool(has), r.value, w.value

    def slab_plan(self, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in=SOME_DEFINED, undef=UNDEF,
                  n_undefined=None):
        """mifc_slab_plan_create on device tensors: u_halo, v_halo (nlev, ny_local + 2, nx) or (ny_local + 2, nx); xmapr, ymapr
        (ny_local, nx); rvort, diverg (nlev, ny_local, nx) or (ny_local, nx); n_undefined int64[nlev].  -> SlabPlan"""
        return SlabPlan(self, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in, undef, n_undefined)

    def halo_copy_enqueue(self, dst, src_ctx, src):
        """dst (tensor on this context's device) <- src (tensor on src_ctx's device), see mifc_halo_copy_enqueue."""
        if dst.numel() != src.numel() or not dst.is_contiguous() or not src.is_contiguous():
            raise ValueError("halo rows must be contiguous and of equal length")
        return bool(self._call("mifc_halo_copy_enqueue", [dst.data_ptr(), src_ctx._ctx, src.data_ptr(), dst.numel()]))


class SlabPlan:
    """One rank's row slab of a horizontally decomposed level batch, bound to its buffers (mifc_slab_plan_*): step() enqueues
    the whole decomposed step -- RCCL halo exchange, interior rows meanwhile, boundary strips, count all-reduce -- as one
    call that replays a HIP graph; begin() / finish() bracket a halo exchange the caller does itself."""

    def __init__(self, ctx, nx, ny_global, j0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in, undef, n_undefined):
        a = [_Arg(x, allow_none=True) for x in (u_halo, v_halo, xmapr, ymapr, rvort, diverg)]
        nlev = u_halo.shape[0] if u_halo.dim() == 3 else 1
        halo_shape = (nlev, ny_local + 2, nx) if u_halo.dim() == 3 else (ny_local + 2, nx)
        out_shape = (nlev, ny_local, nx) if u_halo.dim() == 3 else (ny_local, nx)
        if not _same_shape(a[:2], halo_shape) or not _same_shape(a[2:4], (ny_local, nx)) or not _same_shape(a[4:], out_shape):
            raise ValueError("u_halo, v_halo must be ([nlev,] ny_local + 2, nx); xmapr, ymapr (ny_local, nx); rvort, diverg ([nlev,] ny_local, nx)")
        if _memkind(a, ctx.device) != MEM_DEVICE:
            raise ValueError("a slab plan takes device tensors only")
        if n_undefined is not None and n_undefined.numel() < nlev:
            raise ValueError("n_undefined needs one int64 per level")
        self._ctx, self._keep = ctx, (u_halo, v_halo, xmapr, ymapr, rvort, diverg, n_undefined)
        ctx._bind_stream(MEM_DEVICE)
        self._plan = ctx._lib.mifc_slab_plan_create(ctx._ctx, int(nx), int(ny_global), int(j0), int(ny_local), int(nlev), *[x.addr for x in a],
                                                    int(fdefined_in), float(undef), None if n_undefined is None else n_undefined.data_ptr())
        if not self._plan:
            raise RuntimeError("mifc_slab_plan_create: " + (ctx.last_error() or "invalid arguments"))

    def _run(self, name):
        self._ctx._bind_stream(MEM_DEVICE)
        if not getattr(self._ctx._lib, name)(self._plan):
            raise RuntimeError("%s: %s" % (name, self._ctx.last_error()))
        return True

    def step(self):
        return self._run("mifc_slab_plan_step")

    def begin(self):
        return self._run("mifc_slab_plan_begin")

    def finish(self):
        return self._run("mifc_slab_plan_finish")

    @property
    def uses_graph(self):
        return bool(self._ctx._lib.mifc_slab_plan_uses_graph(self._plan))

    def close(self):
        if self._plan:
            self._ctx._lib.mifc_slab_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Graph:
    """A recorded sequence of asynchronous calls (mifc_graph_begin / _end / _launch).  The tensors passed to the recorded
    calls must stay alive and in place for as long as the graph is launched: the graph holds their addresses."""

    def __init__(self, ctx, max_levels_per_call=0, lanes=1):
        self._ctx, self._graph, self._max, self._lanes = ctx, None, int(max_levels_per_call), int(lanes)

    def __enter__(self):
        self._ctx._bind_stream(MEM_DEVICE)
        self._ctx._frozen_stream = True  # the recorded calls must not re-bind the stream
        if not self._ctx._lib.mifc_graph_begin_lanes(self._ctx._ctx, self._max, self._lanes):
            self._ctx._frozen_stream = False
            raise RuntimeError("mifc_graph_begin: " + self._ctx.last_error())
        return self

    def __exit__(self, *exc):
        self._graph = self._ctx._lib.mifc_graph_end(self._ctx._ctx)
        self._ctx._frozen_stream = False
        if exc[0] is None and not self._graph:
            raise RuntimeError("mifc_graph_end: " + self._ctx.last_error())
        return False

    def lane(self, k):
        if not self._ctx._lib.mifc_graph_lane(self._ctx._ctx, int(k)):
            raise RuntimeError("mifc_graph_lane: " + self._ctx.last_error())

    def launch(self):
        self._ctx._bind_stream(MEM_DEVICE)
        if not self._ctx._lib.mifc_graph_launch(self._graph):
            raise RuntimeError("mifc_graph_launch: " + self._ctx.last_error())
        return True

    def close(self):
        if self._graph:
            self._ctx._lib.mifc_graph_destroy(self._graph)
            self._graph = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedCalls:
    """The C calls of a recorded wrapper sequence (Context.prepare), ready to be repeated: launch() is one ctypes call per
    recorded call, with the arguments converted once."""

    def __init__(self, ctx, recorded):
        self._ctx = ctx
        self._keep = [k for _, _, _, k in recorded]
        self._calls = []
        for name, fn, cargs, _ in recorded:
            conv = tuple(t(a) if a is not None else None for t, a in zip(fn.argtypes[1:], cargs))
            self._calls.append((name, fn, conv))
        self._ctxp = ctypes.c_void_p(ctx._ctx) if not isinstance(ctx._ctx, ctypes.c_void_p) else ctx._ctx

    def launch(self):
        c = self._ctxp
        for name, fn, cargs in self._calls:
            if not fn(c, *cargs):
                raise RuntimeError("%s: %s" % (name, self._ctx.last_error()))
        return True

    def __len__(self):
        return len(self._calls)
