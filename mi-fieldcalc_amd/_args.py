"""What the wrapper methods do alike before and after a C call: field arguments (_Arg), the shapes a family of methods
accepts, and the small helpers of a level-batch call -- the output, the host tables of pointers and flags, the result."""
import ctypes

import numpy as np

from ._consts import MEM_DEVICE, MEM_HOST, SOME_DEFINED


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class _Arg:
    """Address + keep-alive of one field argument.

    levels=True accepts a (nlev, ny, nx) device tensor whose levels are padded
    (stride(0) >= ny*nx, every level itself contiguous): ``lstride`` is that
    level stride in floats.  output=True refuses host arrays that would have to
    be converted (the caller's array would never be written)."""

    __slots__ = ("addr", "keep", "device", "shape", "dev_index", "lstride")

    def __init__(self, x, allow_none=False, levels=False, output=False):
        self.dev_index, self.lstride = None, None
        if x is None:
            if not allow_none:
                raise ValueError("missing field argument")
            self.addr, self.keep, self.device, self.shape = None, None, None, None
            return
        if _is_torch(x):
            import torch

            if x.dtype != torch.float32:
                raise ValueError("device fields must be float32 tensors")
            if not x.is_cuda:
                raise ValueError("torch tensors must live on the GPU; pass numpy arrays for host memory")
            if levels and x.dim() == 3 and not x.is_contiguous():
                nlev, ny, nx = x.shape
                if x.stride(2) != 1 or x.stride(1) != nx or x.stride(0) < ny * nx or x.stride(0) % 4 != 0:
                    raise ValueError("a level batch must be (nlev, ny, nx) with contiguous levels and a level stride that is a multiple of 4")
            elif not x.is_contiguous():
                raise ValueError("device fields must be contiguous float32 tensors")
            self.addr, self.keep, self.device, self.shape = x.data_ptr(), x, True, tuple(x.shape)
            self.dev_index = x.device.index
            if levels and x.dim() == 3:
                self.lstride = int(x.stride(0)) if x.shape[0] > 1 else int(x.shape[1] * x.shape[2])
        else:
            if output and not (isinstance(x, np.ndarray) and x.dtype == np.float32 and x.flags["C_CONTIGUOUS"]):
                raise ValueError("an output array must be a C-contiguous float32 numpy array (or a CUDA tensor)")
            a = np.ascontiguousarray(x, dtype=np.float32)  # forcecast, like py_mi_fieldcalc.cc:40
            self.addr, self.keep, self.device, self.shape = a.ctypes.data, a, False, a.shape
            if levels and a.ndim == 3:
                self.lstride = int(a.shape[1] * a.shape[2])


def _memkind(args, ctx_device=None):
    present = [a for a in args if a.addr is not None]
    kinds = {a.device for a in present}
    if len(kinds) != 1:
        raise ValueError("all fields of one call must be either numpy (host) or CUDA tensors (device)")
    if ctx_device is not None:
        for a in present:
            if a.device and a.dev_index is not None and a.dev_index != ctx_device:
                raise ValueError("a tensor lives on cuda:%d but this Context was created on device %d" % (a.dev_index, ctx_device))
    return MEM_DEVICE if kinds.pop() else MEM_HOST


def _same_shape(args, shape):
    return all(a.addr is None or tuple(a.shape) == tuple(shape) for a in args)


def _empty_like(ref, shape=None):
    if _is_torch(ref):
        import torch

        return torch.empty(shape or ref.shape, dtype=torch.float32, device=ref.device)
    return np.empty(shape or np.shape(ref), dtype=np.float32)


# ------------------------------------------------------------------------------ the pieces of a level-batch call
def _kept(out, oa):
    """What a method hands back for an output: the caller's tensor itself, or the array its _Arg kept."""
    return out if _is_torch(out) else oa.keep


def _output(out, ref, shape, message=None, fill=None):
    """The output of a call, `out` or a new array / tensor of `shape` where `ref` lives (fill: pre-filled with that
    value): (the object to hand back, its _Arg).  A given `out` of another shape raises ValueError."""
    if out is None:
        out = _empty_like(ref, shape)
        if fill is not None:
            out[...] = float(np.float32(fill))
    oa = _Arg(out, output=True)
    if tuple(oa.shape) != tuple(shape):
        raise ValueError(message or "out must have shape %s" % (shape,))
    return _kept(out, oa), oa


def _pointer_table(addrs, least=0):
    """The host table of pointers a C entry takes for its fields: the caller keeps it alive and passes its addressof()."""
    return (ctypes.c_void_p * max(len(addrs), least))(*addrs)


def _stacked_table(base, n, stride, least=0):
    """The table of pointers to the n parts, `stride` bytes apart, of one stacked output or input at `base`."""
    return _pointer_table([base + k * stride for k in range(n)], least)


def _field_tables(fa, oa, stride):
    """The two tables most level-batch entries take: the fields, and the parts of the stacked output `oa`, one per field."""
    return _pointer_table([a.addr for a in fa]), _stacked_table(oa.addr, len(fa), stride)


def _flag_table(fdefined, nlev, default=SOME_DEFINED):
    """Per-level flags as a fresh int32[nlev] the C side may write into; None gives `default` on every level."""
    return np.full(nlev, default, np.int32) if fdefined is None else np.array(fdefined, dtype=np.int32).reshape(nlev).copy()


def _drop_one(one, res, fd):
    """(res, fd), without the leading axis of the flags for ONE batch (res was shaped without it already)."""
    return (res, fd[0]) if one else (res, fd)


def _parse_form(text, strings=()):
    """The "key=value ..." text of a mifc_last_*_form entry as a dict: the keys in `strings` as they are, the others as ints."""
    form = dict(word.split("=", 1) for word in text.decode().split())
    return {k: (v if k in strings else int(v)) for k, v in form.items()}


# ------------------------------------------------ what the level-batch methods (vinterp, vlayer, vderiv) take alike
def _level_batches(fields):
    """One (nlev, ny, nx) batch, a stacked (nf, nlev, ny, nx) array / tensor or a sequence of batches: (was it one, the
    batches, their _Arg, the shape of a batch)."""
    one = (isinstance(fields, np.ndarray) or _is_torch(fields)) and len(fields.shape) == 3
    if one:
        batches = [fields]
    elif isinstance(fields, np.ndarray) or _is_torch(fields):
        batches = [fields[f] for f in range(fields.shape[0])]
    else:
        batches = list(fields)
    if not batches:
        raise ValueError("no fields")
    fa = [_Arg(b) for b in batches]
    shape = tuple(fa[0].shape)
    if len(shape) != 3:
        raise ValueError("fields must be (nlev, ny, nx) batches")
    if not _same_shape(fa, shape):
        raise ValueError("every field must have the shape %s" % (shape,))
    return one, batches, fa, shape


def _member_batch(fields, fdefined_in, fallback):
    """What ensembleQuantiles and ensembleStatistics take alike: `fields` and `fdefined_in` as their docstrings say; fallback: the
    member shape taken from the output, for a call without members, or None.  Returns (the members, their _Arg, shape, nlev,
    ny, nx, the pointer table, the (nmem, nlev) int32 flags or None)."""
    members = [fields[j] for j in range(fields.shape[0])] if isinstance(fields, np.ndarray) or _is_torch(fields) else list(fields)
    fa = [_Arg(m) for m in members]
    if fa:
        shape = tuple(fa[0].shape)
    elif fallback is not None:
        shape = tuple(fallback)
    else:
        raise ValueError("no member fields and no output to take the shape from")
    if len(shape) not in (2, 3):
        raise ValueError("members must be (ny, nx) or (nlev, ny, nx) fields")
    if not _same_shape(fa, shape):
        raise ValueError("every member must have the shape %s" % (shape,))
    nlev = shape[0] if len(shape) == 3 else 1
    flags = None
    if fdefined_in is not None:
        f = np.asarray(fdefined_in, dtype=np.int32)
        if f.ndim == 1:
            f = np.repeat(f[:, None], nlev, axis=1)
        flags = np.ascontiguousarray(f.reshape(len(fa), nlev), dtype=np.int32)
    return members, fa, shape, nlev, shape[-2], shape[-1], _pointer_table([a.addr for a in fa], 1), flags


def _level_coord(coord, hybrid, shape):
    """The coordinate argument: ps (ny, nx) of the hybrid form, else a batch like the fields."""
    ca = _Arg(coord)
    want = shape[1:] if hybrid else shape
    if tuple(ca.shape) != want:
        raise ValueError("the coordinate must have the shape %s" % (want,))
    return ca


def _level_flags(fdefined_in, nf, nlev):
    """fdefined_in as the (nf, nlev) table the C entries take, None as it is: one flag per field stands for every level
    (nlev >= 2: never mistaken for the full table).  A pair call passes nf = 2 * npairs: its fdefined_in is (2,), (2, nlev),
    (npairs, 2) or (npairs, 2, nlev)."""
    if fdefined_in is None:
        return None
    f = np.asarray(fdefined_in, dtype=np.int32)
    if f.size == nf:
        f = np.repeat(f.reshape(nf, 1), nlev, axis=1)
    return np.ascontiguousarray(f.reshape(nf, nlev), dtype=np.int32)


def _hybrid_levels(fields, alevel, blevel):
    al = np.ascontiguousarray(np.asarray(alevel, dtype=np.float32).ravel())
    bl = np.ascontiguousarray(np.asarray(blevel, dtype=np.float32).ravel())
    nlev = int(fields[0].shape[-3]) if not hasattr(fields, "shape") else int(fields.shape[-3])
    if al.size != nlev or bl.size != nlev:
        raise ValueError("alevel and blevel must hold one value per level")
    return al, bl


def _coord_flags(fdef_coord, coord):
    if fdef_coord is None:
        return None
    fc_ = np.ascontiguousarray(np.asarray(fdef_coord, dtype=np.int32).ravel())
    if fc_.size != int(_Arg(coord).shape[0]):
        raise ValueError("fdef_coord must hold one flag per level")
    return fc_


def _pairs(pairs):
    """The components u0, v0, u1, v1 ... of `pairs` -- one pair (2, nlev, ny, nx), stacked pairs (npairs, 2, nlev, ny, nx),
    a sequence of (u, v) or the flat sequence u0, v0, u1, v1 ... of (nlev, ny, nx) batches -- as _level_batches takes
    them: (was it one pair, the batches, their _Arg, the shape of a batch)."""
    stacked = isinstance(pairs, np.ndarray) or _is_torch(pairs)
    if stacked and len(pairs.shape) not in (4, 5):
        raise ValueError("pairs must be (2, nlev, ny, nx), (npairs, 2, nlev, ny, nx) or a sequence of (u, v)")
    items = [pairs[j] for j in range(pairs.shape[0])] if stacked else list(pairs)
    if items and all(hasattr(i, "shape") and len(i.shape) == 3 for i in items):
        comps, one = items, len(items) == 2  # u, v (, u1, v1 ...)
    else:
        comps, one = [], False
        for pair in items:
            if len(pair) != 2:
                raise ValueError("a pair is (u, v)")
            comps += [pair[0], pair[1]]
    if len(comps) < 2 or len(comps) % 2:
        raise ValueError("pairs must hold u and v of every pair")
    _, batches, fa, shape = _level_batches(comps)
    return one, batches, fa, shape
