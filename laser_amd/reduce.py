"""Reductions on the device -- Laser's reduce_sum / reduce_min / reduce_max (laser/primitives/reductions.nim:48-116) and
forEachReduce, the device form of forEachStaged (laser/strided_iteration/foreach_staged.nim:318):

    forEachStaged x in a, y in b:                 laser_amd.forEachReduce("acc += x * y", merge="acc += other",
      before_loop: var local_sum = 0'f32                                    init=np.float32(0), x=a, y=b)
      in_loop:     local_sum += x * y
      after_loop:  omp_critical: result += local_sum

The order of the operations is fixed (include/laser_hip.h "Reductions"): the result is a function of the values in
logical order and the element count, never of the device, the stream or the layout.  With out=None a call returns a numpy
scalar and synchronises the current torch stream; with a one-element device `out` it writes there asynchronously.
"""
import ctypes as C

import numpy as np

from . import _lib
from .foreach import DT, _View, _device, _param
from .tensor import _bcast_strides, _stream

_SFX = {"float32": "f32", "float64": "f64", "int32": "i32", "int64": "i64"}
_handles = {}   # (device, spec) -> forEachReduce kernel handle


def _result(dtype):
    import torch
    return torch.empty(1, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")


def _finish(dev_out, dtype, out):
    """out=None: copy the one value back (synchronises the current stream); else nothing (asynchronous)."""
    if out is not None:
        return None
    h = np.empty(1, dtype)
    _lib.check(_lib.lib().laser_hip_storage_download_stream(h.ctypes.data_as(C.c_void_p), C.c_void_p(dev_out.data_ptr()),
                                                            h.nbytes, _stream()))
    return h[0]


def _out_view(out, dtype):
    v = _View("out", out)
    if v.dtype != np.dtype(dtype) or int(np.prod(v.shape, dtype=np.int64)) != 1:
        raise ValueError(f"out must be a one-element device array of {np.dtype(dtype)}, got {v.dtype} of shape {v.shape}")
    return v.ptr


def _reduce(op, t, out):
    if isinstance(t, np.ndarray):   # the host-pointer drop-in of the reference: contiguous float32
        if t.dtype != np.float32:
            raise TypeError(f"host arrays: float32 only (got {t.dtype}); move other types to the device")
        if out is not None:
            raise TypeError("out= is for device inputs; a host array returns its result")
        a = np.ascontiguousarray(t).reshape(-1)
        r = C.c_float()
        _lib.check(getattr(_lib.lib(), f"laser_hip_reduce_{op}_f32")(a.ctypes.data_as(C.c_void_p), a.size, C.byref(r)))
        return np.float32(r.value)
    v = _View("t", t)
    if v.dtype.name not in _SFX:
        raise TypeError(f"reduce_{op}: element type {v.dtype} (float32, float64, int32, int64)")
    dev_out = None
    if out is None:
        dev_out = _result(v.dtype)
        optr = dev_out.data_ptr()
    else:
        optr = _out_view(out, v.dtype)
    r = v.rank
    _lib.check(getattr(_lib.lib(), f"laser_hip_reduce_{op}_{_SFX[v.dtype.name]}_dev")(
        C.c_void_p(v.ptr), (C.c_int64 * max(r, 1))(*v.strides), (C.c_int64 * max(r, 1))(*v.shape), r, C.c_void_p(optr),
        _stream()))
    return _finish(dev_out, v.dtype, out)


def reduce_sum(t, out=None):
    """Sum of every element of `t` (a Tensor, a torch device tensor or a host float32 numpy array)."""
    return _reduce("sum", t, out)


def reduce_min(t, out=None):
    """Minimum of every element: NaN if any is NaN, -0 below +0; +Inf (integers: the type's max) when empty."""
    return _reduce("min", t, out)


def reduce_max(t, out=None):
    """Maximum of every element: NaN if any is NaN, +0 above -0; -Inf (integers: the type's min) when empty."""
    return _reduce("max", t, out)


def forEachReduce(body, *, merge, init, acc_name="acc", params=None, writable=(), out=None, **operands):
    """Run `body` once per index of the first operand's shape into private accumulators named `acc_name`, then merge them
    with `merge` (a statement over `acc_name` and `other`).  The accumulator's type is the numpy dtype of `init`, which
    must be an identity of `merge`.  `writable` operands are stored back as in forEach."""
    if not operands:
        raise ValueError("forEachReduce needs at least one operand")
    ini = np.asarray(init)
    if ini.shape != () or ini.dtype.name not in DT:
        raise TypeError(f"init must be a numpy scalar of a supported element type, got {init!r}")
    names = list(operands)
    views = [_View(n, operands[n]) for n in names]
    wset = {writable} if isinstance(writable, str) else set(writable)
    for w in wset:
        if w not in operands:
            raise ValueError(f"writable operand {w!r} is not an operand")
    shape = views[0].shape
    params = dict(params or {})
    pspec = [_param(k, v) for k, v in params.items()]
    acc_dt = DT[ini.dtype.name]
    key = (_device(), body, merge, acc_name, acc_dt, tuple(names), tuple(DT[v.dtype.name] for v in views),
           tuple(n in wset for n in names), tuple(params), tuple(p[0] for p in pspec))
    L = _lib.lib()
    h = _handles.get(key)
    if h is None:
        n, m = len(names), len(params)
        hh = C.c_int64()
        _lib.check(L.laser_hip_foreach_reduce_kernel(
            body.encode(), n, (C.c_char_p * n)(*[s.encode() for s in names]), (C.c_int * n)(*key[6]),
            (C.c_int * n)(*[int(w) for w in key[7]]), m, (C.c_char_p * max(m, 1))(*[s.encode() for s in params]),
            (C.c_int * max(m, 1))(*key[9]), acc_name.encode(), acc_dt, merge.encode(), C.byref(hh)))
        h = _handles[key] = hh.value
    r = len(shape)
    strides = []
    for name, v in zip(names, views):
        if name in wset:
            if v.shape != shape:
                raise ValueError(f"writable operand {name}: shape {v.shape} differs from the iteration shape {shape}")
            strides += v.strides
        else:
            strides += _bcast_strides(v, shape)
    dev_out = None
    if out is None:
        dev_out = _result(ini.dtype)
        optr = dev_out.data_ptr()
    else:
        optr = _out_view(out, ini.dtype)
    ptrs = (C.c_void_p * len(views))(*[v.ptr for v in views])
    prm = C.create_string_buffer(b"".join(p[1] for p in pspec), 8 * len(pspec)) if pspec else None
    slot = C.create_string_buffer(ini.tobytes().ljust(8, b"\0"), 8)
    _lib.check(L.laser_hip_foreach_reduce_dev(h, ptrs, (C.c_int64 * max(len(strides), 1))(*strides),
                                              (C.c_int64 * max(r, 1))(*shape), r, prm, slot, C.c_void_p(optr), _stream()))
    return _finish(dev_out, ini.dtype, out)
