"""Laser's table-driven exp and the row softmax on top of it (laser/primitives/simd_math/exp_log_*.nim; include/laser_hip.h
"exp and row softmax"), float32:

    laser_amd.exp(t)        lexp of every element: the exported SIMD `exp*` of the reference, bit for bit
    laser_amd.softmax(t)    softmax over the rows of a 2-D tensor, summed in the fixed order of the reductions

An operand is a laser_amd.Tensor or a torch CUDA tensor (anything with __cuda_array_interface__); `exp` also takes a host
float32 numpy array, like the reference's benchmark loop.  With out=None a device call returns a fresh row-major Tensor;
with `out` it writes there (out may be the input) and returns it.  Device calls are asynchronous on the current torch
stream.  Inside forEach / forEachReduce bodies the same function is `laser_exp(x)`.
"""
import ctypes as C

import numpy as np

from . import _lib
from .foreach import _View
from .tensor import _bcast_strides, _stream, newTensor


def _f32(name, obj):
    v = _View(name, obj)
    if v.dtype != np.float32:
        raise TypeError(f"{name}: element type {v.dtype} (float32 only)")
    return v


def exp(t, out=None):
    """lexp(t), elementwise.  `t` broadcasts against `out` like numpy; out=None: a fresh Tensor of t's shape."""
    if isinstance(t, np.ndarray):   # the host-pointer form: contiguous float32, synchronous
        if t.dtype != np.float32:
            raise TypeError(f"host arrays: float32 only (got {t.dtype})")
        if out is not None:
            raise TypeError("out= is for device inputs; a host array returns its result")
        a = np.ascontiguousarray(t)
        r = np.empty_like(a)
        _lib.check(_lib.lib().laser_hip_exp_f32(r.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), a.size))
        return r
    src = _f32("t", t)
    if out is None:
        out = newTensor(np.float32, *src.shape)
    dst = _f32("out", out)
    r = dst.rank
    arr = lambda v: (C.c_int64 * max(r, 1))(*v)
    _lib.check(_lib.lib().laser_hip_exp_f32_dev(C.c_void_p(dst.ptr), arr(dst.strides), C.c_void_p(src.ptr),
                                                arr(_bcast_strides(src, dst.shape)), arr(dst.shape), r, _stream()))
    return out


def softmax(t, out=None):
    """Softmax over the rows of the 2-D `t` (last stride 1): y = lexp(x - max) / sum, the sum in the order of reduce_sum, so
    a row's result depends on its values and length alone.  A NaN in a row, or a row of all -Inf, gives a NaN row."""
    src = _f32("t", t)
    if out is None:
        out = newTensor(np.float32, *src.shape)
    dst = _f32("out", out)
    for name, v in (("t", src), ("out", dst)):
        if v.rank != 2:
            raise ValueError(f"softmax: {name} has rank {v.rank} (a 2-D tensor is needed)")
        if v.shape[1] != 1 and v.strides[1] != 1:
            raise ValueError(f"softmax: {name} has last stride {v.strides[1]} (the elements of a row must be contiguous)")
    if dst.shape != src.shape:
        raise ValueError(f"softmax: out has shape {dst.shape}, t has {src.shape}")
    rows, n = src.shape
    if n < 1:
        raise ValueError("softmax: empty rows")
    # a single row has no row stride to speak of
    ds, ss = (dst.strides[0], src.strides[0]) if rows > 1 else (n, n)
    _lib.check(_lib.lib().laser_hip_softmax_rows_f32_dev(C.c_void_p(dst.ptr), ds, C.c_void_p(src.ptr), ss, rows, n, _stream()))
    return out
