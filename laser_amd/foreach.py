"""forEach with an arbitrary body over device arrays -- Laser's forEach (laser/strided_iteration/foreach.nim:192-264):

    forEach x in a, y in b, z in c:          laser_amd.forEach("x += y * z", x=a, y=b, z=c)
      x += y * z

The body is HIP C++ compiled at run time (laser_hip_foreach_* in include/laser_hip.h): the statement syntax of Laser's
examples is valid C++, and the device math library (expf, logf, sqrtf, fmaxf, ...) can be called, as can laser_exp(x),
Laser's own table-driven exp (laser_amd/csrc/exp_core.h, the function behind laser_amd.exp), and laser_log(x), the
bit-defined logarithm behind laser_amd.log (laser_amd/csrc/log_core.h), and laser_tanh(x) and laser_sigmoid(x), the functions
behind laser_amd.tanh and laser_amd.sigmoid (laser_amd/csrc/act_core.h), and laser_sin(x) and laser_cos(x), the bit-defined
sine and cosine behind laser_amd.sin and laser_amd.cos (laser_amd/csrc/sincos_core.h).  An operand is anything
with __cuda_array_interface__ -- a laser_amd.Tensor or a torch CUDA tensor -- of one of ten element types (f32, f64,
int8..int64, uint8..uint64), mixed freely.  The first operand gives the iteration shape and is the writable one unless
`writable` names others; writable operands have exactly that shape, read-only ones broadcast like numpy.  `params` are
scalar parameters: a numpy scalar keeps its dtype, a Python float is float64, a Python int is int64.
"""
import ctypes as C

import numpy as np

from . import _lib
from .tensor import LASER_MAXRANK, _bcast_strides, _stream

DT = {"float32": 0, "float64": 1, "int8": 2, "int16": 3, "int32": 4, "int64": 5,
      "uint8": 6, "uint16": 7, "uint32": 8, "uint64": 9}   # LASER_HIP_DT_*

_handles = {}   # (device, spec) -> kernel handle: a warm call marshals no strings and compiles nothing


class _View:
    """shape / strides in elements / address / dtype of a __cuda_array_interface__ operand"""
    __slots__ = ("shape", "strides", "ptr", "dtype", "rank")

    def __init__(self, name, obj):
        try:
            cai = obj.__cuda_array_interface__
        except AttributeError:
            raise TypeError(f"operand {name}: {type(obj).__name__} has no __cuda_array_interface__ (a device array is needed)")
        self.dtype = np.dtype(cai["typestr"])
        if self.dtype.name not in DT:
            raise TypeError(f"operand {name}: element type {self.dtype} is not supported")
        self.shape = tuple(int(s) for s in cai["shape"])
        self.rank = len(self.shape)
        if self.rank > LASER_MAXRANK:
            raise ValueError(f"operand {name}: rank {self.rank} > LASER_MAXRANK")
        st = cai.get("strides")
        if st is None:
            out, acc = [], 1
            for n in reversed(self.shape):
                out.append(acc)
                acc *= n
            self.strides = tuple(reversed(out))
        else:
            if any(s % self.dtype.itemsize for s in st):
                raise ValueError(f"operand {name}: byte strides {st} are not whole elements")
            self.strides = tuple(s // self.dtype.itemsize for s in st)
        self.ptr = cai["data"][0]


def _param(name, v):
    if isinstance(v, np.generic):
        a = np.asarray(v)
    elif isinstance(v, bool):
        raise TypeError(f"parameter {name}: bool is not an element type (pass an int or a numpy scalar)")
    elif isinstance(v, float):
        a = np.asarray(v, np.float64)
    elif isinstance(v, int):
        a = np.asarray(v, np.int64)
    else:
        raise TypeError(f"parameter {name}: {type(v).__name__} (a Python float / int or a numpy scalar is needed)")
    if a.dtype.name not in DT:
        raise TypeError(f"parameter {name}: element type {a.dtype} is not supported")
    return DT[a.dtype.name], a.tobytes().ljust(8, b"\0")


def _device():
    try:
        import torch
        return torch.cuda.current_device()
    except Exception:  # pragma: no cover
        return 0


def forEach(body, *, params=None, writable=None, **operands):
    """Run `body` for every index of the first operand's shape; returns None.  Asynchronous on the current torch stream."""
    if not operands:
        raise ValueError("forEach needs at least one operand")
    names = list(operands)
    views = [_View(n, operands[n]) for n in names]
    if writable is None:
        writable = (names[0],)
    elif isinstance(writable, str):
        writable = (writable,)
    wset = set(writable)
    for w in wset:
        if w not in operands:
            raise ValueError(f"writable operand {w!r} is not an operand")
    shape = views[0].shape
    params = dict(params or {})
    pspec = [_param(k, v) for k, v in params.items()]
    key = (_device(), body, tuple(names), tuple(DT[v.dtype.name] for v in views), tuple(n in wset for n in names),
           tuple(params), tuple(p[0] for p in pspec))
    L = _lib.lib()
    h = _handles.get(key)
    if h is None:
        n, m = len(names), len(params)
        hh = C.c_int64()
        _lib.check(L.laser_hip_foreach_kernel(
            body.encode(), n, (C.c_char_p * n)(*[s.encode() for s in names]), (C.c_int * n)(*key[3]),
            (C.c_int * n)(*[int(w) for w in key[4]]), m, (C.c_char_p * max(m, 1))(*[s.encode() for s in params]),
            (C.c_int * max(m, 1))(*key[6]), C.byref(hh)))
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
    ptrs = (C.c_void_p * len(views))(*[v.ptr for v in views])
    prm = C.create_string_buffer(b"".join(p[1] for p in pspec), 8 * len(pspec)) if pspec else None
    _lib.check(L.laser_hip_foreach_dev(h, ptrs, (C.c_int64 * max(len(strides), 1))(*strides),
                                       (C.c_int64 * max(r, 1))(*shape), r, prm, _stream()))
