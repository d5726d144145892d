"""The backward pass of a dense layer Y = act(X W + b), float32 (include/laser_hip.h "Dense-layer backward"):

    laser_amd.bias_grad(dy, y=None, activation=None, dz=None, out=None) -> (db, dz)
        dz = dy * f'(y) by the rule of activation_grad (dz = dy without an activation) and db[j] = reduce_sum(dz[:, j]),
        both from one read of dy and y
    laser_amd.linear_backward(x, w, dy, y=None, activation=None, need_dx=True) -> (dx, dw, db)
        one bias_grad call, then dw = matmul(x.T, dz) and dx = matmul(dz, w.T) on the strided GEMM

With matmul(..., bias=, activation=) as the forward layer, softmax_cross_entropy(grad=True) as the loss and forEach for
`w -= lr * dw`, a multi-layer perceptron trains without leaving the device, every bit of every step defined by the headers.
Operands are laser_amd.Tensors or torch CUDA tensors; calls are asynchronous on the current torch stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from .primitives import ACTIVATIONS, matmul
from .simd_math import _f32
from .tensor import _stream, newTensor

__all__ = ["bias_grad", "linear_backward"]


def _act(activation):
    if activation not in ACTIVATIONS:
        raise ValueError(f"bias_grad: activation {activation!r} (one of {sorted(k for k in ACTIVATIONS if k)} or None)")
    return ACTIVATIONS[activation]


def _rows(name, obj, shape=None):
    """(view, row stride) of a 2-D operand whose columns have unit stride"""
    v = _f32(name, obj)
    if v.rank != 2:
        raise ValueError(f"bias_grad: {name} has rank {v.rank} (a 2-D tensor or view is needed)")
    if shape is not None and v.shape != shape:
        raise ValueError(f"bias_grad: {name} has shape {v.shape}, dy has {shape}")
    rows, n = v.shape
    if n > 1 and v.strides[1] != 1:
        raise ValueError(f"bias_grad: {name} has column stride {v.strides[1]} (1 is needed: transposed views are not taken)")
    return v, (v.strides[0] if rows > 1 else n)  # (the stride of a lone row is never applied)


def bias_grad(dy, y=None, activation=None, dz=None, out=None):
    """dz = the gradient of `activation` ("relu", "tanh", "sigmoid"; None: dz = dy) from the incoming gradient `dy` and the
    forward OUTPUT `y`, exactly activation_grad's bits, and db[j] = the sum of dz[:, j] in the order of reduce_sum applied
    to that column alone -- one pass over dy and y.  `dy`, `y` and `dz` are 2-D (rows, n) device tensors or views with
    unit column stride; rows <= 2^26.  dz=None: a fresh Tensor; dz=False: not stored (only db); dz may be `dy` or `y`.
    `out`: a 1-D tensor or view of n elements for db (None: fresh).  Returns (db, dz), dz None when it was not stored."""
    code = _act(activation)
    vdy, dys = _rows("dy", dy)
    rows, n = vdy.shape
    if code and y is None:
        raise ValueError(f"bias_grad: activation {activation!r} needs the forward output y")
    vy, ys = _rows("y", y, vdy.shape) if code else (None, 0)
    if dz is False:
        dz, vdz, dzs = None, None, 0
    else:
        if dz is None:
            dz = newTensor(np.float32, rows, n)
        vdz, dzs = _rows("dz", dz, vdy.shape)
    if out is None:
        out = newTensor(np.float32, n)
    vdb = _f32("out", out)
    if vdb.shape != (n,):
        raise ValueError(f"bias_grad: out has shape {vdb.shape}, ({n},) is needed")
    ptr = lambda v: C.c_void_p(v.ptr) if v is not None and v.ptr else None
    _lib.check(_lib.lib().laser_hip_bias_grad_f32_dev(ptr(vdb), vdb.strides[0] if n > 1 else 1, ptr(vdz), dzs, ptr(vdy), dys, ptr(vy),
                                                      ys, rows, n, code, _stream()))
    return out, dz


def linear_backward(x, w, dy, y=None, activation=None, need_dx=True):
    """The gradients of the layer Y = act(X W + b) -- X (M, K), W (K, N), as matmul takes them -- from dY (M, N) and the forward
    output Y: one bias_grad call gives dZ = dY * f'(Y) and db; dw = matmul(x.T, dz) and dx = matmul(dz, w.T) go through
    the strided GEMM in the current float mode, the transposes as strides: no operand is copied.  Returns (dx, dw, db),
    dx None with need_dx=False (the first layer of a network)."""
    db, dz = bias_grad(dy, y, activation)
    dw = matmul(x.T, dz)
    dx = matmul(dz, w.T) if need_dx else None
    return dx, dw, db
