"""The backward pass of a dense layer Y = act(X W + b), float32 (include/laser_hip.h "Dense-layer backward"):

    laser_amd.bias_grad(dy, y=None, activation=None, dz=None, out=None) -> (db, dz)
        dz = dy * f'(y) by the rule of activation_grad (dz = dy without an activation) and db[j] = reduce_sum(dz[:, j]),
        both from one read of dy and y
    laser_amd.linear_backward(x, w, dy, y=None, activation=None, need_dx=True) -> (dx, dw, db)
        one bias_grad call, then dw = matmul(x.T, dz) and dx = matmul(dz, w.T) on the strided GEMM

and layer normalization over the rows of a matrix, forward and backward (include/laser_hip.h "Layer normalization"):

    laser_amd.layer_norm(x, gamma=None, beta=None, eps=1e-5, out=None, stats=True) -> (y, mean, rstd)
    laser_amd.layer_norm_backward(dy, x, mean, rstd, gamma=None, need_dx=True, need_params=True) -> (dx, dgamma, dbeta)

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

__all__ = ["bias_grad", "linear_backward", "layer_norm", "layer_norm_backward"]


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


# ---- layer normalization ------------------------------------------------------------------------------------------------------
LAYER_NORM_MAX_N = 1 << 26


def _ln_rows(fn, name, obj, shape=None):
    """(view, rows, n, row stride) of a row operand: a 2-D tensor or view whose columns have unit stride, or a C-contiguous
    tensor of higher rank, taken as (prod(leading), n)"""
    v = _f32(name, obj)
    if v.rank < 2:
        raise ValueError(f"{fn}: {name} has rank {v.rank} (rows of a 2-D tensor or view, or a contiguous tensor of higher rank)")
    if shape is not None and v.shape != shape:
        raise ValueError(f"{fn}: {name} has shape {v.shape}, {shape} is needed")
    n = v.shape[-1]
    if n < 1 or n > LAYER_NORM_MAX_N:
        raise ValueError(f"{fn}: {name} has rows of {n} elements (1 <= n <= 2^26)")
    if v.rank == 2:
        rows = v.shape[0]
        if n > 1 and v.strides[1] != 1:
            raise ValueError(f"{fn}: {name} has column stride {v.strides[1]} (1 is needed: transposed views are not taken)")
        return v, rows, n, (v.strides[0] if rows > 1 else n)  # (the stride of a lone row is never applied)
    rows, acc = 1, 1
    for e, st in zip(reversed(v.shape), reversed(v.strides)):
        if e > 1 and st != acc:
            raise ValueError(f"{fn}: {name} of rank {v.rank} has strides {v.strides} (C-contiguous is needed above rank 2)")
        acc *= e
    for e in v.shape[:-1]:
        rows *= e
    return v, rows, n, n


def _ln_vector(fn, name, obj, shape):
    """(view, stride) of `count` elements, one per row or per column: a 1-D tensor or view of any stride, or a C-contiguous
    tensor of the shape given"""
    v = _f32(name, obj)
    count = 1
    for e in shape:
        count *= e
    if v.rank == 1 and v.shape == (count,):
        return v, (v.strides[0] if count > 1 else 1)
    acc = 1
    for e, st in zip(reversed(v.shape), reversed(v.strides)):
        if e > 1 and st != acc:
            break
        acc *= e
    else:
        if v.shape == tuple(shape):
            return v, 1
    raise ValueError(f"{fn}: {name} has shape {v.shape}, strides {v.strides} (({count},) or contiguous {tuple(shape)} is needed)")


def _ptr(v):
    return C.c_void_p(v.ptr) if v is not None and v.ptr else None


def layer_norm(x, gamma=None, beta=None, eps=1e-5, out=None, stats=True):
    """Every row of `x` normalized to mean 0 and variance 1, then scaled by gamma and shifted by beta, each float32 operation
    rounded on its own and every sum in reduce_sum's order: mean = rsum(x) / n, d = x - mean, var = rsum(d * d) / n,
    rstd = 1 / sqrt(var + eps), y = (d * rstd) * gamma + beta (no multiply without gamma, no add without beta).  `x` is a 2-D
    (rows, n) device tensor or view with unit column stride, or a contiguous tensor of higher rank taken as
    (prod(leading), n); `gamma` and `beta` are 1-D of n elements; `out` takes y and may be `x`.  Returns (y, mean, rstd): the
    statistics the backward pass needs, fresh Tensors of x's leading shape, or None, None with stats=False (inference).
    eps = 0 is allowed and follows IEEE (a constant row gives NaN)."""
    eps = float(eps)
    if not eps >= 0.0:
        raise ValueError(f"layer_norm: eps = {eps!r} (eps >= 0 is needed)")
    vx, rows, n, xs = _ln_rows("layer_norm", "x", x)
    vg, gs = _ln_vector("layer_norm", "gamma", gamma, (n,)) if gamma is not None else (None, 1)
    vb, bs = _ln_vector("layer_norm", "beta", beta, (n,)) if beta is not None else (None, 1)
    if out is None:
        out = newTensor(np.float32, *vx.shape)
    vy, _, _, ys = _ln_rows("layer_norm", "out", out, vx.shape)
    mean = newTensor(np.float32, *vx.shape[:-1]) if stats else None
    rstd = newTensor(np.float32, *vx.shape[:-1]) if stats else None
    vm = _f32("mean", mean) if stats else None
    vr = _f32("rstd", rstd) if stats else None
    _lib.check(_lib.lib().laser_hip_layer_norm_f32_dev(_ptr(vy), ys, _ptr(vm), 1, _ptr(vr), 1, _ptr(vx), xs, _ptr(vg), gs, _ptr(vb), bs,
                                                       rows, n, eps, _stream()))
    return out, mean, rstd


def layer_norm_backward(dy, x, mean, rstd, gamma=None, need_dx=True, need_params=True):
    """The gradients of layer_norm from the incoming gradient `dy`, the forward INPUT `x`, the saved `mean` and `rstd` and
    `gamma`: with xhat = (x - mean) * rstd and g = dy * gamma (dy without gamma), dx = ((g - rsum(g) / n) - xhat *
    (rsum(g * xhat) / n)) * rstd, dbeta[j] = reduce_sum(dy[:, j]) -- the bits of bias_grad(dy)[0] -- and dgamma[j] =
    reduce_sum((dy * xhat)[:, j]).  need_dx: True for a fresh Tensor, False for none, or the destination, which may be `dy` or
    `x`; need_params: True for both parameter gradients, False for none, "gamma" or "beta" for one alone (rows <= 2^26).
    What is asked for has the same bits whatever else is asked for.  Returns (dx, dgamma, dbeta), None where not asked for."""
    fn = "layer_norm_backward"
    if need_params not in (True, False, "gamma", "beta"):
        raise ValueError(f'{fn}: need_params = {need_params!r} (True, False, "gamma" or "beta")')
    vdy, rows, n, dys = _ln_rows(fn, "dy", dy)
    vx, _, _, xs = _ln_rows(fn, "x", x, vdy.shape)
    vm, ms = _ln_vector(fn, "mean", mean, vdy.shape[:-1])
    vr, rs = _ln_vector(fn, "rstd", rstd, vdy.shape[:-1])
    vg, gs = _ln_vector(fn, "gamma", gamma, (n,)) if gamma is not None else (None, 1)
    if need_dx is False:
        dx, vdx, dxs = None, None, 0
    else:
        dx = newTensor(np.float32, *vdy.shape) if need_dx is True else need_dx
        vdx, _, _, dxs = _ln_rows(fn, "dx", dx, vdy.shape)
    dgamma = newTensor(np.float32, n) if need_params in (True, "gamma") else None
    dbeta = newTensor(np.float32, n) if need_params in (True, "beta") else None
    if dx is None and dgamma is None and dbeta is None:
        raise ValueError(f"{fn}: nothing is asked for (need_dx and need_params are both False)")
    vdg = _f32("dgamma", dgamma) if dgamma is not None else None
    vdb = _f32("dbeta", dbeta) if dbeta is not None else None
    if rows == 0 and vdg is None and vdb is None:
        return dx, dgamma, dbeta  # (no rows, no column sums: nothing to compute, and an empty dx has no address to pass)
    _lib.check(_lib.lib().laser_hip_layer_norm_grad_f32_dev(_ptr(vdx), dxs, _ptr(vdg), 1, _ptr(vdb), 1, _ptr(vdy), dys, _ptr(vx), xs,
                                                            _ptr(vm), ms, _ptr(vr), rs, _ptr(vg), gs, rows, n, _stream()))
    return dx, dgamma, dbeta
