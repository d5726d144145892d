"""The backward pass of a dense layer Y = act(X W + b), float32 (include/laser_hip.h "Dense-layer backward"):

    laser_amd.bias_grad(dy, y=None, activation=None, dz=None, out=None) -> (db, dz)
        dz = dy * f'(y) by the rule of activation_grad (dz = dy without an activation) and db[j] = reduce_sum(dz[:, j]),
        both from one read of dy and y
    laser_amd.linear_backward(x, w, dy, y=None, activation=None, need_dx=True) -> (dx, dw, db)
        one bias_grad call, then dw = matmul(x.T, dz) and dx = matmul(dz, w.T) on the strided GEMM

and layer normalization over the rows of a matrix, forward and backward (include/laser_hip.h "Layer normalization"):

    laser_amd.layer_norm(x, gamma=None, beta=None, eps=1e-5, out=None, stats=True) -> (y, mean, rstd)
    laser_amd.layer_norm_backward(dy, x, mean, rstd, gamma=None, need_dx=True, need_params=True) -> (dx, dgamma, dbeta)

and the embedding layer, a row gather by int32 ids with a deterministic gradient (include/laser_hip.h "Embedding"):

    laser_amd.embedding(w, idx, out=None) -> y                                   y[..., :] = w[idx[...], :], a bit copy
    laser_amd.embedding_group(idx, vocab) -> (order, starts)                     the stable grouping of the positions by id
    laser_amd.embedding_backward(dy, idx, vocab, out=None, group=None) -> dw     dw[v, :] = reduce_sum over the tokens of id v

With matmul(..., bias=, activation=) as the forward layer, softmax_cross_entropy(grad=True) as the loss and sgd_step or
adam_step (laser_amd/optim.py) for the update of every parameter in one launch, a multi-layer perceptron trains without
leaving the device, every bit of every step defined by the headers.
Operands are laser_amd.Tensors or torch CUDA tensors; calls are asynchronous on the current torch stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from .primitives import ACTIVATIONS, matmul
from .foreach import _View
from .simd_math import _f32
from .tensor import _stream, newTensor

__all__ = ["bias_grad", "linear_backward", "layer_norm", "layer_norm_backward", "embedding", "embedding_group", "embedding_backward"]


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


# ---- embedding ----------------------------------------------------------------------------------------------------------------
EMBEDDING_MAX_TOKENS = 1 << 26
EMBEDDING_MAX_VOCAB = 1 << 30


def _emb_ids(fn, name, obj, count=None):
    """the view of a contiguous int32 operand of any shape (`count`: the number of elements it must have)"""
    v = _View(name, obj)
    if v.dtype == np.int64:
        raise ValueError(f"{fn}: {name} is int64; convert it to int32 (int64 ids are not built: the samplers return int32)")
    if v.dtype != np.int32:
        raise TypeError(f"{fn}: {name} has element type {v.dtype} (int32 only)")
    acc = 1
    for e, st in zip(reversed(v.shape), reversed(v.strides)):
        if e > 1 and st != acc:
            raise ValueError(f"{fn}: {name} has shape {v.shape}, strides {v.strides} (contiguous is needed)")
        acc *= e
    if count is not None and acc != count:
        raise ValueError(f"{fn}: {name} has {acc} elements, {count} are needed")
    return v, acc


def _emb_rows(fn, name, obj, lead, dim):
    """(view, row stride) of a (tokens, dim) operand: contiguous of shape lead + (dim,), or a 2-D (tokens, dim) view with unit
    column stride"""
    tokens = 1
    for e in lead:
        tokens *= e
    v, rows, n, stride = _ln_rows(fn, name, obj)
    if v.shape != tuple(lead) + (dim,) and v.shape != (tokens, dim):
        raise ValueError(f"{fn}: {name} has shape {v.shape}, {tuple(lead) + (dim,)} or {(tokens, dim)} is needed")
    return v, stride


def _emb_vocab(fn, vocab):
    vocab = int(vocab)
    if vocab < 0 or vocab > EMBEDDING_MAX_VOCAB:
        raise ValueError(f"{fn}: vocab = {vocab} (0 <= vocab <= 2^30)")
    return vocab


def embedding(w, idx, out=None):
    """y[..., :] = w[idx[...], :], a bit copy (NaN payloads and -0 survive).  `w` is a 2-D (vocab, dim) device tensor or view
    with unit column stride; `idx` is a contiguous int32 tensor of any shape -- what the samplers return and the cross-entropy
    takes.  An id of -1 gives a row of +0, any other id outside [0, vocab) a row of NaN.  `out`: the destination, contiguous
    of shape idx.shape + (dim,) or a 2-D (tokens, dim) view (None: a fresh Tensor); it may not overlap `w`."""
    fn = "embedding"
    vw, vocab, dim, ws = _ln_rows(fn, "w", w)
    if vw.rank != 2:
        raise ValueError(f"{fn}: w has rank {vw.rank} (a 2-D (vocab, dim) tensor or view is needed)")
    vi, tokens = _emb_ids(fn, "idx", idx)
    if tokens > EMBEDDING_MAX_TOKENS or vocab > EMBEDDING_MAX_VOCAB:
        raise ValueError(f"{fn}: {tokens} tokens, vocab {vocab} (tokens <= 2^26, vocab <= 2^30)")
    if out is None:
        out = newTensor(np.float32, *(vi.shape + (dim,)))
    vy, ys = _emb_rows(fn, "out", out, vi.shape, dim)
    if tokens:
        _lib.check(_lib.lib().laser_hip_embedding_f32_dev(_ptr(vy), ys, _ptr(vw), ws, _ptr(vi), tokens, vocab, dim, _stream()))
    return out


def embedding_group(idx, vocab):
    """The stable grouping of the token positions by id: (order, starts), int32 Tensors of idx.size and vocab + 1 elements.
    `order` holds the positions of the tokens with 0 <= id < vocab sorted by (id, position), then all other positions in
    ascending order; id v owns order[starts[v] : starts[v + 1]].  Pass the pair as embedding_backward(group=) when one id
    vector feeds several tables."""
    fn = "embedding_group"
    vocab = _emb_vocab(fn, vocab)
    vi, tokens = _emb_ids(fn, "idx", idx)
    if tokens > EMBEDDING_MAX_TOKENS:
        raise ValueError(f"{fn}: {tokens} tokens (tokens <= 2^26)")
    order, starts = newTensor(np.int32, tokens), newTensor(np.int32, vocab + 1)
    _lib.check(_lib.lib().laser_hip_embedding_group_i32_dev(_ptr(_View("order", order)), _ptr(_View("starts", starts)), _ptr(vi), tokens,
                                                            vocab, _stream()))
    return order, starts


def embedding_backward(dy, idx, vocab, out=None, group=None):
    """The gradient of embedding's table: dw[v, j] = the sum of dy[t, j] over the tokens t of id v, in token order, in the
    order of reduce_sum applied to that sequence alone -- the same bits on every run, grid and stream; with vocab = 1 and
    every id 0 they are bias_grad(dy)[0]'s.  Every element of dw is written (+0 for an id that never occurs); tokens whose id
    is outside [0, vocab), -1 included, contribute nothing.  `dy` is contiguous of shape idx.shape + (dim,) or a 2-D
    (tokens, dim) view with unit column stride; `out`: a 2-D (vocab, dim) tensor or view (None: fresh); `group`: the pair
    embedding_group(idx, vocab) returned (None: grouped here)."""
    fn = "embedding_backward"
    vocab = _emb_vocab(fn, vocab)
    vi, tokens = _emb_ids(fn, "idx", idx)
    if tokens > EMBEDDING_MAX_TOKENS:
        raise ValueError(f"{fn}: {tokens} tokens (tokens <= 2^26)")
    vdy = _f32("dy", dy)
    if vdy.rank < 2:
        raise ValueError(f"{fn}: dy has rank {vdy.rank} (idx.shape + (dim,) or (tokens, dim) is needed)")
    dim = vdy.shape[-1]
    vdy, dys = _emb_rows(fn, "dy", dy, vi.shape, dim)
    if out is None:
        out = newTensor(np.float32, vocab, dim)
    vdw, rows, n, dws = _ln_rows(fn, "out", out)
    if vdw.shape != (vocab, dim):
        raise ValueError(f"{fn}: out has shape {vdw.shape}, {(vocab, dim)} is needed")
    vo = vs = None
    if group is not None:
        try:
            order, starts = group
        except (TypeError, ValueError):
            raise ValueError(f"{fn}: group is the pair (order, starts) of embedding_group")
        vo, _ = _emb_ids(fn, "group[0] (order)", order, tokens)
        vs, _ = _emb_ids(fn, "group[1] (starts)", starts, vocab + 1)
    if vocab:
        _lib.check(_lib.lib().laser_hip_embedding_grad_f32_dev(_ptr(vdw), dws, _ptr(vdy), dys, _ptr(vi), _ptr(vo), _ptr(vs), tokens, vocab,
                                                               dim, _stream()))
    return out
