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

and attention, the one layer of a transformer block the list above lacks (include/laser_hip.h "Attention"):

    laser_amd.attention(q, k, v, scale=None, causal=False, out=None, probs=None, stats=False)    the fused forward
    laser_amd.attention_backward(dout, q, k, v, scale=None, causal=False, need=("q", "k", "v")) -> (dq, dk, dv)

Operands are laser_amd.Tensors or torch CUDA tensors; calls are asynchronous on the current torch stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from .primitives import ACTIVATIONS, matmul
from .foreach import _View
from .simd_math import _f32
from .tensor import _stream, newTensor

__all__ = ["bias_grad", "linear_backward", "layer_norm", "layer_norm_backward", "embedding", "embedding_group", "embedding_backward",
           "attention", "attention_backward"]


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


# ---- attention ----------------------------------------------------------------------------------------------------------------
ATTENTION_MAX_D = 128
ATTENTION_MAX_KEYS = 65536


def _attn_view(fn, name, obj, width=None):
    """(view, B, H, T, width, (batch, head, position strides)) of an attention operand: a 3-D (BH, T, width) or 4-D
    (B, H, T, width) device tensor or view of any outer strides, the feature index unit-stride.  A 3-D operand is B = BH
    batches of one head."""
    v = _f32(name, obj)
    if v.rank not in (3, 4):
        raise ValueError(f"{fn}: {name} has rank {v.rank} (a 3-D (BH, T, d) or 4-D (B, H, T, d) tensor or view is needed)")
    w = v.shape[-1]
    if width is not None and w != width:
        raise ValueError(f"{fn}: {name} has {w} features, {width} are needed")
    if w > 1 and v.strides[-1] != 1:
        raise ValueError(f"{fn}: {name} has feature stride {v.strides[-1]} (1 is needed)")
    if any(s < 0 for s in v.strides[:-1]):
        raise ValueError(f"{fn}: {name} has strides {v.strides} (negative strides are not taken)")
    t = v.shape[-2]
    if v.rank == 3:
        b, h, st = v.shape[0], 1, (v.strides[0], 0, v.strides[1])
    else:
        b, h, st = v.shape[0], v.shape[1], (v.strides[0], v.strides[1], v.strides[2])
    if t > 1 and st[2] < w:
        raise ValueError(f"{fn}: {name} has position stride {st[2]} below its {w} features")
    return v, b, h, t, w, st


def _attn_scale(fn, scale, d):
    """float32(1 / sqrt(float64(d))) by default"""
    s = np.float32(1.0 / np.sqrt(np.float64(d))) if scale is None else np.float32(scale)
    return float(s)


def _i64x3(st):
    return (C.c_int64 * 3)(*st)


def attention(q, k, v, scale=None, causal=False, out=None, probs=None, stats=False):
    """O = softmax(scale * Q K^T) V per (batch, head) slice in one fused kernel: the scores never reach global memory
    (include/laser_hip.h "Attention" defines every bit: scores as k-ascending fmaf chains, the row softmax of
    laser_amd.softmax on the visible scores, P V in laser-order).  `q` is (B, H, Tq, d) or (BH, Tq, d), `k` (.., Tk, d),
    `v` (.., Tk, dv): device tensors or views of any outer strides with unit feature stride, so slices of one fused
    projection output (B, T, 3, H, d) need no copy.  1 <= d, dv <= 128, 1 <= Tk <= 65536.  scale=None:
    float32(1 / sqrt(d)).  causal: row i sees keys [0, i + (Tk - Tq) + 1); Tq <= Tk is needed.
    out: None for a fresh Tensor of q's leading shape + (dv,), a destination, or False for no O (probs or stats must then
    be asked for; the P V sweep is skipped).  probs: None / False for none, True for a fresh (.., Tq, Tk) Tensor, or a
    destination; masked positions are written as +0.  stats=True: also the row maxima and row sums, fresh contiguous
    Tensors of q's leading shape.  Returns O alone, or (O, probs, row_max, row_sum) when probs or stats is asked for (None
    where not).  What is asked for has the same bits whatever else is asked for."""
    fn = "attention"
    vq, b, h, tq, d, qs = _attn_view(fn, "q", q)
    vk, bk, hk, tk, _, ks = _attn_view(fn, "k", k, d)
    vv, bv, hv, tkv, dv, vs = _attn_view(fn, "v", v)
    if vk.rank != vq.rank or vv.rank != vq.rank or (bk, hk) != (b, h) or (bv, hv) != (b, h):
        raise ValueError(f"{fn}: q, k and v have leading shapes {vq.shape[:-2]}, {vk.shape[:-2]} and {vv.shape[:-2]}")
    if tkv != tk:
        raise ValueError(f"{fn}: k has {tk} positions, v has {tkv}")
    if not 1 <= d <= ATTENTION_MAX_D or not 1 <= dv <= ATTENTION_MAX_D:
        raise ValueError(f"{fn}: d = {d}, dv = {dv} (1 .. {ATTENTION_MAX_D})")
    if not 1 <= tk <= ATTENTION_MAX_KEYS:
        raise ValueError(f"{fn}: Tk = {tk} (1 .. {ATTENTION_MAX_KEYS})")
    if causal and tq > tk:
        raise ValueError(f"{fn}: causal with Tq = {tq} > Tk = {tk}")
    scale = _attn_scale(fn, scale, d)
    lead = vq.shape[:-2]
    want_probs = probs is not None and probs is not False
    if out is False and not want_probs and not stats:
        raise ValueError(f"{fn}: nothing is asked for (out=False needs probs or stats)")
    # (what was passed in is checked before anything fresh is allocated)
    if out is not None and out is not False:
        vo, bo, ho, to, _, _ = _attn_view(fn, "out", out, dv)
        if vo.rank != vq.rank or (bo, ho, to) != (b, h, tq):
            raise ValueError(f"{fn}: out has shape {vo.shape}, {lead + (tq, dv)} is needed")
    if want_probs and probs is not True:
        vp, bp, hp, tp, _, _ = _attn_view(fn, "probs", probs, tk)
        if vp.rank != vq.rank or (bp, hp, tp) != (b, h, tq):
            raise ValueError(f"{fn}: probs has shape {vp.shape}, {lead + (tq, tk)} is needed")
    vo, os_, vp, ps = None, (0, 0, 0), None, (0, 0, 0)
    if out is False:
        out = None
    else:
        if out is None:
            out = newTensor(np.float32, *(lead + (tq, dv)))
        vo, _, _, _, _, os_ = _attn_view(fn, "out", out, dv)
    if want_probs:
        if probs is True:
            probs = newTensor(np.float32, *(lead + (tq, tk)))
        vp, _, _, _, _, ps = _attn_view(fn, "probs", probs, tk)
    else:
        probs = None
    rmax = newTensor(np.float32, *(lead + (tq,))) if stats else None
    rsum = newTensor(np.float32, *(lead + (tq,))) if stats else None
    vm = _f32("row_max", rmax) if stats else None
    vs_ = _f32("row_sum", rsum) if stats else None
    if b * h * tq > 0:
        _lib.check(_lib.lib().laser_hip_attention_f32_dev(_ptr(vo), _i64x3(os_), _ptr(vq), _i64x3(qs), _ptr(vk), _i64x3(ks), _ptr(vv),
                                                          _i64x3(vs), _ptr(vp), _i64x3(ps), _ptr(vm), _ptr(vs_), b, h, tq, tk, d, dv,
                                                          scale, 1 if causal else 0, _stream()))
    if want_probs or stats:
        return out, probs, rmax, rsum
    return out


def _attn_gemm(b, h, m, n, kk, alpha, a_st, a_ptr, b_st, b_ptr, c_st, c_ptr):
    """C[b, h] = alpha * A[b, h] B[b, h] for every slice on gemm_strided_batched in the current float mode: strides are
    (batch, head, row, column) in elements.  One launch when the (batch, head) dims of all three collapse into one batch
    stride, else one per batch."""
    L = _lib.lib()

    def one(batch, off, pick):
        _lib.check(L.laser_hip_gemm_strided_batched_f32_dev(
            batch, m, n, kk, C.c_float(alpha), C.c_void_p(a_ptr + 4 * off(a_st)), a_st[2], a_st[3], pick(a_st),
            C.c_void_p(b_ptr + 4 * off(b_st)), b_st[2], b_st[3], pick(b_st), C.c_float(0.0),
            C.c_void_p(c_ptr + 4 * off(c_st)), c_st[2], c_st[3], pick(c_st), _stream()))

    if b * h == 0 or m == 0 or n == 0:
        return
    if h == 1 or b == 1 or all(st[0] == st[1] * h for st in (a_st, b_st, c_st)):
        one(b * h, lambda st: 0, (lambda st: st[0]) if h == 1 else (lambda st: st[1]))
    else:
        for i in range(b):
            one(h, lambda st, i=i: i * st[0], lambda st: st[1])


def attention_backward(dout, q, k, v, scale=None, causal=False, need=("q", "k", "v")):
    """The gradients of attention(q, k, v, scale, causal) from the incoming gradient `dout` (shape of O), as a composition
    of steps that each have defined bits (include/laser_hip.h "Attention"): P from the fused forward kernel (probs only);
    dV = P^T dO; dP = dO V^T; dS = softmax_backward(dP, P) over the full Tk (masked positions give +-0); dQ = scale * (dS K);
    dK = scale * (dS^T Q).  The four products run on gemm_strided_batched in the current float mode, the transposes as
    strides and `scale` as the GEMM's alpha; no operand is copied.  Memory: B*H*Tq*Tk floats twice (P, and dP / dS in
    place), freed on return.  `need`: which of "q", "k", "v" to compute; what is asked for has the same bits whatever else
    is asked for.  Returns (dq, dk, dv), fresh contiguous Tensors of the operands' shapes, None where not asked for."""
    fn = "attention_backward"
    need = (need,) if isinstance(need, str) else tuple(need)
    if not need or any(x not in ("q", "k", "v") for x in need):
        raise ValueError(f'{fn}: need = {need!r} (a non-empty subset of ("q", "k", "v"))')
    vq, b, h, tq, d, qs = _attn_view(fn, "q", q)
    vk, _, _, tk, _, ks = _attn_view(fn, "k", k, d)
    vv, _, _, _, dv, vs = _attn_view(fn, "v", v)
    vdo, bo, ho, to, _, dos = _attn_view(fn, "dout", dout, dv)
    if vdo.rank != vq.rank or (bo, ho, to) != (b, h, tq):
        raise ValueError(f"{fn}: dout has shape {vdo.shape}, {vq.shape[:-1] + (dv,)} is needed")
    sc = _attn_scale(fn, scale, d)
    lead = vq.shape[:-2]
    probs = newTensor(np.float32, *(lead + (tq, tk)))
    attention(q, k, v, scale=scale, causal=causal, out=False, probs=probs)       # (checks q, k and v against each other)
    vp = _f32("probs", probs)
    pst = (h * tq * tk, tq * tk, tk, 1)                                          # (batch, head, row, column)
    four = lambda st: (st[0], st[1], st[2], 1)
    tr = lambda st: (st[0], st[1], st[3], st[2])
    dq = dk = dvv = None
    if "v" in need:
        dvv = newTensor(np.float32, *(lead + (tk, dv)))
        _attn_gemm(b, h, tk, dv, tq, 1.0, tr(pst), vp.ptr, four(dos), vdo.ptr, (h * tk * dv, tk * dv, dv, 1),
                   _f32("dv", dvv).ptr)
    if "q" in need or "k" in need:
        ds = newTensor(np.float32, *(lead + (tq, tk)))
        vds = _f32("ds", ds)
        _attn_gemm(b, h, tq, tk, dv, 1.0, four(dos), vdo.ptr, tr(four(vs)), vv.ptr, pst, vds.ptr)
        from .simd_math import softmax_backward
        if b * h * tq > 0:
            softmax_backward(ds, probs, out=ds)
        if "q" in need:
            dq = newTensor(np.float32, *(lead + (tq, d)))
            _attn_gemm(b, h, tq, d, tk, sc, pst, vds.ptr, four(ks), vk.ptr, (h * tq * d, tq * d, d, 1), _f32("dq", dq).ptr)
        if "k" in need:
            dk = newTensor(np.float32, *(lead + (tk, d)))
            _attn_gemm(b, h, tk, d, tq, sc, tr(pst), vds.ptr, four(qs), vq.ptr, (h * tk * d, tk * d, d, 1), _f32("dk", dk).ptr)
    return dq, dk, dvv
