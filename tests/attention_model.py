"""numpy model of the fused attention, the softmax gradient and the composed attention backward (include/laser_hip.h
"Attention", "Softmax gradient"): a direct transcription of the definition.  The fmaf chains are the oracle's
(oracle.matmul: laser-order, one chain for K <= 512), the visible scores go through exp_model.softmax_row, the sums through
reduce_model.model_sum, everything else is plain float32 numpy."""
import numpy as np

from oracle import oracle
from tests import exp_model, reduce_model

KC = 512          # keys of one chain of P V (the laser-order slice)
f32 = np.float32


def default_scale(d):
    return f32(1.0 / np.sqrt(np.float64(d)))


def visible(i, tq, tk, causal):
    """n_i: row i sees keys [0, n_i)"""
    return i + (tk - tq) + 1 if causal else tk


def chain(a, b):
    """the k-ascending fmaf chain from +0 of a (M, K <= 512) times b (K, N)"""
    assert a.shape[1] <= KC
    return oracle.matmul(np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32))


def scores(q, k, scale):
    with np.errstate(all="ignore"):
        return (f32(scale) * chain(q, k.T)).astype(f32)


def pv(p, v):
    """O = ((S_0 + S_1) + S_2) + .., S_p the chain over keys [512 p, 512 (p + 1))"""
    out = None
    with np.errstate(all="ignore"):
        for j0 in range(0, p.shape[1], KC):
            s = chain(p[:, j0:j0 + KC], v[j0:j0 + KC])
            out = s if out is None else (out + s).astype(f32)
    return out


def forward(q, k, v, scale=None, causal=False, rows=None, need_out=True):
    """one slice: q (Tq, d), k (Tk, d), v (Tk, dv) -> (O, P, row_max, row_sum) for the query rows `rows` (default: all; the
    returned arrays have one row per entry).  A row depends on its own q row, K, V, scale, n_i and Tk alone."""
    q, k, v = (np.asarray(x, f32) for x in (q, k, v))
    tq, tk = q.shape[0], k.shape[0]
    scale = default_scale(q.shape[1]) if scale is None else f32(scale)
    rows = np.arange(tq) if rows is None else np.asarray(rows)
    s = scores(q[rows], k, scale) if len(rows) else np.zeros((0, tk), f32)
    p = np.zeros((len(rows), tk), f32)
    m = np.zeros(len(rows), f32)
    z = np.zeros(len(rows), f32)
    with np.errstate(all="ignore"):
        for r, i in enumerate(rows):
            n = visible(int(i), tq, tk, causal)
            x = s[r, :n]
            m[r] = reduce_model.model_minmax(x, "max")
            e = exp_model.lexp((x - m[r]).astype(f32))
            z[r] = reduce_model.model_sum(e)
            p[r, :n] = (e / z[r]).astype(f32)
    o = pv(p, v) if need_out and len(rows) else np.zeros((len(rows), v.shape[1]), f32)
    return o, p, m, z


def softmax_grad_row(dy, y):
    dy, y = np.asarray(dy, f32).reshape(-1), np.asarray(y, f32).reshape(-1)
    with np.errstate(all="ignore"):
        big_d = f32(reduce_model.model_sum((dy * y).astype(f32)))
        return (y * (dy - big_d).astype(f32)).astype(f32)


def softmax_grad(dy, y):
    dy, y = np.asarray(dy, f32), np.asarray(y, f32)
    out = np.empty_like(dy)
    for idx in np.ndindex(*dy.shape[:-1]):
        out[idx] = softmax_grad_row(dy[idx], y[idx])
    return out


def gemm(a, b, alpha=1.0):
    """gemm_strided in laser-order mode: alpha * (a b), the chains in slices of 512"""
    return oracle.matmul(np.asarray(a, f32), np.asarray(b, f32), alpha=float(alpha))


def backward(dout, q, k, v, scale=None, causal=False):
    """one slice: (dq, dk, dv) by the composition of the header"""
    q, k, v, dout = (np.asarray(x, f32) for x in (q, k, v, dout))
    scale = default_scale(q.shape[1]) if scale is None else f32(scale)
    _, p, _, _ = forward(q, k, v, scale, causal, need_out=False)
    dv = gemm(p.T, dout)
    dp = gemm(dout, v.T)
    ds = softmax_grad(dp, p)
    dq = gemm(ds, k, scale)
    dk = gemm(ds.T, q, scale)
    return dq, dk, dv


def same_bits(a, b, zeros_equal=False):
    """bit-for-bit equality of float32 arrays, any NaN equal to any NaN; zeros_equal: +0 and -0 too"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if zeros_equal:
        a, b = a + f32(0), b + f32(0)
    return exp_model.same_bits(a, b)


def reference64(q, k, v, scale, causal=False):
    """float64 attention of one slice: (O, P)"""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    tq, tk = q.shape[0], k.shape[0]
    s = np.float64(scale) * (q @ k.T)
    if causal:
        s = np.where(np.arange(tk)[None, :] < (np.arange(tq)[:, None] + (tk - tq) + 1), s, -np.inf)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p @ v, p
