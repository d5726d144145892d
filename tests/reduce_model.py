"""numpy model of the canonical reduction order of liblaser_hip.so (laser_amd/csrc/reduce_core.h, include/laser_hip.h
"Reductions").  W and R are read from reduce_core.h, so the model follows the header if its constants change."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "laser_amd", "csrc", "reduce_core.h")


def constants():
    """(W, R) = (LH_REDUCE_LANES, LH_REDUCE_STEPS) of reduce_core.h"""
    text = open(CORE).read()
    w = int(re.search(r"#define LH_REDUCE_LANES (\d+)", text).group(1))
    r = int(re.search(r"#define LH_REDUCE_STEPS (\d+)", text).group(1))
    return w, r


def vec(itemsize):
    """E: elements of 16 bytes"""
    return 16 // itemsize


def _fold(acc, merge):
    """halving fold over the last axis: element j merges j + h, h = m/2, m/4, .., 1"""
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = merge(acc[..., :h], acc[..., h:])
    return acc[..., 0]


def level(x, e, init, body, merge, acc_dtype):
    """one level: the partial of every chunk of R*W*e elements of the 1-D array x"""
    W, R = constants()
    n = x.size
    S = R * W * e
    C = max(1, -(-n // S))
    xp = np.zeros(C * S, x.dtype)
    xp[:n] = x
    valid = (np.arange(C * S) < n).reshape(C, R, W, e)
    xp = xp.reshape(C, R, W, e)
    acc = np.full((C, W, e), init, acc_dtype)
    with np.errstate(all="ignore"):
        for r in range(R):
            acc = np.where(valid[:, r], body(acc, xp[:, r]), acc).astype(acc_dtype)
        return _fold(_fold(acc, merge), merge)   # E accumulators, then the W lanes


def reduce(x, init, body, merge, acc_dtype=None, e0=None):
    """The whole reduction of the 1-D array x (logical order) with `body(acc, x)` and `merge(acc, other)` as numpy
    functions; e0 = E of the first level (default: 16 bytes of x's type)."""
    acc_dtype = np.dtype(acc_dtype or x.dtype)
    p = level(np.asarray(x).reshape(-1), e0 or vec(x.dtype.itemsize), init, body, merge, acc_dtype)
    while p.size > 1:
        p = level(p, vec(acc_dtype.itemsize), init, merge, merge, acc_dtype)
    return p[0]


def add(a, b):
    return a + b


def model_sum(x):
    """reduce_sum of x in the canonical order, in x's element type"""
    x = np.asarray(x).reshape(-1)
    return reduce(x, x.dtype.type(0), add, add)


def levels(n, itemsize):
    """launches a reduction of n elements of `itemsize` bytes takes"""
    W, R = constants()
    c = max(1, -(-n // (R * W * vec(itemsize))))
    k = 1
    while c > 1:
        c = -(-c // (R * W * vec(itemsize)))
        k += 1
    return k


def model_minmax(x, op):
    """reduce_min / reduce_max under the NaN / signed-zero rule (order-independent)"""
    x = np.asarray(x).reshape(-1)
    if x.size == 0:
        if x.dtype.kind == "f":
            return x.dtype.type(np.inf if op == "min" else -np.inf)
        return x.dtype.type(np.iinfo(x.dtype).max if op == "min" else np.iinfo(x.dtype).min)
    if x.dtype.kind == "f" and np.isnan(x).any():
        return x.dtype.type(np.nan)
    v = x.min() if op == "min" else x.max()
    if x.dtype.kind == "f" and v == 0:
        z = x[x == 0]
        neg = np.signbit(z)
        v = x.dtype.type(-0.0) if (op == "min" and neg.any()) or (op == "max" and neg.all()) else x.dtype.type(0.0)
    return v
