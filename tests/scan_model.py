"""numpy model of the row prefix sum, the sorted search and the inverse-CDF draws (include/laser_hip.h "Row cumsum,
searchsorted and the inverse-CDF sampler"; laser_amd/csrc/scan_core.h is the definition the kernels include).

    run()                          R = LH_SCAN_RUN, read from scan_core.h
    cumsum(x, R=None)              the scan order along the last axis of a (rows, n) or (n,) array, in x's type
    serial(x)                      the reference's order (bench_multinomial_samplers.nim:49-53): one running sum per row
    searchsorted(a, v, right)      the descent rule, written out, on (rows, n) against (rows, m)
    draw(cdf, u01)                 the CDF draw; draw(..., branch=True) also tells which draws took the idx == n branch
    draw_remove(w, u01)            min(k, n) rounds of scan, draw, zero; mutates w
"""
import os
import re

import numpy as np

CORE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "laser_amd", "csrc", "scan_core.h")


def run():
    """R = LH_SCAN_RUN of scan_core.h"""
    return int(re.search(r"#define LH_SCAN_RUN (\d+)", open(CORE).read()).group(1))


def cumsum(x, R=None):
    """R steps across all runs at once for loc, one loop over the runs for the chain of carries, one addition per element"""
    R = R or run()
    x = np.asarray(x)
    one = x.ndim == 1
    x2 = x.reshape(1, -1) if one else x
    rows, n = x2.shape
    runs = -(-n // R)
    with np.errstate(over="ignore", invalid="ignore"):
        loc = np.zeros((rows, runs * R), x.dtype)
        loc[:, :n] = x2
        loc = loc.reshape(rows, runs, R)
        for j in range(1, R):
            loc[:, :, j] = loc[:, :, j - 1] + loc[:, :, j]
        out = loc.copy()
        if runs > 1:
            carry = np.empty((rows, runs), x.dtype)            # carry[:, r] is added to run r (column 0 is not used)
            c = loc[:, 0, R - 1].copy()                          # run 0 has no carry: its total is taken as it is
            for r in range(1, runs):
                carry[:, r] = c
                c = c + loc[:, r, R - 1]
            out[:, 1:, :] = carry[:, 1:, None] + loc[:, 1:, :]
    out = out.reshape(rows, runs * R)[:, :n]
    return np.ascontiguousarray(out[0] if one else out)


def serial(x):
    """result[0] = x[0]; result[i] = x[i] + result[i - 1], in x's type"""
    x = np.asarray(x)
    out = x.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(1, x.shape[-1]):
            out[..., i] = x[..., i] + out[..., i - 1]
    return out


def searchsorted(a, v, right=False):
    """lo = 0, count = n; while count > 0: step = count / 2, pos = lo + step; right iff a[pos] < v (<= on the right side)"""
    a, v = np.asarray(a), np.asarray(v)
    one = a.ndim == 1
    a2 = a.reshape(1, -1) if one else a
    v2 = v.reshape(a2.shape[0], -1)
    n = a2.shape[1]
    lo = np.zeros(v2.shape, np.int64)
    count = np.full(v2.shape, n, np.int64)
    with np.errstate(invalid="ignore"):
        while np.any(count > 0):
            active = count > 0
            step = count // 2
            pos = lo + step
            x = np.take_along_axis(a2, np.minimum(pos, n - 1), 1)
            go = active & ((x <= v2) if right else (x < v2))
            lo = np.where(go, pos + 1, lo)
            count = np.where(go, count - step - 1, np.where(active, step, count))
    return lo.astype(np.int32).reshape(v.shape)


def draw(cdf, u01, branch=False):
    """(rows, m) indices for cdf (rows, n) and u01 (rows, m), float32"""
    cdf, u01 = np.asarray(cdf, np.float32), np.asarray(u01, np.float32)
    n = cdf.shape[1]
    total = cdf[:, n - 1:n]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(total) & (total > 0)
        u = (u01 * total).astype(np.float32)
    idx = searchsorted(cdf, u, right=True)
    past = idx == n
    again = searchsorted(cdf, np.broadcast_to(total, u.shape).copy(), right=False)
    idx = np.where(past, again, idx)
    idx = np.where(ok, idx, -1).astype(np.int32)
    return (idx, past & ok) if branch else idx


def draw_remove(w, u01, R=None):
    """k = u01.shape[1] draws per row without replacement; w (float32, (rows, n)) is overwritten like the caller's weights"""
    rows, n = w.shape
    k = u01.shape[1]
    idx = np.full((rows, k), -1, np.int32)
    for s in range(min(k, n)):
        i = draw(cumsum(w, R), u01[:, s:s + 1])[:, 0]
        idx[:, s] = i
        hit = np.flatnonzero(i >= 0)
        w[hit, i[hit]] = np.float32(0)
    return idx
