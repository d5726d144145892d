"""numpy model of llog -- the bit-defined float32 logarithm of laser_amd/csrc/log_core.h -- and of logsumexp, log-softmax and
the softmax cross-entropy on top of it, as include/laser_hip.h ("log, logsumexp, log-softmax and cross-entropy") states
them.  lexp is tests/exp_model.py's and the sum is the canonical order of tests/reduce_model.py, both as they stand.
Nothing is read from the code under test except the table literals of log_core.h (header_table), which the tests compare
with the table kept here."""
import os
import re

import numpy as np

from tests import exp_model, reduce_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "laser_amd", "csrc", "log_core.h")

OFF = 0x3f330000                                   # bits of 0.69921875


def _f64(bits):
    return np.array(bits, np.uint64).view(np.float64)


LN2 = _f64([0x3fe62e42fefa39ef])[0]
C2, C3, C4, C5, C6 = (np.float64(c) for c in (-1.0 / 2, 1.0 / 3, -1.0 / 4, 1.0 / 5, -1.0 / 6))   # each one correctly rounded division


def intervals():
    """(lo, hi) of the 16 intervals of the reduced range, as float64"""
    lo = (OFF + (np.arange(16, dtype=np.uint32) << 19)).astype(np.uint32).view(np.float32).astype(np.float64)
    hi = (OFF + (np.arange(1, 17, dtype=np.uint32) << 19)).astype(np.uint32).view(np.float32).astype(np.float64)
    return lo, hi


def invc_table():
    """INVC[i] = float64(1 / midpoint of interval i) (the midpoint is exact in float64, the division correctly rounded);
    1 for the interval that holds 1"""
    lo, hi = intervals()
    inv = 1.0 / ((lo + hi) / 2)
    inv[9] = 1.0
    return inv


# LOGC[i] = float64(-ln INVC[i]), correctly rounded (computed once with 200-bit arithmetic and kept as bits: numpy's float64 log
# is within an ulp but promises no more; the tests check these against it to that ulp)
LOGC = _f64([0xbfd57bf753c8d1fb, 0xbfd2bef07cdc9355, 0xbfd01eae5626c691, 0xbfcb31d8575bce3b, 0xbfc6574ebe8c1339, 0xbfc1aa2b7e23f729,
             0xbfba4e7640b1bc38, 0xbfb1973bd1465561, 0xbfa252f32f8d1840, 0x0000000000000000, 0x3fab42dd711971b9, 0x3fbc5e548f5bc743,
             0x3fc526e5e3a1b438, 0x3fcbc286742d8cd4, 0x3fd1058bf9ae4ad4, 0x3fd404308686a7e4])
INVC = invc_table()


def header_table():
    """the literals of lh_log_tab in log_core.h: (INVC, LOGC) as float64"""
    text = open(CORE).read()
    body = re.search(r"lh_log_tab\[32\] = \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    w = np.array([int(x[:-3], 16) for x in re.findall(r"0x[0-9a-fA-F]{16}ull", body)], np.uint64).view(np.float64)
    return w[0::2].copy(), w[1::2].copy()


def llog(x):
    """llog of a float32 array, step by step as log_core.h numbers them"""
    x = np.asarray(x, np.float32)
    shape = x.shape
    x = x.reshape(-1)
    b = x.view(np.uint32).astype(np.int64)
    nan, zero, neg, inf = np.isnan(x), (b & 0x7fffffff) == 0, (b >> 31) != 0, b == 0x7f800000
    special = nan | zero | neg | inf
    b = np.where(special, 0x3f800000, b)                      # any harmless value: overwritten below
    # 2. subnormals, in integers
    sub = b < 0x00800000
    bl = np.array([int(v).bit_length() for v in b[sub]], np.int64)   # clz(b) = 32 - bit_length
    n = np.zeros_like(b)
    n[sub] = (32 - bl) - 8
    b = b << n
    k = -n
    # 3.
    t = (b - OFF) & 0xffffffff
    ts = np.where(t >= 1 << 31, t - (1 << 32), t)             # int32(t)
    k = k + (ts >> 23)                                        # arithmetic shift
    i = (t >> 19) & 15
    zb = (b - (t & 0xff800000)) & 0xffffffff
    z = zb.astype(np.uint32).view(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        # 4. - 6., every operation a float64 one rounded on its own
        r = z * INVC[i] - 1.0
        q = C6 * r
        q = q + C5
        q = q * r
        q = q + C4
        q = q * r
        q = q + C3
        q = q * r
        q = q + C2
        y = ((k.astype(np.float64) * LN2 + LOGC[i]) + r) + (r * r) * q
        out = y.astype(np.float32)                            # 7. round to nearest even
    out = np.where(inf, np.float32(np.inf), out)
    out = np.where(neg, np.float32(np.nan), out)
    out = np.where(zero, np.float32(-np.inf), out)
    out = np.where(nan, np.float32(np.nan), out)
    return out.astype(np.float32).reshape(shape)


def _m_s(x):
    """(m, d, e, s) of a row: the softmax's maximum, x - m, lexp of that and its sum in the order of reduce_sum"""
    x = np.asarray(x, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        m = np.float32(reduce_model.model_minmax(x, "max"))
        d = (x - m).astype(np.float32)
        e = exp_model.lexp(d)
        s = np.float32(reduce_model.model_sum(e))
    return m, d, e, s


def logsumexp_row(x):
    m, _, _, s = _m_s(x)
    if np.isinf(m):
        return m
    with np.errstate(all="ignore"):
        return np.float32(m + llog(s))


def log_softmax_row(x):
    _, d, _, s = _m_s(x)
    with np.errstate(all="ignore"):
        return (d - llog(s)).astype(np.float32)


def xent_row(x, label, scale=1.0):
    """(loss, grad row) of one row"""
    x = np.asarray(x, np.float32).reshape(-1)
    n = x.size
    if label == -1:
        return np.float32(0), np.zeros(n, np.float32)
    if not 0 <= label < n:
        return np.float32(np.nan), np.full(n, np.nan, np.float32)
    m, d, e, s = _m_s(x)
    with np.errstate(all="ignore"):
        loss = np.float32(llog(s) - d[label])
        hot = np.zeros(n, np.float32)
        hot[label] = 1
        g = ((e / s).astype(np.float32) - hot).astype(np.float32)
        g = (g * np.float32(scale)).astype(np.float32)
    return loss, g


def logsumexp_rows(x):
    return np.array([logsumexp_row(r) for r in np.asarray(x, np.float32)], np.float32)


def log_softmax_rows(x):
    return np.stack([log_softmax_row(r) for r in np.asarray(x, np.float32)])


def xent_rows(x, labels, scale=1.0):
    out = [xent_row(r, int(l), scale) for r, l in zip(np.asarray(x, np.float32), labels)]
    return np.array([o[0] for o in out], np.float32), np.stack([o[1] for o in out])


same_bits = exp_model.same_bits


def edges():
    """the edge set of the tests: +-0, the smallest and largest subnormal, FLT_MIN, the floats either side of 1, sqrt(1/2),
    sqrt(2) and their neighbours, the ends of the reduced range, FLT_MAX, +-Inf, NaN, negatives"""
    f = np.float32
    fi = np.finfo(np.float32)
    one = f(1)
    e = [f(0.0), f(-0.0), f(1e-45), np.nextafter(fi.tiny, f(0)), fi.tiny, np.nextafter(fi.tiny, f(1)), f(1e-39),
         np.nextafter(one, f(0)), one, np.nextafter(one, f(2)), f(np.sqrt(0.5)), f(np.sqrt(2.0)), fi.max, f(np.inf), f(-np.inf),
         f(np.nan), f(-1), f(-1e-45), -fi.max, f(0.5), f(2), f(np.e), f(10), f(1e-10), f(1e10)]
    for bits in (OFF, 2 * 0x00800000 + OFF - 0x00800000, 0x3f7b0000, 0x3f830000):     # interval ends
        v = np.array([bits], np.uint32).view(np.float32)[0]
        e += [np.nextafter(v, f(0)), v, np.nextafter(v, f(4))]
    for v in (f(np.sqrt(0.5)), f(np.sqrt(2.0))):
        e += [np.nextafter(v, f(0)), np.nextafter(v, f(4))]
    return np.array(e, np.float32)
