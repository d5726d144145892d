"""numpy model of ltanh and lsigmoid -- the bit-defined float32 tanh and logistic function of laser_amd/csrc/act_core.h --
and of the relu / tanh / sigmoid forward rules and their gradients from the output, as include/laser_hip.h ("Activations")
states them.  Every floating-point operation is a float64 (or, in the gradients, float32) numpy operation rounded on its
own; the constants are regenerated here from exact arithmetic (decimal, 80 digits).  Nothing is read from the code under
test except the literals of act_core.h (header_constants), which the tests compare with the ones made here."""
import os
import re
from decimal import Decimal, getcontext

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "laser_amd", "csrc", "act_core.h")

RELU, TANH, SIGMOID = 1, 2, 3                       # LASER_HIP_ACT_*
KINDS = {"relu": RELU, "tanh": TANH, "sigmoid": SIGMOID}


def _bits(v):
    return int(np.array([v], np.float64).view(np.uint64)[0])


def _f64(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


def _constants():
    getcontext().prec = 80
    ln2 = Decimal(2).ln()
    inv = np.float64(float(Decimal(64) / ln2))                     # float(Decimal) rounds correctly
    step = ln2 / 64
    hi = _f64(_bits(float(step)) & ~0xffffff)                      # the low 24 significand bits cleared: k * HI is exact
    lo = np.float64(float(step - Decimal(float(hi))))
    tab = np.array([float(Decimal(2) ** (Decimal(j) / 64)) for j in range(64)], np.float64)
    return inv, hi, lo, tab


INV, HI, LO, T = _constants()
C2, C3, C4, C5 = (np.float64(c) for c in (1 / 2, 1 / 6, 1 / 24, 1 / 120))      # each a correctly rounded division
D3, D5, D7 = (np.float64(c) for c in (-1 / 3, 2 / 15, -17 / 315))
SIG_CLAMP, TANH_CLAMP, TANH_SMALL = np.float64(104), np.float64(10), np.float64(2.0 ** -6)


def header_constants():
    """the literals of act_core.h: ({name: float64}, table of 64 float64)"""
    text = open(CORE).read()
    names = {m.group(1): _f64(int(m.group(2), 16))
             for m in re.finditer(r"#define LH_ACT_(\w+)_BITS (0x[0-9a-fA-F]{16})ull", text)}
    body = re.search(r"lh_act_tab\[64\] = \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    tab = np.array([int(x[:-3], 16) for x in re.findall(r"0x[0-9a-fA-F]{16}ull", body)], np.uint64).view(np.float64)
    return names, tab


def exp_piece(a, lo=None):
    """E(a) for float64 a in [-208, 0]: exp(a) as a float64, every operation rounded on its own"""
    lo = LO if lo is None else np.float64(lo)
    a = np.asarray(a, np.float64)
    kf = np.rint(a * INV)
    k = kf.astype(np.int64)
    r = (a - kf * HI) - kf * lo
    q = C5 * r
    q = q + C4
    q = q * r
    q = q + C3
    q = q * r
    q = q + C2
    p = r + (r * r) * q
    t = T[k & 63]
    e = t + t * p
    scale = (((k >> 6) + 1023) << 52).astype(np.uint64).view(np.float64)
    return e * scale


def tanh_small(a):
    """the odd polynomial of ltanh for float64 0 <= a < 2^-6"""
    a = np.asarray(a, np.float64)
    s = a * a
    q = D7 * s
    q = q + D5
    q = q * s
    q = q + D3
    q = q * s
    return a + a * q


def lsigmoid(x, lo=None):
    x = np.asarray(x, np.float32)
    shape = x.shape
    x = x.reshape(-1)
    nan = np.isnan(x)
    neg = (x.view(np.uint32) >> 31) != 0
    with np.errstate(all="ignore"):
        c = np.minimum(np.abs(np.where(nan, np.float32(0), x)).astype(np.float64), SIG_CLAMP)
        e = exp_piece(-c, lo)
        d = 1.0 + e
        y = np.where(neg, e / d, 1.0 / d).astype(np.float32)       # one division either way, one rounding to float32
    return np.where(nan, np.float32(np.nan), y).astype(np.float32).reshape(shape)


def ltanh(x, lo=None):
    x = np.asarray(x, np.float32)
    shape = x.shape
    x = x.reshape(-1)
    nan = np.isnan(x)
    sign = x.view(np.uint32) & np.uint32(0x80000000)
    with np.errstate(all="ignore"):
        a = np.minimum(np.abs(np.where(nan, np.float32(0), x)).astype(np.float64), TANH_CLAMP)
        small = a < TANH_SMALL
        e = exp_piece(np.where(small, 0.0, -2.0 * a), lo)
        big = (1.0 - e) / (1.0 + e)
        y = np.where(small, tanh_small(np.where(small, a, 0.0)), big).astype(np.float32)
    y = (y.view(np.uint32) | sign).view(np.float32)
    return np.where(nan, np.float32(np.nan), y).astype(np.float32).reshape(shape)


def relu(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.where(x > 0, x, np.float32(0)).astype(np.float32)     # NaN and -0 give +0


def activation(x, kind):
    return {RELU: relu, TANH: ltanh, SIGMOID: lsigmoid}[KINDS.get(kind, kind)](x)


def activation_grad(dy, y, kind):
    """dx from dy and the forward OUTPUT y: float32 operations, each rounded on its own, in the stated order"""
    f = np.float32
    dy, y = np.asarray(dy, f), np.asarray(y, f)
    kind = KINDS.get(kind, kind)
    with np.errstate(all="ignore"):
        if kind == RELU:
            return np.where(y > 0, dy, f(0)).astype(f)
        if kind == TANH:
            t = (y * y).astype(f)
            u = (f(1) - t).astype(f)
            return (dy * u).astype(f)
        if kind == SIGMOID:
            u = (f(1) - y).astype(f)
            v = (y * u).astype(f)
            return (dy * v).astype(f)
    raise ValueError(kind)


def same_bits(a, b):
    """bit equality of float32 arrays, any NaN equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    both = np.isnan(a) & np.isnan(b)
    return bool(np.all(both | (a.view(np.uint32) == b.view(np.uint32))))


def same_bits64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(both | (a.view(np.uint64) == b.view(np.uint64))))


TANH_ONE_BITS, SIG_ONE_BITS, SIG_ZERO_BITS = 0x41102cb4, 0x418aa123, 0xc2cff1b5    # numpy's float64 functions saturate here


def edges():
    """+-0, +-smallest subnormal, +-2^-6 and its neighbours, +-1, the three saturation points and their neighbours,
    -87.3365 (sigmoid turns subnormal), +-104, +-10, FLT_MAX, +-Inf, NaN"""
    f = np.float32
    fi = np.finfo(np.float32)
    e = [f(0.0), f(-0.0), f(1e-45), f(-1e-45), fi.tiny, -fi.tiny, f(1), f(-1), f(-87.3365), f(-87.3366), f(-87.3364), f(-104), f(104),
         f(10), f(-10), f(0.5), f(-0.5), f(3), f(-20), f(88), fi.max, -fi.max, f(np.inf), f(-np.inf), f(np.nan), -f(np.nan)]
    b = [0x3c800000, TANH_ONE_BITS, SIG_ONE_BITS, SIG_ZERO_BITS & 0x7fffffff, 0x42d00000, 0x41200000]
    bits = []
    for v in b:
        for d in (-2, -1, 0, 1, 2):
            bits += [v + d, (v + d) | 0x80000000]
    return np.concatenate([np.array(e, np.float32), np.array(bits, np.uint32).view(np.float32)])
