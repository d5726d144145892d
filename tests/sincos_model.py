"""numpy model of lsin and lcos -- the bit-defined float32 sine and cosine of laser_amd/csrc/sincos_core.h -- as
include/laser_hip.h ("Sine and cosine") states them: integer operations on uint64 arrays, float64 operations each rounded on
its own, the same operations in the same order as the header.  The constants come from scripts/gen_sincos_constants.py
(integer and fraction arithmetic); nothing is read from the code under test except its literals (header_constants), which
the tests compare with the ones made here."""
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "laser_amd", "csrc", "sincos_core.h")

_spec = importlib.util.spec_from_file_location("gen_sincos_constants", os.path.join(ROOT, "scripts", "gen_sincos_constants.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

BITS = gen.constants()                                  # name -> float64 bits, "TWO_OVER_PI" -> eight 32-bit words
TABLE = np.array([0] + BITS["TWO_OVER_PI"], np.uint64)  # one zero word in front, as in the header


def _f64(bits):
    return np.array([bits], np.uint64).view(np.float64)[0]


K = {k: _f64(v) for k, v in BITS.items() if k != "TWO_OVER_PI"}
BIG = 0x49800000                                        # bits of 2^20: Payne-Hanek from here on
NAN = 0x7fc00000
U = np.uint64
M32 = U(0xffffffff)


def header_constants():
    """the literals of sincos_core.h: ({name: bits}, the 9 table words, BIG, NAN)"""
    text = open(CORE).read()
    names = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define LH_SC_(\w+)_BITS (0x[0-9a-fA-F]{16})ull", text)}
    body = re.search(r"lh_sc_two_over_pi\[9\] = \{(.*?)\};", text, re.S).group(1)
    tab = [int(x[:-1], 16) for x in re.findall(r"0x[0-9a-fA-F]{8}u", body)]
    big = int(re.search(r"#define LH_SC_BIG (0x[0-9a-fA-F]{8})u", text).group(1), 16)
    nan = int(re.search(r"#define LH_SC_NAN (0x[0-9a-fA-F]{8})u", text).group(1), 16)
    return names, tab, big, nan


def sin_kernel(r):
    r = np.asarray(r, np.float64)
    s = r * r
    q = K["S15"] * s
    for name in ("S13", "S11", "S9", "S7", "S5", "S3"):
        q = q + K[name]
        q = q * s
    w = r * q
    return r + w


def cos_kernel(r):
    r = np.asarray(r, np.float64)
    s = r * r
    q = K["C16"] * s
    for name in ("C14", "C12", "C10", "C8", "C6", "C4"):
        q = q + K[name]
        q = q * s
    q = q + K["C2"]
    w = s * q
    return 1.0 + w


def reduce_small(b, p3=None):
    """b: uint32 bits of finite a < 2^20 -> (quadrant int64, r float64)"""
    p3 = K["P3"] if p3 is None else np.float64(p3)
    a = np.asarray(b, np.uint32).view(np.float32).astype(np.float64)
    z = a * K["INV"]
    zr = z + K["RND"]
    kf = zr - K["RND"]
    h1 = kf * K["P1"]
    h2 = kf * K["P2"]
    h3 = kf * p3
    r1 = a - h1
    r2 = r1 - h2
    return kf.astype(np.int64) & 3, r2 - h3


def _clz64(v):
    """leading zeros of nonzero uint64 values"""
    v = v.copy()
    n = np.zeros(v.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (v >> U(64 - s)) == 0
        n = np.where(m, n + s, n)
        v = np.where(m, v << U(s), v)
    return n


def reduce_big(b):
    """b: uint32 bits of finite a >= 2^20 -> (quadrant int64, r float64), Payne-Hanek in integers"""
    b = np.asarray(b, np.uint32).astype(np.uint64)
    with np.errstate(over="ignore"):
        m = (b & U(0x7fffff)) | U(0x800000)
        tb = (b >> U(23)).astype(np.int64) - 150 - 2 + 32
        wi, sh = tb >> 5, (tb & 31).astype(np.uint64)
        h = [((((TABLE[wi + j] << U(32)) | TABLE[wi + j + 1]) >> (U(32) - sh)) & M32) for j in range(4)]
        p3 = m * h[3]
        p2 = m * h[2] + (p3 >> U(32))
        p1 = m * h[1] + (p2 >> U(32))
        p0 = m * h[0] + (p1 >> U(32))
        hi = (p0 << U(32)) | (p1 & M32)
        lo = (p2 << U(32)) | (p3 & M32)
        q = ((hi + U(1 << 61)) >> U(62)).astype(np.int64)
        fh = (hi << U(2)) | (lo >> U(62))
        fl = lo << U(2)
        neg = (fh >> U(63)) == 1
        nl = ~fl + U(1)
        nh = ~fh + (nl == 0).astype(np.uint64)
        fl = np.where(neg, nl, fl)
        fh = np.where(neg, nh, fh)
        low = fh == 0
        drop = np.where(low, 64, 0)
        fh, fl = np.where(low, fl, fh), np.where(low, U(0), fl)
        zero = fh == 0
        fh1 = np.where(zero, U(1), fh)
        n = _clz64(fh1)
        nu = n.astype(np.uint64)
        top = np.where(n > 0, (fh1 << nu) | (fl >> (U(64) - np.where(n > 0, nu, U(1)))), fh1)
        mant = (top >> U(11)).astype(np.int64).astype(np.float64)            # 53 bits: exact
        scale = ((1023 - 53 - n - drop).astype(np.uint64) << U(52)).view(np.float64)
        f = np.where(zero, 0.0, mant * scale)
        f = np.where(neg, -f, f)
    return q, f * K["PIO2"]


def reduce(babs, p3=None):
    """babs: uint32 bits of finite magnitudes -> (quadrant, r)"""
    babs = np.asarray(babs, np.uint32)
    big = babs >= BIG
    q = np.zeros(babs.shape, np.int64)
    r = np.zeros(babs.shape, np.float64)
    if (~big).any():
        q[~big], r[~big] = reduce_small(babs[~big], p3)
    if big.any():
        q[big], r[big] = reduce_big(babs[big])
    return q, r


def pick(q, r, want_cos):
    """the float64 sine (want_cos = 0) or cosine (1) of the angle (q + r * 2/pi) * pi/2"""
    j = (np.asarray(q, np.int64) + want_cos) & 3
    y = np.where((j & 1) == 1, cos_kernel(r), sin_kernel(r))
    return np.where((j & 2) == 2, -y, y)


def _both(x, p3=None):
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32)
    babs = b & np.uint32(0x7fffffff)
    special = babs >= 0x7f800000
    q, r = reduce(np.where(special, np.uint32(0), babs), p3)
    with np.errstate(all="ignore"):
        s = pick(q, r, 0).astype(np.float32).view(np.uint32) ^ (b & np.uint32(0x80000000))
        c = pick(q, r, 1).astype(np.float32).view(np.uint32)
    s = np.where(special, np.uint32(NAN), s).astype(np.uint32)
    c = np.where(special, np.uint32(NAN), c).astype(np.uint32)
    return s.view(np.float32), c.view(np.float32)


def lsin(x, p3=None):
    return _both(x, p3)[0]


def lcos(x, p3=None):
    return _both(x, p3)[1]


def lsincos(x):
    return _both(x)


def same_bits(a, b):
    """equal as uint32, NaN compared as masks"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def returns_x_boundary():
    """the bits of the largest float32 up to which lsin(x) = x without a gap.  Inside a binade the ulp is fixed and x^3 / 6
    grows, so "returns x" holds up to a point and then no more (it can hold again at the start of the next binade, where
    the ulp doubles): the first binade whose top value fails, then a bisection inside it."""
    f = lambda bits: lsin(np.array([bits], np.uint32).view(np.float32)).view(np.uint32)[0] == bits
    e = 0x60
    while f(((e + 1) << 23) - 1):
        e += 1
    lo, hi = e << 23, ((e + 1) << 23) - 1
    assert f(lo) and not f(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if f(mid) else (lo, mid)
    return lo


def edges():
    """the edge list of the issue, both signs: zeros, subnormals, the "returns x" boundary, the floats next to k pi/2 for
    k <= 16, the reduction threshold +-1 ulp, every power of two, the largest finite value, infinities and two NaNs"""
    f = np.float32
    b = [0, 1, 0x007fffff, 0x00800000, 0x7f7fffff, 0x7f800000, 0x7fc00000, 0x7f800001, 0x7fffffff, BIG - 1, BIG, BIG + 1]
    rx = returns_x_boundary()
    b += [rx - 1, rx, rx + 1, rx + 2]
    for k in range(1, 17):
        c = int(np.array([k * np.pi / 2], f).view(np.uint32)[0])
        b += [c - 2, c - 1, c, c + 1, c + 2]
    b += [int(np.array([np.pi / 4], f).view(np.uint32)[0]) + d for d in (-1, 0, 1)]
    b += [e << 23 for e in range(1, 255)]               # 2^-126 .. 2^127
    b = np.array(b, np.uint32)
    return np.concatenate([b, b | np.uint32(0x80000000)]).view(f)
