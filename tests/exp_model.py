"""numpy model of lexp -- Laser's table-driven float32 exp (laser/primitives/simd_math/exp_log_*.nim, the exported SIMD
forms) -- and of the row softmax on top of it, as include/laser_hip.h ("exp and row softmax") states them.  The sum is the
canonical order of tests/reduce_model.py.  Nothing is read from the code under test except the table literals of
laser_amd/csrc/exp_core.h (header_table), which the tests compare with the table computed here."""
import os
import re

import numpy as np

from tests import reduce_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = os.path.join(ROOT, "laser_amd", "csrc", "exp_core.h")

EXP_A = np.array([0x44b8aa3b], np.uint32).view(np.float32)[0]   # float32(1024 / ln 2)
EXP_B = np.array([0x3a317218], np.uint32).view(np.float32)[0]   # float32(ln 2 / 1024)
TABLE_CRC = 0x0c4cd4ff


def table():
    """LUT[i] = bits(correctly rounded float32 of 2^(i/1024)) & 0x7fffff.  2.0 ** (i / 1024) in float64 is within an ulp of
    float64 of the true value, far closer than any float32 rounding boundary comes (tests check it against fractions)."""
    i = np.arange(1024, dtype=np.float64)
    return (np.float32(2.0 ** (i / 1024)).view(np.uint32) & np.uint32(0x7fffff)).astype("<u4")


LUT = table()


def header_table():
    """the literals of lh_exp_lut in exp_core.h"""
    text = open(CORE).read()
    body = re.search(r"lh_exp_lut\[LH_EXP_LUT_SIZE\] = \{(.*?)\};", text, re.S).group(1)
    return np.array([int(w.rstrip("u"), 16) for w in re.findall(r"0x[0-9a-fA-F]+u?", body)], dtype="<u4")


def lexp(x):
    """lexp of a float32 array, every operation rounded to float32 on its own"""
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    with np.errstate(all="ignore"):
        c = np.where(nan, np.float32(0), np.maximum(np.minimum(x, np.float32(88)), np.float32(-88))).astype(np.float32)
        r = np.rint(c * EXP_A).astype(np.int32)                      # round to nearest even
        t = ((c - r.astype(np.float32) * EXP_B) + np.float32(1)).astype(np.float32)
        v = r & 1023
        u = ((r + (127 << 10)) >> 10) << 23
        f = (LUT[v].astype(np.uint32) | u.astype(np.uint32)).view(np.float32)
        out = (t * f).astype(np.float32)
    return np.where(nan, np.float32(np.nan), out).astype(np.float32)


def softmax_row(x):
    """softmax of one row (1-D float32): max under reduce_max's rule, lexp(x - m), the sum in reduce_sum's order, a division"""
    x = np.asarray(x, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        m = np.float32(reduce_model.model_minmax(x, "max"))
        e = lexp((x - m).astype(np.float32))
        s = np.float32(reduce_model.model_sum(e))
        return (e / s).astype(np.float32)


def softmax_rows(x):
    return np.stack([softmax_row(r) for r in np.asarray(x, np.float32)])


def same_bits(a, b):
    """bit-for-bit equality of float32 arrays, except that any NaN equals any NaN (the payload is unspecified)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def edges():
    """the edge set of the tests: signed zeros, the clamp, infinities, NaN, the subnormal threshold and subnormals"""
    f = np.float32
    e = [f(0.0), f(-0.0), f(88), f(-88), f(88.0001), f(-88.0001), f(np.inf), f(-np.inf), f(np.nan), f(1), f(-1), f(0.5)]
    t = f(-87.3369)
    lo = hi = t
    e.append(t)
    for _ in range(4):
        lo, hi = np.nextafter(lo, f(-np.inf)), np.nextafter(hi, f(np.inf))
        e += [lo, hi]
    tiny = np.finfo(np.float32).tiny
    e += [f(1e-45), f(-1e-45), f(1e-39), f(-1e-39), tiny, -tiny, np.nextafter(tiny, f(0))]
    return np.array(e, np.float32)


def ties(count=8, seed=0):
    """float32 inputs in [-30, 0] whose float32 product with ExpA has fraction exactly .5: the first by construction (scan
    the neighbours of (k + 0.5) / ExpA), the others by filtering random values (about 0.2 % qualify)"""
    out = []
    for k in range(-2000, -44000, -1):
        h = np.float32(k + 0.5)
        c = np.float32(np.float64(h) / np.float64(EXP_A))
        cand, up, dn = [c], c, c
        for _ in range(8):
            up, dn = np.nextafter(up, np.float32(0)), np.nextafter(dn, np.float32(-40))
            cand += [up, dn]
        hit = [q for q in cand if np.float32(q * EXP_A) == h]
        if hit:
            out.append(hit[0])
            break
    assert out, "no tie found by construction"
    rng = np.random.default_rng(seed)
    x = rng.uniform(-30, 0, 200000).astype(np.float32)
    p = (x * EXP_A).astype(np.float32)
    x = x[np.abs(p - np.trunc(p)) == 0.5]
    assert x.size >= count
    return np.concatenate([np.array(out, np.float32), x[:count]])
