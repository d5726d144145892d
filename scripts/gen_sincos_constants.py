#!/usr/bin/env python3
"""The constants of laser_amd/csrc/sincos_core.h, from integer and `fractions` arithmetic alone (no mpmath, no libm):

    python3 scripts/gen_sincos_constants.py        prints the #define block and the 2/pi table as they stand in the header

pi comes from Machin's formula in fixed point with 64 guard bits; a Fraction is rounded to the nearest float64 (ties to even)
in integers.  tests/sincos_model.py takes its constants from constants() and tests/test_sincos_cpu.py compares them with the
literals of the header.

    TWO_OVER_PI   256 bits of 2/pi after the binary point, as eight 32-bit words, most significant first; the header's
                  table puts one zero word in front (the bits before the point)
    INV           float64(2/pi)
    P1, P2        pi/2 and what is left of it, each cut (not rounded) to 24 significant bits: k * P1 and k * P2 are exact
                  for |k| < 2^29
    P3            float64(pi/2 - P1 - P2)
    PIO2          float64(pi/2)
    S3 .. S15     float64((-1)^j / (2j+1)!), the sine series;  C2 .. C16  float64((-1)^j / (2j)!), the cosine series
"""
from fractions import Fraction

PI_BITS = 400


def _arctan_inv(n, bits):
    """atan(1/n) * 2^bits, truncated, by the alternating series in integers"""
    one = 1 << bits
    term = one // n
    total, k, n2, sign = term, 1, n * n, 1
    while term:
        term //= n2
        k += 2
        sign = -sign
        total += sign * (term // k)
    return total


def pi_fixed(bits=PI_BITS):
    """floor-ish pi * 2^bits (exact to well below one unit: 64 guard bits)"""
    g = bits + 64
    return (16 * _arctan_inv(5, g) - 4 * _arctan_inv(239, g)) >> 64


PI = Fraction(pi_fixed(), 1 << PI_BITS)      # pi to 2^-399: far beyond anything rounded below


def f64_bits(q):
    """the bits of the float64 nearest to the Fraction q (ties to even); q in the normal range"""
    if q == 0:
        return 0
    sign = (1 << 63) if q < 0 else 0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                # 2^e <= q < 2^(e+1)
    scaled = q / Fraction(2) ** (e - 52)      # in [2^52, 2^53)
    m = scaled.numerator // scaled.denominator
    rem = scaled - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and m & 1):
        m += 1
    if m == 1 << 53:
        m >>= 1
        e += 1
    assert 0 < e + 1023 < 2047
    return sign | ((e + 1023) << 52) | (m - (1 << 52))


def f64_value(bits):
    """the exact value of a (normal or zero) float64 given as bits"""
    if bits & ~(1 << 63) == 0:
        return Fraction(0)
    s = -1 if bits >> 63 else 1
    e = ((bits >> 52) & 0x7ff) - 1075
    return s * ((bits & ((1 << 52) - 1)) | (1 << 52)) * Fraction(2) ** e


def cut(q, sig):
    """q > 0 truncated to `sig` significant bits, as float64 bits"""
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    unit = Fraction(2) ** (e - sig + 1)
    m = (q / unit).numerator // (q / unit).denominator
    return f64_bits(m * unit)


def factorial(n):
    r = 1
    for i in range(2, n + 1):
        r *= i
    return r


def constants():
    c = {}
    two_over_pi = 2 / PI
    w = (two_over_pi * (1 << 256)).numerator // (two_over_pi * (1 << 256)).denominator
    c["TWO_OVER_PI"] = [(w >> (32 * (7 - i))) & 0xffffffff for i in range(8)]
    c["INV"] = f64_bits(two_over_pi)
    half = PI / 2
    c["P1"] = cut(half, 24)
    c["P2"] = cut(half - f64_value(c["P1"]), 24)
    c["P3"] = f64_bits(half - f64_value(c["P1"]) - f64_value(c["P2"]))
    c["PIO2"] = f64_bits(half)
    for j in range(1, 8):
        c["S%d" % (2 * j + 1)] = f64_bits(Fraction((-1) ** j, factorial(2 * j + 1)))
    for j in range(1, 9):
        c["C%d" % (2 * j)] = f64_bits(Fraction((-1) ** j, factorial(2 * j)))
    c["RND"] = f64_bits(Fraction(3 << 51))
    return c


def main():
    c = constants()
    for k, v in c.items():
        if k != "TWO_OVER_PI":
            print("#define LH_SC_%s_BITS 0x%016xull" % (k, v))
    words = [0] + c["TWO_OVER_PI"]
    print("static const unsigned int lh_sc_two_over_pi[9] = {")
    print("  " + ", ".join("0x%08xu" % x for x in words[:5]) + ",")
    print("  " + ", ".join("0x%08xu" % x for x in words[5:]) + ",")
    print("};")


if __name__ == "__main__":
    main()
