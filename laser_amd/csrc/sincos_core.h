// laser_amd/csrc/sincos_core.h -- lsin and lcos, a bit-defined float32 sine and cosine, as one definition: the precompiled
// kernels (sincos.hip) and the normal random fill (normal_core.h, random.hip) include it, the run-time-compiled forEach /
// forEachReduce kernels get it in the prelude of their source when a body names laser_sin or laser_cos (foreach.cpp embeds
// this file), and a host program can include it too.  include/laser_hip.h ("Sine and cosine") states it in words;
// tests/sincos_model.py is the numpy model; scripts/gen_sincos_constants.py makes every constant below from integer and
// fraction arithmetic.
//
// Only integer operations, bit casts, one exact float32 -> float64 conversion, exact integer -> float64 conversions (at
// most 53 significant bits), float64 + - x each rounded on its own (never a fused multiply-add) and one float64 -> float32
// rounding (nearest even).  No division, no libm, no device transcendental instruction.
//
// For a float32 x with bits b, a = |x|:
//   1. NaN and +-Inf give the NaN with bits 0x7fc00000, whatever the sign and payload of the input.
//   2. Reduction to a quadrant q in 0..3 and a float64 r in about [-pi/4, pi/4] with a = (k + r * 2/pi) * pi/2, q = k mod 4:
//      a < 2^20 (LH_SC_BIG, bits 0x49800000) -- three-part pi/2:
//        kf = (float64(a) * INV + R) - R        R = 1.5 x 2^52: the product rounded to an integer, ties to even; k = int(kf)
//        r  = ((float64(a) - kf * P1) - kf * P2) - kf * P3
//        P1 and P2 are pi/2 and its remainder cut to 24 significant bits, so kf * P1 and kf * P2 are exact (k < 2^20), and so
//        are the first two subtractions (both operands are multiples of 2^-48 and the results stay below 1); P3 is the
//        float64 of what is left, and P1 + P2 + P3 is pi/2 to 2^-101.  For a < pi/4: k = 0 and r = a exactly, so tiny and
//        subnormal inputs take the same path and nothing is flushed.
//      a >= 2^20 -- Payne-Hanek on the bits of 2/pi, in integers:
//        a = m x 2^e with the 24-bit integer m and e = exponent field - 150 in -3 .. 104.  The bits of 2/pi at positions
//        <= e - 2 after the binary point multiply a to multiples of 4 and are dropped.  H = the next 128 bits (positions
//        e - 1 .. e + 126), taken from a table of 9 words: one zero word for the positions before the point, then 256 bits of
//        2/pi, of which the largest float32 (e = 104) reaches bit 230.  P = m * H mod 2^128: its top two bits are the
//        quadrant, the 126 below them the fraction of a * 2/pi, short of the truth by less than m x 2^-126 < 2^-102 (the bits
//        of 2/pi past the window).  Rounding to the nearest quadrant: q = top two bits of (P + 2^125), and P << 2 read as a
//        signed 128-bit number F is the fraction in [-1/2, 1/2) in units of 2^-128.  |F| is shifted left until its top bit
//        is set and cut to 53 bits, which converts to float64 exactly; f = that times an exact power of two, with F's sign;
//        r = f * PIO2 (one rounding).
//        Guard bits: no float32 from pi/4 on is closer to a multiple of pi/2 than 1.6148e-9 (bits 0x6f79be45; the sweep below
//        reports it), which is 2^-29.9 of a quadrant, so at most 30 of the 126 fraction bits are leading zeros, 53 are
//        kept, and 43 or more guard bits lie below the kept ones: the 2^-102 that the window misses is 19 bits below the last
//        kept bit (2^-83 at worst).  A 96-bit window would leave 11 guard bits; the product is four word multiplies either way.
//   3. s = r * r and one kernel on the reduced interval for each function, Horner in s, every operation rounded:
//        sin kernel  r + r * (s * (S3 + s (S5 + s (S7 + s (S9 + s (S11 + s (S13 + s S15)))))))     S_j = float64(-+1 / j!)
//        cos kernel  1 + s * (C2 + s (C4 + s (C6 + s (C8 + s (C10 + s (C12 + s (C14 + s C16)))))))  C_j = float64(-+1 / j!)
//      cut after r^15 / 15! and r^16 / 16!: the next terms are below 2^-54 and 2^-62 of the results on |r| <= 0.786.
//   4. lsin: q = 0: sin kernel, 1: cos kernel, 2: -sin kernel, 3: -cos kernel.  lcos: q = 0: cos kernel, 1: -sin kernel,
//      2: -cos kernel, 3: sin kernel.  The float64 is rounded to float32 once; lsin then XORs x's sign bit into the result.
//   So lsin(-x) has the bits of -lsin(x) and lcos(-x) those of lcos(x); lsin(+-0) = +-0, lcos(+-0) = 1; lsin(x) = x and
//   lcos(x) = 1 wherever the float64 polynomial rounds to them, which is wherever the true value does; the cos kernel is
//   1 + (something <= 0) and the sin kernel stays below 0.71, so |result| <= 1.
//
// Measured over every finite float32 (2 x 2139095040 inputs per function) against sinl and cosl in 80-bit long double
// (tests/cpp/sincos_core_host.cpp "sweep"; profiles/sincos/README.md has the output): faithful (one of the two float32 that
// bracket the true value) at every input, lsin odd and lcos even bit for bit, |result| <= 1, lsin non-decreasing and lcos
// non-increasing over the float32 in [0, pi/2].  Maximum error 0.500000 ulp for both; 2 of the 4278190080 lsin results and 8 of
// the lcos results are the other neighbour of the true value instead of the nearest.  lsin(x) = x for every |x| up to bits
// 0x39e89768 (4.4363e-4), lcos(x) = 1 up to bits 0x39800000 (2^-12).
//
// Plain C++ with no includes: hiprtc compiles it as it stands.  A host build needs -ffp-contract=off (the pragma below
// covers clang).  Names start with lh_, and laser_sin and laser_cos are the two names meant for forEach bodies.
#ifndef LASER_HIP_SINCOS_CORE_H
#define LASER_HIP_SINCOS_CORE_H

#if defined(__HIPCC_RTC__)
#define LH_SC_FN __device__ inline __attribute__((always_inline))
#elif defined(__HIP__)
#define LH_SC_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LH_SC_FN static inline
#endif

#define LH_SC_BIG 0x49800000u  // bits of 2^20: from here on the reduction is Payne-Hanek
#define LH_SC_NAN 0x7fc00000u  // the result for NaN and +-Inf

#define LH_SC_INV_BITS 0x3fe45f306dc9c883ull   // 2 / pi = 0.6366197723675814
#define LH_SC_P1_BITS 0x3ff921fb40000000ull    // 1.5707963109016418
#define LH_SC_P2_BITS 0x3e74442d00000000ull    // 7.5497894158615964e-08
#ifndef LH_SC_P3_BITS                          // (a test builds a deliberately wrong copy with another value)
#define LH_SC_P3_BITS 0x3cf8469898cc5170ull    // 5.3903025299577648e-15
#endif
#define LH_SC_PIO2_BITS 0x3ff921fb54442d18ull  // pi / 2 = 1.5707963267948966
#define LH_SC_S3_BITS 0xbfc5555555555555ull    // -1/3!
#define LH_SC_S5_BITS 0x3f81111111111111ull    //  1/5!
#define LH_SC_S7_BITS 0xbf2a01a01a01a01aull    // -1/7!
#define LH_SC_S9_BITS 0x3ec71de3a556c734ull    //  1/9!
#define LH_SC_S11_BITS 0xbe5ae64567f544e4ull   // -1/11!
#define LH_SC_S13_BITS 0x3de6124613a86d09ull   //  1/13!
#define LH_SC_S15_BITS 0xbd6ae7f3e733b81full   // -1/15!
#define LH_SC_C2_BITS 0xbfe0000000000000ull    // -1/2!
#define LH_SC_C4_BITS 0x3fa5555555555555ull    //  1/4!
#define LH_SC_C6_BITS 0xbf56c16c16c16c17ull    // -1/6!
#define LH_SC_C8_BITS 0x3efa01a01a01a01aull    //  1/8!
#define LH_SC_C10_BITS 0xbe927e4fb7789f5cull   // -1/10!
#define LH_SC_C12_BITS 0x3e21eed8eff8d898ull   //  1/12!
#define LH_SC_C14_BITS 0xbda93974a8c07c9dull   // -1/14!
#define LH_SC_C16_BITS 0x3d2ae7f3e733b81full   //  1/16!
#define LH_SC_RND_BITS 0x4338000000000000ull   // 1.5 x 2^52: adding and subtracting it rounds to an integer

// one zero word (the bits before the binary point), then 256 bits of 2/pi, most significant word first; in device code a
// const array with a constant initialiser lives in constant memory (36 bytes)
static const unsigned int lh_sc_two_over_pi[9] = {
  0x00000000u, 0xa2f9836eu, 0x4e441529u, 0xfc2757d1u, 0xf534ddc0u,
  0xdb629599u, 0x3c439041u, 0xfe5163abu, 0xdebbc561u,
};

LH_SC_FN float lh_sc_f32_from_bits(const unsigned int b) {
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}
LH_SC_FN double lh_sc_f64_from_bits(const unsigned long long b) {
  double f;
  __builtin_memcpy(&f, &b, 8);
  return f;
}

// the sine kernel on the reduced interval
LH_SC_FN double lh_sc_sin_kernel(const double r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double s = r * r;
  double q = lh_sc_f64_from_bits(LH_SC_S15_BITS) * s;
  q = q + lh_sc_f64_from_bits(LH_SC_S13_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_S11_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_S9_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_S7_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_S5_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_S3_BITS);
  q = q * s;
  const double w = r * q;
  return r + w;
}

// the cosine kernel on the reduced interval
LH_SC_FN double lh_sc_cos_kernel(const double r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double s = r * r;
  double q = lh_sc_f64_from_bits(LH_SC_C16_BITS) * s;
  q = q + lh_sc_f64_from_bits(LH_SC_C14_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_C12_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_C10_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_C8_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_C6_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_C4_BITS);
  q = q * s;
  q = q + lh_sc_f64_from_bits(LH_SC_C2_BITS);
  const double w = s * q;
  return 1.0 + w;
}

// the three-part reduction: b = bits of a finite a = |x| < 2^20; returns the quadrant
LH_SC_FN int lh_sc_reduce_small(const unsigned int b, double *r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double a = (double)lh_sc_f32_from_bits(b);
  const double z = a * lh_sc_f64_from_bits(LH_SC_INV_BITS);
  const double zr = z + lh_sc_f64_from_bits(LH_SC_RND_BITS);
  const double kf = zr - lh_sc_f64_from_bits(LH_SC_RND_BITS);
  const double h1 = kf * lh_sc_f64_from_bits(LH_SC_P1_BITS);
  const double h2 = kf * lh_sc_f64_from_bits(LH_SC_P2_BITS);
  const double h3 = kf * lh_sc_f64_from_bits(LH_SC_P3_BITS);
  const double r1 = a - h1;
  const double r2 = r1 - h2;
  *r = r2 - h3;
  return (int)kf & 3;
}

// Payne-Hanek: b = bits of a finite a = |x| >= 2^20; returns the quadrant
LH_SC_FN int lh_sc_reduce_big(const unsigned int b, double *r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  typedef unsigned long long u64;
  const u64 m = (u64)((b & 0x007fffffu) | 0x00800000u);
  const int tb = (int)(b >> 23) - 150 - 2 + 32;  // the window's first bit, counted from the table's first: 27 .. 134
  const int wi = tb >> 5, sh = tb & 31;
  unsigned int h[4];
  for (int j = 0; j < 4; j++)
    h[j] = (unsigned int)((((u64)lh_sc_two_over_pi[wi + j] << 32) | (u64)lh_sc_two_over_pi[wi + j + 1]) >> (32 - sh));
  const u64 p3 = m * h[3];
  const u64 p2 = m * h[2] + (p3 >> 32);
  const u64 p1 = m * h[1] + (p2 >> 32);
  const u64 p0 = m * h[0] + (p1 >> 32);
  const u64 hi = (p0 << 32) | (p1 & 0xffffffffull), lo = (p2 << 32) | (p3 & 0xffffffffull);
  const int q = (int)((hi + (1ull << 61)) >> 62);
  u64 fh = (hi << 2) | (lo >> 62), fl = lo << 2;  // F, signed
  const u64 neg = fh >> 63;
  if (neg) {
    fl = ~fl + 1ull;
    fh = ~fh + (fl == 0ull ? 1ull : 0ull);
  }
  int drop = 0;
  if (fh == 0ull) {  // (no float32 comes this close to a multiple of pi/2; kept so that every input is defined)
    fh = fl;
    fl = 0ull;
    drop = 64;
  }
  double f = 0.0;
  if (fh != 0ull) {
    const int n = __builtin_clzll(fh);
    const u64 top = n ? (fh << n) | (fl >> (64 - n)) : fh;
    const double mant = (double)(long long)(top >> 11);  // 53 bits: exact
    f = mant * lh_sc_f64_from_bits((u64)(1023 - 53 - n - drop) << 52);  // exact
  }
  if (neg) f = -f;
  *r = f * lh_sc_f64_from_bits(LH_SC_PIO2_BITS);
  return q;
}

// the float64 sine (want_cos = 0) or cosine (1) of the angle (q + r * 2/pi) * pi/2 from the two kernels
LH_SC_FN double lh_sc_pick(const int q, const double r, const int want_cos) {
  const int j = (q + want_cos) & 3;  // cos(t) = sin(t + pi/2)
  const double y = (j & 1) ? lh_sc_cos_kernel(r) : lh_sc_sin_kernel(r);
  return (j & 2) ? -y : y;
}

// the same from the two kernels' values ks = sin kernel(r), kc = cos kernel(r), when both functions are wanted
LH_SC_FN double lh_sc_pick_of(const int q, const double ks, const double kc, const int want_cos) {
  const int j = (q + want_cos) & 3;
  const double y = (j & 1) ? kc : ks;
  return (j & 2) ? -y : y;
}

LH_SC_FN int lh_sc_reduce(const unsigned int babs, double *r) {
  return babs < LH_SC_BIG ? lh_sc_reduce_small(babs, r) : lh_sc_reduce_big(babs, r);
}

LH_SC_FN float lh_sin(const float x) {
  unsigned int b;
  __builtin_memcpy(&b, &x, 4);
  const unsigned int babs = b & 0x7fffffffu;
  if (babs >= 0x7f800000u) return lh_sc_f32_from_bits(LH_SC_NAN);
  double r;
  const int q = lh_sc_reduce(babs, &r);
  const float f = (float)lh_sc_pick(q, r, 0);
  unsigned int fb;
  __builtin_memcpy(&fb, &f, 4);
  return lh_sc_f32_from_bits(fb ^ (b & 0x80000000u));
}

LH_SC_FN float lh_cos(const float x) {
  unsigned int b;
  __builtin_memcpy(&b, &x, 4);
  const unsigned int babs = b & 0x7fffffffu;
  if (babs >= 0x7f800000u) return lh_sc_f32_from_bits(LH_SC_NAN);
  double r;
  const int q = lh_sc_reduce(babs, &r);
  return (float)lh_sc_pick(q, r, 1);
}

// both from one reduction: *s has the bits of lh_sin(x), *c those of lh_cos(x)
LH_SC_FN void lh_sincos(const float x, float *s, float *c) {
  unsigned int b;
  __builtin_memcpy(&b, &x, 4);
  const unsigned int babs = b & 0x7fffffffu;
  if (babs >= 0x7f800000u) {
    *s = lh_sc_f32_from_bits(LH_SC_NAN);
    *c = lh_sc_f32_from_bits(LH_SC_NAN);
    return;
  }
  double r;
  const int q = lh_sc_reduce(babs, &r);
  const double ks = lh_sc_sin_kernel(r), kc = lh_sc_cos_kernel(r);
  const float fs = (float)lh_sc_pick_of(q, ks, kc, 0), fc = (float)lh_sc_pick_of(q, ks, kc, 1);
  unsigned int fb;
  __builtin_memcpy(&fb, &fs, 4);
  *s = lh_sc_f32_from_bits(fb ^ (b & 0x80000000u));
  *c = fc;
}

// the names for forEach / forEachReduce bodies: "o = x + y - laser_sin(z)", "acc += laser_cos(x)"
LH_SC_FN float laser_sin(const float x) { return lh_sin(x); }
LH_SC_FN float laser_cos(const float x) { return lh_cos(x); }

#endif  // LASER_HIP_SINCOS_CORE_H
