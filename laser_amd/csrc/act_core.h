// laser_amd/csrc/act_core.h -- ltanh and lsigmoid, a bit-defined float32 hyperbolic tangent and logistic function, as one
// definition: the precompiled activation kernels (activation.hip) include it, the run-time-compiled forEach / forEachReduce
// kernels get it in the prelude of their source after log_core.h (foreach.cpp embeds this file), and a host program can
// include it too.  include/laser_hip.h ("Activations") states it in words; tests/act_model.py is the numpy model.
//
// Only integer operations, bit casts, one exact float32 -> float64 conversion, float64 + - x / each rounded on its own (never
// a fused multiply-add in the parts written here), exactly one float64 division per result (IEEE correctly rounded on the
// host and in hipcc's default lowering, which builds it from fmas of its own) and one float64 -> float32 rounding (nearest
// even).  No libm, no device transcendental instruction.
//
// Constants (float64, kept as bit patterns):
//   INV = float64(64 / ln 2);  HI = float64(ln 2 / 64) with its low 24 significand bits cleared, so k * HI is exact for
//   |k| < 2^24;  LO = float64(ln 2 / 64 - HI);  T[j] = the correctly rounded float64 of 2^(j/64), j = 0..63;
//   C2..C5 = float64(1/2, 1/6, 1/24, 1/120);  D3, D5, D7 = float64(-1/3, 2/15, -17/315);  R = 1.5 x 2^52.
//
// E(a) for a float64 a in [-208, 0] (lh_act_exp):
//   1. kf = (a * INV + R) - R, which is a * INV rounded to the nearest integer, ties to even (|a * INV| < 2^15);
//      k = int(kf).
//   2. r = (a - kf * HI) - kf * LO                                    |r| <= ln 2 / 128 (+ a rounding)
//   3. q = ((C5 r + C4) r + C3) r + C2
//   4. p = r + (r * r) * q                                            e^r - 1, cut after r^5 / 120 (next term < 3.5e-17)
//   5. e = T[k & 63] + T[k & 63] * p
//   6. E = e * bitcast<float64>(uint64((k >> 6) + 1023) << 52)        an exact multiply by 2^(k >> 6) (arithmetic shift);
//                                                                     k >> 6 >= -301, never subnormal in float64
//
// lsigmoid(x) for a float32 x (lh_act_sigmoid):
//   1. NaN gives NaN (payload unspecified).
//   2. c = min(float64(|x|), 104); +-Inf clamp like any other value.  e = E(-c), d = 1 + e.
//   3. sign bit clear (+0 too): float32(1 / d);  sign bit set (-0 too): float32(e / d).
//   lsigmoid(+-0) = 0.5 (e = 1, d = 2).  For x in about [-103.97, -87.34] the result is a float32 subnormal, rounded once
//   from the float64 quotient: no denormal is flushed.
//
// ltanh(x) for a float32 x (lh_act_tanh):
//   1. NaN gives NaN (payload unspecified).
//   2. a = min(float64(|x|), 10).
//   3. a < 2^-6:  s = a * a,  q = ((D7 s + D5) s + D3) s,  y = a + a * q     (lh_act_tanh_small; the next term of the
//                 series, 62/2835 a^9, is below 2^-59 a)
//      otherwise: e = E(-2 a),  y = (1 - e) / (1 + e)
//   4. ltanh(x) = float32(y) with x's sign bit ORed into its bits.
//   So ltanh(-x) has the bits of -ltanh(x), ltanh(-0) = -0, ltanh(+-Inf) = +-1, and ltanh(x) = x for subnormal and tiny x.
//
// Measured over every finite float32 (2 x 2139095040 inputs) against tanhl and expl in 80-bit long double
// (tests/cpp/act_core_host.cpp "sweep"; profiles/activation/README.md has the output):
//   faithful (one of the two float32 that bracket the true value) at every input, non-decreasing over all of them in
//   increasing order, |ltanh| <= 1, 0 <= lsigmoid <= 1, ltanh(-x) = -ltanh(x) bit for bit;
//   ltanh: the correctly rounded float32 at every input (maximum error 0.500000 ulp, mean 0.015762); 1 from bits 0x41102cb4
//   (9.010914);
//   lsigmoid: maximum error 0.500000 ulp, mean 0.031307; 73 of the 4278190080 results are the other neighbour of the true value
//   instead of the nearest; 1 from bits 0x418aa123 (17.32868), 0 from bits 0xc2cff1b5 (-103.972084).
//   These are the points at which numpy's float64 tanh and logistic function, rounded to float32, saturate.
//
// Plain C++ with no includes: hiprtc compiles it as it stands.  A host build needs -ffp-contract=off (the pragma below
// covers clang).  Names start with lh_act_, and laser_tanh and laser_sigmoid are the two names meant for forEach bodies.
#ifndef LASER_HIP_ACT_CORE_H
#define LASER_HIP_ACT_CORE_H

#if defined(__HIPCC_RTC__)
#define LH_ACT_FN __device__ inline __attribute__((always_inline))
#elif defined(__HIP__)
#define LH_ACT_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LH_ACT_FN static inline
#endif

#define LH_ACT_INV_BITS 0x40571547652b82feull  // 64 / ln 2 = 92.33248261689366
#define LH_ACT_HI_BITS 0x3f862e42fe000000ull   // 0.010830424667801708
#ifndef LH_ACT_LO_BITS                         // (a test builds a deliberately wrong copy with another value)
#define LH_ACT_LO_BITS 0x3dbf473de6af278full   // 2.8447437476627285e-11
#endif
#define LH_ACT_C2_BITS 0x3fe0000000000000ull   // 1/2
#define LH_ACT_C3_BITS 0x3fc5555555555555ull   // 1/6
#define LH_ACT_C4_BITS 0x3fa5555555555555ull   // 1/24
#define LH_ACT_C5_BITS 0x3f81111111111111ull   // 1/120
#define LH_ACT_D3_BITS 0xbfd5555555555555ull   // -1/3
#define LH_ACT_D5_BITS 0x3fc1111111111111ull   // 2/15
#define LH_ACT_D7_BITS 0xbfaba1ba1ba1ba1cull   // -17/315
#define LH_ACT_RND_BITS 0x4338000000000000ull  // 1.5 x 2^52: adding and subtracting it rounds to an integer
#define LH_ACT_SIG_CLAMP_BITS 0x405a000000000000ull   // 104
#define LH_ACT_TANH_CLAMP_BITS 0x4024000000000000ull  // 10
#define LH_ACT_TANH_SMALL_BITS 0x3f90000000000000ull  // 2^-6

// T[j] = float64(2^(j/64)) as bit patterns; in device code a const array with a constant initialiser lives in constant
// memory (512 bytes: four cache lines)
alignas(16) static const unsigned long long lh_act_tab[64] = {
  0x3ff0000000000000ull, 0x3ff02c9a3e778061ull,  //  0  1  1.0108892860517005
  0x3ff059b0d3158574ull, 0x3ff0874518759bc8ull,  //  2  1.0218971486541166  1.0330248790212284
  0x3ff0b5586cf9890full, 0x3ff0e3ec32d3d1a2ull,  //  4  1.0442737824274138  1.0556451783605572
  0x3ff11301d0125b51ull, 0x3ff1429aaea92de0ull,  //  6  1.0671404006768237  1.0787607977571199
  0x3ff172b83c7d517bull, 0x3ff1a35beb6fcb75ull,  //  8  1.0905077326652577  1.1023825833078409
  0x3ff1d4873168b9aaull, 0x3ff2063b88628cd6ull,  // 10  1.1143867425958924  1.1265216186082418
  0x3ff2387a6e756238ull, 0x3ff26b4565e27cddull,  // 12  1.1387886347566916  1.1511892299529827
  0x3ff29e9df51fdee1ull, 0x3ff2d285a6e4030bull,  // 14  1.1637248587775775  1.1763969916502812
  0x3ff306fe0a31b715ull, 0x3ff33c08b26416ffull,  // 16  1.189207115002721  1.2021567314527031
  0x3ff371a7373aa9cbull, 0x3ff3a7db34e59ff7ull,  // 18  1.215247359980469  1.22848053610687
  0x3ff3dea64c123422ull, 0x3ff4160a21f72e2aull,  // 20  1.241857812073484  1.2553807570246911
  0x3ff44e086061892dull, 0x3ff486a2b5c13cd0ull,  // 22  1.2690509571917332  1.2828700160787783
  0x3ff4bfdad5362a27ull, 0x3ff4f9b2769d2ca7ull,  // 24  1.2968395546510096  1.3109612115247644
  0x3ff5342b569d4f82ull, 0x3ff56f4736b527daull,  // 26  1.3252366431597413  1.3396675240533029
  0x3ff5ab07dd485429ull, 0x3ff5e76f15ad2148ull,  // 28  1.3542555469368927  1.3690024229745905
  0x3ff6247eb03a5585ull, 0x3ff6623882552225ull,  // 30  1.383909881963832  1.3989796725383112
  0x3ff6a09e667f3bcdull, 0x3ff6dfb23c651a2full,  // 32  1.4142135623730951  1.42961333839197
  0x3ff71f75e8ec5f74ull, 0x3ff75feb564267c9ull,  // 34  1.4451808069770467  1.460917794180647
  0x3ff7a11473eb0187ull, 0x3ff7e2f336cf4e62ull,  // 36  1.4768261459394993  1.4929077282912648
  0x3ff82589994cce13ull, 0x3ff868d99b4492edull,  // 38  1.5091644275934228  1.5255981507445384
  0x3ff8ace5422aa0dbull, 0x3ff8f1ae99157736ull,  // 40  1.5422108254079407  1.5590044002378369
  0x3ff93737b0cdc5e5ull, 0x3ff97d829fde4e50ull,  // 42  1.5759808451078865  1.593142151342267
  0x3ff9c49182a3f090ull, 0x3ffa0c667b5de565ull,  // 44  1.6104903319492543  1.6280274218573478
  0x3ffa5503b23e255dull, 0x3ffa9e6b5579fdbfull,  // 46  1.6457554781539649  1.6636765803267364
  0x3ffae89f995ad3adull, 0x3ffb33a2b84f15fbull,  // 48  1.681792830507429  1.7001063537185235
  0x3ffb7f76f2fb5e47ull, 0x3ffbcc1e904bc1d2ull,  // 50  1.7186192981224779  1.7373338352737062
  0x3ffc199bdd85529cull, 0x3ffc67f12e57d14bull,  // 52  1.7562521603732995  1.7753764925265212
  0x3ffcb720dcef9069ull, 0x3ffd072d4a07897cull,  // 54  1.7947090750031072  1.8142521755003989
  0x3ffd5818dcfba487ull, 0x3ffda9e603db3285ull,  // 56  1.8340080864093424  1.8539791250833855
  0x3ffdfc97337b9b5full, 0x3ffe502ee78b3ff6ull,  // 58  1.8741676341103  1.8945759815869656
  0x3ffea4afa2a490daull, 0x3ffefa1bee615a27ull,  // 60  1.9152065613971474  1.9360617934922943
  0x3fff50765b6e4540ull, 0x3fffa7c1819e90d8ull,  // 62  1.9571441241754002  1.9784560263879509
};

LH_ACT_FN float lh_act_f32_from_bits(const unsigned int b) {
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}
LH_ACT_FN double lh_act_f64_from_bits(const unsigned long long b) {
  double f;
  __builtin_memcpy(&f, &b, 8);
  return f;
}

// E(a), a in [-208, 0]
LH_ACT_FN double lh_act_exp(const double a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double z = a * lh_act_f64_from_bits(LH_ACT_INV_BITS);
  const double zr = z + lh_act_f64_from_bits(LH_ACT_RND_BITS);
  const double kf = zr - lh_act_f64_from_bits(LH_ACT_RND_BITS);
  const int k = (int)kf;
  const double h = kf * lh_act_f64_from_bits(LH_ACT_HI_BITS);
  const double l = kf * lh_act_f64_from_bits(LH_ACT_LO_BITS);
  const double r0 = a - h;
  const double r = r0 - l;
  double q = lh_act_f64_from_bits(LH_ACT_C5_BITS) * r;
  q = q + lh_act_f64_from_bits(LH_ACT_C4_BITS);
  q = q * r;
  q = q + lh_act_f64_from_bits(LH_ACT_C3_BITS);
  q = q * r;
  q = q + lh_act_f64_from_bits(LH_ACT_C2_BITS);
  const double r2 = r * r;
  const double w = r2 * q;
  const double p = r + w;
  const double t = lh_act_f64_from_bits(lh_act_tab[k & 63]);
  const double tp = t * p;
  const double e = t + tp;
  const double scale = lh_act_f64_from_bits((unsigned long long)((k >> 6) + 1023) << 52);
  return e * scale;
}

// the odd polynomial of ltanh, 0 <= a < 2^-6
LH_ACT_FN double lh_act_tanh_small(const double a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double s = a * a;
  double q = lh_act_f64_from_bits(LH_ACT_D7_BITS) * s;
  q = q + lh_act_f64_from_bits(LH_ACT_D5_BITS);
  q = q * s;
  q = q + lh_act_f64_from_bits(LH_ACT_D3_BITS);
  q = q * s;
  const double w = a * q;
  return a + w;
}

LH_ACT_FN float lh_act_sigmoid(const float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  unsigned int b;
  __builtin_memcpy(&b, &x, 4);
  if (x != x) return x;
  const double ax = (double)lh_act_f32_from_bits(b & 0x7fffffffu), top = lh_act_f64_from_bits(LH_ACT_SIG_CLAMP_BITS);
  const double c = ax < top ? ax : top;
  const double e = lh_act_exp(-c);
  const double d = 1.0 + e;
  const double num = (b >> 31) ? e : 1.0;
  return (float)(num / d);
}

LH_ACT_FN float lh_act_tanh(const float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  unsigned int b;
  __builtin_memcpy(&b, &x, 4);
  if (x != x) return x;
  const double ax = (double)lh_act_f32_from_bits(b & 0x7fffffffu), top = lh_act_f64_from_bits(LH_ACT_TANH_CLAMP_BITS);
  const double a = ax < top ? ax : top;
  double y;
  if (a < lh_act_f64_from_bits(LH_ACT_TANH_SMALL_BITS)) {
    y = lh_act_tanh_small(a);
  } else {
    const double a2 = -2.0 * a;
    const double e = lh_act_exp(a2);
    const double num = 1.0 - e, den = 1.0 + e;
    y = num / den;
  }
  const float f = (float)y;
  unsigned int fb;
  __builtin_memcpy(&fb, &f, 4);
  return lh_act_f32_from_bits(fb | (b & 0x80000000u));
}

// the names for forEach / forEachReduce bodies: "y = laser_tanh(x)", "y = laser_sigmoid(x)"
LH_ACT_FN float laser_tanh(const float x) { return lh_act_tanh(x); }
LH_ACT_FN float laser_sigmoid(const float x) { return lh_act_sigmoid(x); }

#endif  // LASER_HIP_ACT_CORE_H
