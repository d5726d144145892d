// laser_amd/csrc/normal_core.h -- the normal distribution on the library's Philox streams (float32), as one definition: the
// fill kernel (random.hip) includes it, and a host program built with a plain C++ compiler can include it too.
// include/laser_hip.h ("Random numbers") states it in words; tests/normal_model.py is the numpy model.
//
// Box-Muller, fixed so that a fill can be cut anywhere.  Element i of a call with `offset` is stream position
// p = (offset + i) mod 2^64, one word per element, so offsets count elements exactly as for the 32-bit uniform fills.  Pair
// q = p >> 1 owns words 2q and 2q + 1 of the stream (seed, subseq); position p is the pair's cosine branch if it is even and
// its sine branch if it is odd.  A pair never straddles a Philox block, and a fill that starts or ends inside a pair stores
// only its half.  With w0 = word(2q), w1 = word(2q + 1):
//   radius   u = float((w0 >> 8) + 1) * 2^-24       in (0, 1], both steps exact
//            L = llog(u)                             log_core.h: <= +0, and +0 only for u = 1
//            r = sqrt(|-2 L|)                        -2 L is exact; |.| keeps u = 1 at +0; a correctly rounded float32 square
//                                                    root: __builtin_sqrtf, which is the IEEE instruction on the host and, in
//                                                    device code built without fast-math or -fno-hip-fp32-correctly-rounded-
//                                                    divide-sqrt (this library's flags), the compiler's correctly rounded
//                                                    expansion (v_sqrt_f32 and a fixup by fma and compare).  No float64 detour.
//   angle    k = w1 >> 8: the angle is 2 pi k / 2^24.  Reduced on the integer: j = (k + 2^21) >> 22 (0 .. 4),
//            quadrant j & 3, fraction f = int(k) - j 2^22 in [-2^21, 2^21); a = (float64(f) * 2^-22) * PIO2: the first product
//            is exact, the second is the one rounding, by sincos_core.h's float64(pi/2).  t = float32 of sincos_core.h's sine or
//            cosine kernel at a, chosen and signed by the quadrant exactly as lsin / lcos do (lh_sc_pick), rounded once.
//   result   z = r * t (one float32 rounding);  out = mean + std * z (two more, never contracted).
// |t| <= 1 and L >= llog(2^-24), so |z| <= sqrt(2 x 24 x ln 2) < 5.77 and every result is finite.  mean = 0, std = 1 return
// z's value (a -0 becomes +0).  Valid: mean finite, std finite and >= 0.
//
// Plain C++; includes philox_core.h, log_core.h and sincos_core.h and nothing else.  A host build needs -ffp-contract=off (the
// pragmas below cover clang).  Names start with lh_.
#ifndef LASER_HIP_NORMAL_CORE_H
#define LASER_HIP_NORMAL_CORE_H

#include "log_core.h"
#include "philox_core.h"
#include "sincos_core.h"

// r of a pair from its first word
LH_PHILOX_FN float lh_normal_radius(const unsigned int w0) {
  const float u = (float)((w0 >> 8) + 1u) * 5.9604644775390625e-8f;  // 2^-24; both steps exact
  const float t = -2.0f * lh_log(u);                                 // exact
  unsigned int tb;
  __builtin_memcpy(&tb, &t, 4);
  return __builtin_sqrtf(lh_sc_f32_from_bits(tb & 0x7fffffffu));
}

// quadrant and reduced argument of a pair's angle from its second word
LH_PHILOX_FN int lh_normal_angle(const unsigned int w1, double *a) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const unsigned int k = w1 >> 8;
  const unsigned int j = (k + (1u << 21)) >> 22;
  const int f = (int)k - (int)(j << 22);
  const double frac = (double)f * 2.384185791015625e-7;  // 2^-22: exact
  *a = frac * lh_sc_f64_from_bits(LH_SC_PIO2_BITS);
  return (int)(j & 3u);
}

// z of the pair's cosine branch (odd = 0) or sine branch (odd = 1)
LH_PHILOX_FN float lh_normal_z(const unsigned int w0, const unsigned int w1, const int odd) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double a;
  const int q = lh_normal_angle(w1, &a);
  const float t = (float)lh_sc_pick(q, a, odd ? 0 : 1);
  return lh_normal_radius(w0) * t;
}

// both branches of a pair: radius and angle reduction shared
LH_PHILOX_FN void lh_normal_pair(const unsigned int w0, const unsigned int w1, float *zc, float *zs) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double a;
  const int q = lh_normal_angle(w1, &a);
  const float r = lh_normal_radius(w0);
  const double ks = lh_sc_sin_kernel(a), kc = lh_sc_cos_kernel(a);
  const float tc = (float)lh_sc_pick_of(q, ks, kc, 1), ts = (float)lh_sc_pick_of(q, ks, kc, 0);
  *zc = r * tc;
  *zs = r * ts;
}

LH_PHILOX_FN float lh_normal_scale_f32(const float z, const float mean, const float std) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float t = std * z;
  return mean + t;
}

// mean finite, std finite and >= 0 (NaN fails every comparison)
LH_PHILOX_FN int lh_normal_params_ok_f32(const float mean, const float std) {
  const float big = 3.40282346638528859812e38f;
  return mean >= -big && mean <= big && std >= 0.0f && std <= big;
}

#endif  // LASER_HIP_NORMAL_CORE_H
