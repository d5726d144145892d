// laser_amd/csrc/log_core.h -- llog, a bit-defined float32 natural logarithm, as one definition: the precompiled log,
// logsumexp, log-softmax and cross-entropy kernels (log_softmax.hip) include it, the run-time-compiled forEach /
// forEachReduce kernels get it in the prelude of their source after exp_core.h (foreach.cpp embeds this file), and a host
// program can include it too.  include/laser_hip.h ("log, logsumexp, log-softmax and cross-entropy") states it in words;
// tests/log_model.py is the numpy model.  The reference's files are named exp_log_* but hold no logarithm: this one is ours.
//
// Only integer operations, bit casts, an exact float32 -> float64 conversion, float64 + - x each rounded on its own (never
// a fused multiply-add), and one float64 -> float32 rounding (nearest even).  No division, no libm.  For a float32 x with
// bits b:
//   1. NaN gives NaN (payload unspecified).  +-0 gives -Inf.  Sign bit set otherwise (-Inf too) gives NaN.  +Inf gives +Inf.
//   2. A subnormal is normalised in integers: n = clz(b) - 8, b <<= n, k0 = -n (so b now reads as 1.f x 2^-126 and the value
//      is that times 2^k0); otherwise k0 = 0.  No floating-point operation sees a subnormal.
//   3. t = b - 0x3f330000 (mod 2^32);  k = k0 + (int32(t) >> 23) (arithmetic shift);  i = (t >> 19) & 15;
//      z = float64(bitcast<float>(b - (t & 0xff800000))).  So x = 2^k z with z in [0.69921875, 1.3984375): reduced around 1,
//      and i is the sixteenth of that range z lies in.
//   4. r = z * INVC[i] - 1      INVC[i] = float64(1 / c_i), c_i the midpoint of interval i; interval 9, which holds 1, has
//                               INVC = 1 and LOGC = +0, so there r = z - 1 exactly.  |r| < 0.02963.
//   5. q = (((C6 r + C5) r + C4) r + C3) r + C2      C_j = float64((-1)^(j+1) / j): log(1 + r) = r + r^2 (C2 + C3 r + ..)
//   6. y = ((float64(k) * LN2 + LOGC[i]) + r) + (r * r) * q      LOGC[i] = float64(-ln INVC[i]), LN2 = float64(ln 2)
//   7. llog(x) = float32(y)
// llog(1) = +0: k = 0, i = 9, r = +0, and every sum above is +0.  The series is cut after r^6 / 6: the next term is below
// 2.9e-12, against results that are at least 0.0234 in magnitude outside interval 9 and r itself inside it, so y is the true
// logarithm to 2^-32 relative or better and the one float32 rounding decides the error.
//
// Measured over all 2^31 - 2^23 positive finite float32 against (float)log((double)x) of glibc (tests/cpp/log_core_host.cpp
// "sweep"; profiles/log_softmax/README.md has the output):
//   faithful (one of the two float32 that bracket the true value) for every input, non-decreasing over all of them;
//   maximum error 0.501403 ulp at x = bits 0x3f8301a3 (1.0234874), mean error 0.250000 ulp; 229 of the 2139095039 inputs
//   do not get the correctly rounded float32 (each the other neighbour of the true value).
//
// float64 inside, not a float32-only form: profiles/log_softmax/README.md ("float64 inside") has the reasoning and the
// measurement of the elementwise kernel against lexp's (1.38 times its time at 2^26 elements).  A float32-only form would
// need two-float arithmetic without fma (Dekker splits) to stay faithful next to 1.
//
// Plain C++ with no includes: hiprtc compiles it as it stands.  A host build needs -ffp-contract=off (the pragma below
// covers clang).  Names start with lh_, and laser_log is the one name meant for forEach bodies.
#ifndef LASER_HIP_LOG_CORE_H
#define LASER_HIP_LOG_CORE_H

#if defined(__HIPCC_RTC__)
#define LH_LOG_FN __device__ inline __attribute__((always_inline))
#elif defined(__HIP__)
#define LH_LOG_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LH_LOG_FN static inline
#endif

#define LH_LOG_OFF 0x3f330000u               // bits of 0.69921875, the low end of the reduced range
#define LH_LOG_LN2_BITS 0x3fe62e42fefa39efull  // float64(ln 2)
#define LH_LOG_C2_BITS 0xbfe0000000000000ull   // -1/2
#define LH_LOG_C3_BITS 0x3fd5555555555555ull   //  1/3
#define LH_LOG_C4_BITS 0xbfd0000000000000ull   // -1/4
#define LH_LOG_C5_BITS 0x3fc999999999999aull   //  1/5
#define LH_LOG_C6_BITS 0xbfc5555555555555ull   // -1/6

// {INVC[i], LOGC[i]} as float64 bit patterns; in device code a const array with a constant initialiser lives in constant
// memory (256 bytes: two cache lines)
alignas(16) static const unsigned long long lh_log_tab[32] = {
  0x3ff661ec6a5122f9ull, 0xbfd57bf753c8d1fbull,  //  0  [0.6992188, 0.7304688)  1.3989071038251366  -0.33569129163814154
  0x3ff571ed3c506b3aull, 0xbfd2bef07cdc9355ull,  //  1  [0.7304688, 0.7617188)  1.3403141361256545  -0.29290401643293268
  0x3ff49539e3b2d067ull, 0xbfd01eae5626c691ull,  //  2  [0.7617188, 0.7929688)  1.2864321608040201  -0.25187261975507008
  0x3ff3c995a47babe7ull, 0xbfcb31d8575bce3bull,  //  3  [0.7929688, 0.8242188)  1.2367149758454106  -0.21245865121419336
  0x3ff30d190130d190ull, 0xbfc6574ebe8c1339ull,  //  4  [0.8242188, 0.8554688)  1.1906976744186046  -0.17453941635189965
  0x3ff25e22708092f1ull, 0xbfc1aa2b7e23f729ull,  //  5  [0.8554688, 0.8867188)  1.147982062780269   -0.13800567301944369
  0x3ff1bb4a4046ed29ull, 0xbfba4e7640b1bc38ull,  //  6  [0.8867188, 0.9179688)  1.1082251082251082  -0.10275973395776894
  0x3ff12358e75d3033ull, 0xbfb1973bd1465561ull,  //  7  [0.9179688, 0.9492188)  1.0711297071129706  -0.068713892548051728
  0x3ff0953f39010954ull, 0xbfa252f32f8d1840ull,  //  8  [0.9492188, 0.9804688)  1.0364372469635628  -0.035789107851585289
  0x3ff0000000000000ull, 0x0000000000000000ull,  //  9  [0.9804688, 1.0234375)  1                   0
  0x3fee573ac901e574ull, 0x3fab42dd711971b9ull,  // 10  [1.0234375, 1.0859375)  0.94814814814814818 0.053244514518812243
  0x3feca4b3055ee191ull, 0x3fbc5e548f5bc743ull,  // 11  [1.0859375, 1.1484375)  0.8951048951048951  0.11081436634029011
  0x3feb2036406c80d9ull, 0x3fc526e5e3a1b438ull,  // 12  [1.1484375, 1.2109375)  0.84768211920529801 0.16524957289530717
  0x3fe9c2d14ee4a102ull, 0x3fcbc286742d8cd4ull,  // 13  [1.2109375, 1.2734375)  0.80503144654088055 0.2168739383006143
  0x3fe886e5f0abb04aull, 0x3fd1058bf9ae4ad4ull,  // 14  [1.2734375, 1.3359375)  0.76646706586826352 0.26596354849713788
  0x3fe767dce434a9b1ull, 0x3fd404308686a7e4ull,  // 15  [1.3359375, 1.3984375)  0.73142857142857143 0.3127557100038969
};

LH_LOG_FN float lh_log_f32_from_bits(const unsigned int b) {
  float f;
  __builtin_memcpy(&f, &b, 4);
  return f;
}
LH_LOG_FN double lh_log_f64_from_bits(const unsigned long long b) {
  double f;
  __builtin_memcpy(&f, &b, 8);
  return f;
}

LH_LOG_FN float lh_log(const float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  unsigned int b;
  __builtin_memcpy(&b, &x, 4);
  if (x != x) return x;
  if ((b << 1) == 0u) return lh_log_f32_from_bits(0xff800000u);  // +-0
  if (b >> 31) return lh_log_f32_from_bits(0x7fc00000u);         // negative, -Inf
  if (b == 0x7f800000u) return x;
  int k = 0;
  if (b < 0x00800000u) {  // subnormal: b != 0, at least 9 leading zeros
    const int n = __builtin_clz(b) - 8;
    b <<= n;
    k = -n;
  }
  const unsigned int t = b - LH_LOG_OFF;
  k += (int)t >> 23;
  const unsigned int i = (t >> 19) & 15u;
  const double z = (double)lh_log_f32_from_bits(b - (t & 0xff800000u));
  const double invc = lh_log_f64_from_bits(lh_log_tab[2 * i]), logc = lh_log_f64_from_bits(lh_log_tab[2 * i + 1]);
  const double p = z * invc;
  const double r = p - 1.0;
  double q = lh_log_f64_from_bits(LH_LOG_C6_BITS) * r;
  q = q + lh_log_f64_from_bits(LH_LOG_C5_BITS);
  q = q * r;
  q = q + lh_log_f64_from_bits(LH_LOG_C4_BITS);
  q = q * r;
  q = q + lh_log_f64_from_bits(LH_LOG_C3_BITS);
  q = q * r;
  q = q + lh_log_f64_from_bits(LH_LOG_C2_BITS);
  const double kl = (double)k * lh_log_f64_from_bits(LH_LOG_LN2_BITS);
  const double y0 = kl + logc;
  const double y1 = y0 + r;
  const double r2 = r * r;
  const double w = r2 * q;
  return (float)(y1 + w);
}

// the name for forEach / forEachReduce bodies: "y = laser_log(x)"
LH_LOG_FN float laser_log(const float x) { return lh_log(x); }

#endif  // LASER_HIP_LOG_CORE_H
