// laser_amd/csrc/philox_core.h -- the library's random number generator, Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel
// random numbers: as easy as 1, 2, 3", SC'11), and the uniform distributions on top of it, as one definition: the fill kernels
// (random.hip) and the sampler's self-drawing kernels (sampler.hip) include it, and a host program built with a plain C++
// compiler can include it too.  include/laser_hip.h ("Random numbers") states it in words; tests/philox_model.py is the numpy
// model.
//
// Counter-based: word w of a stream is a function of (seed, subseq, w) and of nothing else.  No state lives on the device, a
// call captured in a graph replays the same numbers, and a result never depends on the grid, the stream or the alignment.
//
// One block: counter c[0..3], key k[0..1], ten rounds of
//     (hi0, lo0) = 0xD2511F53 * c[0],  (hi1, lo1) = 0xCD9E8D57 * c[2]        (32 x 32 -> 64 bit products)
//     c = {hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0}
// with the key bumped by the Weyl increments (0x9E3779B9, 0xBB67AE85) between rounds (nine bumps).
// Stream layout: a stream is named by (seed, subseq), both 64 bits.  Word w (64 bits) is word w & 3 of the block with
//     counter {lo32(b), hi32(b), lo32(subseq), hi32(subseq)},  b = w >> 2,     key {lo32(seed), hi32(seed)}.
// Element i of a call with `offset` uses word (offset + i) mod 2^64; a 64-bit element type uses the pair
// (offset + 2 i, offset + 2 i + 1), low word first: x = w0 | w1 << 32.
//
// Distributions.  Every float operation is rounded on its own in the element type, nothing is contracted into an FMA.
//   bits u32        the word itself
//   u01 f32         float(x >> 8) * 2^-24: in [0, 1), the largest value 1 - 2^-24 (both steps exact)
//   u01 f64         double(x >> 11) * 2^-53 of the 64-bit x
//   uniform f32/f64 on [lo, hi]: t = u01 * (hi - lo), v = lo + t, the result min(v, hi).  The interval is closed like Nim's
//                   rand(a..b); the min is needed (float32 lo = 1, hi = 2 and lo = 0.1, hi = 0.3 round up to hi at the largest
//                   u01, and others could pass it).  lo = 0, hi = 1 returns u01's bits.  Valid: lo, hi, hi - lo finite, lo <= hi.
//   uniform i32     on [lo, hi]: span = hi - lo + 1 in 1 .. 2^32; lo + int32((uint64(x) * span) >> 32), wrapping
//   uniform i64     span = hi - lo + 1 mod 2^64; span == 0 is the full range and the result is x as a signed value; otherwise
//                   lo + mulhi64(x, span), wrapping
// The integer multiply-shift is not exactly uniform: a value is hit by floor or ceil of 2^32 / span words (2^64 / span), so a
// probability is off by at most a factor 1 +- span / 2^32 (i32) or span / 2^64 (i64).  There is no rejection loop: an element
// costs a fixed number of words, which is what makes offsets and chunked fills add up.
// The normal distribution (float32, Box-Muller on pairs of words) is normal_core.h, on top of this file, log_core.h and
// sincos_core.h.
// Not built: float64 normals, other distributions, the other six element types, strided destinations, a laser_rand callable in
// forEach bodies.
//
// Plain C++ with no includes.  A host build needs -ffp-contract=off (the pragma below covers clang).  Names start with lh_.
#ifndef LASER_HIP_PHILOX_CORE_H
#define LASER_HIP_PHILOX_CORE_H

#if defined(__HIP__)
#define LH_PHILOX_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LH_PHILOX_FN static inline
#endif

#define LH_PHILOX_M0 0xD2511F53u
#define LH_PHILOX_M1 0xCD9E8D57u
#define LH_PHILOX_W0 0x9E3779B9u
#define LH_PHILOX_W1 0xBB67AE85u

// ten rounds on c[0..3] in place; k0, k1 are copies and the caller's key is not changed
LH_PHILOX_FN void lh_philox4x32_10(unsigned int c[4], unsigned int k0, unsigned int k1) {
#if defined(__clang__)
#pragma unroll
#endif
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = (unsigned long long)LH_PHILOX_M0 * c[0];
    const unsigned long long p1 = (unsigned long long)LH_PHILOX_M1 * c[2];
    const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0;
    const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (unsigned int)p1;
    c[2] = n2;
    c[3] = (unsigned int)p0;
    k0 += LH_PHILOX_W0;
    k1 += LH_PHILOX_W1;
  }
}

// block b of the stream (seed, subseq): words 4 b .. 4 b + 3
LH_PHILOX_FN void lh_philox_block(const unsigned long long seed, const unsigned long long subseq, const unsigned long long b,
                                  unsigned int out[4]) {
  out[0] = (unsigned int)b;
  out[1] = (unsigned int)(b >> 32);
  out[2] = (unsigned int)subseq;
  out[3] = (unsigned int)(subseq >> 32);
  lh_philox4x32_10(out, (unsigned int)seed, (unsigned int)(seed >> 32));
}

// word w of the stream, on its own (a whole block is computed for it)
LH_PHILOX_FN unsigned int lh_philox_word(const unsigned long long seed, const unsigned long long subseq, const unsigned long long w) {
  unsigned int o[4];
  lh_philox_block(seed, subseq, w >> 2, o);
  const int j = (int)(w & 3);
  return j == 0 ? o[0] : j == 1 ? o[1] : j == 2 ? o[2] : o[3];  // selects, not an indexed load: the block stays in registers
}

LH_PHILOX_FN unsigned long long lh_mulhi64(const unsigned long long a, const unsigned long long b) {
#if defined(__SIZEOF_INT128__) && !defined(__HIP_DEVICE_COMPILE__)
  return (unsigned long long)(((unsigned __int128)a * b) >> 64);
#else
  const unsigned long long al = a & 0xffffffffull, ah = a >> 32, bl = b & 0xffffffffull, bh = b >> 32;
  const unsigned long long ll = al * bl, lh = al * bh, hl = ah * bl, hh = ah * bh;
  const unsigned long long mid = (ll >> 32) + (lh & 0xffffffffull) + (hl & 0xffffffffull);
  return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
#endif
}

LH_PHILOX_FN float lh_u01_f32(const unsigned int x) {
  return (float)(x >> 8) * 5.9604644775390625e-8f;  // 2^-24; both steps exact
}
LH_PHILOX_FN double lh_u01_f64(const unsigned long long x) {
  return (double)(x >> 11) * 1.1102230246251565404e-16;  // 2^-53; both steps exact
}
LH_PHILOX_FN float lh_uniform_f32(const unsigned int x, const float lo, const float hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float d = hi - lo;
  const float t = lh_u01_f32(x) * d;
  const float v = lo + t;
  return v < hi ? v : hi;
}
LH_PHILOX_FN double lh_uniform_f64(const unsigned long long x, const double lo, const double hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = hi - lo;
  const double t = lh_u01_f64(x) * d;
  const double v = lo + t;
  return v < hi ? v : hi;
}
LH_PHILOX_FN int lh_uniform_i32(const unsigned int x, const int lo, const int hi) {
  const unsigned long long span = (unsigned long long)((long long)hi - (long long)lo) + 1ull;  // 1 .. 2^32
  return (int)((unsigned int)lo + (unsigned int)(((unsigned long long)x * span) >> 32));
}
LH_PHILOX_FN long long lh_uniform_i64(const unsigned long long x, const long long lo, const long long hi) {
  const unsigned long long span = (unsigned long long)hi - (unsigned long long)lo + 1ull;  // mod 2^64; 0: the full range
  if (span == 0) return (long long)x;
  return (long long)((unsigned long long)lo + lh_mulhi64(x, span));
}

// lo, hi, hi - lo finite and lo <= hi (NaN fails every comparison)
LH_PHILOX_FN int lh_uniform_range_ok_f32(const float lo, const float hi) {
  const float big = 3.40282346638528859812e38f, d = hi - lo;
  return lo >= -big && lo <= big && hi >= -big && hi <= big && lo <= hi && d <= big;
}
LH_PHILOX_FN int lh_uniform_range_ok_f64(const double lo, const double hi) {
  const double big = 1.79769313486231570815e308, d = hi - lo;
  return lo >= -big && lo <= big && hi >= -big && hi <= big && lo <= hi && d <= big;
}

#endif  // LASER_HIP_PHILOX_CORE_H
