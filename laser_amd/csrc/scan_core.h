// laser_amd/csrc/scan_core.h -- the order of the row prefix sum, the sorted search and the inverse-CDF draw, as one definition:
// the kernels (scan.hip) include it, and a host program built with a plain C++ compiler can include it too.
// include/laser_hip.h ("Row cumsum, searchsorted and the inverse-CDF sampler") states it in words with the proofs;
// tests/scan_model.py is the numpy model and reads LH_SCAN_RUN from here.
//
// Scan.  An inclusive prefix sum of a row x[0..n), R = LH_SCAN_RUN.  The row is cut into runs, run r = [r R, min(n, (r + 1) R)).
//     loc(i) = x[i] at the first element of a run, else fl(loc(i - 1) + x[i])          a serial sum inside the run
//     run 0:      out[i] = loc(i)
//     run r >= 1: out[i] = fl(carry_r + loc(i)),  carry_r = out[r R - 1]                one addition per element
// so carry_1 = loc(R - 1) and carry_{r+1} = fl(carry_r + loc((r + 1) R - 1)): a chain of ceil(n / R) - 1 dependent additions.
// Every addition is rounded on its own in the element type; no denormal is flushed, nothing is reassociated.  The integer
// types wrap mod 2^32 / 2^64 (the kernels add in the unsigned type), where every order gives the serial result.
//
// Search.  lh_search(a, n, v, right): lo = 0, count = n; while count > 0: step = count / 2, pos = lo + step; go right
// (lo = pos + 1, count -= step + 1) iff a[pos] < v (left side) or a[pos] <= v (right side), else count = step.  The result is
// lo in [0, n] on any input; a comparison with NaN is false, so NaN goes left.  At most 25 steps for n <= 2^24.
//
// Draw.  lh_cdf_draw(cdf, n, u01): total = cdf[n - 1]; not finite or not > 0: -1.  u = u01 * total (one multiply); idx = the
// right-side search of u; idx == n (u rounded up to total): the left-side search of total.
//
// Plain C++ with no includes.  A host build needs -ffp-contract=off (only additions and one multiply: nothing to contract, but
// the pragma below covers clang all the same).  Names start with lh_.
#ifndef LASER_HIP_SCAN_CORE_H
#define LASER_HIP_SCAN_CORE_H

#ifndef LH_SCAN_RUN  // a diagnostic build may pass another run (the sweep of profiles/scan); the tests hold for this one
#define LH_SCAN_RUN 32
#endif

#if defined(__HIP__)
#define LH_SCAN_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define LH_SCAN_FN static inline
#endif

// loc of one run held in x[0..R): x[j] becomes loc of the run's element j
template <class T, int R>
LH_SCAN_FN void lh_scan_local(T x[R]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#pragma unroll
#endif
  for (int j = 1; j < R; j++) x[j] = x[j - 1] + x[j];
}

// out of a run r >= 1 from its loc and its carry
template <class T, int R>
LH_SCAN_FN void lh_scan_add_carry(T x[R], const T carry) {
#if defined(__clang__)
#pragma clang fp contract(off)
#pragma unroll
#endif
  for (int j = 0; j < R; j++) x[j] = carry + x[j];
}

// the whole order on one row, one element after the other (the definition; dst == src is allowed)
template <class T>
LH_SCAN_FN void lh_scan_row(T *dst, const T *src, const long long n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  T carry = T(0), loc = T(0);
  for (long long i = 0; i < n; i++) {
    loc = i % LH_SCAN_RUN == 0 ? src[i] : loc + src[i];
    const T out = i < LH_SCAN_RUN ? loc : carry + loc;
    dst[i] = out;
    if (i % LH_SCAN_RUN == LH_SCAN_RUN - 1) carry = out;
  }
}

template <class T>
LH_SCAN_FN int lh_search(const T *a, const int n, const T v, const bool right) {
  int lo = 0, count = n;
  while (count > 0) {
    const int step = count / 2, pos = lo + step;
    const T x = a[pos];
    if (right ? x <= v : x < v) {
      lo = pos + 1;
      count -= step + 1;
    } else {
      count = step;
    }
  }
  return lo;
}

LH_SCAN_FN int lh_cdf_draw(const float *cdf, const int n, const float u01) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float total = cdf[n - 1];
  if (!(total > 0.0f) || total == __builtin_inff()) return -1;
  const float u = u01 * total;
  int idx = lh_search<float>(cdf, n, u, true);
  if (idx == n) idx = lh_search<float>(cdf, n, total, false);
  return idx;
}

#endif  // LASER_HIP_SCAN_CORE_H
