// laser_amd/csrc/reduce_core.h -- the canonical reduction order of liblaser_hip.so: the one implementation that the
// precompiled reductions (reduce.hip) and the run-time-compiled forEachReduce kernels (foreach.cpp, which embeds this file
// in the source it hands to hiprtc) share.  include/laser_hip.h ("Reductions") states the order in words; the numpy model of
// the tests reads LH_REDUCE_LANES and LH_REDUCE_STEPS from here.
//
// The order is a function of the element count alone:
//   x[0..n) are the elements in the row-major logical order of the iteration shape.  E = 16 / sizeof(widest operand)
//   (4 for f32 / i32, 2 for f64 / i64, 16 for int8), W = LH_REDUCE_LANES, R = LH_REDUCE_STEPS; a chunk is S = R*W*E elements.
//   In chunk c, lane t keeps E accumulators, each starting at `init`; for r = 0..R-1, then j = 0..E-1, it applies the body
//   to element c*S + r*W*E + t*E + j and accumulator j (elements at or past n are skipped).  The E accumulators are folded
//   by halving (accumulator j merges j + h for h = E/2, E/4, .., 1), then the W lane results the same way (lane t merges
//   lane t + h for h = W/2, .., 1).  That is the chunk's partial.  More than one chunk: the array of partials is reduced by
//   the same rule, with E = 16 / sizeof(accumulator) and `merge` as the body, until one value is left.
// Nothing here depends on the device, the grid, the stream, the base alignment or the strides: a traversal only says how
// element i is found (the visitor), never which lane or step takes it.
//
// Plain C++ with no includes: hiprtc compiles it as it stands.  Names start with lh_ (forEach spec names may not).
#ifndef LASER_HIP_REDUCE_CORE_H
#define LASER_HIP_REDUCE_CORE_H

#define LH_REDUCE_LANES 256  // W: lanes of a chunk = threads of a workgroup
#define LH_REDUCE_STEPS 8    // R: vector steps per lane and chunk (profiles/reduce/README.md)

// The partial of chunk `chunk` of n elements (returned on lane 0; every lane of the workgroup must call).
//   V  visitor:  vis.group(i, acc)  applies the body to elements i .. i+E-1 (all < n), element i + j into acc[j], j ascending
//                vis.one(i, a)      applies the body to element i and accumulator a
//   M  merge:    M::merge(acc, other)
// `lds` holds LH_REDUCE_LANES accumulators.
template <typename Acc, int E, class M, class V>
__device__ __forceinline__ Acc lh_reduce_chunk(V &vis, long long chunk, long long n, const Acc init, Acc *lds) {
  constexpr int W = LH_REDUCE_LANES, R = LH_REDUCE_STEPS;
  constexpr long long S = (long long)R * W * E;
  const int t = threadIdx.x;
  Acc acc[E];
#pragma unroll
  for (int j = 0; j < E; j++) acc[j] = init;
  const long long first = chunk * S + (long long)t * E;
  if (chunk * S + S <= n) {  // a full chunk: no bounds checks, every step's loads can be in flight together
#pragma unroll
    for (int r = 0; r < R; r++) vis.group(first + (long long)r * W * E, acc);
  } else {
    for (int r = 0; r < R; r++) {
      const long long i = first + (long long)r * W * E;
      if (i + E <= n) {
        vis.group(i, acc);
      } else {
#pragma unroll
        for (int j = 0; j < E; j++)
          if (i + j < n) vis.one(i + j, acc[j]);
      }
    }
  }
#pragma unroll
  for (int h = E / 2; h >= 1; h /= 2)
#pragma unroll
    for (int j = 0; j < h; j++) M::merge(acc[j], acc[j + h]);
  Acc v = acc[0];
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int h = W / 2; h >= 1; h /= 2) {
    if (t < h) {  // readers take lds[h .. 2h), writers lds[0 .. h): no overlap within a step
      M::merge(v, lds[t + h]);
      lds[t] = v;
    }
    __syncthreads();
  }
  return v;
}

// min / max of reduce_min / reduce_max: any NaN gives NaN, -0 ranks below +0, otherwise the true min / max -- so the result
// does not depend on the order.  (fminf / fmaxf do not order signed zeros and drop NaNs.)
template <typename T>
__device__ __forceinline__ T lh_reduce_min(const T a, const T b) {
  if (a != a) return a;
  if (b != b) return b;
  if (a == b) return __builtin_signbit(a) ? a : b;
  return b < a ? b : a;
}
template <typename T>
__device__ __forceinline__ T lh_reduce_max(const T a, const T b) {
  if (a != a) return a;
  if (b != b) return b;
  if (a == b) return __builtin_signbit(a) ? b : a;
  return b > a ? b : a;
}

#endif  // LASER_HIP_REDUCE_CORE_H
