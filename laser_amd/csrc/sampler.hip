// laser_amd/csrc/sampler.hip -- the F+tree weighted sampler of benchmarks/random_sampling/fenwicktree.nim on device rows
// (include/laser_hip.h "F+tree weighted sampler"): the tree image of a row of n float32 weights is 2 P elements, P the next
// power of two >= n; slot 0 is +0, slot P + i the weight (or +0 padding), slot j = slot[2 j] + slot[2 j + 1] for j < P.  Every
// sum is one float32 addition of exactly those two slots: which elements get paired is the definition, and the kernels below
// only ever add a node's own two children.
//
// Build (sampler_plan.h picks between the two):
//   sampler_build_small_kernel   P <= 512: a workgroup owns 1024 / P whole rows.  Leaves into LDS (+0 past n), level after
//                                level in LDS, then the images leave as contiguous runs of 2 P elements.
//   sampler_build_seg_kernel     a workgroup owns 1024 consecutive leaves of one row, 4 per lane (one 16-byte load where the
//                                weights' base and stride allow).  The lane stores its 4 leaves (16 bytes), the two sums of
//                                adjacent leaves (8 bytes) and their sum (4 bytes, the lanes of a wave 256 contiguous bytes);
//                                then lanes that differ in bit 0, 1, .., 5 are paired -- after the step for bit b the 2^(b+1)
//                                lanes of a group all hold the group's node, and the group's first lane stores it -- and the
//                                four wave nodes meet in LDS for the last two levels.  The segment's own node is slot
//                                P / 1024 + segment.
//   sampler_build_top_kernel     the second launch, ordered by the stream: one workgroup per row forms the levels above the
//                                segment nodes (at most 2^14 - 1 nodes) and writes slot 0.  No workgroup waits on another.
// Draw: one lane per (row, draw), one 8-byte load of the (left, right) pair per level.  Draw-and-remove and update: one lane
// per row does the draws and the walks back up; no other lane touches that row's tree inside the launch.
// The draw kernels take the source of their uniform numbers as a parameter: the caller's buffer, or (the _rng forms) a Philox
// stream, u01[row, j] being the float32 u01 (philox_core.h) of word offset + row * m + j, one Philox block per draw, no buffer
// of uniform numbers written or read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/laser_hip.h"
#include "common.h"
#include "philox_core.h"
#include "sampler_plan.h"

static_assert(LH_SAMPLER_MAX_N == LASER_HIP_SAMPLER_MAX_N, "plan and header agree");
static_assert(LH_SAMPLER_SEG == 1024 && LH_SAMPLER_SMALL_LEAVES == 1024 && LH_SAMPLER_SMALL_P * 2 <= LH_SAMPLER_SEG,
              "the kernels below are written for 256 lanes x 4 leaves");

namespace laser_hip {
namespace {

struct alignas(16) SF4 {
  float v[4];
};
struct alignas(8) SF2 {
  float v[2];
};

struct BuildArgs {
  float *tree;
  const float *w;
  long long ts, ws;  // row strides of the tree and of the weights, in elements
  long long rows, n, P;
  int log2P;
  long long units;  // seg kernel: rows * P / 1024; small kernel: workgroup-sized groups of rows
};

__global__ void __launch_bounds__(256) sampler_build_small_kernel(const BuildArgs a) {
#pragma clang fp contract(off)
  __shared__ float img[2 * LH_SAMPLER_SMALL_LEAVES];
  const int t = threadIdx.x;
  const int lp = a.log2P, P = (int)a.P;
  const int per = LH_SAMPLER_SMALL_LEAVES >> lp;  // rows of this workgroup
  for (long long g = blockIdx.x; g < a.units; g += gridDim.x) {
    const long long row0 = g * per;
    __syncthreads();  // the last readers of img are done
    for (int e = t; e < LH_SAMPLER_SMALL_LEAVES; e += 256) {
      const int r = e >> lp, i = e & (P - 1);
      const long long row = row0 + r;
      img[(r << (lp + 1)) + P + i] = (row < a.rows && i < a.n) ? a.w[row * a.ws + i] : 0.0f;
    }
    for (int ls = lp - 1; ls >= 0; ls--) {  // the level of 2^ls nodes
      __syncthreads();
      const int size = 1 << ls;
      for (int e = t; e < (per << ls); e += 256) {
        const int r = e >> ls, j = size + (e & (size - 1));
        float *im = img + (r << (lp + 1));
        im[j] = im[2 * j] + im[2 * j + 1];
      }
    }
    __syncthreads();
    for (int e = t; e < 2 * LH_SAMPLER_SMALL_LEAVES; e += 256) {
      const int r = e >> (lp + 1), j = e & (2 * P - 1);
      const long long row = row0 + r;
      if (row < a.rows) a.tree[row * a.ts + j] = j == 0 ? 0.0f : img[e];
    }
  }
}

// VW: the weights allow 16-byte loads; VT: the tree allows 16-byte and 8-byte stores
template <bool VW, bool VT>
__global__ void __launch_bounds__(256) sampler_build_seg_kernel(const BuildArgs a) {
#pragma clang fp contract(off)
  __shared__ float wave_node[4];
  const int t = threadIdx.x;
  const long long P = a.P;
  const int segs_log2 = a.log2P - 10;
  for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
    const long long row = unit >> segs_log2, seg = unit & ((1ll << segs_log2) - 1);
    const float *w = a.w + row * a.ws;
    float *tree = a.tree + row * a.ts;
    const long long base = seg * LH_SAMPLER_SEG + t * 4;  // the lane's first leaf
    float q[4];
    if (VW && base + 4 <= a.n) {
      const SF4 f = *(const SF4 *)(w + base);
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] = f.v[j];
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) q[j] = base + j < a.n ? w[base + j] : 0.0f;
    }
    const float s01 = q[0] + q[1], s23 = q[2] + q[3];
    float v = s01 + s23;
    float *leaf = tree + P + base, *half = tree + (P >> 1) + (base >> 1);
    if (VT) {
      SF4 f;
#pragma unroll
      for (int j = 0; j < 4; j++) f.v[j] = q[j];
      *(SF4 *)leaf = f;
      SF2 h;
      h.v[0] = s01;
      h.v[1] = s23;
      *(SF2 *)half = h;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) leaf[j] = q[j];
      half[0] = s01;
      half[1] = s23;
    }
    tree[(P >> 2) + seg * 256 + t] = v;
    // lanes that differ in bit b hold sibling nodes; afterwards every lane of the group holds the parent
#pragma unroll
    for (int b = 0; b < 6; b++) {
      v = v + __shfl_xor(v, 1 << b);
      if ((t & ((2 << b) - 1)) == 0) tree[(P >> (3 + b)) + seg * (128 >> b) + (t >> (b + 1))] = v;
    }
    __syncthreads();  // the last reader of wave_node is done
    if ((t & 63) == 0) wave_node[t >> 6] = v;
    __syncthreads();
    if (t == 0) {
      const float lo = wave_node[0] + wave_node[1], hi = wave_node[2] + wave_node[3];
      tree[(P >> 9) + seg * 2] = lo;
      tree[(P >> 9) + seg * 2 + 1] = hi;
      tree[(P >> 10) + seg] = lo + hi;
    }
  }
}

// T = P / 1024 nodes at slots T .. 2 T - 1 are there; the levels above them, and slot 0
__global__ void __launch_bounds__(256) sampler_build_top_kernel(float *tree, const long long ts, const long long rows, const int T) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
    float *tr = tree + row * ts;
    for (int size = T / 2; size >= 1; size /= 2) {
      for (int i = t; i < size; i += 256) {
        const int j = size + i;
        tr[j] = tr[2 * j] + tr[2 * j + 1];
      }
      __syncthreads();  // the level is visible to the workgroup before the next one reads it
    }
    if (t == 0) tr[0] = 0.0f;
  }
}

// (left, right) of node j; A8: the tree's base and row stride keep the pair on an 8-byte boundary
template <bool A8>
__device__ __forceinline__ void load_pair(const float *tr, const int j, float &l, float &r) {
  if (A8) {
    const SF2 p = *(const SF2 *)(tr + 2 * j);
    l = p.v[0];
    r = p.v[1];
  } else {
    l = tr[2 * j];
    r = tr[2 * j + 1];
  }
}

// the draw of the header: -1 without a finite positive root, else the guarded descent
template <bool A8>
__device__ __forceinline__ int draw(const float *tr, const int P, const float u01) {
#pragma clang fp contract(off)
  const float root = tr[1];
  if (!(root > 0.0f) || root == __builtin_inff()) return -1;
  float u = u01 * root;
  int j = 1;
  while (j < P) {
    float l, r;
    load_pair<A8>(tr, j, l, r);
    if (u >= l && r > 0.0f) {
      u = u - l;
      j = 2 * j + 1;
    } else {
      j = 2 * j;
    }
  }
  return j - P;
}

// slot[P + idx] = w, then every node above it from its two children
template <bool A8>
__device__ __forceinline__ void update(float *tr, const int P, const int idx, const float w) {
#pragma clang fp contract(off)
  tr[P + idx] = w;
  for (int j = (P + idx) >> 1; j >= 1; j >>= 1) {
    float l, r;
    load_pair<A8>(tr, j, l, r);
    tr[j] = l + r;
  }
}

// where the uniform number of draw e = row * m + j comes from: the caller's buffer, or word offset + e of a Philox stream
struct U01Buffer {
  const float *u01;
  __device__ __forceinline__ float operator()(const long long e) const { return u01[e]; }
};
struct U01Philox {
  unsigned long long seed, subseq, offset;
  __device__ __forceinline__ float operator()(const long long e) const {
    return lh_u01_f32(lh_philox_word(seed, subseq, offset + (unsigned long long)e));
  }
};

template <bool A8, class U01>
__global__ void __launch_bounds__(256) sampler_sample_kernel(int *idx, const float *tree, const long long ts, const U01 u01,
                                                             const long long rows, const long long m, const int P) {
  const long long total = rows * m;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256)
    idx[e] = draw<A8>(tree + (e / m) * ts, P, u01(e));
}

template <bool A8, class U01>
__global__ void __launch_bounds__(256) sampler_sample_remove_kernel(int *idx, float *tree, const long long ts, const U01 u01,
                                                                    const long long rows, const long long k, const int P) {
  for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < rows; row += (long long)gridDim.x * 256) {
    float *tr = tree + row * ts;
    for (long long s = 0; s < k; s++) {
      const int i = draw<A8>(tr, P, u01(row * k + s));
      idx[row * k + s] = i;
      if (i >= 0) update<A8>(tr, P, i, 0.0f);
    }
  }
}

template <bool A8>
__global__ void __launch_bounds__(256) sampler_update_kernel(float *tree, const long long ts, const int *elem, const float *weight,
                                                             const long long rows, const int n, const int P) {
  for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < rows; row += (long long)gridDim.x * 256) {
    const int i = elem[row];
    if (i >= 0 && i < n) update<A8>(tree + row * ts, P, i, weight[row]);  // -1 and anything else outside the row: skipped
  }
}

inline bool pair_aligned(const float *tree, int64_t ts, int64_t rows) { return (uintptr_t)tree % 8 == 0 && (rows == 1 || ts % 2 == 0); }
inline unsigned lane_grid(long long lanes) { return (unsigned)std::min<long long>((lanes + 255) / 256, LH_SAMPLER_MAX_WORKGROUPS); }

}  // namespace

hipError_t launch_sampler_build_f32(float *tree, int64_t ts, const float *w, int64_t ws, int64_t rows, int64_t n, hipStream_t s) {
  if (rows == 0) return hipSuccess;
  long long plan[4];
  if (lh_sampler_plan(rows, n, plan) != 0) return hipErrorInvalidValue;
  BuildArgs a;
  a.tree = tree;
  a.w = w;
  a.ts = ts;
  a.ws = ws;
  a.rows = rows;
  a.n = n;
  a.P = lh_sampler_leaves(n, &a.log2P);
  if (plan[0] == 0) {
    const long long per = LH_SAMPLER_SMALL_LEAVES >> a.log2P;
    a.units = (rows + per - 1) / per;
    hipLaunchKernelGGL(sampler_build_small_kernel, dim3((unsigned)plan[2]), dim3(256), 0, s, a);
    return hipGetLastError();
  }
  a.units = rows * (a.P / LH_SAMPLER_SEG);
  // (a row stride that is never applied does not count)
  const bool vw = (uintptr_t)w % 16 == 0 && (rows == 1 || ws % 4 == 0);
  const bool vt = (uintptr_t)tree % 16 == 0 && (rows == 1 || ts % 4 == 0);
  const dim3 grid((unsigned)plan[2]);
  if (vw && vt) hipLaunchKernelGGL((sampler_build_seg_kernel<true, true>), grid, dim3(256), 0, s, a);
  else if (vw) hipLaunchKernelGGL((sampler_build_seg_kernel<true, false>), grid, dim3(256), 0, s, a);
  else if (vt) hipLaunchKernelGGL((sampler_build_seg_kernel<false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((sampler_build_seg_kernel<false, false>), grid, dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sampler_build_top_kernel, dim3((unsigned)plan[3]), dim3(256), 0, s, tree, (long long)ts, (long long)rows,
                     (int)(a.P / LH_SAMPLER_SEG));
  return hipGetLastError();
}

template <class U01>
static hipError_t sample_from(int32_t *idx, const float *tree, int64_t ts, const U01 &u01, int64_t rows, int64_t n, int64_t m, hipStream_t s) {
  if (rows == 0 || m == 0) return hipSuccess;
  const int P = (int)lh_sampler_leaves(n, 0);
  const dim3 grid(lane_grid((long long)rows * m));
  if (pair_aligned(tree, ts, rows))
    hipLaunchKernelGGL((sampler_sample_kernel<true, U01>), grid, dim3(256), 0, s, idx, tree, (long long)ts, u01, (long long)rows, (long long)m, P);
  else
    hipLaunchKernelGGL((sampler_sample_kernel<false, U01>), grid, dim3(256), 0, s, idx, tree, (long long)ts, u01, (long long)rows, (long long)m, P);
  return hipGetLastError();
}

template <class U01>
static hipError_t sample_remove_from(int32_t *idx, float *tree, int64_t ts, const U01 &u01, int64_t rows, int64_t n, int64_t k, hipStream_t s) {
  if (rows == 0 || k == 0) return hipSuccess;
  const int P = (int)lh_sampler_leaves(n, 0);
  const dim3 grid(lane_grid(rows));
  if (pair_aligned(tree, ts, rows))
    hipLaunchKernelGGL((sampler_sample_remove_kernel<true, U01>), grid, dim3(256), 0, s, idx, tree, (long long)ts, u01, (long long)rows, (long long)k, P);
  else
    hipLaunchKernelGGL((sampler_sample_remove_kernel<false, U01>), grid, dim3(256), 0, s, idx, tree, (long long)ts, u01, (long long)rows, (long long)k, P);
  return hipGetLastError();
}

hipError_t launch_sampler_sample_f32(int32_t *idx, const float *tree, int64_t ts, const float *u01, int64_t rows, int64_t n, int64_t m,
                                     hipStream_t s) {
  return sample_from(idx, tree, ts, U01Buffer{u01}, rows, n, m, s);
}

hipError_t launch_sampler_sample_remove_f32(int32_t *idx, float *tree, int64_t ts, const float *u01, int64_t rows, int64_t n, int64_t k,
                                            hipStream_t s) {
  return sample_remove_from(idx, tree, ts, U01Buffer{u01}, rows, n, k, s);
}

hipError_t launch_sampler_sample_rng_f32(int32_t *idx, const float *tree, int64_t ts, uint64_t seed, uint64_t subseq, uint64_t offset,
                                         int64_t rows, int64_t n, int64_t m, hipStream_t s) {
  return sample_from(idx, tree, ts, U01Philox{seed, subseq, offset}, rows, n, m, s);
}

hipError_t launch_sampler_sample_remove_rng_f32(int32_t *idx, float *tree, int64_t ts, uint64_t seed, uint64_t subseq, uint64_t offset,
                                                int64_t rows, int64_t n, int64_t k, hipStream_t s) {
  return sample_remove_from(idx, tree, ts, U01Philox{seed, subseq, offset}, rows, n, k, s);
}

hipError_t launch_sampler_update_f32(float *tree, int64_t ts, const int32_t *elem, const float *weight, int64_t rows, int64_t n,
                                     hipStream_t s) {
  if (rows == 0) return hipSuccess;
  const int P = (int)lh_sampler_leaves(n, 0);
  const dim3 grid(lane_grid(rows));
  if (pair_aligned(tree, ts, rows))
    hipLaunchKernelGGL(sampler_update_kernel<true>, grid, dim3(256), 0, s, tree, (long long)ts, elem, weight, (long long)rows, (int)n, P);
  else
    hipLaunchKernelGGL(sampler_update_kernel<false>, grid, dim3(256), 0, s, tree, (long long)ts, elem, weight, (long long)rows, (int)n, P);
  return hipGetLastError();
}

}  // namespace laser_hip
