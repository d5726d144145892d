// laser_amd/csrc/optim.hip -- multi-tensor SGD and Adam steps and the global gradient norm (include/laser_hip.h, "Optimizer
// steps").  The arithmetic of an element is optim_core.h's, the launches are optim_plan.h's; this file is the traversal.
//
// Step kernels.  One launch updates up to LH_OPTIM_TENSORS tensors.  Their table -- per tensor the base pointers, the length,
// the running chunk count and one bit "every base is 16-byte aligned" -- is a kernel argument passed by value: nothing is
// copied to the device and nothing outlives the call.  Work is cut into chunks of LH_OPTIM_CHUNK = 4096 elements (256 lanes,
// one 16-byte vector each, four steps); min(2048, chunks) workgroups stride over the chunks of all tensors of the launch.
// A workgroup finds the tensor of a chunk by bisecting the chunk prefix; chunk and prefix are the same for every lane and the
// result goes through readfirstlane, so the table is read with scalar loads from the argument segment.  Per tensor the
// vector instance runs when all its bases are 16-byte aligned (a group that crosses the tensor's end goes element by
// element: the tail of len % 4), otherwise the single-element instance: the same elements meet the same function, so the
// bits agree.  A lane loads every input of a step before it stores.
//
// Gradient norm.  Per group of LH_OPTIM_NORM_TENSORS tensors: norm_partials_kernel, a workgroup per (tensor, chunk of 8192
// elements), is lh_reduce_chunk of reduce_core.h with a visitor that squares (the product rounded, then added); then
// norm_fold_kernel, a workgroup per tensor, reduces the tensor's partials by the same rule (one partial is the sum).  Last,
// norm_final_kernel: one lane adds the sums left to right in list order, takes the square root and the clip factor.
//
// No atomics, no workgroup waits on another, every access is bounded by the tensor's length.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/laser_hip.h"
#include "common.h"
#include "reduce_core.h"

#define LH_OPTIM_FN __host__ __device__ __forceinline__
#include "optim_core.h"
#include "optim_plan.h"

#pragma clang fp contract(off)

static_assert(LH_OPTIM_CHUNK == 256 * 4 * 4, "256 lanes, one 16-byte vector each, four steps");
static_assert(LH_OPTIM_RCHUNK == LH_REDUCE_STEPS * LH_REDUCE_LANES * 4, "a chunk of the order");
static_assert(LH_OPTIM_MAX_LEN / LH_OPTIM_RCHUNK <= LH_OPTIM_RCHUNK, "the chunk partials of a tensor fit one chunk");
static_assert(LH_OPTIM_MAX_LEN == LASER_HIP_OPTIM_MAX_LEN && LH_OPTIM_MAX_COUNT == LASER_HIP_OPTIM_MAX_COUNT, "plan and header agree");
static_assert(LH_OPTIM_TENSORS <= 64, "one alignment bit per tensor in a 64-bit word");

namespace laser_hip {

namespace {

constexpr int kSteps = 4;                       // vector steps of a lane per chunk
constexpr int kStride = 256 * 4;                // elements between two steps of a lane

struct alignas(16) F4 {
  float v[4];
};

// NP base pointers per tensor: w, g, then the state (m; m and v)
template <int NP>
struct StepTab {
  float *p[NP][LH_OPTIM_TENSORS];
  int first[LH_OPTIM_TENSORS + 1];              // chunks before tensor k of this launch; [ntensors] = all
  int len[LH_OPTIM_TENSORS];
  unsigned long long vec;                       // bit k: every base of tensor k is 16-byte aligned
};
static_assert(sizeof(StepTab<4>) + 128 <= 4096, "the table and the scalars fit the 4 KB of kernel arguments");

struct NormTab {
  const float *g[LH_OPTIM_NORM_TENSORS];
  int first[LH_OPTIM_NORM_TENSORS + 1];         // reduction chunks before tensor k of this launch
  int len[LH_OPTIM_NORM_TENSORS];
};
static_assert(sizeof(NormTab) + 64 <= 4096, "the table fits the 4 KB of kernel arguments");

// the rules as the kernel sees them: x[0] = w, x[1] = g, then the state; x[1] is never stored
template <bool HAS_M>
struct SgdOp {
  static constexpr int NP = HAS_M ? 3 : 2;
  lh_sgd_rule r;
  __device__ __forceinline__ bool has_clip() const { return r.has_clip; }
  __device__ __forceinline__ void apply(const float c, float (&x)[NP]) const {
    float m = 0.0f;
    if constexpr (HAS_M) m = x[2];
    lh_sgd_elem(r, c, x[0], x[1], m);
    if constexpr (HAS_M) x[2] = m;
  }
};
struct AdamOp {
  static constexpr int NP = 4;
  lh_adam_rule r;
  __device__ __forceinline__ bool has_clip() const { return r.has_clip; }
  __device__ __forceinline__ void apply(const float c, float (&x)[NP]) const { lh_adam_elem(r, c, x[0], x[1], x[2], x[3]); }
};

// the last k in [0, n) with first[k] <= chunk (first[0] = 0 <= chunk < first[n]): tensor k owns the chunk, and the empty
// tensors before it, which share its prefix, do not
template <class Tab>
__device__ __forceinline__ int find_tensor(const Tab &tab, const int n, const int chunk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab.first[mid] <= chunk)
      lo = mid;
    else
      hi = mid - 1;
  }
  return __builtin_amdgcn_readfirstlane(lo);
}

// elements i .. i + 3 (all below the tensor's length) of operand q
template <bool VEC>
__device__ __forceinline__ void load4(const float *p, const int i, float (&x)[4]) {
  if (VEC) {
    const F4 t = *(const F4 *)(p + i);
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = t.v[j];
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) x[j] = p[i + j];
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(float *p, const int i, const float (&x)[4]) {
  if (VEC) {
    F4 t;
#pragma unroll
    for (int j = 0; j < 4; j++) t.v[j] = x[j];
    *(F4 *)(p + i) = t;
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++) p[i + j] = x[j];
  }
}

// one chunk of one tensor: elements base .. base + 4095, those below len
template <class Op, bool VEC>
__device__ __forceinline__ void step_chunk(const Op &op, const float c, float *const (&p)[Op::NP], const int base, const int len) {
  constexpr int NP = Op::NP;
  const int i0 = base + (int)threadIdx.x * 4;
  if (base + LH_OPTIM_CHUNK <= len) {  // a full chunk: no bounds checks, every load of the chunk in flight before the first store
    float x[kSteps][NP][4];
#pragma unroll
    for (int r = 0; r < kSteps; r++)
#pragma unroll
      for (int a = 0; a < NP; a++) load4<VEC>(p[a], i0 + r * kStride, x[r][a]);
#pragma unroll
    for (int r = 0; r < kSteps; r++) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float e[NP];
#pragma unroll
        for (int a = 0; a < NP; a++) e[a] = x[r][a][j];
        op.apply(c, e);
#pragma unroll
        for (int a = 0; a < NP; a++) x[r][a][j] = e[a];
      }
#pragma unroll
      for (int a = 0; a < NP; a++)
        if (a != 1) store4<VEC>(p[a], i0 + r * kStride, x[r][a]);
    }
    return;
  }
  for (int r = 0; r < kSteps; r++) {
    const int i = i0 + r * kStride;
    if (i + 4 <= len) {
      float x[NP][4];
#pragma unroll
      for (int a = 0; a < NP; a++) load4<VEC>(p[a], i, x[a]);
#pragma unroll
      for (int j = 0; j < 4; j++) {
        float e[NP];
#pragma unroll
        for (int a = 0; a < NP; a++) e[a] = x[a][j];
        op.apply(c, e);
#pragma unroll
        for (int a = 0; a < NP; a++) x[a][j] = e[a];
      }
#pragma unroll
      for (int a = 0; a < NP; a++)
        if (a != 1) store4<VEC>(p[a], i, x[a]);
    } else {
      for (int j = 0; j < 4; j++) {  // the tail of the tensor: len % 4 elements, one lane
        if (i + j >= len) break;
        float e[NP];
#pragma unroll
        for (int a = 0; a < NP; a++) e[a] = p[a][i + j];
        op.apply(c, e);
#pragma unroll
        for (int a = 0; a < NP; a++)
          if (a != 1) p[a][i + j] = e[a];
      }
    }
  }
}

template <class Op>
__global__ void __launch_bounds__(256) step_kernel(const StepTab<Op::NP> tab, const int ntensors, const Op op, const float *d_clip) {
  const float c = op.has_clip() ? *d_clip : 1.0f;
  const int total = tab.first[ntensors];
  for (int chunk = blockIdx.x; chunk < total; chunk += gridDim.x) {
    const int k = find_tensor(tab, ntensors, chunk);
    float *p[Op::NP];
#pragma unroll
    for (int a = 0; a < Op::NP; a++) p[a] = tab.p[a][k];
    const int base = (chunk - tab.first[k]) * LH_OPTIM_CHUNK;  // < 2^26
    const int len = tab.len[k];
    if (tab.vec >> k & 1ull)
      step_chunk<Op, true>(op, c, p, base, len);
    else
      step_chunk<Op, false>(op, c, p, base, len);
  }
}

// ---- the gradient norm ------------------------------------------------------------------------------------------------------
struct SumOp {
  static __device__ __forceinline__ void merge(float &a, const float b) { a = a + b; }
};
// acc += x * x: the product rounded to float32, then the sum
template <bool VEC>
struct SquareVisit {
  const float *p;
  __device__ __forceinline__ void group(const long long i, float (&acc)[4]) {
    float x[4];
    load4<VEC>(p, (int)i, x);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const float q = x[j] * x[j];
      acc[j] = acc[j] + q;
    }
  }
  __device__ __forceinline__ void one(const long long i, float &acc) {
    const float x = p[i];
    const float q = x * x;
    acc = acc + q;
  }
};
struct PlainVisit {
  const float *p;
  __device__ __forceinline__ void group(const long long i, float (&acc)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = acc[j] + p[i + j];
  }
  __device__ __forceinline__ void one(const long long i, float &acc) { acc = acc + p[i]; }
};

// part[chunk] = the partial of reduction chunk `chunk` of the group: chunk c of tensor k's g * g
__global__ void __launch_bounds__(256) norm_partials_kernel(const NormTab tab, const int ntensors, float *part) {
  __shared__ float lds[LH_REDUCE_LANES];
  const int chunk = blockIdx.x;
  const int k = find_tensor(tab, ntensors, chunk);
  const float *g = tab.g[k];
  const long long c = chunk - tab.first[k], n = tab.len[k];
  float x;
  if (((uintptr_t)g & 15) == 0) {
    SquareVisit<true> vis{g};
    x = lh_reduce_chunk<float, 4, SumOp>(vis, c, n, 0.0f, lds);
  } else {
    SquareVisit<false> vis{g};
    x = lh_reduce_chunk<float, 4, SumOp>(vis, c, n, 0.0f, lds);
  }
  if (threadIdx.x == 0) part[chunk] = x;
}

// sums[k] = the sum of tensor k's partials by the same rule (at most 8192: one chunk); one partial is the sum itself
__global__ void __launch_bounds__(256) norm_fold_kernel(const NormTab tab, const float *part, float *sums) {
  __shared__ float lds[LH_REDUCE_LANES];
  const int k = blockIdx.x;
  const int first = tab.first[k], chunks = tab.first[k + 1] - first;
  if (chunks == 1) {
    if (threadIdx.x == 0) sums[k] = part[first];
    return;
  }
  PlainVisit vis{part + first};
  const float x = lh_reduce_chunk<float, 4, SumOp>(vis, 0, chunks, 0.0f, lds);
  if (threadIdx.x == 0) sums[k] = x;
}

// total = ((+0 + s_0) + s_1) + ..., norm = sqrt(total), clip = norm > max_norm ? max_norm / norm : 1: one lane
__global__ void __launch_bounds__(64) norm_final_kernel(const float *sums, const int count, const float max_norm, float *d_norm,
                                                        float *d_clip) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float total = 0.0f;
  int k = 0;
  for (; k + 8 <= count; k += 8) {  // eight loads in flight, added in list order
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = sums[k + j];
#pragma unroll
    for (int j = 0; j < 8; j++) total = total + s[j];
  }
  for (; k < count; k++) total = total + sums[k];
  float norm, clip;
  lh_optim_clip(total, max_norm, norm, clip);
  if (d_norm) *d_norm = norm;
  if (d_clip) *d_clip = clip;
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the launches of a step: groups of LH_OPTIM_TENSORS consecutive tensors; lists[a][k] = base a of tensor k
template <class Op>
hipError_t run_steps(const Op &op, float *const *const (&lists)[Op::NP], const int64_t *lens, const int count, const float *d_clip,
                     hipStream_t s) {
  for (int k0 = 0; k0 < count; k0 += LH_OPTIM_TENSORS) {
    StepTab<Op::NP> tab = {};
    const int nt = count - k0 < LH_OPTIM_TENSORS ? count - k0 : LH_OPTIM_TENSORS;
    int chunks = 0;
    for (int k = 0; k < nt; k++) {
      bool vec = true;
      for (int a = 0; a < Op::NP; a++) {
        tab.p[a][k] = lens[k0 + k] ? lists[a][k0 + k] : nullptr;
        vec = vec && aligned16(tab.p[a][k]);
      }
      tab.first[k] = chunks;
      tab.len[k] = (int)lens[k0 + k];
      if (vec) tab.vec |= 1ull << k;
      chunks += (int)lh_optim_chunks(lens[k0 + k]);  // <= 64 * 2^14
    }
    for (int k = nt; k <= LH_OPTIM_TENSORS; k++) tab.first[k] = chunks;
    if (chunks == 0) continue;
    const int grid = chunks < LH_OPTIM_MAX_WORKGROUPS ? chunks : LH_OPTIM_MAX_WORKGROUPS;
    hipLaunchKernelGGL((step_kernel<Op>), dim3((unsigned)grid), dim3(256), 0, s, tab, nt, op, d_clip);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

float optim_bias_correction(float beta, int64_t step) { return lh_adam_bias_correction(beta, (long long)step); }

hipError_t launch_sgd_step_f32(float *const *w, const float *const *g, float *const *m, const int64_t *lens, int count, float lr, float mu,
                               float wd, int nesterov, float gscale, const float *d_clip, hipStream_t s) {
  const lh_sgd_rule r = lh_sgd_rule_make(lr, mu, wd, nesterov, gscale, m != nullptr, d_clip != nullptr);
  float *const *gl = const_cast<float *const *>(reinterpret_cast<const float *const *>(g));  // (never stored through)
  if (m) {
    float *const *const lists[3] = {w, gl, m};
    return run_steps(SgdOp<true>{r}, lists, lens, count, d_clip, s);
  }
  float *const *const lists[2] = {w, gl};
  return run_steps(SgdOp<false>{r}, lists, lens, count, d_clip, s);
}

hipError_t launch_adam_step_f32(float *const *w, const float *const *g, float *const *m, float *const *v, const int64_t *lens, int count,
                                float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2, float gscale,
                                const float *d_clip, hipStream_t s) {
  const lh_adam_rule r = lh_adam_rule_make(lr, b1, b2, eps, wd, decoupled, bc1, bc2, gscale, d_clip != nullptr);
  float *const *gl = const_cast<float *const *>(reinterpret_cast<const float *const *>(g));
  float *const *const lists[4] = {w, gl, m, v};
  return run_steps(AdamOp{r}, lists, lens, count, d_clip, s);
}

hipError_t launch_grad_norm_f32(float *d_norm, float *d_clip, const float *const *g, const int64_t *lens, int count, float max_norm,
                                hipStream_t s) {
  long long plan[4];
  if (lh_optim_plan(LH_OPTIM_GRAD_NORM, lens, count, plan) != 0) return hipErrorInvalidValue;
  char *buf = nullptr;
  if (count > 0) {
    const hipError_t e = scratch_alloc_async((void **)&buf, (size_t)plan[3], s);
    if (e != hipSuccess) return e;
  }
  float *part = (float *)buf;                                                        // plan[2] chunk partials
  float *sums = (float *)(buf + ((size_t)plan[2] * 4 + 15) / 16 * 16);                // one sum per tensor
  hipError_t e = hipSuccess;
  long long done = 0;
  for (int k0 = 0; k0 < count && e == hipSuccess; k0 += LH_OPTIM_NORM_TENSORS) {
    NormTab tab = {};
    const int nt = count - k0 < LH_OPTIM_NORM_TENSORS ? count - k0 : LH_OPTIM_NORM_TENSORS;
    int chunks = 0;
    for (int k = 0; k < nt; k++) {
      tab.g[k] = lens[k0 + k] ? g[k0 + k] : nullptr;
      tab.first[k] = chunks;
      tab.len[k] = (int)lens[k0 + k];
      chunks += (int)lh_optim_rchunks(lens[k0 + k]);  // <= 192 * 2^13
    }
    for (int k = nt; k <= LH_OPTIM_NORM_TENSORS; k++) tab.first[k] = chunks;
    hipLaunchKernelGGL(norm_partials_kernel, dim3((unsigned)chunks), dim3(256), 0, s, tab, nt, part + done);
    e = hipGetLastError();
    if (e != hipSuccess) break;
    hipLaunchKernelGGL(norm_fold_kernel, dim3((unsigned)nt), dim3(256), 0, s, tab, (const float *)(part + done), sums + k0);
    e = hipGetLastError();
    done += chunks;
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(64), 0, s, (const float *)sums, count, max_norm, d_norm, d_clip);
    e = hipGetLastError();
  }
  if (buf) {
    const hipError_t f = scratch_free_async(buf, s);
    if (e == hipSuccess) e = f;
  }
  return e;
}

}  // namespace laser_hip
