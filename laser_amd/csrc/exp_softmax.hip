// laser_amd/csrc/exp_softmax.hip -- lexp over strided device views (include/laser_hip.h, "exp and row softmax"): the device form
// of laser/primitives/simd_math/exp_log_*.nim.  The row softmax its README promises on top of it is the kSm ending of the row
// kernels in log_softmax.hip; the softmax along a strided axis is softmax_axis.hip's.
//
// lexp is exp_core.h's.  ExpOp is the elementwise rule as an Op of pointwise.h, which holds the kernels, the grid and the
// vector choice.  Its per-workgroup setup copies the 4 KiB table into LDS (256 lanes x one 16-byte vector) and the elements
// gather from there: a wave's 64 table indices are scattered, which LDS serves at a word per bank and cycle while the vector
// L1 would serialise cache lines.  Workgroups are capped and stride over their work, so the table fill is paid once per
// workgroup.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/laser_hip.h"
#include "common.h"
#include "pointwise.h"

namespace laser_hip {

// option "last_softmax_kernel": written by launch_softmax_rows_f32 (log_softmax.hip) and launch_softmax_axis_f32 (softmax_axis.hip)
std::atomic<int> g_last_softmax_kernel{-1};

namespace {

struct ExpOp : PointwiseOp<1, 1> {
  const unsigned int *lut;
  __device__ __forceinline__ void setup() {
    __shared__ U4 lut4[LH_EXP_LUT_SIZE / 4];
    lut = (const unsigned int *)lut4;
    lut_to_lds((unsigned int *)lut4);
  }
  __device__ __forceinline__ void apply(const float (&x)[1], float (&y)[1]) const { y[0] = lh_exp_with(x[0], lut); }
};

}  // namespace

hipError_t launch_exp_f32(float *dst, const int64_t *dstrides, const float *src, const int64_t *sstrides, const int64_t *shape,
                          int rank, hipStream_t s) {
  return launch_pointwise<ExpOp>({dst}, {dstrides}, {src}, {sstrides}, shape, rank, s);
}

}  // namespace laser_hip
