// laser_amd/csrc/gemm_args.h -- the description of one GEMM / convolution problem that every launcher and launch planner takes.
// No HIP type: host programs built without the HIP headers include it.
#pragma once
#include <stdint.h>

namespace laser_hip {

// One (possibly batched) strided GEMM problem: C <- alpha*A*B + beta*C, element X[r,c] at
// X[r*rs + c*cs] (strides in elements) -- the MatrixView triple of gemm_utils.nim:36-60.
template <typename T>
struct GemmArgs {
  int64_t M, N, K;
  T alpha, beta;
  const T *A;
  int64_t rsA, csA, bsA;
  const T *B;
  int64_t rsB, csB, bsB;
  T *C;
  int64_t rsC, csC, bsC;
  // Readable extents of the operand allocations: rows of A / cols of B / k of both may be read up to
  // these bounds (values beyond M/N/K are zero).  Equal to M, N, K for plain operands; larger for the
  // tile-padded panel images made by the pre-pack API, which lets ragged shapes use the vector loaders.
  int64_t Mext, Next, Kext;
  int32_t tiles_m, tiles_n;  // grid decomposition (filled by the launcher)
  int32_t kc;                // accumulation slice in k (Laser's kc; 0 = one chain over all K)
  int32_t batch;
  int32_t dbg;  // ablation switches for the tuning probe build only (0 in production)
  // Implicit-GEMM convolution (B loader LOAD_IM2COL): B is never materialised; element (k, j) of
  // image b's [C*kH*kW, oH*oW] matrix is gathered from the NCHW input at B + b*bsB with the index
  // arithmetic of im2col (benchmarks/convolution/conv2d_im2col.nim:62-87).
  int32_t cH, cW, ckH, ckW, coW, cpH, cpW, csH, csW;
  // Fused epilogue (the reference plans it: README.md:238-242, TODOs gemm.nim:196,
  // gemm_ukernel_generic.nim:78-79): C = act(alpha*AB + beta*C + bias), bias a strided (broadcastable:
  // strides may be 0) M x N view, applied ONCE after the last accumulation slice.  bias == nullptr / act == 0: off.
  const T *bias;
  int64_t rsBias, csBias, bsBias;
  int32_t act;  // laser_hip_activation
  int32_t cRp, cPWs, cCHM;  // LOAD_CONV_PATCH: patch rows per channel, patch row stride (floats), channels per K-tile
  int32_t cdc, cdr, cdq;  // per-K-tile advance of the implicit-GEMM loader's (channel, kernel row, kernel col): BK = cdc*kH*kW + cdr*kW + cdq
  // First column of C this launch computes: the launch covers columns [col0, N).  Lets one problem be cut into a
  // "main" launch of whole rounds of large tiles (N = the cut) and a "tail" launch of small tiles (col0 = the cut);
  // tiles are independent and every configuration is bit-identical, so the result does not depend on the cut.
  int64_t col0;
  // Implicit-GEMM conv, K-slice-parallel form (tail launches of the laser-order conv): batch = cs_imgs images x nsl kc slices,
  // workgroup z = blockIdx.y computes image z % cs_imgs over k in [slice*cs_len, min(K, (slice+1)*cs_len)), slice = z / cs_imgs,
  // as ONE chain into C + z*bsC (a workspace the ordered combine pass folds); cs_len is a multiple of every BK.  0 = off.
  int32_t cs_imgs, cs_len;
  // Completion flags (small-matrix kernel on host-mapped operands only; nullptr = off): workgroup w stores done_seq to
  // done_flags[w] (system scope, after its C stores) so the host-pointer entry point can poll mapped memory instead of
  // paying a stream synchronise.
  uint32_t *done_flags;
  uint32_t done_seq;
  // Fused prologue (README.md:243-244: "fuse operations before the matrix multiplication kernel, during the prepacking"): relu
  // (x > 0 ? x : 0) applied to the elements of A / of B as they are read.  Only run_gemm and the assembly launcher look at these:
  // run_gemm either hands the problem to the `_pre` assembly kernels (the operation happens in the staging registers, on the way
  // into the LDS panel image) or materialises the operand once and clears the flag.
  int32_t preA, preB;
};

}  // namespace laser_hip
