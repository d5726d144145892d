// laser_amd/csrc/optim_plan.h -- what laser_hip_sgd_step_f32_dev, laser_hip_adam_step_f32_dev and laser_hip_grad_norm_f32_dev
// launch for a list of tensor lengths (include/laser_hip.h "Optimizer steps"; the kernels are in optim.hip).  Plain C++ with
// no includes and no HIP: the library's launchers and a host program read the same function.
//
//   what 0 (SGD) and 1 (Adam): the list is cut into groups of LH_OPTIM_TENSORS consecutive tensors, one launch per group (a
//     group whose tensors are all empty launches nothing).  A tensor of len elements is ceil(len / LH_OPTIM_CHUNK) chunks; a
//     launch has min(LH_OPTIM_MAX_WORKGROUPS, chunks of its group) workgroups, which stride over the group's chunks.  No
//     scratch.
//   what 2 (the gradient norm): groups of LH_OPTIM_NORM_TENSORS tensors.  Per group one launch with a workgroup per
//     (tensor, reduction chunk of LH_OPTIM_RCHUNK elements) -- an empty tensor is one empty chunk, as in "Reductions" -- and
//     one launch with a workgroup per tensor that folds its partials; then one launch of one workgroup for the list sum, the
//     square root and the clip factor: 2 * groups + 1 launches, three up to LH_OPTIM_NORM_TENSORS tensors, one for an empty
//     list.  Scratch: the chunk partials of every tensor, then one sum per tensor, each array rounded up to 16 bytes.
#ifndef LASER_HIP_OPTIM_PLAN_H
#define LASER_HIP_OPTIM_PLAN_H

#define LH_OPTIM_TENSORS 64            // tensors of one step launch: the table travels in the kernel arguments
#define LH_OPTIM_NORM_TENSORS 192      // tensors of one gradient-norm launch (one pointer per tensor: a longer table fits)
#define LH_OPTIM_CHUNK 4096            // elements of a step chunk: 256 lanes x one 16-byte vector x 4 steps
#define LH_OPTIM_RCHUNK 8192           // one chunk of the reduction order: LH_REDUCE_STEPS x LH_REDUCE_LANES x 4
#define LH_OPTIM_MAX_WORKGROUPS 2048
#define LH_OPTIM_MAX_LEN (1ll << 26)   // LASER_HIP_OPTIM_MAX_LEN: a tensor's chunk partials fit one reduction chunk
#define LH_OPTIM_MAX_COUNT 65536       // LASER_HIP_OPTIM_MAX_COUNT
#define LH_OPTIM_SGD 0
#define LH_OPTIM_ADAM 1
#define LH_OPTIM_GRAD_NORM 2

// 0 when the list is one the entry points take: 0 <= count <= 65536, lens non-NULL for count > 0, 0 <= lens[k] <= 2^26
template <typename I>
static inline int lh_optim_list_ok(const I *lens, const long long count) {
  if (count < 0 || count > LH_OPTIM_MAX_COUNT || (count > 0 && !lens)) return -1;
  for (long long k = 0; k < count; k++)
    if (lens[k] < 0 || lens[k] > LH_OPTIM_MAX_LEN) return -1;
  return 0;
}

static inline long long lh_optim_chunks(const long long len) { return len / LH_OPTIM_CHUNK + (len % LH_OPTIM_CHUNK != 0); }
static inline long long lh_optim_rchunks(const long long len) {
  return len == 0 ? 1 : len / LH_OPTIM_RCHUNK + (len % LH_OPTIM_RCHUNK != 0);
}

// out4 = {launches, workgroups of the first launch (0: none), chunks in all, scratch bytes}.  Returns 0, or -1 with nothing
// written for a list the entry points refuse or an unknown `what`.
template <typename I>
static inline int lh_optim_plan(const int what, const I *lens, const long long count, long long *out4) {
  if (what < LH_OPTIM_SGD || what > LH_OPTIM_GRAD_NORM || lh_optim_list_ok(lens, count) != 0) return -1;
  long long launches = 0, first = 0, total = 0;  // total <= 2^16 * 2^14
  if (what == LH_OPTIM_GRAD_NORM) {
    for (long long k0 = 0; k0 < count; k0 += LH_OPTIM_NORM_TENSORS) {
      long long group = 0;
      for (long long k = k0; k < count && k < k0 + LH_OPTIM_NORM_TENSORS; k++) group += lh_optim_rchunks(lens[k]);
      if (k0 == 0) first = group;
      total += group;
      launches += 2;
    }
    out4[0] = launches + 1;
    out4[1] = count ? first : 1;
    out4[2] = total;
    out4[3] = count ? (total * 4 + 15) / 16 * 16 + (count * 4 + 15) / 16 * 16 : 0;
    return 0;
  }
  for (long long k0 = 0; k0 < count; k0 += LH_OPTIM_TENSORS) {
    long long group = 0;
    for (long long k = k0; k < count && k < k0 + LH_OPTIM_TENSORS; k++) group += lh_optim_chunks(lens[k]);
    if (group == 0) continue;
    if (launches == 0) first = group < LH_OPTIM_MAX_WORKGROUPS ? group : LH_OPTIM_MAX_WORKGROUPS;
    total += group;
    launches++;
  }
  out4[0] = launches;
  out4[1] = first;
  out4[2] = total;
  out4[3] = 0;
  return 0;
}

#endif  // LASER_HIP_OPTIM_PLAN_H
