// include/laser.hpp -- C++ host-side mirror of Laser's procs for the GEMM hot path, over the C-ABI
// of liblaser_hip.so (include/laser_hip.h).  Same names, argument order and meaning as the Nim
// originals (file:line per function); errors become exceptions where the reference doAsserts.
// Header-only; link with -llaser_hip.  No compute happens on the host.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <vector>
#include <string>
#include <type_traits>
#include <utility>

#include "laser_hip.h"
#include "laser_hip_select.h"

namespace laser {

struct Error : std::runtime_error {
  int code;
  Error(int c, const char *m) : std::runtime_error(std::string("laser_hip error ") + std::to_string(c) + ": " + m), code(c) {}
};
inline void check(int rc) {
  if (rc != 0) throw Error(rc, laser_hip_last_error());
}

// shapes of benchmarks/convolution/conv2d_common.nim:6-13
struct TensorShape { int64_t n, c, h, w; };
struct KernelShape { int64_t c_out, c_in, kH, kW; };
struct Padding { int64_t h, w; };
struct Strides { int64_t h, w; };

#define LASER_DISPATCH(T, CALL_F32, CALL_F64, CALL_I32, CALL_I64)                         \
  if constexpr (std::is_same_v<T, float>) { CALL_F32; }                                   \
  else if constexpr (std::is_same_v<T, double>) { CALL_F64; }                             \
  else if constexpr (std::is_same_v<T, int32_t>) { CALL_I32; }                            \
  else { static_assert(std::is_same_v<T, int64_t>, "float, double, int32_t or int64_t"); CALL_I64; }

// The GEMM entry points take every integer type of 1, 2, 4 or 8 bytes, signed or not (gemm.nim:184-248: every SomeNumber):
// arithmetic mod 2^n, so each is the signed entry point of its width on the same bits.  CALL(SFX, E, S) is expanded with the
// suffix, the element type the pointers are cast to and the scalar type alpha / beta are passed as (int32_t for i8 / i16).
#define LASER_GEMM_DISPATCH(T, CALL)                                                                                    \
  if constexpr (std::is_same_v<T, float>) { CALL(f32, float, float); }                                                 \
  else if constexpr (std::is_same_v<T, double>) { CALL(f64, double, double); }                                         \
  else {                                                                                                                \
    static_assert(std::is_integral_v<T> && !std::is_same_v<T, bool>, "float, double or an integer type");             \
    if constexpr (sizeof(T) == 1) { CALL(i8, int8_t, int32_t); }                                                       \
    else if constexpr (sizeof(T) == 2) { CALL(i16, int16_t, int32_t); }                                                \
    else if constexpr (sizeof(T) == 4) { CALL(i32, int32_t, int32_t); }                                                \
    else { CALL(i64, int64_t, int64_t); }                                                                               \
  }

// gemm.nim:184-193
template <typename T>
void gemm_strided(int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rowStrideA, int64_t colStrideA,
                  const T *B, int64_t rowStrideB, int64_t colStrideB, T beta, T *C, int64_t rowStrideC,
                  int64_t colStrideC) {
#define LASER_CALL(SFX, E, S)                                                                                             \
  check(laser_hip_gemm_strided_##SFX(M, N, K, (S)(E)alpha, (const E *)A, rowStrideA, colStrideA, (const E *)B, rowStrideB, \
                                     colStrideB, (S)(E)beta, (E *)C, rowStrideC, colStrideC))
  LASER_GEMM_DISPATCH(T, LASER_CALL)
#undef LASER_CALL
}

// device-resident flavour (device pointers, hipStream_t as void*)
template <typename T>
void gemm_strided_dev(int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rsA, int64_t csA, const T *B,
                      int64_t rsB, int64_t csB, T beta, T *C, int64_t rsC, int64_t csC, void *stream = nullptr) {
#define LASER_CALL(SFX, E, S)                                                                                     \
  check(laser_hip_gemm_strided_##SFX##_dev(M, N, K, (S)(E)alpha, (const E *)A, rsA, csA, (const E *)B, rsB, csB, (S)(E)beta, \
                                           (E *)C, rsC, csC, stream))
  LASER_GEMM_DISPATCH(T, LASER_CALL)
#undef LASER_CALL
}

// Fused epilogue -- planned by the reference (README.md:238-242; TODO gemm.nim:196), not present in it:
//   C = act(alpha*A*B + beta*C + bias),  bias a strided M x N view (strides may be 0), float/double only.
enum class Activation : int { none = LASER_HIP_ACT_NONE, relu = LASER_HIP_ACT_RELU, tanh = LASER_HIP_ACT_TANH, sigmoid = LASER_HIP_ACT_SIGMOID };
template <typename T>
void gemm_strided_fused(int64_t M, int64_t N, int64_t K, T alpha, const T *A, int64_t rowStrideA, int64_t colStrideA,
                        const T *B, int64_t rowStrideB, int64_t colStrideB, T beta, T *C, int64_t rowStrideC,
                        int64_t colStrideC, const T *bias, int64_t rowStrideBias, int64_t colStrideBias,
                        Activation act = Activation::none) {
  static_assert(std::is_floating_point_v<T>, "the fused epilogue is float / double only");
  if constexpr (std::is_same_v<T, float>)
    check(laser_hip_gemm_strided_ex_f32(M, N, K, alpha, A, rowStrideA, colStrideA, B, rowStrideB, colStrideB, beta, C,
                                        rowStrideC, colStrideC, bias, rowStrideBias, colStrideBias, (int)act));
  else
    check(laser_hip_gemm_strided_ex_f64(M, N, K, alpha, A, rowStrideA, colStrideA, B, rowStrideB, colStrideB, beta, C,
                                        rowStrideC, colStrideC, bias, rowStrideBias, colStrideBias, (int)act));
}

// gemm_prepacked.nim:76-85, :157-167
template <typename T>
int64_t gemm_prepackB_mem_required(int64_t M, int64_t N, int64_t K) {
#define LASER_CALL(SFX, E, S) return laser_hip_gemm_prepackB_mem_required_##SFX(M, N, K)
  LASER_GEMM_DISPATCH(T, LASER_CALL)
#undef LASER_CALL
}
template <typename T>
int64_t gemm_prepackA_mem_required(int64_t M, int64_t N, int64_t K) {
#define LASER_CALL(SFX, E, S) return laser_hip_gemm_prepackA_mem_required_##SFX(M, N, K)
  LASER_GEMM_DISPATCH(T, LASER_CALL)
#undef LASER_CALL
}
// gemm_prepacked.nim:111-135, :193-218 (dst must be 64-byte aligned, like the reference's doAssert)
template <typename T>
void gemm_prepackB(void *dst_packedB, int64_t M, int64_t N, int64_t K, const T *src_B, int64_t rowStrideB, int64_t colStrideB) {
#define LASER_CALL(SFX, E, S) check(laser_hip_gemm_prepackB_##SFX(dst_packedB, M, N, K, (const E *)src_B, rowStrideB, colStrideB))
  LASER_GEMM_DISPATCH(T, LASER_CALL)
#undef LASER_CALL
}
template <typename T>
void gemm_prepackA(void *dst_packedA, int64_t M, int64_t N, int64_t K, const T *src_A, int64_t rowStrideA, int64_t colStrideA) {
#define LASER_CALL(SFX, E, S) check(laser_hip_gemm_prepackA_##SFX(dst_packedA, M, N, K, (const E *)src_A, rowStrideA, colStrideA))
  LASER_GEMM_DISPATCH(T, LASER_CALL)
#undef LASER_CALL
}
// gemm_prepacked.nim:275-292
template <typename T>
void gemm_packed(int64_t M, int64_t N, int64_t K, T alpha, const void *packedA, const void *packedB, T beta, T *C,
                 int64_t rowStrideC, int64_t colStrideC) {
#define LASER_CALL(SFX, E, S) \
  check(laser_hip_gemm_packed_##SFX(M, N, K, (S)(E)alpha, packedA, packedB, (S)(E)beta, (E *)C, rowStrideC, colStrideC))
  LASER_GEMM_DISPATCH(T, LASER_CALL)
#undef LASER_CALL
}
inline void gemm_prepack_release(void *packed) { check(laser_hip_gemm_prepack_release(packed)); }

// swapaxes.nim:16-112
template <typename T>
void transpose2D_copy(T *dst, const T *src, int64_t NR, int64_t NC) {
  static_assert(sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8, "1-, 2-, 4- or 8-byte elements");
  if constexpr (sizeof(T) == 4) check(laser_hip_transpose2d_copy_b32(dst, src, NR, NC));
  else if constexpr (sizeof(T) == 8) check(laser_hip_transpose2d_copy_b64(dst, src, NR, NC));
  else if constexpr (sizeof(T) == 2) check(laser_hip_transpose2d_copy_b16(dst, src, NR, NC));
  else check(laser_hip_transpose2d_copy_b8(dst, src, NR, NC));
}
template <typename T>
void transpose2D_batched(T *dst, const T *src, int64_t N, int64_t NR, int64_t NC) {
  static_assert(sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8, "1-, 2-, 4- or 8-byte elements");
  if constexpr (sizeof(T) == 4) check(laser_hip_transpose2d_batched_b32(dst, src, N, NR, NC));
  else if constexpr (sizeof(T) == 8) check(laser_hip_transpose2d_batched_b64(dst, src, N, NR, NC));
  else if constexpr (sizeof(T) == 2) check(laser_hip_transpose2d_batched_b16(dst, src, N, NR, NC));
  else check(laser_hip_transpose2d_batched_b8(dst, src, N, NR, NC));
}
template <typename T>
void nchw2nhwc(T *dst_nhwc, const T *src_nchw, int64_t N, int64_t C, int64_t H, int64_t W) {
  transpose2D_batched(dst_nhwc, src_nchw, N, C, H * W);
}
template <typename T>
void nhwc2nchw(T *dst_nchw, const T *src_nhwc, int64_t N, int64_t C, int64_t H, int64_t W) {
  transpose2D_batched(dst_nchw, src_nhwc, N, H * W, C);
}

// conv2d_common.nim:15-45, conv2d_im2col.nim:10-166
inline TensorShape conv2d_out_shape(TensorShape i, KernelShape k, Padding p, Strides s) {
  TensorShape o{};
  check(laser_hip_conv2d_out_shape(i.n, i.c, i.h, i.w, k.c_out, k.c_in, k.kH, k.kW, p.h, p.w, s.h, s.w, &o.n, &o.c, &o.h, &o.w));
  return o;
}
inline int64_t im2col_workspace_size(TensorShape i, KernelShape k, Padding p, Strides s) {
  return laser_hip_im2col_workspace_size(i.n, i.c, i.h, i.w, k.c_out, k.c_in, k.kH, k.kW, p.h, p.w, s.h, s.w);
}
// (conv2d_im2col.nim:42-50: generic in T; pure data movement, so dispatched on the element size)
template <typename T>
void im2col(T *pworkspace, TensorShape oshape, const T *pinput, TensorShape ishape, KernelShape kshape, Padding padding,
            Strides strides) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4- or 8-byte elements");
  if constexpr (sizeof(T) == 4)
    check(laser_hip_im2col_f32(reinterpret_cast<float *>(pworkspace), oshape.h, oshape.w, reinterpret_cast<const float *>(pinput),
                               ishape.c, ishape.h, ishape.w, kshape.kH, kshape.kW, padding.h, padding.w, strides.h, strides.w));
  else
    check(laser_hip_im2col_f64(reinterpret_cast<double *>(pworkspace), oshape.h, oshape.w, reinterpret_cast<const double *>(pinput),
                               ishape.c, ishape.h, ishape.w, kshape.kH, kshape.kW, padding.h, padding.w, strides.h, strides.w));
}
inline void conv2d_im2col(float *output, TensorShape oshape, const float *input, TensorShape ishape, const float *kernel,
                          KernelShape kshape, Padding padding, Strides strides, float *pworkspace) {
  if (oshape.c != kshape.c_out) throw Error(LASER_HIP_E_INVALID, "oshape.c != kshape.c_out");  // conv2d_im2col.nim:109
  check(laser_hip_conv2d_im2col_f32(output, input, ishape.n, ishape.c, ishape.h, ishape.w, kernel, kshape.c_out, kshape.c_in,
                                    kshape.kH, kshape.kW, padding.h, padding.w, strides.h, strides.w, pworkspace));
}

// ---- device-resident Tensor[T] -- laser/tensor/datatypes.nim:18-52, initialization.nim:42-202 ------
// Same fields as the reference's Tensor (shape, strides, offset, storage); the storage's raw_buffer is a
// DEVICE address, so gemm_strided_dev / transposes / conv chained on Tensors never cross PCIe.
constexpr int LASER_MAXRANK = 6;  // laser/dynamic_stack_arrays.nim:6

template <typename T>
struct HipStorage {  // CpuStorage's twin (datatypes.nim:24-30); freed by the destructor = the Nim finalizer
  T *raw_buffer = nullptr;
  void *memalloc = nullptr;
  bool memowner = false;
  explicit HipStorage(int64_t size) {  // allocCpuStorage (allocator.nim:17-29): aligned, zero-filled
    check(laser_hip_storage_alloc(&memalloc, size * (int64_t)sizeof(T)));
    raw_buffer = static_cast<T *>(memalloc);
    memowner = true;
  }
  HipStorage(const HipStorage &) = delete;
  HipStorage &operator=(const HipStorage &) = delete;
  ~HipStorage() {
    if (memowner && memalloc) (void)laser_hip_storage_free(memalloc);
  }
};

template <typename T>
struct Tensor {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "float, double, int32_t or int64_t");
  std::vector<int64_t> shape, strides;
  int64_t offset = 0;
  std::shared_ptr<HipStorage<T>> storage;

  int rank() const { return (int)shape.size(); }
  int64_t size() const {
    int64_t n = 1;
    for (int64_t s : shape) n *= s;
    return n;
  }
  bool is_C_contiguous() const {  // datatypes.nim:38-47
    int64_t cur = 1;
    for (int i = rank() - 1; i >= 0; i--) {
      if (shape[i] != 1 && strides[i] != cur) return false;
      cur *= shape[i];
    }
    return true;
  }
  T *unsafe_raw_data() { return storage->raw_buffer + offset; }              // device pointer
  const T *unsafe_raw_data() const { return storage->raw_buffer + offset; }
  Tensor transposed() const {  // view: reversed axes
    Tensor t = *this;
    t.shape.assign(shape.rbegin(), shape.rend());
    t.strides.assign(strides.rbegin(), strides.rend());
    return t;
  }
  std::vector<T> to_host() const;
};

template <typename T>
Tensor<T> newTensor(std::initializer_list<int64_t> shape) {  // initialization.nim:156-166 (zero-initialised)
  if ((int)shape.size() > LASER_MAXRANK) throw Error(LASER_HIP_E_INVALID, "rank > LASER_MAXRANK");
  Tensor<T> t;
  t.shape.assign(shape.begin(), shape.end());
  t.strides.resize(t.shape.size());
  int64_t size = 1;
  for (int i = t.rank() - 1; i >= 0; i--) {
    t.strides[i] = size;
    size *= t.shape[i];
  }
  t.storage = std::make_shared<HipStorage<T>>(size);
  return t;
}
template <typename T>
void copy_strided_dev(Tensor<T> &dst, const Tensor<T> &src) {
  if (dst.shape != src.shape) throw Error(LASER_HIP_E_INVALID, "shapes differ");
  if constexpr (sizeof(T) == 4)
    check(laser_hip_copy_strided_b32_dev(dst.unsafe_raw_data(), dst.strides.data(), src.unsafe_raw_data(), src.strides.data(),
                                         dst.shape.data(), dst.rank(), nullptr));
  else
    check(laser_hip_copy_strided_b64_dev(dst.unsafe_raw_data(), dst.strides.data(), src.unsafe_raw_data(), src.strides.data(),
                                         dst.shape.data(), dst.rank(), nullptr));
}
template <typename T>
void copyFrom(Tensor<T> &dst, const Tensor<T> &src) { copy_strided_dev(dst, src); }  // initialization.nim:77-110
template <typename T>
void deepCopy(Tensor<T> &dst, const Tensor<T> &src) {  // initialization.nim:42-75: fresh row-major storage
  Tensor<T> fresh;
  fresh.shape = src.shape;
  fresh.strides.resize(src.shape.size());
  int64_t size = 1;
  for (int i = fresh.rank() - 1; i >= 0; i--) {
    fresh.strides[i] = size;
    size *= fresh.shape[i];
  }
  fresh.storage = std::make_shared<HipStorage<T>>(size);
  copy_strided_dev(fresh, src);
  dst = fresh;
}
template <typename T>
void copyFromRaw(Tensor<T> &dst, const T *buffer, int64_t len) {  // initialization.nim:112-128
  if (dst.size() != len) throw Error(LASER_HIP_E_INVALID, "Tensor size and buffer length should be the same");
  if (!dst.is_C_contiguous()) throw Error(LASER_HIP_E_INVALID, "copyFromRaw needs a contiguous destination");
  check(laser_hip_storage_upload(dst.unsafe_raw_data(), buffer, len * (int64_t)sizeof(T)));
}
template <typename T>
void setZero(Tensor<T> &t) {  // initialization.nim:130-154
  if (!t.is_C_contiguous()) throw Error(LASER_HIP_E_INVALID, "Input tensor is not contiguous.");
  check(laser_hip_storage_set_zero(t.unsafe_raw_data(), t.size() * (int64_t)sizeof(T), nullptr));
}
template <typename T>
std::vector<T> Tensor<T>::to_host() const {
  Tensor<T> c;
  const Tensor<T> *src = this;
  if (!is_C_contiguous()) {
    deepCopy(c, *this);
    src = &c;
  }
  std::vector<T> out((size_t)size());
  check(laser_hip_storage_download(out.data(), src->unsafe_raw_data(), size() * (int64_t)sizeof(T)));
  return out;
}
// forEach's device twin (laser/strided_iteration/foreach.nim:192-264): dst[idx] = f(a[idx]) / f(a[idx], b[idx]) over strided
// views of one shape (b may broadcast through zero strides set by the caller); op = LASER_HIP_MAP_* of laser_hip.h
template <typename T>
void forEachMap(int op, Tensor<T> &dst, const Tensor<T> &a, T alpha = T(1), T beta = T(0)) {
  if (dst.shape != a.shape) throw Error(LASER_HIP_E_INVALID, "shapes differ");
#define LASER_ARGS op, dst.unsafe_raw_data(), dst.strides.data(), a.unsafe_raw_data(), a.strides.data(), dst.shape.data(), dst.rank(), alpha, beta, nullptr
  LASER_DISPATCH(T, check(laser_hip_map_strided_unary_f32_dev(LASER_ARGS)), check(laser_hip_map_strided_unary_f64_dev(LASER_ARGS)),
                 check(laser_hip_map_strided_unary_i32_dev(LASER_ARGS)), check(laser_hip_map_strided_unary_i64_dev(LASER_ARGS)))
#undef LASER_ARGS
}
template <typename T>
void forEachMap(int op, Tensor<T> &dst, const Tensor<T> &a, const Tensor<T> &b, T alpha = T(1), T beta = T(1)) {
  if (dst.shape != a.shape || dst.shape != b.shape) throw Error(LASER_HIP_E_INVALID, "shapes differ");
#define LASER_ARGS op, dst.unsafe_raw_data(), dst.strides.data(), a.unsafe_raw_data(), a.strides.data(), b.unsafe_raw_data(), b.strides.data(), dst.shape.data(), dst.rank(), alpha, beta, nullptr
  LASER_DISPATCH(T, check(laser_hip_map_strided_binary_f32_dev(LASER_ARGS)), check(laser_hip_map_strided_binary_f64_dev(LASER_ARGS)),
                 check(laser_hip_map_strided_binary_i32_dev(LASER_ARGS)), check(laser_hip_map_strided_binary_i64_dev(LASER_ARGS)))
#undef LASER_ARGS
}
// every tuning / A-B switch by name, and the diagnostics of the last launch (include/laser_hip.h lists them)
inline void set_option(const char *name, int value) { check(laser_hip_set_option(name, value)); }
inline int64_t get_option(const char *name) {
  int64_t v = 0;
  check(laser_hip_get_option(name, &v));
  return v;
}
// the node behind an unchanged host-pointer gemm_strided call (0 = every visible GPU, 1 = off)
inline void set_shard_devices(int ndev) { check(laser_hip_set_shard_devices(ndev)); }

// One gemm_strided over every GPU with the operands resident in HBM and C all-gathered over xGMI
// (laser_hip_gemm_strided_*_sharded_dev): block-cyclic row panels, no K split -- bit-identical to one GPU.
struct ShardPlan {
  int64_t rows_per_panel = 0, padded_M = 0;
  int panels_per_dev = 0;
};
inline ShardPlan shard_plan(int64_t M, int ndev, int panels_per_dev = 4) {
  ShardPlan p;
  check(laser_hip_shard_plan(M, ndev, panels_per_dev, &p.rows_per_panel, &p.panels_per_dev, &p.padded_M));
  return p;
}
template <typename T>
void gemm_strided_sharded_dev(const std::vector<int> &devices, int64_t M, int64_t N, int64_t K, T alpha,
                              const std::vector<const T *> &dA_panels, int64_t rsA, int64_t csA, const std::vector<const T *> &dB,
                              int64_t rsB, int64_t csB, T beta, const std::vector<T *> &dC, int64_t rsC, int panels_per_dev = 4,
                              int gather = LASER_HIP_GATHER_PEER, int flags = 0) {
  if (dA_panels.size() != devices.size() || dB.size() != devices.size() || dC.size() != devices.size())
    throw Error(LASER_HIP_E_INVALID, "gemm_strided_sharded_dev: one pointer per device slot");
#define LASER_ARGS (int)devices.size(), devices.data(), M, N, K, alpha, dA_panels.data(), rsA, csA, dB.data(), rsB, csB, beta, dC.data(), rsC, panels_per_dev, gather, flags
  LASER_DISPATCH(T, check(laser_hip_gemm_strided_f32_sharded_dev(LASER_ARGS)), check(laser_hip_gemm_strided_f64_sharded_dev(LASER_ARGS)),
                 check(laser_hip_gemm_strided_i32_sharded_dev(LASER_ARGS)), check(laser_hip_gemm_strided_i64_sharded_dev(LASER_ARGS)))
#undef LASER_ARGS
}

// C (M x N) = alpha * A (M x K) * B (K x N) + beta * C on 2-D Tensors of any strides, all device-resident
template <typename T>
void gemm(T alpha, const Tensor<T> &A, const Tensor<T> &B, T beta, Tensor<T> &C) {
  if (A.rank() != 2 || B.rank() != 2 || C.rank() != 2 || A.shape[1] != B.shape[0] || C.shape[0] != A.shape[0] ||
      C.shape[1] != B.shape[1])
    throw Error(LASER_HIP_E_INVALID, "gemm: shapes do not agree");
  gemm_strided_dev<T>(A.shape[0], B.shape[1], A.shape[1], alpha, A.unsafe_raw_data(), A.strides[0], A.strides[1],
                      B.unsafe_raw_data(), B.strides[0], B.strides[1], beta, C.unsafe_raw_data(), C.strides[0], C.strides[1]);
}

// ---- forEach with a body (include/laser_hip.h "forEach with a body"): Laser's forEach over device Tensors --------------
//   laser::forEach("x += y * z", {laser::out("x", tx), laser::in("y", ty), laser::in("z", tz)}, {laser::param("alpha", 0.5f)});
// The first operand gives the iteration shape; writable operands (out) have exactly that shape, read-only ones (in)
// broadcast like numpy.  Element types may differ between operands; a parameter keeps the C++ type it is given.
// Asynchronous on `stream`.  The library compiles a spec once per device and process.
template <typename T>
constexpr int dtype_code() {
  static_assert(std::is_arithmetic<T>::value && !std::is_same<T, bool>::value, "an element type of LASER_HIP_DT_*");
  if constexpr (std::is_floating_point<T>::value) return sizeof(T) == 4 ? LASER_HIP_DT_F32 : LASER_HIP_DT_F64;
  else if constexpr (std::is_signed<T>::value)
    return sizeof(T) == 1 ? LASER_HIP_DT_I8 : sizeof(T) == 2 ? LASER_HIP_DT_I16 : sizeof(T) == 4 ? LASER_HIP_DT_I32 : LASER_HIP_DT_I64;
  else return sizeof(T) == 1 ? LASER_HIP_DT_U8 : sizeof(T) == 2 ? LASER_HIP_DT_U16 : sizeof(T) == 4 ? LASER_HIP_DT_U32 : LASER_HIP_DT_U64;
}
struct ForEachOperand {
  std::string name;
  int dtype;
  bool writable;
  void *ptr;
  std::vector<int64_t> shape, strides;
};
struct ForEachParam {
  std::string name;
  int dtype;
  uint64_t slot;  // the value in the low bytes
};
template <typename T>
ForEachOperand out(const char *name, Tensor<T> &t) {
  return {name, dtype_code<T>(), true, t.unsafe_raw_data(), t.shape, t.strides};
}
template <typename T>
ForEachOperand in(const char *name, const Tensor<T> &t) {
  return {name, dtype_code<T>(), false, const_cast<T *>(t.unsafe_raw_data()), t.shape, t.strides};
}
template <typename T>
ForEachParam param(const char *name, T value) {
  ForEachParam p{name, dtype_code<T>(), 0};
  std::memcpy(&p.slot, &value, sizeof(T));
  return p;
}
// the spec arrays and launch arrays of a forEach / forEachReduce call (numpy broadcasting of the read-only operands)
struct ForEachCall {
  std::vector<const char *> names, pnames;
  std::vector<int> dtypes, writable, pdtypes;
  std::vector<void *> ptrs;
  std::vector<uint64_t> slots;
  std::vector<int64_t> strides, shape;
  ForEachCall(const char *what, const std::vector<ForEachOperand> &ops, const std::vector<ForEachParam> &params) {
    if (ops.empty()) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": no operand").c_str());
    shape = ops[0].shape;
    const int r = (int)shape.size();
    for (const ForEachOperand &o : ops) {
      names.push_back(o.name.c_str());
      dtypes.push_back(o.dtype);
      writable.push_back(o.writable);
      ptrs.push_back(o.ptr);
      const int pad = r - (int)o.shape.size();
      if (pad < 0 || (o.writable && o.shape != shape))
        throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": operand " + o.name + " does not fit the iteration shape").c_str());
      for (int d = 0; d < r; d++) {  // numpy broadcasting: missing / extent-1 dimensions get stride 0
        const int64_t e = d < pad ? 1 : o.shape[d - pad];
        if (e != shape[d] && e != 1)
          throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": operand " + o.name + " does not broadcast").c_str());
        strides.push_back(d < pad || (e == 1 && !o.writable) ? 0 : o.strides[d - pad]);
      }
    }
    for (const ForEachParam &p : params) {
      pnames.push_back(p.name.c_str());
      pdtypes.push_back(p.dtype);
      slots.push_back(p.slot);
    }
  }
};
inline void forEach(const std::string &body, const std::vector<ForEachOperand> &ops, const std::vector<ForEachParam> &params = {},
                    void *stream = nullptr) {
  ForEachCall c("forEach", ops, params);
  int64_t handle = 0;
  check(laser_hip_foreach_kernel(body.c_str(), (int)ops.size(), c.names.data(), c.dtypes.data(), c.writable.data(),
                                 (int)params.size(), c.pnames.data(), c.pdtypes.data(), &handle));
  check(laser_hip_foreach_dev(handle, c.ptrs.data(), c.strides.data(), c.shape.data(), (int)c.shape.size(), c.slots.data(), stream));
}

// ---- reductions (include/laser_hip.h "Reductions"): reductions.nim:48-116 over a device Tensor, in the fixed order ------
//   float s = laser::reduce_sum(t);     (synchronous: the one value comes back to the host)
template <typename T>
T reduce(int op, const Tensor<T> &t, void *stream = nullptr) {
  static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value || std::is_same<T, int32_t>::value ||
                    std::is_same<T, int64_t>::value, "reductions: float, double, int32_t or int64_t");
  void *d = nullptr;
  check(laser_hip_storage_alloc_stream(&d, sizeof(T), stream));
  const int r = (int)t.shape.size();
  int rc;
#define LASER_REDUCE_CALL(SFX, U)                                                                                     \
  rc = op == 0 ? laser_hip_reduce_sum_##SFX##_dev((const U *)t.unsafe_raw_data(), t.strides.data(), t.shape.data(), r, (U *)d, stream) \
     : op == 1 ? laser_hip_reduce_min_##SFX##_dev((const U *)t.unsafe_raw_data(), t.strides.data(), t.shape.data(), r, (U *)d, stream) \
               : laser_hip_reduce_max_##SFX##_dev((const U *)t.unsafe_raw_data(), t.strides.data(), t.shape.data(), r, (U *)d, stream);
  if constexpr (std::is_same<T, float>::value) { LASER_REDUCE_CALL(f32, float) }
  else if constexpr (std::is_same<T, double>::value) { LASER_REDUCE_CALL(f64, double) }
  else if constexpr (std::is_same<T, int32_t>::value) { LASER_REDUCE_CALL(i32, int32_t) }
  else { LASER_REDUCE_CALL(i64, int64_t) }
#undef LASER_REDUCE_CALL
  T v{};
  if (rc == LASER_HIP_OK) rc = laser_hip_storage_download_stream(&v, d, sizeof(T), stream);
  laser_hip_storage_free(d);
  check(rc);
  return v;
}
template <typename T> T reduce_sum(const Tensor<T> &t, void *stream = nullptr) { return reduce<T>(0, t, stream); }
template <typename T> T reduce_min(const Tensor<T> &t, void *stream = nullptr) { return reduce<T>(1, t, stream); }
template <typename T> T reduce_max(const Tensor<T> &t, void *stream = nullptr) { return reduce<T>(2, t, stream); }

// ---- forEachReduce (include/laser_hip.h "forEachReduce"): forEachStaged (foreach_staged.nim:318) over device Tensors ------
//   double dot = laser::forEachReduce<double>("acc += x * y", "acc += other", 0.0, {laser::in("x", tx), laser::in("y", ty)});
// The accumulator type is Acc; `init` must be an identity of `merge`.  Synchronous (returns the value).
template <typename Acc>
Acc forEachReduce(const std::string &body, const std::string &merge, Acc init, const std::vector<ForEachOperand> &ops,
                  const std::vector<ForEachParam> &params = {}, const char *acc_name = "acc", void *stream = nullptr) {
  ForEachCall c("forEachReduce", ops, params);
  int64_t handle = 0;
  check(laser_hip_foreach_reduce_kernel(body.c_str(), (int)ops.size(), c.names.data(), c.dtypes.data(), c.writable.data(),
                                        (int)params.size(), c.pnames.data(), c.pdtypes.data(), acc_name, dtype_code<Acc>(),
                                        merge.c_str(), &handle));
  uint64_t slot = 0;
  std::memcpy(&slot, &init, sizeof(Acc));
  void *d = nullptr;
  check(laser_hip_storage_alloc_stream(&d, sizeof(Acc), stream));
  int rc = laser_hip_foreach_reduce_dev(handle, c.ptrs.data(), c.strides.data(), c.shape.data(), (int)c.shape.size(),
                                        c.slots.data(), &slot, d, stream);
  Acc v{};
  if (rc == LASER_HIP_OK) rc = laser_hip_storage_download_stream(&v, d, sizeof(Acc), stream);
  laser_hip_storage_free(d);
  check(rc);
  return v;
}

// ---- exp and row softmax (include/laser_hip.h "exp and row softmax"): simd_math/exp_log_*.nim over device Tensors ---------
//   laser::exp(y, x);  laser::softmax(y, x);  laser::softmax_axis(y, x, axis);     (asynchronous on `stream`; y may be x)
// exp: Laser's table-driven exp, bit for bit; x broadcasts against y.  softmax: over the rows of a 2-D Tensor whose last
// stride is 1, summed in the fixed order of the reductions.
inline void exp(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) {
  const int r = dst.rank(), pad = r - src.rank();
  if (pad < 0) throw Error(LASER_HIP_E_INVALID, "exp: the source has more dimensions than the destination");
  std::vector<int64_t> ss((size_t)(r > 0 ? r : 1), 0);
  for (int d = pad; d < r; d++) {  // numpy broadcasting: missing / extent-1 dimensions get stride 0
    const int64_t e = src.shape[d - pad];
    if (e != dst.shape[d] && e != 1) throw Error(LASER_HIP_E_INVALID, "exp: the source does not broadcast to the destination");
    ss[d] = e == 1 ? 0 : src.strides[d - pad];
  }
  check(laser_hip_exp_f32_dev(dst.unsafe_raw_data(), dst.strides.data(), src.unsafe_raw_data(), ss.data(), dst.shape.data(), r, stream));
}
inline Tensor<float> exp_result_like(const Tensor<float> &src) {  // fresh row-major storage of src's shape
  Tensor<float> t;
  t.shape = src.shape;
  t.strides.resize(src.shape.size());
  int64_t size = 1;
  for (int i = t.rank() - 1; i >= 0; i--) {
    t.strides[i] = size;
    size *= t.shape[i];
  }
  t.storage = std::make_shared<HipStorage<float>>(size);
  return t;
}
inline Tensor<float> exp(const Tensor<float> &src, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  exp(dst, src, stream);
  return dst;
}
inline void softmax(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) {
  if (src.rank() != 2 || dst.shape != src.shape) throw Error(LASER_HIP_E_INVALID, "softmax: two 2-D tensors of one shape");
  if (src.shape[1] < 1 || (src.shape[1] != 1 && (src.strides[1] != 1 || dst.strides[1] != 1)))
    throw Error(LASER_HIP_E_INVALID, "softmax: the elements of a row must be contiguous");
  const int64_t rows = src.shape[0], n = src.shape[1];
  check(laser_hip_softmax_rows_f32_dev(dst.unsafe_raw_data(), rows > 1 ? dst.strides[0] : n, src.unsafe_raw_data(),
                                       rows > 1 ? src.strides[0] : n, rows, n, stream));
}
inline Tensor<float> softmax(const Tensor<float> &src, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  softmax(dst, src, stream);
  return dst;
}
// softmax along `axis` (negative counts from the end) of a Tensor of rank 1 .. 6: every 1-D slice along the axis exactly as a
// row of softmax above.  In dst and in src the dims before the axis must collapse into one stride and the dims after it into
// one unit-stride run (any row-major Tensor does).  (Not an overload of softmax: a literal 0 stream would turn into an axis.)
namespace detail {
// the (extent, stride) pairs [first, last) as one dimension: false when they do not collapse; extent-1 dims do not count
inline bool collapse(const std::vector<int64_t> &shape, const std::vector<int64_t> &strides, int first, int last, int64_t &count,
                     int64_t &stride) {
  count = 1;
  stride = 0;
  bool any = false;
  int64_t below = 0;  // extent * stride of the dimension before
  for (int d = last - 1; d >= first; d--) {
    if (shape[d] == 1) continue;
    if (any && strides[d] != below) return false;
    if (!any) stride = strides[d];
    any = true;
    below = strides[d] * shape[d];
    count *= shape[d];
  }
  return true;
}
}  // namespace detail
inline void softmax_axis(Tensor<float> &dst, const Tensor<float> &src, int axis, void *stream = nullptr) {
  const int r = src.rank();
  if (r < 1 || r > 6 || dst.shape != src.shape) throw Error(LASER_HIP_E_INVALID, "softmax_axis: two tensors of one shape, rank 1 .. 6");
  if (axis < -r || axis >= r) throw Error(LASER_HIP_E_INVALID, "softmax_axis: axis outside the rank");
  if (axis < 0) axis += r;
  const int64_t n = src.shape[axis];
  int64_t outer, inner, d_os, s_os, d_in, s_in, c2;
  if (!detail::collapse(src.shape, src.strides, 0, axis, outer, s_os) || !detail::collapse(dst.shape, dst.strides, 0, axis, c2, d_os) ||
      !detail::collapse(src.shape, src.strides, axis + 1, r, inner, s_in) || !detail::collapse(dst.shape, dst.strides, axis + 1, r, c2, d_in) ||
      (inner > 1 && (s_in != 1 || d_in != 1)))
    throw Error(LASER_HIP_E_INVALID, "softmax_axis: the dims before the axis must collapse into one stride, the dims after it into one "
                                     "unit-stride run (make the tensor contiguous)");
  if (n < 1) throw Error(LASER_HIP_E_INVALID, "softmax_axis: empty axis");
  if (inner == 0) return;
  const int64_t d_as = n > 1 ? dst.strides[axis] : inner, s_as = n > 1 ? src.strides[axis] : inner;
  check(laser_hip_softmax_axis_f32_dev(dst.unsafe_raw_data(), d_os, d_as, src.unsafe_raw_data(), s_os, s_as, outer, n, inner, stream));
}
inline Tensor<float> softmax_axis(const Tensor<float> &src, int axis, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  softmax_axis(dst, src, axis, stream);
  return dst;
}

// ---- log, logsumexp, log-softmax and cross-entropy (include/laser_hip.h, the section of that name) over device Tensors ------
//   laser::log(y, x);  laser::logsumexp(x);  laser::log_softmax(y, x);  laser::softmax_cross_entropy(logits, labels[, &grad, scale])
// log: llog of log_core.h, faithful and monotone; x broadcasts against y.  The others run over the rows of a 2-D Tensor whose
// last stride is 1, with exactly the maximum and the sum of laser::softmax.  (asynchronous on `stream`)
inline void log(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) {
  const int r = dst.rank(), pad = r - src.rank();
  if (pad < 0) throw Error(LASER_HIP_E_INVALID, "log: the source has more dimensions than the destination");
  std::vector<int64_t> ss((size_t)(r > 0 ? r : 1), 0);
  for (int d = pad; d < r; d++) {  // numpy broadcasting: missing / extent-1 dimensions get stride 0
    const int64_t e = src.shape[d - pad];
    if (e != dst.shape[d] && e != 1) throw Error(LASER_HIP_E_INVALID, "log: the source does not broadcast to the destination");
    ss[d] = e == 1 ? 0 : src.strides[d - pad];
  }
  check(laser_hip_log_f32_dev(dst.unsafe_raw_data(), dst.strides.data(), src.unsafe_raw_data(), ss.data(), dst.shape.data(), r, stream));
}
inline Tensor<float> log(const Tensor<float> &src, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  log(dst, src, stream);
  return dst;
}
namespace detail {
inline void rows_operand(const char *what, const Tensor<float> &t) {
  if (t.rank() != 2 || t.shape[1] < 1 || (t.shape[1] != 1 && t.strides[1] != 1))
    throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": a 2-D tensor with contiguous, non-empty rows is needed").c_str());
}
}  // namespace detail
// one value per row: max + llog(sum); a fresh Tensor (rows)
inline Tensor<float> logsumexp(const Tensor<float> &src, void *stream = nullptr) {
  detail::rows_operand("logsumexp", src);
  const int64_t rows = src.shape[0], n = src.shape[1];
  Tensor<float> dst = newTensor<float>({rows});
  check(laser_hip_logsumexp_rows_f32_dev(dst.unsafe_raw_data(), 1, src.unsafe_raw_data(), rows > 1 ? src.strides[0] : n, rows, n, stream));
  return dst;
}
// y = (x - max) - llog(sum); dst may be src
inline void log_softmax(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) {
  detail::rows_operand("log_softmax", src);
  detail::rows_operand("log_softmax", dst);
  if (dst.shape != src.shape) throw Error(LASER_HIP_E_INVALID, "log_softmax: two 2-D tensors of one shape");
  const int64_t rows = src.shape[0], n = src.shape[1];
  check(laser_hip_log_softmax_rows_f32_dev(dst.unsafe_raw_data(), rows > 1 ? dst.strides[0] : n, src.unsafe_raw_data(),
                                           rows > 1 ? src.strides[0] : n, rows, n, stream));
}
inline Tensor<float> log_softmax(const Tensor<float> &src, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  log_softmax(dst, src, stream);
  return dst;
}
// the per-row loss for int32 labels (one per row, contiguous; -1: ignore, any other label outside [0, n): NaN); with `grad`
// also *grad = (softmax - onehot) * scale, a fresh row-major Tensor like logits (scale 1: a sum, 1 / rows: a mean)
inline Tensor<float> softmax_cross_entropy(const Tensor<float> &logits, const Tensor<int32_t> &labels, Tensor<float> *grad = nullptr,
                                           float scale = 1.0f, void *stream = nullptr) {
  detail::rows_operand("softmax_cross_entropy", logits);
  const int64_t rows = logits.shape[0], n = logits.shape[1];
  if (labels.rank() != 1 || labels.shape[0] != rows || (rows > 1 && labels.strides[0] != 1))
    throw Error(LASER_HIP_E_INVALID, "softmax_cross_entropy: one contiguous int32 label per row is needed");
  Tensor<float> loss = newTensor<float>({rows});
  if (grad) *grad = exp_result_like(logits);
  check(laser_hip_softmax_xent_rows_f32_dev(loss.unsafe_raw_data(), 1, grad ? grad->unsafe_raw_data() : nullptr, n, logits.unsafe_raw_data(),
                                            rows > 1 ? logits.strides[0] : n, labels.unsafe_raw_data(), rows, n, scale, stream));
  return loss;
}

// ---- activations (include/laser_hip.h "Activations") over device Tensors ----------------------------------------------------
//   laser::tanh(y, x);  laser::sigmoid(y, x);  laser::activation(y, x, Activation::relu);
//   laser::activation_grad(dx, dy, y, Activation::tanh);                           (asynchronous on `stream`)
// tanh and sigmoid are ltanh and lsigmoid of act_core.h (faithful, monotone, tanh odd bit for bit); relu is the fused
// epilogue's rule.  The gradient takes the forward OUTPUT y; its float32 operations are rounded one by one.  x (dy, y)
// broadcast against the destination, which may be one of them.
namespace detail {
inline std::vector<int64_t> bcast_strides(const char *what, const Tensor<float> &dst, const Tensor<float> &src) {
  const int r = dst.rank(), pad = r - src.rank();
  if (pad < 0) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": an operand has more dimensions than the destination").c_str());
  std::vector<int64_t> ss((size_t)(r > 0 ? r : 1), 0);
  for (int d = pad; d < r; d++) {  // numpy broadcasting: missing / extent-1 dimensions get stride 0
    const int64_t e = src.shape[d - pad];
    if (e != dst.shape[d] && e != 1) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": an operand does not broadcast to the destination").c_str());
    ss[d] = e == 1 ? 0 : src.strides[d - pad];
  }
  return ss;
}
}  // namespace detail
inline void activation(Tensor<float> &dst, const Tensor<float> &src, Activation act, void *stream = nullptr) {
  const std::vector<int64_t> ss = detail::bcast_strides("activation", dst, src);
  check(laser_hip_act_f32_dev((int)act, dst.unsafe_raw_data(), dst.strides.data(), src.unsafe_raw_data(), ss.data(), dst.shape.data(),
                              dst.rank(), stream));
}
inline Tensor<float> activation(const Tensor<float> &src, Activation act, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  activation(dst, src, act, stream);
  return dst;
}
inline void tanh(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) { activation(dst, src, Activation::tanh, stream); }
inline Tensor<float> tanh(const Tensor<float> &src, void *stream = nullptr) { return activation(src, Activation::tanh, stream); }
inline void sigmoid(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) { activation(dst, src, Activation::sigmoid, stream); }
inline Tensor<float> sigmoid(const Tensor<float> &src, void *stream = nullptr) { return activation(src, Activation::sigmoid, stream); }
inline void activation_grad(Tensor<float> &dx, const Tensor<float> &dy, const Tensor<float> &y, Activation act, void *stream = nullptr) {
  const std::vector<int64_t> gs = detail::bcast_strides("activation_grad", dx, dy), ys = detail::bcast_strides("activation_grad", dx, y);
  check(laser_hip_act_grad_f32_dev((int)act, dx.unsafe_raw_data(), dx.strides.data(), dy.unsafe_raw_data(), gs.data(), y.unsafe_raw_data(),
                                   ys.data(), dx.shape.data(), dx.rank(), stream));
}
inline Tensor<float> activation_grad(const Tensor<float> &dy, const Tensor<float> &y, Activation act, void *stream = nullptr) {
  Tensor<float> dx = exp_result_like(y);
  activation_grad(dx, dy, y, act, stream);
  return dx;
}

// ---- dense-layer backward (include/laser_hip.h "Dense-layer backward") over device Tensors -----------------------------------
//   laser::bias_grad(db, &dz, dy, &y, Activation::tanh);                           (asynchronous on `stream`)
//   auto g = laser::linear_backward(x, w, dy, &y, Activation::tanh);               g.dx, g.dw, g.db
// dz = dy * f'(y) by activation_grad's rule (dz = dy with Activation::none, y may be null) and db[j] = reduce_sum of dz's column
// j, from one read of dy and y.  2-D (rows, n) Tensors or views with unit column stride; dz null: only db; dz may be dy or y.
namespace detail {
inline int64_t grad_rows(const char *what, const Tensor<float> &t, const Tensor<float> &like) {
  if (t.rank() != 2 || t.shape != like.shape || (t.shape[1] > 1 && t.strides[1] != 1))
    throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": 2-D operands of one shape with unit column stride are needed").c_str());
  return t.shape[0] > 1 ? t.strides[0] : t.shape[1];  // (the stride of a lone row is never applied)
}
}  // namespace detail
inline void bias_grad(Tensor<float> &db, Tensor<float> *dz, const Tensor<float> &dy, const Tensor<float> *y, Activation act,
                      void *stream = nullptr) {
  const int64_t dys = detail::grad_rows("bias_grad", dy, dy), rows = dy.shape[0], n = dy.shape[1];
  const bool has_y = act != Activation::none;
  if (has_y && !y) throw Error(LASER_HIP_E_INVALID, "bias_grad: an activation needs the forward output y");
  if (db.rank() != 1 || db.shape[0] != n) throw Error(LASER_HIP_E_INVALID, "bias_grad: db must be a 1-D tensor of n elements");
  check(laser_hip_bias_grad_f32_dev(db.unsafe_raw_data(), n > 1 ? db.strides[0] : 1, dz ? dz->unsafe_raw_data() : nullptr,
                                    dz ? detail::grad_rows("bias_grad", *dz, dy) : 0, dy.unsafe_raw_data(), dys,
                                    has_y ? y->unsafe_raw_data() : nullptr, has_y ? detail::grad_rows("bias_grad", *y, dy) : 0, rows, n,
                                    (int)act, stream));
}
struct LinearGrads {
  Tensor<float> dx, dw, db;  // dx is empty (no storage) when it was not asked for
};
// the layer Y = act(X W + b), X (M, K), W (K, N): one bias_grad call, then dw = X^T dZ and dx = dZ W^T on the strided GEMM in
// the current float mode, the transposes as strides (no operand is copied)
inline LinearGrads linear_backward(const Tensor<float> &x, const Tensor<float> &w, const Tensor<float> &dy, const Tensor<float> *y,
                                   Activation act, bool need_dx = true, void *stream = nullptr) {
  if (x.rank() != 2 || w.rank() != 2 || dy.rank() != 2 || x.shape[0] != dy.shape[0] || w.shape[1] != dy.shape[1] || x.shape[1] != w.shape[0])
    throw Error(LASER_HIP_E_INVALID, "linear_backward: x (M, K), w (K, N) and dy (M, N) are needed");
  const int64_t M = x.shape[0], K = x.shape[1], N = w.shape[1];
  LinearGrads g;
  g.db = newTensor<float>({N});
  Tensor<float> dz = newTensor<float>({M, N});
  bias_grad(g.db, &dz, dy, y, act, stream);
  g.dw = newTensor<float>({K, N});
  gemm_strided_dev<float>(K, N, M, 1.0f, x.unsafe_raw_data(), x.strides[1], x.strides[0], dz.unsafe_raw_data(), dz.strides[0], dz.strides[1],
                          0.0f, g.dw.unsafe_raw_data(), g.dw.strides[0], g.dw.strides[1], stream);
  if (need_dx) {
    g.dx = newTensor<float>({M, K});
    gemm_strided_dev<float>(M, K, N, 1.0f, dz.unsafe_raw_data(), dz.strides[0], dz.strides[1], w.unsafe_raw_data(), w.strides[1], w.strides[0],
                            0.0f, g.dx.unsafe_raw_data(), g.dx.strides[0], g.dx.strides[1], stream);
  }
  return g;
}

// ---- layer normalization (include/laser_hip.h "Layer normalization") over device Tensors ---------------------------------------
//   auto f = laser::layer_norm(x, &gamma, &beta, 1e-5f);                           f.y, f.mean, f.rstd  (asynchronous on `stream`)
//   auto g = laser::layer_norm_backward(dy, x, f.mean, f.rstd, &gamma);            g.dx, g.dgamma, g.dbeta
// 2-D (rows, n) Tensors or views with unit column stride; gamma, beta, mean and rstd 1-D; gamma and beta may be null.
struct LayerNormResult {
  Tensor<float> y, mean, rstd;  // mean and rstd are empty (no storage) when they were not asked for
};
struct LayerNormGrads {
  Tensor<float> dx, dgamma, dbeta;  // empty (no storage) when not asked for
};
namespace detail {
inline int64_t norm_vec(const char *what, const Tensor<float> &t, int64_t count) {
  if (t.rank() != 1 || t.shape[0] != count) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": a 1-D tensor of the right length is needed").c_str());
  return count > 1 ? t.strides[0] : 1;
}
}  // namespace detail
// y into `y` (which may be x); mean and rstd may be null (inference)
inline void layer_norm(Tensor<float> &y, Tensor<float> *mean, Tensor<float> *rstd, const Tensor<float> &x, const Tensor<float> *gamma,
                       const Tensor<float> *beta, float eps = 1e-5f, void *stream = nullptr) {
  const int64_t xs = detail::grad_rows("layer_norm", x, x), rows = x.shape[0], n = x.shape[1];
  check(laser_hip_layer_norm_f32_dev(y.unsafe_raw_data(), detail::grad_rows("layer_norm", y, x), mean ? mean->unsafe_raw_data() : nullptr,
                                     mean ? detail::norm_vec("layer_norm", *mean, rows) : 1, rstd ? rstd->unsafe_raw_data() : nullptr,
                                     rstd ? detail::norm_vec("layer_norm", *rstd, rows) : 1, x.unsafe_raw_data(), xs,
                                     gamma ? gamma->unsafe_raw_data() : nullptr, gamma ? detail::norm_vec("layer_norm", *gamma, n) : 1,
                                     beta ? beta->unsafe_raw_data() : nullptr, beta ? detail::norm_vec("layer_norm", *beta, n) : 1, rows, n,
                                     eps, stream));
}
inline LayerNormResult layer_norm(const Tensor<float> &x, const Tensor<float> *gamma, const Tensor<float> *beta, float eps = 1e-5f,
                                  bool stats = true, void *stream = nullptr) {
  detail::grad_rows("layer_norm", x, x);
  LayerNormResult f;
  f.y = newTensor<float>({x.shape[0], x.shape[1]});
  if (stats) {
    f.mean = newTensor<float>({x.shape[0]});
    f.rstd = newTensor<float>({x.shape[0]});
  }
  layer_norm(f.y, stats ? &f.mean : nullptr, stats ? &f.rstd : nullptr, x, gamma, beta, eps, stream);
  return f;
}
// dx = ((g - rsum(g) / n) - xhat * (rsum(g * xhat) / n)) * rstd with g = dy * gamma, dbeta = the column sums of dy (bias_grad's
// bits) and dgamma those of dy * xhat; what is not asked for stays empty
inline LayerNormGrads layer_norm_backward(const Tensor<float> &dy, const Tensor<float> &x, const Tensor<float> &mean,
                                          const Tensor<float> &rstd, const Tensor<float> *gamma, bool need_dx = true,
                                          bool need_params = true, void *stream = nullptr) {
  const int64_t dys = detail::grad_rows("layer_norm_backward", dy, dy), rows = dy.shape[0], n = dy.shape[1];
  LayerNormGrads g;
  if (need_dx) g.dx = newTensor<float>({rows, n});
  if (need_params) {
    g.dgamma = newTensor<float>({n});
    g.dbeta = newTensor<float>({n});
  }
  check(laser_hip_layer_norm_grad_f32_dev(need_dx ? g.dx.unsafe_raw_data() : nullptr, n, need_params ? g.dgamma.unsafe_raw_data() : nullptr, 1,
                                          need_params ? g.dbeta.unsafe_raw_data() : nullptr, 1, dy.unsafe_raw_data(), dys,
                                          x.unsafe_raw_data(), detail::grad_rows("layer_norm_backward", x, dy), mean.unsafe_raw_data(),
                                          detail::norm_vec("layer_norm_backward", mean, rows), rstd.unsafe_raw_data(),
                                          detail::norm_vec("layer_norm_backward", rstd, rows), gamma ? gamma->unsafe_raw_data() : nullptr,
                                          gamma ? detail::norm_vec("layer_norm_backward", *gamma, n) : 1, rows, n, stream));
  return g;
}

// ---- the softmax gradient and attention (include/laser_hip.h "Softmax gradient", "Attention") over device Tensors ----------------
//   auto dx = laser::softmax_backward(dy, y);                                      dx = y * (dy - reduce_sum(dy * y)) per row
//   auto f = laser::attention(q, k, v, scale, causal, /*probs*/ false, /*stats*/ false);    f.out (f.probs, f.row_max, f.row_sum)
//   auto g = laser::attention_backward(dout, q, k, v, scale, causal);              g.dq, g.dk, g.dv
// softmax_backward: 2-D (rows, n) Tensors or views with unit column stride; dx may be dy or y.  attention: q (B, H, Tq, d) or
// (BH, Tq, d), k (.., Tk, d), v (.., Tk, dv), Tensors or views of any outer strides with unit feature stride; scale < 0 or NaN
// is taken as given, laser::attention_default_scale(d) is float(1 / sqrt(double(d))).
inline void softmax_backward(Tensor<float> &dx, const Tensor<float> &dy, const Tensor<float> &y, void *stream = nullptr) {
  const int64_t dys = detail::grad_rows("softmax_backward", dy, dy), rows = dy.shape[0], n = dy.shape[1];
  check(laser_hip_softmax_grad_rows_f32_dev(dx.unsafe_raw_data(), detail::grad_rows("softmax_backward", dx, dy), dy.unsafe_raw_data(), dys,
                                            y.unsafe_raw_data(), detail::grad_rows("softmax_backward", y, dy), rows, n, stream));
}
inline Tensor<float> softmax_backward(const Tensor<float> &dy, const Tensor<float> &y, void *stream = nullptr) {
  Tensor<float> dx = exp_result_like(dy);
  softmax_backward(dx, dy, y, stream);
  return dx;
}
struct AttentionResult {
  Tensor<float> out, probs, row_max, row_sum;  // empty (no storage) when not asked for
};
struct AttentionGrads {
  Tensor<float> dq, dk, dv;  // empty (no storage) when not asked for
};
inline float attention_default_scale(int64_t d) { return (float)(1.0 / std::sqrt((double)d)); }
namespace detail {
struct AttnView {
  int64_t b, h, t, w, st[4];  // strides of batch, head, position, feature (1)
};
inline AttnView attn_view(const char *what, const Tensor<float> &x) {
  const int r = x.rank();
  if ((r != 3 && r != 4) || (x.shape[r - 1] > 1 && x.strides[r - 1] != 1))
    throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": 3-D (BH, T, d) or 4-D (B, H, T, d) operands with unit feature stride are needed").c_str());
  AttnView v;
  v.b = x.shape[0], v.h = r == 4 ? x.shape[1] : 1, v.t = x.shape[r - 2], v.w = x.shape[r - 1];
  v.st[0] = x.strides[0], v.st[1] = r == 4 ? x.strides[1] : 0, v.st[2] = x.strides[r - 2], v.st[3] = 1;
  return v;
}
inline Tensor<float> attn_new(const AttnView &like, bool four, int64_t t, int64_t w) {
  return four ? newTensor<float>({like.b, like.h, t, w}) : newTensor<float>({like.b, t, w});
}
// C[b, h] = alpha * A[b, h] B[b, h] on gemm_strided_batched: strides {batch, head, row, column}; one launch per batch unless
// the (batch, head) dims of all three collapse into one batch stride
inline void attn_gemm(int64_t b, int64_t h, int64_t M, int64_t N, int64_t K, float alpha, const float *A, const int64_t *as, const float *B,
                      const int64_t *bs, float *Cm, const int64_t *cs, void *stream) {
  if (b * h == 0 || M == 0 || N == 0) return;
  const bool one = h == 1 || b == 1 || (as[0] == as[1] * h && bs[0] == bs[1] * h && cs[0] == cs[1] * h);
  const int pick = h == 1 ? 0 : 1;
  for (int64_t i = 0; i < (one ? 1 : b); i++)
    check(laser_hip_gemm_strided_batched_f32_dev(one ? b * h : h, M, N, K, alpha, A + i * as[0], as[2], as[3], as[pick], B + i * bs[0], bs[2],
                                                 bs[3], bs[pick], 0.0f, Cm + i * cs[0], cs[2], cs[3], cs[pick], stream));
}
}  // namespace detail
// the fused forward: out (unless need_out is false), P with probs, the row maxima and sums with stats
inline AttentionResult attention(const Tensor<float> &q, const Tensor<float> &k, const Tensor<float> &v, float scale, bool causal = false,
                                 bool probs = false, bool stats = false, bool need_out = true, void *stream = nullptr) {
  const detail::AttnView vq = detail::attn_view("attention", q), vk = detail::attn_view("attention", k), vv = detail::attn_view("attention", v);
  if (q.rank() != k.rank() || q.rank() != v.rank() || vk.b != vq.b || vk.h != vq.h || vv.b != vq.b || vv.h != vq.h || vk.w != vq.w || vv.t != vk.t)
    throw Error(LASER_HIP_E_INVALID, "attention: q (.., Tq, d), k (.., Tk, d) and v (.., Tk, dv) with one leading shape are needed");
  const bool four = q.rank() == 4;
  AttentionResult f;
  int64_t os[3] = {0, 0, 0}, ps[3] = {0, 0, 0};
  if (need_out) {
    f.out = detail::attn_new(vq, four, vq.t, vv.w);
    os[0] = vq.h * vq.t * vv.w, os[1] = four ? vq.t * vv.w : 0, os[2] = vv.w;
  }
  if (probs) {
    f.probs = detail::attn_new(vq, four, vq.t, vk.t);
    ps[0] = vq.h * vq.t * vk.t, ps[1] = four ? vq.t * vk.t : 0, ps[2] = vk.t;
  }
  if (stats) {
    f.row_max = four ? newTensor<float>({vq.b, vq.h, vq.t}) : newTensor<float>({vq.b, vq.t});
    f.row_sum = four ? newTensor<float>({vq.b, vq.h, vq.t}) : newTensor<float>({vq.b, vq.t});
  }
  check(laser_hip_attention_f32_dev(need_out ? f.out.unsafe_raw_data() : nullptr, os, q.unsafe_raw_data(), vq.st, k.unsafe_raw_data(), vk.st,
                                    v.unsafe_raw_data(), vv.st, probs ? f.probs.unsafe_raw_data() : nullptr, ps,
                                    stats ? f.row_max.unsafe_raw_data() : nullptr, stats ? f.row_sum.unsafe_raw_data() : nullptr, vq.b, vq.h,
                                    vq.t, vk.t, vq.w, vv.w, scale, causal ? 1 : 0, stream));
  return f;
}
// the composed backward: P from the forward kernel, dV = P^T dO, dP = dO V^T, dS = softmax_backward(dP, P) in place,
// dQ = scale * (dS K), dK = scale * (dS^T Q); needs B*H*Tq*Tk floats twice
inline AttentionGrads attention_backward(const Tensor<float> &dout, const Tensor<float> &q, const Tensor<float> &k, const Tensor<float> &v,
                                         float scale, bool causal = false, bool need_q = true, bool need_k = true, bool need_v = true,
                                         void *stream = nullptr) {
  if (!need_q && !need_k && !need_v) throw Error(LASER_HIP_E_INVALID, "attention_backward: nothing is asked for");
  AttentionResult f = attention(q, k, v, scale, causal, true, false, false, stream);
  const detail::AttnView vq = detail::attn_view("attention_backward", q), vk = detail::attn_view("attention_backward", k),
                         vv = detail::attn_view("attention_backward", v), vo = detail::attn_view("attention_backward", dout);
  if (dout.rank() != q.rank() || vo.b != vq.b || vo.h != vq.h || vo.t != vq.t || vo.w != vv.w)
    throw Error(LASER_HIP_E_INVALID, "attention_backward: dout must have the shape of the forward output");
  const bool four = q.rank() == 4;
  const int64_t b = vq.b, h = vq.h, tq = vq.t, tk = vk.t, d = vq.w, dv = vv.w;
  const int64_t ps[4] = {h * tq * tk, tq * tk, tk, 1}, pt[4] = {h * tq * tk, tq * tk, 1, tk};
  const int64_t vt[4] = {vv.st[0], vv.st[1], 1, vv.st[2]};
  AttentionGrads g;
  if (need_v) {
    g.dv = detail::attn_new(vq, four, tk, dv);
    const int64_t cs[4] = {h * tk * dv, tk * dv, dv, 1};
    detail::attn_gemm(b, h, tk, dv, tq, 1.0f, f.probs.unsafe_raw_data(), pt, dout.unsafe_raw_data(), vo.st, g.dv.unsafe_raw_data(), cs, stream);
  }
  if (need_q || need_k) {
    Tensor<float> ds = detail::attn_new(vq, four, tq, tk);
    detail::attn_gemm(b, h, tq, tk, dv, 1.0f, dout.unsafe_raw_data(), vo.st, v.unsafe_raw_data(), vt, ds.unsafe_raw_data(), ps, stream);
    check(laser_hip_softmax_grad_rows_f32_dev(ds.unsafe_raw_data(), tk, ds.unsafe_raw_data(), tk, f.probs.unsafe_raw_data(), tk, b * h * tq, tk,
                                              stream));
    if (need_q) {
      g.dq = detail::attn_new(vq, four, tq, d);
      const int64_t cs[4] = {h * tq * d, tq * d, d, 1};
      detail::attn_gemm(b, h, tq, d, tk, scale, ds.unsafe_raw_data(), ps, k.unsafe_raw_data(), vk.st, g.dq.unsafe_raw_data(), cs, stream);
    }
    if (need_k) {
      g.dk = detail::attn_new(vq, four, tk, d);
      const int64_t cs[4] = {h * tk * d, tk * d, d, 1};
      detail::attn_gemm(b, h, tk, d, tq, scale, ds.unsafe_raw_data(), pt, q.unsafe_raw_data(), vq.st, g.dk.unsafe_raw_data(), cs, stream);
    }
  }
  return g;
}

// ---- embedding (include/laser_hip.h "Embedding") over device Tensors -----------------------------------------------------------
//   auto y = laser::embedding(w, idx);                                             y[t, :] = w[idx[t], :]  (asynchronous on `stream`)
//   auto g = laser::embedding_group(idx, vocab);                                   g.order, g.starts
//   auto dw = laser::embedding_backward(dy, idx, vocab, &g);                       dw[v, :] = reduce_sum over the tokens of id v
// w and dw are 2-D (vocab, dim), y and dy 2-D (tokens, dim), Tensors or views with unit column stride; idx is 1-D int32 with
// unit stride.  An id of -1 gives a row of +0 and no gradient, any other id outside [0, vocab) a row of NaN and no gradient.
struct EmbeddingGroup {
  Tensor<int32_t> order, starts;  // id v owns order[starts[v] .. starts[v + 1])
};
namespace detail {
inline int64_t embedding_ids(const char *what, const Tensor<int32_t> &idx) {
  if (idx.rank() != 1 || (idx.shape[0] > 1 && idx.strides[0] != 1))
    throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": idx must be a 1-D int32 tensor with unit stride").c_str());
  return idx.shape[0];
}
}  // namespace detail
inline void embedding(Tensor<float> &y, const Tensor<float> &w, const Tensor<int32_t> &idx, void *stream = nullptr) {
  const int64_t ws = detail::grad_rows("embedding", w, w), tokens = detail::embedding_ids("embedding", idx);
  if (y.rank() != 2 || y.shape[0] != tokens || y.shape[1] != w.shape[1]) throw Error(LASER_HIP_E_INVALID, "embedding: y must be (tokens, dim)");
  check(laser_hip_embedding_f32_dev(y.unsafe_raw_data(), detail::grad_rows("embedding", y, y), w.unsafe_raw_data(), ws, idx.unsafe_raw_data(),
                                    tokens, w.shape[0], w.shape[1], stream));
}
inline Tensor<float> embedding(const Tensor<float> &w, const Tensor<int32_t> &idx, void *stream = nullptr) {
  detail::grad_rows("embedding", w, w);
  Tensor<float> y = newTensor<float>({detail::embedding_ids("embedding", idx), w.shape[1]});
  embedding(y, w, idx, stream);
  return y;
}
inline EmbeddingGroup embedding_group(const Tensor<int32_t> &idx, int64_t vocab, void *stream = nullptr) {
  const int64_t tokens = detail::embedding_ids("embedding_group", idx);
  if (vocab < 0 || vocab > LASER_HIP_EMBEDDING_MAX_VOCAB) throw Error(LASER_HIP_E_INVALID, "embedding_group: 0 <= vocab <= 2^30 is needed");
  EmbeddingGroup g;
  g.order = newTensor<int32_t>({tokens});
  g.starts = newTensor<int32_t>({vocab + 1});
  check(laser_hip_embedding_group_i32_dev(g.order.unsafe_raw_data(), g.starts.unsafe_raw_data(), idx.unsafe_raw_data(), tokens, vocab, stream));
  return g;
}
// dw into `dw` (vocab, dim); group null: the call groups by itself
inline void embedding_backward(Tensor<float> &dw, const Tensor<float> &dy, const Tensor<int32_t> &idx, const EmbeddingGroup *group = nullptr,
                               void *stream = nullptr) {
  const int64_t dys = detail::grad_rows("embedding_backward", dy, dy), tokens = detail::embedding_ids("embedding_backward", idx);
  const int64_t dws = detail::grad_rows("embedding_backward", dw, dw), vocab = dw.shape[0];
  if (dy.shape[0] != tokens || dw.shape[1] != dy.shape[1])
    throw Error(LASER_HIP_E_INVALID, "embedding_backward: dy (tokens, dim) and dw (vocab, dim) are needed");
  if (group && (detail::embedding_ids("embedding_backward", group->order) != tokens ||
                detail::embedding_ids("embedding_backward", group->starts) != vocab + 1))
    throw Error(LASER_HIP_E_INVALID, "embedding_backward: the group is not embedding_group's for these ids and this vocab");
  check(laser_hip_embedding_grad_f32_dev(dw.unsafe_raw_data(), dws, dy.unsafe_raw_data(), dys, idx.unsafe_raw_data(),
                                         group ? group->order.unsafe_raw_data() : nullptr, group ? group->starts.unsafe_raw_data() : nullptr,
                                         tokens, vocab, dy.shape[1], stream));
}
inline Tensor<float> embedding_backward(const Tensor<float> &dy, const Tensor<int32_t> &idx, int64_t vocab, const EmbeddingGroup *group = nullptr,
                                        void *stream = nullptr) {
  if (dy.rank() != 2 || vocab < 0) throw Error(LASER_HIP_E_INVALID, "embedding_backward: dy (tokens, dim) and vocab >= 0 are needed");
  Tensor<float> dw = newTensor<float>({vocab, dy.shape[1]});
  embedding_backward(dw, dy, idx, group, stream);
  return dw;
}

// ---- optimizer steps (include/laser_hip.h "Optimizer steps") over lists of device Tensors ------------------------------------------
//   laser::sgd_step({&w1, &b1}, {&dw1, &db1}, &momentum, lr, mu);                 every tensor of the list, one call, in place
//   laser::adam_step(params, grads, m, v, step, lr);                             step counts from 1; m and v start as zeros
//   auto n = laser::grad_norm(grads, 1.0f);  laser::sgd_step(params, grads, nullptr, lr, 0, 0, false, 1, &n.clip);
// Every float32 operation is rounded on its own (laser_amd/csrc/optim_core.h); the clip factor never leaves the device.
// Tensors are float32 and C-contiguous, of any shape; the lists of one call have equal lengths and element counts.
typedef std::vector<Tensor<float> *> TensorList;
struct GradNorm {
  Tensor<float> norm, clip;  // one element each, on the device
};
namespace detail {
// the device pointers of a list (nullptr for an empty tensor); `lens` is filled by the first list and checked by the others
inline std::vector<float *> optim_list(const char *what, const TensorList &list, std::vector<int64_t> &lens, bool first) {
  if (!first && list.size() != lens.size()) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": lists of unequal length").c_str());
  if (first) lens.assign(list.size(), 0);
  std::vector<float *> p(list.size(), nullptr);
  for (size_t k = 0; k < list.size(); k++) {
    if (!list[k] || !list[k]->is_C_contiguous())
      throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": a tensor of a list is null or not C-contiguous").c_str());
    const int64_t n = list[k]->size();
    if (first) lens[k] = n;
    if (n != lens[k]) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": tensors of unequal size at one list position").c_str());
    p[k] = n ? list[k]->unsafe_raw_data() : nullptr;
  }
  return p;
}
}  // namespace detail
inline float adam_bias_correction(float beta, int64_t step) {
  float out = 0.0f;
  check(laser_hip_adam_bias_correction(beta, step, &out));
  return out;
}
inline void sgd_step(const TensorList &params, const TensorList &grads, const TensorList *momentum, float lr, float mu = 0.0f,
                     float wd = 0.0f, bool nesterov = false, float gscale = 1.0f, const Tensor<float> *clip = nullptr,
                     void *stream = nullptr) {
  std::vector<int64_t> lens;
  const std::vector<float *> w = detail::optim_list("sgd_step", params, lens, true), g = detail::optim_list("sgd_step", grads, lens, false);
  std::vector<float *> m;
  if (momentum) m = detail::optim_list("sgd_step", *momentum, lens, false);
  if (clip && clip->size() != 1) throw Error(LASER_HIP_E_INVALID, "sgd_step: clip is one device float");
  check(laser_hip_sgd_step_f32_dev(w.data(), g.data(), momentum ? m.data() : nullptr, lens.data(), (int)lens.size(), lr, mu, wd,
                                   nesterov ? 1 : 0, gscale, clip ? clip->unsafe_raw_data() : nullptr, stream));
}
inline void adam_step(const TensorList &params, const TensorList &grads, const TensorList &m, const TensorList &v, int64_t step, float lr,
                      float b1 = 0.9f, float b2 = 0.999f, float eps = 1e-8f, float wd = 0.0f, bool decoupled = false, float gscale = 1.0f,
                      const Tensor<float> *clip = nullptr, void *stream = nullptr) {
  std::vector<int64_t> lens;
  const std::vector<float *> w = detail::optim_list("adam_step", params, lens, true), g = detail::optim_list("adam_step", grads, lens, false),
                             pm = detail::optim_list("adam_step", m, lens, false), pv = detail::optim_list("adam_step", v, lens, false);
  if (clip && clip->size() != 1) throw Error(LASER_HIP_E_INVALID, "adam_step: clip is one device float");
  check(laser_hip_adam_step_f32_dev(w.data(), g.data(), pm.data(), pv.data(), lens.data(), (int)lens.size(), lr, b1, b2, eps, wd,
                                    decoupled ? 1 : 0, adam_bias_correction(b1, step), adam_bias_correction(b2, step), gscale,
                                    clip ? clip->unsafe_raw_data() : nullptr, stream));
}
inline GradNorm grad_norm(const TensorList &grads, float max_norm, void *stream = nullptr) {
  std::vector<int64_t> lens;
  const std::vector<float *> g = detail::optim_list("grad_norm", grads, lens, true);
  GradNorm r{newTensor<float>({1}), newTensor<float>({1})};
  check(laser_hip_grad_norm_f32_dev(r.norm.unsafe_raw_data(), r.clip.unsafe_raw_data(), g.data(), lens.data(), (int)lens.size(), max_norm,
                                    stream));
  return r;
}

// ---- sine and cosine (include/laser_hip.h "Sine and cosine") over device Tensors -----------------------------------------------
//   laser::sin(y, x);  laser::cos(y, x);  laser::sincos(s, c, x);   y = laser::sin(x);              (asynchronous on `stream`)
// lsin and lcos of sincos_core.h: faithful for every finite float32, lsin odd and lcos even bit for bit, NaN for NaN and +-Inf.
// x broadcasts against the destination, which may be x itself; sincos shares one argument reduction and gives the same bits.
inline void sin(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) {
  const std::vector<int64_t> ss = detail::bcast_strides("sin", dst, src);
  check(laser_hip_sin_f32_dev(dst.unsafe_raw_data(), dst.strides.data(), src.unsafe_raw_data(), ss.data(), dst.shape.data(), dst.rank(), stream));
}
inline Tensor<float> sin(const Tensor<float> &src, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  sin(dst, src, stream);
  return dst;
}
inline void cos(Tensor<float> &dst, const Tensor<float> &src, void *stream = nullptr) {
  const std::vector<int64_t> ss = detail::bcast_strides("cos", dst, src);
  check(laser_hip_cos_f32_dev(dst.unsafe_raw_data(), dst.strides.data(), src.unsafe_raw_data(), ss.data(), dst.shape.data(), dst.rank(), stream));
}
inline Tensor<float> cos(const Tensor<float> &src, void *stream = nullptr) {
  Tensor<float> dst = exp_result_like(src);
  cos(dst, src, stream);
  return dst;
}
inline void sincos(Tensor<float> &s, Tensor<float> &c, const Tensor<float> &src, void *stream = nullptr) {
  if (s.shape != c.shape) throw Error(LASER_HIP_E_INVALID, "sincos: the two destinations differ in shape");
  const std::vector<int64_t> ss = detail::bcast_strides("sincos", s, src);
  check(laser_hip_sincos_f32_dev(s.unsafe_raw_data(), s.strides.data(), c.unsafe_raw_data(), c.strides.data(), src.unsafe_raw_data(),
                                 ss.data(), s.shape.data(), s.rank(), stream));
}
inline std::pair<Tensor<float>, Tensor<float>> sincos(const Tensor<float> &src, void *stream = nullptr) {
  Tensor<float> s = exp_result_like(src), c = exp_result_like(src);
  sincos(s, c, src, stream);
  return {std::move(s), std::move(c)};
}

// ---- Random numbers (include/laser_hip.h "Random numbers"): Philox4x32-10 streams and the reference's randomTensor ----------
//   laser::Rng rng(seed, subseq);               names a stream; (seed, subseq, offset) live on the host, nothing on the device
//   laser::randomTensor<T>({2, 3}, lo, hi, rng) uniform on the closed interval [lo, hi], T = float, double, int32_t, int64_t:
//                                               element k of the row-major order from word rng.offset + k (pair 2 k, 2 k + 1 for
//                                               the 64-bit types); the rng advances by the words used
//   laser::randomTensor<T>({2, 3}, max, rng)    [0, max], the reference's second form
//   laser::randomBits(n, rng)                   n raw words as a Tensor<int32_t> holding the bits
//   rng.randomNormalTensor({2, 3}, mean, std)   float normal draws (Box-Muller on pairs of words, normal_core.h): element k from
//   laser::randomNormalTensor({2, 3}, mean, std, rng)       stream position rng.offset + k; the rng advances by the element count
// A result is a function of (seed, subseq, offset) and the arguments alone.  Asynchronous on `stream`.
struct Rng {
  uint64_t seed = 0, subseq = 0, offset = 0;
  explicit Rng(uint64_t seed_, uint64_t subseq_ = 0, uint64_t offset_ = 0) : seed(seed_), subseq(subseq_), offset(offset_) {}
  uint64_t advance(uint64_t words) {  // the offset before; wraps mod 2^64
    const uint64_t before = offset;
    offset += words;
    return before;
  }
  Tensor<float> randomNormalTensor(std::initializer_list<int64_t> shape, float mean = 0.0f, float std = 1.0f, void *stream = nullptr) {
    Tensor<float> t = newTensor<float>(shape);
    const int64_t n = t.size();
    check(laser_hip_random_normal_f32_dev(t.unsafe_raw_data(), n, mean, std, (int64_t)seed, (int64_t)subseq, (int64_t)offset, stream));
    advance((uint64_t)n);
    return t;
  }
};
inline Tensor<float> randomNormalTensor(std::initializer_list<int64_t> shape, float mean, float std, Rng &rng, void *stream = nullptr) {
  return rng.randomNormalTensor(shape, mean, std, stream);
}
template <typename T>
Tensor<T> randomTensor(std::initializer_list<int64_t> shape, T lo, T hi, Rng &rng, void *stream = nullptr) {
  static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value || std::is_same<T, int32_t>::value ||
                    std::is_same<T, int64_t>::value,
                "randomTensor: float, double, int32_t or int64_t");
  Tensor<T> t = newTensor<T>(shape);
  const int64_t n = t.size(), sd = (int64_t)rng.seed, sq = (int64_t)rng.subseq, off = (int64_t)rng.offset;
  if constexpr (std::is_same<T, float>::value) check(laser_hip_random_uniform_f32_dev(t.unsafe_raw_data(), n, lo, hi, sd, sq, off, stream));
  else if constexpr (std::is_same<T, double>::value) check(laser_hip_random_uniform_f64_dev(t.unsafe_raw_data(), n, lo, hi, sd, sq, off, stream));
  else if constexpr (std::is_same<T, int32_t>::value) check(laser_hip_random_uniform_i32_dev(t.unsafe_raw_data(), n, lo, hi, sd, sq, off, stream));
  else check(laser_hip_random_uniform_i64_dev(t.unsafe_raw_data(), n, lo, hi, sd, sq, off, stream));
  rng.advance((uint64_t)n * (sizeof(T) / 4));
  return t;
}
template <typename T>
Tensor<T> randomTensor(std::initializer_list<int64_t> shape, T max, Rng &rng, void *stream = nullptr) {
  return randomTensor<T>(shape, T(0), max, rng, stream);
}
inline Tensor<int32_t> randomBits(int64_t n, Rng &rng, void *stream = nullptr) {
  Tensor<int32_t> t = newTensor<int32_t>({n});
  check(laser_hip_random_bits_u32_dev(reinterpret_cast<uint32_t *>(t.unsafe_raw_data()), n, (int64_t)rng.seed, (int64_t)rng.subseq,
                                      (int64_t)rng.offset, stream));
  rng.advance((uint64_t)n);
  return t;
}

// ---- F+tree weighted sampler (include/laser_hip.h "F+tree weighted sampler"): fenwicktree.nim's Sampler, one per row --------
//   laser::Sampler s(weights);                  weights: a 2-D Tensor<float> whose rows are contiguous (1-D: one row)
//   s.sample(u);  s.sampleAndRemove(u);         u: a row-major (rows, num) Tensor<float> of numbers in [0, 1), the caller's
//                                               -> Tensor<int32_t> (rows, num)
//   s.sample(rng, num);  s.sampleAndRemove(rng, num);   the uniform numbers made in the kernel from the stream of a laser::Rng
//                                               (below "Random numbers"): u[row, j] from word rng.offset + row * num + j; the
//                                               rng advances by rows * num
//   s.update(elem, weight);                     one (elem, weight) per row, Tensor<int32_t> / Tensor<float> of `rows` elements
// Asynchronous on `stream`.  sampleAndRemove and update mutate `tree`.
struct Sampler {
  Tensor<float> tree;  // (rows, 2 P): the images
  int64_t rows = 0, n = 0;

  explicit Sampler(const Tensor<float> &weights, void *stream = nullptr) {
    const int r = weights.rank();
    if (r != 1 && r != 2) throw Error(LASER_HIP_E_INVALID, "Sampler: a matrix of weights (or a vector for one row) is needed");
    rows = r == 2 ? weights.shape[0] : 1;
    n = weights.shape[r - 1];
    if (n != 1 && weights.strides[r - 1] != 1) throw Error(LASER_HIP_E_INVALID, "Sampler: the elements of a row must be contiguous");
    int64_t elems = 0;
    check(laser_hip_sampler_tree_elems(n, &elems));
    tree = newTensor<float>({rows, elems});
    check(laser_hip_sampler_build_f32_dev(tree.unsafe_raw_data(), elems, weights.unsafe_raw_data(), rows > 1 ? weights.strides[0] : n,
                                          rows, n, stream));
  }
  Tensor<int32_t> sample(const Tensor<float> &u, void *stream = nullptr) const {
    Tensor<int32_t> idx = result_for(u);
    check(laser_hip_sampler_sample_f32_dev(idx.unsafe_raw_data(), tree.unsafe_raw_data(), tree.shape[1], u.unsafe_raw_data(), rows, n,
                                           u.shape[1], stream));
    return idx;
  }
  Tensor<int32_t> sampleAndRemove(const Tensor<float> &u, void *stream = nullptr) {
    Tensor<int32_t> idx = result_for(u);
    check(laser_hip_sampler_sample_remove_f32_dev(idx.unsafe_raw_data(), tree.unsafe_raw_data(), tree.shape[1], u.unsafe_raw_data(),
                                                  rows, n, u.shape[1], stream));
    return idx;
  }
  Tensor<int32_t> sample(Rng &rng, int64_t num = 1, void *stream = nullptr) const {
    if (num < 0) throw Error(LASER_HIP_E_INVALID, "Sampler: a count >= 0 is needed");
    Tensor<int32_t> idx = newTensor<int32_t>({rows, num});
    check(laser_hip_sampler_sample_rng_f32_dev(idx.unsafe_raw_data(), tree.unsafe_raw_data(), tree.shape[1], (int64_t)rng.seed,
                                               (int64_t)rng.subseq, (int64_t)rng.offset, rows, n, num, stream));
    rng.advance((uint64_t)(rows * num));
    return idx;
  }
  Tensor<int32_t> sampleAndRemove(Rng &rng, int64_t num = 1, void *stream = nullptr) {
    if (num < 0) throw Error(LASER_HIP_E_INVALID, "Sampler: a count >= 0 is needed");
    Tensor<int32_t> idx = newTensor<int32_t>({rows, num});
    check(laser_hip_sampler_sample_remove_rng_f32_dev(idx.unsafe_raw_data(), tree.unsafe_raw_data(), tree.shape[1], (int64_t)rng.seed,
                                                      (int64_t)rng.subseq, (int64_t)rng.offset, rows, n, num, stream));
    rng.advance((uint64_t)(rows * num));
    return idx;
  }
  void update(const Tensor<int32_t> &elem, const Tensor<float> &weight, void *stream = nullptr) {
    if (elem.rank() != 1 || weight.rank() != 1 || elem.shape[0] != rows || weight.shape[0] != rows || !elem.is_C_contiguous() ||
        !weight.is_C_contiguous())
      throw Error(LASER_HIP_E_INVALID, "Sampler::update: one contiguous (elem, weight) per row");
    check(laser_hip_sampler_update_f32_dev(tree.unsafe_raw_data(), tree.shape[1], elem.unsafe_raw_data(), weight.unsafe_raw_data(), rows,
                                           n, stream));
  }

 private:
  Tensor<int32_t> result_for(const Tensor<float> &u) const {
    if (u.rank() != 2 || u.shape[0] != rows || !u.is_C_contiguous())
      throw Error(LASER_HIP_E_INVALID, "Sampler: a row-major (rows, num) tensor of uniform numbers is needed");
    return newTensor<int32_t>({rows, u.shape[1]});
  }
};

// ---- Row cumsum, searchsorted and the inverse-CDF sampler (include/laser_hip.h, the section of that name):
// cumsum, searchsorted and sample of bench_multinomial_samplers.nim over device Tensors -------------------------------------
//   laser::cumsum(t)                            inclusive prefix sum along the last axis of a 1-D or 2-D Tensor<T> whose rows
//                                               are contiguous, T = float, double, int32_t, int64_t -> Tensor<T> of t's shape
//   laser::searchsorted(a, v, leftSide)         v: (rows) or a row-major (rows, m) Tensor<T> -> Tensor<int32_t> of v's shape
//   laser::cdfSample(cdf, u)                    u: a row-major (rows, num) Tensor<float> in [0, 1) -> Tensor<int32_t> (rows, num)
//   laser::cdfSampleAndRemove(weights, u)       without replacement, on a private copy of the weights
//   laser::cdfSample(cdf, rng, num);  laser::cdfSampleAndRemove(weights, rng, num)   the uniform numbers from a laser::Rng
// Asynchronous on `stream`.
namespace detail {
template <typename T>
void scan_rows(const Tensor<T> &t, const char *what, int64_t &rows, int64_t &n, int64_t &rs) {
  const int r = t.rank();
  if (r != 1 && r != 2) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": a matrix (or a vector for one row) is needed").c_str());
  rows = r == 2 ? t.shape[0] : 1;
  n = t.shape[r - 1];
  if (n < 1) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": empty rows").c_str());
  if (n != 1 && t.strides[r - 1] != 1) throw Error(LASER_HIP_E_INVALID, (std::string(what) + ": the elements of a row must be contiguous").c_str());
  rs = rows > 1 ? t.strides[0] : n;
}
inline Tensor<int32_t> scan_result_for(const Tensor<float> &u, int64_t rows) {
  if (u.rank() != 2 || u.shape[0] != rows || !u.is_C_contiguous())
    throw Error(LASER_HIP_E_INVALID, "cdfSample: a row-major (rows, num) tensor of uniform numbers is needed");
  return newTensor<int32_t>({rows, u.shape[1]});
}
}  // namespace detail
template <typename T>
Tensor<T> cumsum(const Tensor<T> &t, void *stream = nullptr) {
  int64_t rows, n, rs;
  detail::scan_rows(t, "cumsum", rows, n, rs);
  Tensor<T> out = t.rank() == 1 ? newTensor<T>({n}) : newTensor<T>({rows, n});
  LASER_DISPATCH(T, check(laser_hip_cumsum_f32_dev(out.unsafe_raw_data(), n, t.unsafe_raw_data(), rs, rows, n, stream)),
                 check(laser_hip_cumsum_f64_dev(out.unsafe_raw_data(), n, t.unsafe_raw_data(), rs, rows, n, stream)),
                 check(laser_hip_cumsum_i32_dev(out.unsafe_raw_data(), n, t.unsafe_raw_data(), rs, rows, n, stream)),
                 check(laser_hip_cumsum_i64_dev(out.unsafe_raw_data(), n, t.unsafe_raw_data(), rs, rows, n, stream)))
  return out;
}
template <typename T>
Tensor<int32_t> searchsorted(const Tensor<T> &a, const Tensor<T> &v, bool leftSide = true, void *stream = nullptr) {
  int64_t rows, n, rs;
  detail::scan_rows(a, "searchsorted", rows, n, rs);
  if ((v.rank() != 1 && v.rank() != 2) || v.shape[0] != rows || !v.is_C_contiguous())
    throw Error(LASER_HIP_E_INVALID, "searchsorted: values of shape (rows) or a row-major (rows, m) are needed");
  const int64_t m = v.rank() == 1 ? 1 : v.shape[1];
  const int right = leftSide ? 0 : 1;
  Tensor<int32_t> idx = v.rank() == 1 ? newTensor<int32_t>({rows}) : newTensor<int32_t>({rows, m});
  LASER_DISPATCH(T, check(laser_hip_searchsorted_f32_dev(idx.unsafe_raw_data(), a.unsafe_raw_data(), rs, v.unsafe_raw_data(), rows, n, m, right, stream)),
                 check(laser_hip_searchsorted_f64_dev(idx.unsafe_raw_data(), a.unsafe_raw_data(), rs, v.unsafe_raw_data(), rows, n, m, right, stream)),
                 check(laser_hip_searchsorted_i32_dev(idx.unsafe_raw_data(), a.unsafe_raw_data(), rs, v.unsafe_raw_data(), rows, n, m, right, stream)),
                 check(laser_hip_searchsorted_i64_dev(idx.unsafe_raw_data(), a.unsafe_raw_data(), rs, v.unsafe_raw_data(), rows, n, m, right, stream)))
  return idx;
}
inline Tensor<int32_t> cdfSample(const Tensor<float> &cdf, const Tensor<float> &u, void *stream = nullptr) {
  int64_t rows, n, rs;
  detail::scan_rows(cdf, "cdfSample", rows, n, rs);
  Tensor<int32_t> idx = detail::scan_result_for(u, rows);
  check(laser_hip_cdf_sample_f32_dev(idx.unsafe_raw_data(), cdf.unsafe_raw_data(), rs, u.unsafe_raw_data(), rows, n, u.shape[1], stream));
  return idx;
}
inline Tensor<int32_t> cdfSample(const Tensor<float> &cdf, Rng &rng, int64_t num = 1, void *stream = nullptr) {
  int64_t rows, n, rs;
  detail::scan_rows(cdf, "cdfSample", rows, n, rs);
  if (num < 0) throw Error(LASER_HIP_E_INVALID, "cdfSample: a count >= 0 is needed");
  Tensor<int32_t> idx = newTensor<int32_t>({rows, num});
  check(laser_hip_cdf_sample_rng_f32_dev(idx.unsafe_raw_data(), cdf.unsafe_raw_data(), rs, (int64_t)rng.seed, (int64_t)rng.subseq,
                                         (int64_t)rng.offset, rows, n, num, stream));
  rng.advance((uint64_t)(rows * num));
  return idx;
}
namespace detail {
// a row-major private copy of the weights and a CDF workspace of the same shape
inline void scan_private(const Tensor<float> &weights, int64_t rows, int64_t n, int64_t rs, Tensor<float> &w, Tensor<float> &cdf, void *stream) {
  w = newTensor<float>({rows, n});
  cdf = newTensor<float>({rows, n});
  const int64_t shape[2] = {rows, n}, dstr[2] = {n, 1}, sstr[2] = {rs, 1};
  check(laser_hip_copy_strided_b32_dev(w.unsafe_raw_data(), dstr, weights.unsafe_raw_data(), sstr, shape, 2, stream));
}
}  // namespace detail
inline Tensor<int32_t> cdfSampleAndRemove(const Tensor<float> &weights, const Tensor<float> &u, void *stream = nullptr) {
  int64_t rows, n, rs;
  detail::scan_rows(weights, "cdfSampleAndRemove", rows, n, rs);
  Tensor<int32_t> idx = detail::scan_result_for(u, rows);
  Tensor<float> w, cdf;
  detail::scan_private(weights, rows, n, rs, w, cdf, stream);
  check(laser_hip_cdf_sample_remove_f32_dev(idx.unsafe_raw_data(), w.unsafe_raw_data(), n, cdf.unsafe_raw_data(), n, u.unsafe_raw_data(),
                                            rows, n, u.shape[1], stream));
  return idx;
}
inline Tensor<int32_t> cdfSampleAndRemove(const Tensor<float> &weights, Rng &rng, int64_t num = 1, void *stream = nullptr) {
  int64_t rows, n, rs;
  detail::scan_rows(weights, "cdfSampleAndRemove", rows, n, rs);
  if (num < 0) throw Error(LASER_HIP_E_INVALID, "cdfSampleAndRemove: a count >= 0 is needed");
  Tensor<int32_t> idx = newTensor<int32_t>({rows, num});
  Tensor<float> w, cdf;
  detail::scan_private(weights, rows, n, rs, w, cdf, stream);
  check(laser_hip_cdf_sample_remove_rng_f32_dev(idx.unsafe_raw_data(), w.unsafe_raw_data(), n, cdf.unsafe_raw_data(), n, (int64_t)rng.seed,
                                                (int64_t)rng.subseq, (int64_t)rng.offset, rows, n, num, stream));
  rng.advance((uint64_t)(rows * num));
  return idx;
}

// ---- Row top-k, argmax and top-k sampling (include/laser_hip_select.h, the section of that name) -------------------------------
//   auto r = laser::topk(x, k, largest);        r.values (bit copies), r.indices: (rows, k), rank 0 first; x: a matrix whose rows
//                                               are contiguous (or a vector for one row)
//   laser::argmax(x), laser::argmin(x)          Tensor<int32_t> (rows): topk's index for k = 1 from a single pass
//   laser::take_rows(src, j)                    out[r, c] = src[r, j[r, c]], -1 where j[r, c] is outside the row
//   laser::sample_top_k(logits, k, u) / (logits, k, rng, num)   draws among the k largest logits of every row in proportion to
//                                               their softmax: topk, softmax, cumsum, cdfSample, take_rows
// The order is one of bit patterns (a positive NaN is the largest element, -0 ranks below +0, identical bits rank by ascending
// column): every bit and index is a function of the row's bits, k and `largest` alone.  Asynchronous on `stream`.
struct TopkResult {
  Tensor<float> values;
  Tensor<int32_t> indices;
};
inline TopkResult topk(const Tensor<float> &x, int64_t k, bool largest = true, void *stream = nullptr) {
  int64_t rows, n, rs;
  detail::scan_rows(x, "topk", rows, n, rs);
  if (k < 1 || k > n || k > LASER_HIP_SELECT_MAX_K) throw Error(LASER_HIP_E_INVALID, "topk: 1 <= k <= min(n, 1024) is needed");
  TopkResult r{newTensor<float>({rows, k}), newTensor<int32_t>({rows, k})};
  check(laser_hip_topk_rows_f32_dev(r.values.unsafe_raw_data(), k, r.indices.unsafe_raw_data(), k, x.unsafe_raw_data(), rs, rows, n, k,
                                    largest ? 1 : 0, stream));
  return r;
}
namespace detail {
inline Tensor<int32_t> arg_rows(const Tensor<float> &x, const char *what, int largest, void *stream) {
  int64_t rows, n, rs;
  scan_rows(x, what, rows, n, rs);
  Tensor<int32_t> idx = newTensor<int32_t>({rows});
  check(laser_hip_argmax_rows_f32_dev(idx.unsafe_raw_data(), 1, nullptr, 1, x.unsafe_raw_data(), rs, rows, n, largest, stream));
  return idx;
}
}  // namespace detail
inline Tensor<int32_t> argmax(const Tensor<float> &x, void *stream = nullptr) { return detail::arg_rows(x, "argmax", 1, stream); }
inline Tensor<int32_t> argmin(const Tensor<float> &x, void *stream = nullptr) { return detail::arg_rows(x, "argmin", 0, stream); }
inline Tensor<int32_t> take_rows(const Tensor<int32_t> &src, const Tensor<int32_t> &j, void *stream = nullptr) {
  int64_t rows, m, ss, jrows, num, js;
  detail::scan_rows(src, "take_rows", rows, m, ss);
  if (j.rank() != 2 || src.rank() != 2) throw Error(LASER_HIP_E_INVALID, "take_rows: two matrices are needed");
  if (j.shape[1] == 0) return newTensor<int32_t>({rows, 0});
  detail::scan_rows(j, "take_rows", jrows, num, js);
  if (jrows != rows) throw Error(LASER_HIP_E_INVALID, "take_rows: src and j need the same number of rows");
  Tensor<int32_t> out = newTensor<int32_t>({rows, num});
  check(laser_hip_take_rows_i32_dev(out.unsafe_raw_data(), num, src.unsafe_raw_data(), ss, j.unsafe_raw_data(), js, rows, m, num, stream));
  return out;
}
inline Tensor<int32_t> sample_top_k(const Tensor<float> &logits, int64_t k, const Tensor<float> &u, void *stream = nullptr) {
  if (logits.rank() != 2) throw Error(LASER_HIP_E_INVALID, "sample_top_k: a matrix of logits is needed");
  const TopkResult r = topk(logits, k, true, stream);
  return take_rows(r.indices, cdfSample(cumsum(softmax(r.values, stream), stream), u, stream), stream);
}
inline Tensor<int32_t> sample_top_k(const Tensor<float> &logits, int64_t k, Rng &rng, int64_t num = 1, void *stream = nullptr) {
  if (logits.rank() != 2) throw Error(LASER_HIP_E_INVALID, "sample_top_k: a matrix of logits is needed");
  const TopkResult r = topk(logits, k, true, stream);
  return take_rows(r.indices, cdfSample(cumsum(softmax(r.values, stream), stream), rng, num, stream), stream);
}

#undef LASER_DISPATCH
#undef LASER_GEMM_DISPATCH
}  // namespace laser
