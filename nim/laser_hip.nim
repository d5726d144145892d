# nim/laser_hip.nim -- the shim a Laser maintainer adds to route the GEMM hot path to an MI355X.
#
# Every exported proc below keeps the SIGNATURE of the reference proc it replaces (file:line given
# per proc) and forwards to the monomorphic C-ABI symbol of liblaser_hip.so (include/laser_hip.h).
# FFI idiom is the one the reference already uses for OpenBLAS (benchmarks/third_party/blas.nim:
# 18-23: `{.dynlib: blas, importc: "cblas_sgemm".}`) and for libjit (gemm_bench_float32.nim:199-202).
#
# NOTE: delivered as SOURCE.  The build image has no Nim compiler (probed: nim/nimble absent, no
# network), so this file has not been compiled here.  What IS checked mechanically
# (tests/test_nim_shim_cpu.py): every `importc: "..."` below names a symbol that liblaser_hip.so
# exports (nm -D) and that include/laser_hip.h declares, with the same number of parameters and
# C-compatible parameter / return types (Nim int == int64_t on amd64, cint == int, float32 == float,
# float64 == double, pointer / ptr T / cstring == pointers); every import is spelled with an explicit
# `importc: "<symbol>"` string (no identifier pasting), one declaration per C symbol.
#
# Usage inside Laser: `import laser_hip` instead of `./gemm` / `./gemm_prepacked` /
# `../swapaxes` / `./conv2d_im2col`; call sites do not change.

const laserHip* = "liblaser_hip.so"

{.pragma: lh, cdecl, dynlib: laserHip.}

# ---- C-ABI imports (Nim int == int64 on amd64, float32 == C float) ---------------------------
proc laser_hip_last_error(): cstring {.lh, importc: "laser_hip_last_error".}
proc laser_hip_abi_version*(): cint {.lh, importc: "laser_hip_abi_version".}
const laserHipAbi* = 3                       # include/laser_hip.h LASER_HIP_ABI_VERSION this shim was written against
proc laser_hip_init*(device: cint): cint {.lh, importc: "laser_hip_init".}
proc laser_hip_finalize*(): cint {.lh, importc: "laser_hip_finalize".}
proc laser_hip_device_count*(): cint {.lh, importc: "laser_hip_device_count".}
proc laser_hip_plan_f32*(M, N, K: int64, laser_order, cus: cint, out8: ptr int64): cint {.lh, importc: "laser_hip_plan_f32".}   # diagnostics: kernel + launch plan for a device of `cus` CUs
proc laser_hip_set_float_mode*(mode: cint): cint {.lh, importc: "laser_hip_set_float_mode".}   # 0 = Laser order (default), 1 = fast
# every tuning / A-B switch by name (include/laser_hip.h lists them), and the read-only diagnostics of the last launch
proc laser_hip_set_option(name: cstring, value: cint): cint {.lh, importc: "laser_hip_set_option".}
proc laser_hip_get_option(name: cstring, value: ptr int): cint {.lh, importc: "laser_hip_get_option".}

proc laserHipCheckAbi*() =
  ## call once at start-up: a library with another ABI number takes other argument types for the same symbol names
  doAssert laser_hip_abi_version() == laserHipAbi, "liblaser_hip.so has ABI " & $laser_hip_abi_version() & ", this shim expects " & $laserHipAbi

template check(rc: cint) =
  # the reference procs return void and doAssert on precondition violations
  # (gemm_prepacked.nim:125,208; conv2d_im2col.nim:109); keep that contract
  let code = rc
  doAssert code == 0, "laser_hip error " & $code & ": " & $laser_hip_last_error()

# gemm_strided, host pointers (blocking, Laser's call semantics)
proc laser_hip_gemm_strided_f32(M, N, K: int, alpha: float32, A: ptr float32, rsA, csA: int, B: ptr float32, rsB, csB: int, beta: float32, C: ptr float32, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_strided_f32".}
proc laser_hip_gemm_strided_f64(M, N, K: int, alpha: float64, A: ptr float64, rsA, csA: int, B: ptr float64, rsB, csB: int, beta: float64, C: ptr float64, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_strided_f64".}
proc laser_hip_gemm_strided_i32(M, N, K: int, alpha: int32, A: ptr int32, rsA, csA: int, B: ptr int32, rsB, csB: int, beta: int32, C: ptr int32, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_strided_i32".}
proc laser_hip_gemm_strided_i64(M, N, K: int, alpha: int64, A: ptr int64, rsA, csA: int, B: ptr int64, rsB, csB: int, beta: int64, C: ptr int64, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_strided_i64".}
# gemm_strided, device pointers + stream (asynchronous; operands resident in HBM)
proc laser_hip_gemm_strided_f32_dev(M, N, K: int, alpha: float32, A: pointer, rsA, csA: int, B: pointer, rsB, csB: int, beta: float32, C: pointer, rsC, csC: int, stream: pointer): cint {.lh, importc: "laser_hip_gemm_strided_f32_dev".}
proc laser_hip_gemm_strided_f64_dev(M, N, K: int, alpha: float64, A: pointer, rsA, csA: int, B: pointer, rsB, csB: int, beta: float64, C: pointer, rsC, csC: int, stream: pointer): cint {.lh, importc: "laser_hip_gemm_strided_f64_dev".}
proc laser_hip_gemm_strided_i32_dev(M, N, K: int, alpha: int32, A: pointer, rsA, csA: int, B: pointer, rsB, csB: int, beta: int32, C: pointer, rsC, csC: int, stream: pointer): cint {.lh, importc: "laser_hip_gemm_strided_i32_dev".}
proc laser_hip_gemm_strided_i64_dev(M, N, K: int, alpha: int64, A: pointer, rsA, csA: int, B: pointer, rsB, csB: int, beta: int64, C: pointer, rsC, csC: int, stream: pointer): cint {.lh, importc: "laser_hip_gemm_strided_i64_dev".}
# int8 / int16 (uint8 / uint16 on the same bits): alpha and beta travel as int32 and the library reduces them mod 2^8 / 2^16
proc laser_hip_gemm_strided_i8(M, N, K: int, alpha: int32, A: ptr int8, rsA, csA: int, B: ptr int8, rsB, csB: int, beta: int32, C: ptr int8, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_strided_i8".}
proc laser_hip_gemm_strided_i16(M, N, K: int, alpha: int32, A: ptr int16, rsA, csA: int, B: ptr int16, rsB, csB: int, beta: int32, C: ptr int16, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_strided_i16".}
proc laser_hip_gemm_strided_i8_dev(M, N, K: int, alpha: int32, A: pointer, rsA, csA: int, B: pointer, rsB, csB: int, beta: int32, C: pointer, rsC, csC: int, stream: pointer): cint {.lh, importc: "laser_hip_gemm_strided_i8_dev".}
proc laser_hip_gemm_strided_i16_dev(M, N, K: int, alpha: int32, A: pointer, rsA, csA: int, B: pointer, rsB, csB: int, beta: int32, C: pointer, rsC, csC: int, stream: pointer): cint {.lh, importc: "laser_hip_gemm_strided_i16_dev".}

# pre-packed GEMM
proc laser_hip_gemm_prepackA_mem_required_f32(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackA_mem_required_f32".}
proc laser_hip_gemm_prepackA_mem_required_f64(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackA_mem_required_f64".}
proc laser_hip_gemm_prepackA_mem_required_i32(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackA_mem_required_i32".}
proc laser_hip_gemm_prepackA_mem_required_i64(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackA_mem_required_i64".}
proc laser_hip_gemm_prepackB_mem_required_f32(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackB_mem_required_f32".}
proc laser_hip_gemm_prepackB_mem_required_f64(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackB_mem_required_f64".}
proc laser_hip_gemm_prepackB_mem_required_i32(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackB_mem_required_i32".}
proc laser_hip_gemm_prepackB_mem_required_i64(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackB_mem_required_i64".}
proc laser_hip_gemm_prepackA_f32(dst: pointer, M, N, K: int, A: ptr float32, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackA_f32".}
proc laser_hip_gemm_prepackA_f64(dst: pointer, M, N, K: int, A: ptr float64, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackA_f64".}
proc laser_hip_gemm_prepackA_i32(dst: pointer, M, N, K: int, A: ptr int32, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackA_i32".}
proc laser_hip_gemm_prepackA_i64(dst: pointer, M, N, K: int, A: ptr int64, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackA_i64".}
proc laser_hip_gemm_prepackB_f32(dst: pointer, M, N, K: int, B: ptr float32, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackB_f32".}
proc laser_hip_gemm_prepackB_f64(dst: pointer, M, N, K: int, B: ptr float64, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackB_f64".}
proc laser_hip_gemm_prepackB_i32(dst: pointer, M, N, K: int, B: ptr int32, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackB_i32".}
proc laser_hip_gemm_prepackB_i64(dst: pointer, M, N, K: int, B: ptr int64, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackB_i64".}
proc laser_hip_gemm_packed_f32(M, N, K: int, alpha: float32, pA, pB: pointer, beta: float32, C: ptr float32, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_packed_f32".}
proc laser_hip_gemm_packed_f64(M, N, K: int, alpha: float64, pA, pB: pointer, beta: float64, C: ptr float64, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_packed_f64".}
proc laser_hip_gemm_packed_i32(M, N, K: int, alpha: int32, pA, pB: pointer, beta: int32, C: ptr int32, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_packed_i32".}
proc laser_hip_gemm_packed_i64(M, N, K: int, alpha: int64, pA, pB: pointer, beta: int64, C: ptr int64, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_packed_i64".}
proc laser_hip_gemm_prepackA_mem_required_i8(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackA_mem_required_i8".}
proc laser_hip_gemm_prepackA_mem_required_i16(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackA_mem_required_i16".}
proc laser_hip_gemm_prepackB_mem_required_i8(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackB_mem_required_i8".}
proc laser_hip_gemm_prepackB_mem_required_i16(M, N, K: int): int {.lh, importc: "laser_hip_gemm_prepackB_mem_required_i16".}
proc laser_hip_gemm_prepackA_i8(dst: pointer, M, N, K: int, A: ptr int8, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackA_i8".}
proc laser_hip_gemm_prepackA_i16(dst: pointer, M, N, K: int, A: ptr int16, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackA_i16".}
proc laser_hip_gemm_prepackB_i8(dst: pointer, M, N, K: int, B: ptr int8, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackB_i8".}
proc laser_hip_gemm_prepackB_i16(dst: pointer, M, N, K: int, B: ptr int16, rs, cs: int): cint {.lh, importc: "laser_hip_gemm_prepackB_i16".}
proc laser_hip_gemm_packed_i8(M, N, K: int, alpha: int32, pA, pB: pointer, beta: int32, C: ptr int8, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_packed_i8".}
proc laser_hip_gemm_packed_i16(M, N, K: int, alpha: int32, pA, pB: pointer, beta: int32, C: ptr int16, rsC, csC: int): cint {.lh, importc: "laser_hip_gemm_packed_i16".}
proc laser_hip_gemm_prepack_release*(packed: pointer): cint {.lh, importc: "laser_hip_gemm_prepack_release".}

# physical transposes
proc laser_hip_transpose2d_copy_b32(dst, src: pointer, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_copy_b32".}
proc laser_hip_transpose2d_copy_b64(dst, src: pointer, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_copy_b64".}
proc laser_hip_transpose2d_batched_b32(dst, src: pointer, N, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_batched_b32".}
proc laser_hip_transpose2d_batched_b64(dst, src: pointer, N, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_batched_b64".}
proc laser_hip_transpose2d_copy_b16(dst, src: pointer, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_copy_b16".}
proc laser_hip_transpose2d_copy_b8(dst, src: pointer, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_copy_b8".}
proc laser_hip_transpose2d_batched_b16(dst, src: pointer, N, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_batched_b16".}
proc laser_hip_transpose2d_batched_b8(dst, src: pointer, N, NR, NC: int): cint {.lh, importc: "laser_hip_transpose2d_batched_b8".}

# im2col + GEMM convolution, cblas-shaped gemm
proc laser_hip_im2col_workspace_size(iN, iC, iH, iW, cOut, cIn, kH, kW, pH, pW, sH, sW: int): int {.lh, importc: "laser_hip_im2col_workspace_size".}
proc laser_hip_im2col_f32(ws: ptr float32, oH, oW: int, input: ptr float32, iC, iH, iW, kH, kW, pH, pW, sH, sW: int): cint {.lh, importc: "laser_hip_im2col_f32".}
proc laser_hip_im2col_f64(ws: ptr float64, oH, oW: int, input: ptr float64, iC, iH, iW, kH, kW, pH, pW, sH, sW: int): cint {.lh, importc: "laser_hip_im2col_f64".}
proc laser_hip_conv2d_im2col_f32(output, input: ptr float32, iN, iC, iH, iW: int, kernel: ptr float32, cOut, cIn, kH, kW, pH, pW, sH, sW: int, ws: ptr float32): cint {.lh, importc: "laser_hip_conv2d_im2col_f32".}
proc laser_hip_cblas_sgemm(order, tA, tB: cint, M, N, K: int, alpha: float32, A: ptr float32, lda: int, B: ptr float32, ldb: int, beta: float32, C: ptr float32, ldc: int): cint {.lh, importc: "laser_hip_cblas_sgemm".}
proc laser_hip_cblas_dgemm(order, tA, tB: cint, M, N, K: int, alpha: float64, A: ptr float64, lda: int, B: ptr float64, ldb: int, beta: float64, C: ptr float64, ldc: int): cint {.lh, importc: "laser_hip_cblas_dgemm".}

# fused epilogue
proc laser_hip_gemm_strided_ex_f32(M, N, K: int, alpha: float32, A: ptr float32, rsA, csA: int, B: ptr float32, rsB, csB: int, beta: float32, C: ptr float32, rsC, csC: int, bias: ptr float32, rsBias, csBias: int, activation: cint): cint {.lh, importc: "laser_hip_gemm_strided_ex_f32".}
proc laser_hip_gemm_strided_ex_f64(M, N, K: int, alpha: float64, A: ptr float64, rsA, csA: int, B: ptr float64, rsB, csB: int, beta: float64, C: ptr float64, rsC, csC: int, bias: ptr float64, rsBias, csBias: int, activation: cint): cint {.lh, importc: "laser_hip_gemm_strided_ex_f64".}

# device tensor storage
proc laser_hip_storage_alloc(d: ptr pointer, bytes: int): cint {.lh, importc: "laser_hip_storage_alloc".}
proc laser_hip_storage_free(d: pointer): cint {.lh, importc: "laser_hip_storage_free".}
proc laser_hip_storage_upload(d, host: pointer, bytes: int): cint {.lh, importc: "laser_hip_storage_upload".}
proc laser_hip_storage_download(host, d: pointer, bytes: int): cint {.lh, importc: "laser_hip_storage_download".}
proc laser_hip_storage_set_zero(d: pointer, bytes: int, stream: pointer): cint {.lh, importc: "laser_hip_storage_set_zero".}
proc laser_hip_copy_strided_b32_dev(dst: pointer, dstStrides: ptr int, src: pointer, srcStrides: ptr int, shape: ptr int, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_copy_strided_b32_dev".}
proc laser_hip_copy_strided_b64_dev(dst: pointer, dstStrides: ptr int, src: pointer, srcStrides: ptr int, shape: ptr int, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_copy_strided_b64_dev".}

# ---- gemm_strided -- laser/primitives/matrix_multiplication/gemm.nim:184-193 --------------------
# Element types: every SomeNumber, like the reference (gemm.nim:184-248).  Integer arithmetic wraps modulo 2^n, so each
# unsigned type is the signed entry point of its width on the same bits (gemm.nim:239 does this for int32 / uint32).
proc gemm_strided*[T: SomeNumber](
      M, N, K: int,
      alpha: T,
      A: ptr T,
      rowStrideA, colStrideA: int,
      B: ptr T,
      rowStrideB, colStrideB: int,
      beta: T,
      C: ptr T,
      rowStrideC, colStrideC: int) =
  when T is float32:
    check laser_hip_gemm_strided_f32(M, N, K, alpha, A, rowStrideA, colStrideA, B, rowStrideB, colStrideB, beta, C, rowStrideC, colStrideC)
  elif T is float64:
    check laser_hip_gemm_strided_f64(M, N, K, alpha, A, rowStrideA, colStrideA, B, rowStrideB, colStrideB, beta, C, rowStrideC, colStrideC)
  elif T is int32:
    check laser_hip_gemm_strided_i32(M, N, K, alpha, A, rowStrideA, colStrideA, B, rowStrideB, colStrideB, beta, C, rowStrideC, colStrideC)
  elif T is uint32:
    check laser_hip_gemm_strided_i32(M, N, K, cast[int32](alpha), cast[ptr int32](A), rowStrideA, colStrideA,
                                     cast[ptr int32](B), rowStrideB, colStrideB, cast[int32](beta),
                                     cast[ptr int32](C), rowStrideC, colStrideC)
  elif T is int64 or T is int:
    check laser_hip_gemm_strided_i64(M, N, K, cast[int64](alpha), cast[ptr int64](A), rowStrideA, colStrideA,
                                     cast[ptr int64](B), rowStrideB, colStrideB, cast[int64](beta),
                                     cast[ptr int64](C), rowStrideC, colStrideC)
  elif T is uint64 or T is uint:
    check laser_hip_gemm_strided_i64(M, N, K, cast[int64](alpha), cast[ptr int64](A), rowStrideA, colStrideA,
                                     cast[ptr int64](B), rowStrideB, colStrideB, cast[int64](beta),
                                     cast[ptr int64](C), rowStrideC, colStrideC)
  elif T is int8 or T is uint8:
    check laser_hip_gemm_strided_i8(M, N, K, int32(cast[int8](alpha)), cast[ptr int8](A), rowStrideA, colStrideA,
                                    cast[ptr int8](B), rowStrideB, colStrideB, int32(cast[int8](beta)),
                                    cast[ptr int8](C), rowStrideC, colStrideC)
  elif T is int16 or T is uint16:
    check laser_hip_gemm_strided_i16(M, N, K, int32(cast[int16](alpha)), cast[ptr int16](A), rowStrideA, colStrideA,
                                     cast[ptr int16](B), rowStrideB, colStrideB, int32(cast[int16](beta)),
                                     cast[ptr int16](C), rowStrideC, colStrideC)
  else:
    {.error: "laser_hip: unsupported element type " & $T.}

# ---- fused epilogue -- planned in the reference (README.md:238-242; TODO gemm.nim:196) -------------
# C = act(alpha*A*B + beta*C + bias); bias is a strided M x N view whose strides may be 0.
type Activation* = enum
  actNone = 0, actRelu = 1, actTanh = 2, actSigmoid = 3
# fused PROLOGUE -- "fuse operations before the matrix multiplication kernel, during the prepacking" (README.md:243-244):
# the product is taken of relu(A) and / or relu(B); the bits travel in the activation argument (LASER_HIP_PRE_RELU_A / _B)
type Prologue* = enum
  preNone = 0, preReluA = 0x100, preReluB = 0x200, preReluAB = 0x300

proc gemm_strided_fused*[T: float32 or float64](
      M, N, K: int, alpha: T,
      A: ptr T, rowStrideA, colStrideA: int,
      B: ptr T, rowStrideB, colStrideB: int,
      beta: T,
      C: ptr T, rowStrideC, colStrideC: int,
      bias: ptr T, rowStrideBias, colStrideBias: int,
      activation = actNone, prologue = preNone) =
  let code = cint(ord(activation) or ord(prologue))
  when T is float32:
    check laser_hip_gemm_strided_ex_f32(M, N, K, alpha, A, rowStrideA, colStrideA, B, rowStrideB, colStrideB, beta,
                                        C, rowStrideC, colStrideC, bias, rowStrideBias, colStrideBias, code)
  else:
    check laser_hip_gemm_strided_ex_f64(M, N, K, alpha, A, rowStrideA, colStrideA, B, rowStrideB, colStrideB, beta,
                                        C, rowStrideC, colStrideC, bias, rowStrideBias, colStrideBias, code)

# ---- pre-packed GEMM -- gemm_prepacked.nim:76-292 -----------------------------------------------
proc gemm_prepackB_mem_required*(T: type, M, N, K: int): int =
  when T is float32: laser_hip_gemm_prepackB_mem_required_f32(M, N, K)
  elif T is float64: laser_hip_gemm_prepackB_mem_required_f64(M, N, K)
  elif T is int32 or T is uint32: laser_hip_gemm_prepackB_mem_required_i32(M, N, K)
  elif T is int8 or T is uint8: laser_hip_gemm_prepackB_mem_required_i8(M, N, K)
  elif T is int16 or T is uint16: laser_hip_gemm_prepackB_mem_required_i16(M, N, K)
  else: laser_hip_gemm_prepackB_mem_required_i64(M, N, K)

proc gemm_prepackA_mem_required*(T: type, M, N, K: int): int =
  when T is float32: laser_hip_gemm_prepackA_mem_required_f32(M, N, K)
  elif T is float64: laser_hip_gemm_prepackA_mem_required_f64(M, N, K)
  elif T is int32 or T is uint32: laser_hip_gemm_prepackA_mem_required_i32(M, N, K)
  elif T is int8 or T is uint8: laser_hip_gemm_prepackA_mem_required_i8(M, N, K)
  elif T is int16 or T is uint16: laser_hip_gemm_prepackA_mem_required_i16(M, N, K)
  else: laser_hip_gemm_prepackA_mem_required_i64(M, N, K)

proc gemm_prepackB*[T](dst_packedB: ptr (T or UncheckedArray[T]), M, N, K: int,
                       src_B: ptr T, rowStrideB, colStrideB: int) =
  when T is float32: check laser_hip_gemm_prepackB_f32(dst_packedB, M, N, K, src_B, rowStrideB, colStrideB)
  elif T is float64: check laser_hip_gemm_prepackB_f64(dst_packedB, M, N, K, src_B, rowStrideB, colStrideB)
  elif T is int32: check laser_hip_gemm_prepackB_i32(dst_packedB, M, N, K, src_B, rowStrideB, colStrideB)
  elif T is uint32: check laser_hip_gemm_prepackB_i32(dst_packedB, M, N, K, cast[ptr int32](src_B), rowStrideB, colStrideB)
  elif T is int8 or T is uint8: check laser_hip_gemm_prepackB_i8(dst_packedB, M, N, K, cast[ptr int8](src_B), rowStrideB, colStrideB)
  elif T is int16 or T is uint16: check laser_hip_gemm_prepackB_i16(dst_packedB, M, N, K, cast[ptr int16](src_B), rowStrideB, colStrideB)
  else: check laser_hip_gemm_prepackB_i64(dst_packedB, M, N, K, cast[ptr int64](src_B), rowStrideB, colStrideB)

proc gemm_prepackA*[T](dst_packedA: ptr (T or UncheckedArray[T]), M, N, K: int,
                       src_A: ptr T, rowStrideA, colStrideA: int) =
  when T is float32: check laser_hip_gemm_prepackA_f32(dst_packedA, M, N, K, src_A, rowStrideA, colStrideA)
  elif T is float64: check laser_hip_gemm_prepackA_f64(dst_packedA, M, N, K, src_A, rowStrideA, colStrideA)
  elif T is int32: check laser_hip_gemm_prepackA_i32(dst_packedA, M, N, K, src_A, rowStrideA, colStrideA)
  elif T is uint32: check laser_hip_gemm_prepackA_i32(dst_packedA, M, N, K, cast[ptr int32](src_A), rowStrideA, colStrideA)
  elif T is int8 or T is uint8: check laser_hip_gemm_prepackA_i8(dst_packedA, M, N, K, cast[ptr int8](src_A), rowStrideA, colStrideA)
  elif T is int16 or T is uint16: check laser_hip_gemm_prepackA_i16(dst_packedA, M, N, K, cast[ptr int16](src_A), rowStrideA, colStrideA)
  else: check laser_hip_gemm_prepackA_i64(dst_packedA, M, N, K, cast[ptr int64](src_A), rowStrideA, colStrideA)

proc gemm_packed*[T: SomeNumber](M, N, K: int, alpha: T,
      packedA: ptr (T or UncheckedArray[T]), packedB: ptr (T or UncheckedArray[T]),
      beta: T, C: ptr (T or UncheckedArray[T]), rowStrideC, colStrideC: int) =
  when T is float32: check laser_hip_gemm_packed_f32(M, N, K, alpha, packedA, packedB, beta, cast[ptr float32](C), rowStrideC, colStrideC)
  elif T is float64: check laser_hip_gemm_packed_f64(M, N, K, alpha, packedA, packedB, beta, cast[ptr float64](C), rowStrideC, colStrideC)
  elif T is int32: check laser_hip_gemm_packed_i32(M, N, K, alpha, packedA, packedB, beta, cast[ptr int32](C), rowStrideC, colStrideC)
  elif T is uint32: check laser_hip_gemm_packed_i32(M, N, K, cast[int32](alpha), packedA, packedB, cast[int32](beta), cast[ptr int32](C), rowStrideC, colStrideC)
  elif T is int8 or T is uint8: check laser_hip_gemm_packed_i8(M, N, K, int32(cast[int8](alpha)), packedA, packedB, int32(cast[int8](beta)), cast[ptr int8](C), rowStrideC, colStrideC)
  elif T is int16 or T is uint16: check laser_hip_gemm_packed_i16(M, N, K, int32(cast[int16](alpha)), packedA, packedB, int32(cast[int16](beta)), cast[ptr int16](C), rowStrideC, colStrideC)
  else: check laser_hip_gemm_packed_i64(M, N, K, cast[int64](alpha), packedA, packedB, cast[int64](beta), cast[ptr int64](C), rowStrideC, colStrideC)

# ---- physical transposes -- laser/primitives/swapaxes.nim:16-112 ---------------------------------
proc transpose2D_copy*[T](dst, src: ptr (T or UncheckedArray[T]), NR, NC: Natural) =
  when sizeof(T) == 4: check laser_hip_transpose2d_copy_b32(dst, src, NR, NC)
  elif sizeof(T) == 8: check laser_hip_transpose2d_copy_b64(dst, src, NR, NC)
  elif sizeof(T) == 2: check laser_hip_transpose2d_copy_b16(dst, src, NR, NC)
  elif sizeof(T) == 1: check laser_hip_transpose2d_copy_b8(dst, src, NR, NC)
  else: {.error: "laser_hip transposes support 1-, 2-, 4- and 8-byte elements".}

proc transpose2D_batched*[T](dst, src: ptr (T or UncheckedArray[T]), N, NR, NC: Natural) =
  when sizeof(T) == 4: check laser_hip_transpose2d_batched_b32(dst, src, N, NR, NC)
  elif sizeof(T) == 8: check laser_hip_transpose2d_batched_b64(dst, src, N, NR, NC)
  elif sizeof(T) == 2: check laser_hip_transpose2d_batched_b16(dst, src, N, NR, NC)
  elif sizeof(T) == 1: check laser_hip_transpose2d_batched_b8(dst, src, N, NR, NC)
  else: {.error: "laser_hip transposes support 1-, 2-, 4- and 8-byte elements".}

proc nchw2nhwc*[T](dst_nhwc, src_nchw: ptr (T or UncheckedArray[T]), N, C, H, W: Natural) {.inline.} =
  transpose2D_batched(dst_nhwc, src_nchw, N, C, H*W)       # swapaxes.nim:98

proc nhwc2nchw*[T](dst_nchw, src_nhwc: ptr (T or UncheckedArray[T]), N, C, H, W: Natural) {.inline.} =
  transpose2D_batched(dst_nchw, src_nhwc, N, H*W, C)       # swapaxes.nim:112

# ---- im2col + GEMM convolution -- benchmarks/convolution/conv2d_im2col.nim -----------------------
# The convolution benchmark's own types, conv2d_common.nim:6-13.  Its `Tensor[T]` is a plain `seq[T]`
# (conv2d_common.nim:13: `Tensor*[T] = seq[T]`) -- NOT laser/tensor's Tensor -- which is why
# conv2d_bench.nim:92-102 can hand seqs to conv2d_im2col.  A maintainer who keeps
# `import ./conv2d_common` drops the five declarations below.
type
  TensorShape* = tuple[n, c, h, w: int]
  KernelShape* = tuple[c_out, c_in, kH, kW: int]
  Padding* = tuple[h, w: int]
  Strides* = tuple[h, w: int]
  Tensor*[T] = seq[T]

proc im2col_workspace_size*(ishape: TensorShape, kshape: KernelShape, padding: Padding, strides: Strides): int =
  laser_hip_im2col_workspace_size(ishape.n, ishape.c, ishape.h, ishape.w, kshape.c_out, kshape.c_in,
                                  kshape.kH, kshape.kW, padding.h, padding.w, strides.h, strides.w)

# conv2d_im2col.nim:42-50: generic in T (pure data movement: by element size -- int32 rides on the float32 entry point, int64 on the float64 one)
proc im2col*[T](pworkspace: ptr T, oshape: TensorShape, pinput: ptr UncheckedArray[T],
                ishape: TensorShape, kshape: KernelShape, padding: Padding, strides: Strides) =
  when sizeof(T) == 4:
    check laser_hip_im2col_f32(cast[ptr float32](pworkspace), oshape.h, oshape.w, cast[ptr float32](pinput), ishape.c, ishape.h,
                               ishape.w, kshape.kH, kshape.kW, padding.h, padding.w, strides.h, strides.w)
  elif sizeof(T) == 8:
    check laser_hip_im2col_f64(cast[ptr float64](pworkspace), oshape.h, oshape.w, cast[ptr float64](pinput), ishape.c, ishape.h,
                               ishape.w, kshape.kH, kshape.kW, padding.h, padding.w, strides.h, strides.w)
  else: {.error: "laser_hip im2col supports 4- and 8-byte elements".}

# conv2d_im2col.nim:90-100, parameter for parameter
proc conv2d_im2col*(
    output: var Tensor[float32], # Output tensor
    oshape: TensorShape,         # Shape of output
    input: Tensor[float32],      # Input tensor
    ishape: TensorShape,         # Shape of input
    kernel: Tensor[float32],     # Convolution filter
    kshape: KernelShape,         # kernel shape
    padding: Padding,            # Padding
    strides: Strides,            # Strides
    pworkspace: ptr float32      # Workspace buffer, can be reused between batches
  ) =
  assert oshape.c == kshape.c_out                        # conv2d_im2col.nim:109
  check laser_hip_conv2d_im2col_f32(output[0].addr, input[0].unsafeAddr, ishape.n, ishape.c, ishape.h, ishape.w,
                                    kernel[0].unsafeAddr, kshape.c_out, kshape.c_in, kshape.kH, kshape.kW,
                                    padding.h, padding.w, strides.h, strides.w, pworkspace)

# ---- cblas-shaped gemm -- benchmarks/third_party/blas.nim:12-23 ----------------------------------
type
  TransposeType* {.size: sizeof(cint).} = enum
    noTranspose = 111, transpose = 112, conjTranspose = 113
  OrderType* {.size: sizeof(cint).} = enum
    rowMajor = 101, colMajor = 102

# blas.nim:18-20 (cblas_sgemm)
proc gemm*(ORDER: OrderType, TRANSA, TRANSB: TransposeType, M, N, K: int, ALPHA: float32,
           A: ptr float32, LDA: int, B: ptr float32, LDB: int, BETA: float32, C: ptr float32, LDC: int) =
  check laser_hip_cblas_sgemm(cint(ORDER), cint(TRANSA), cint(TRANSB), M, N, K, ALPHA, A, LDA, B, LDB, BETA, C, LDC)

# blas.nim:21-23 (cblas_dgemm)
proc gemm*(ORDER: OrderType, TRANSA, TRANSB: TransposeType, M, N, K: int, ALPHA: float64,
           A: ptr float64, LDA: int, B: ptr float64, LDB: int, BETA: float64, C: ptr float64, LDC: int) =
  check laser_hip_cblas_dgemm(cint(ORDER), cint(TRANSA), cint(TRANSB), M, N, K, ALPHA, A, LDA, B, LDB, BETA, C, LDC)

# ---- RawTensor / forEach surface ------------------------------------------------------------------
# Nothing to replace for HOST tensors: `Tensor[T]`, `unsafe_raw_data`, `forEach` stay Laser's own
# (laser/tensor/datatypes.nim:13-30, laser/strided_iteration/foreach.nim:192-264).  A caller does
#   gemm_strided(M, N, K, 1'f32, a.unsafe_raw_data, a.strides[0], a.strides[1], ...)
# exactly as before; only raw pointers and element strides cross the ABI.

# ---- device-resident storage: HipStorage, the twin of CpuStorage ---------------------------------
# (SURVEY.md section 8f rank 3.)  A tensor keeps its shape / strides / offset; what changes is where
# `storage.raw_buffer` lives.  GUARD: a device address must never reach Laser's host `forEach`, whose
# duck-typing contract is `rank, size, shape, strides, unsafe_raw_data` (foreach.nim:7-29,
# laser/strided_iteration/README.md:101-107) -- it would dereference the pointer on the CPU.  So
#   * the device pointer type is `DevicePtr[T]`, a `distinct pointer` with NO `[]` and no conversion
#     to `ptr T`: it cannot be passed to gemm_strided / transpose2D_copy (host entry points) by accident;
#   * HipStorage has NO `unsafe_raw_data`; its accessor is `unsafe_device_data`, so `forEach x in t`
#     on a HipStorage-backed tensor fails to COMPILE (undeclared identifier in forEach's expansion);
#   * elementwise work on device tensors goes through `mapStrided` below
#     (laser_hip_map_strided_*_dev), the device-side twin of forEach's strided iteration.
type
  DevicePtr*[T] = distinct pointer       # an HBM address: not dereferenceable on the host
  HipStorage*{.shallow.}[T] = ref object # same layout idea as CpuStorage, datatypes.nim:24-30
    raw_buffer*: DevicePtr[T]
    memalloc*: pointer
    memowner*: bool

func unsafe_device_data*[T](s: HipStorage[T]): DevicePtr[T] {.inline.} = s.raw_buffer
func offsetBy*[T](p: DevicePtr[T], elements: int): DevicePtr[T] {.inline.} =
  DevicePtr[T](cast[pointer](cast[uint](pointer(p)) + uint(elements * sizeof(T))))

proc finalizer[T](storage: HipStorage[T]) =
  if storage.memowner and not storage.memalloc.isNil:
    discard laser_hip_storage_free(storage.memalloc)

proc allocHipStorage*[T](storage: var HipStorage[T], size: int) =
  ## allocCpuStorage's twin (allocator.nim:17-29): `size` elements, aligned >= LASER_MEM_ALIGN, zero-filled.
  new(storage, finalizer[T])
  check laser_hip_storage_alloc(storage.memalloc.addr, sizeof(T) * size)
  storage.memowner = true
  storage.raw_buffer = DevicePtr[T](storage.memalloc)

proc copyFromRaw*[T](dst: HipStorage[T], buffer: ptr T, len: Natural) =
  ## initialization.nim:112-128 for a device storage (host buffer -> HBM).
  check laser_hip_storage_upload(pointer(dst.raw_buffer), buffer, sizeof(T) * len)

proc copyToRaw*[T](buffer: ptr T, src: HipStorage[T], len: Natural) =
  check laser_hip_storage_download(buffer, pointer(src.raw_buffer), sizeof(T) * len)

proc setZero*[T](s: HipStorage[T], len: Natural) =
  check laser_hip_storage_set_zero(pointer(s.raw_buffer), sizeof(T) * len, nil)

proc copyStrided*[T](dst: DevicePtr[T], dstStrides: openarray[int], src: DevicePtr[T], srcStrides: openarray[int],
                     shape: openarray[int]) =
  ## `forEachStrided d in dst, s in src: d = s` on device buffers (deepCopy / copyFrom of views).
  assert shape.len == dstStrides.len and shape.len == srcStrides.len and shape.len <= 6   # LASER_MAXRANK
  when sizeof(T) == 4:
    check laser_hip_copy_strided_b32_dev(pointer(dst), dstStrides[0].unsafeAddr, pointer(src), srcStrides[0].unsafeAddr,
                                         shape[0].unsafeAddr, cint(shape.len), nil)
  else:
    check laser_hip_copy_strided_b64_dev(pointer(dst), dstStrides[0].unsafeAddr, pointer(src), srcStrides[0].unsafeAddr,
                                         shape[0].unsafeAddr, cint(shape.len), nil)

# ---- mapStrided: the device twin of forEach / forEachStrided (foreach.nim:192-264) ----------------
# dst[idx] = f(a[idx]) / f(a[idx], b[idx]) over rank <= 6 (LASER_MAXRANK) strided views, strides in elements, 0 = broadcast.
type MapOp* = enum
  mapCopy = 0, mapFill = 1, mapNeg = 2, mapAbs = 3, mapRelu = 4, mapScale = 5, mapSquare = 6,
  mapAdd = 32, mapSub = 33, mapMul = 34, mapMax = 36, mapMin = 37, mapAxpy = 38, mapAxpby = 39

proc laser_hip_map_strided_unary_f32_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: float32, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_unary_f32_dev".}
proc laser_hip_map_strided_unary_f64_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: float64, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_unary_f64_dev".}
proc laser_hip_map_strided_unary_i32_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: int32, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_unary_i32_dev".}
proc laser_hip_map_strided_unary_i64_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: int64, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_unary_i64_dev".}
proc laser_hip_map_strided_binary_f32_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, b: pointer, bStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: float32, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_binary_f32_dev".}
proc laser_hip_map_strided_binary_f64_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, b: pointer, bStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: float64, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_binary_f64_dev".}
proc laser_hip_map_strided_binary_i32_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, b: pointer, bStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: int32, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_binary_i32_dev".}
proc laser_hip_map_strided_binary_i64_dev(op: cint, dst: pointer, dstStrides: ptr int, a: pointer, aStrides: ptr int, b: pointer, bStrides: ptr int, shape: ptr int, rank: cint, alpha, beta: int64, stream: pointer): cint {.lh, importc: "laser_hip_map_strided_binary_i64_dev".}

proc mapStrided*[T: float32 or float64 or int32 or int64](op: MapOp, dst: DevicePtr[T], dstStrides: openarray[int],
                 a: DevicePtr[T], aStrides: openarray[int], shape: openarray[int],
                 alpha = T(1), beta = T(0), stream: pointer = nil) =
  ## `forEachStrided d in dst, x in a: d = f(x)` on device buffers (fill: `a` may be a nil DevicePtr).
  assert shape.len == dstStrides.len and shape.len == aStrides.len and shape.len <= 6 and ord(op) < 32
  when T is float32:
    check laser_hip_map_strided_unary_f32_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)
  elif T is float64:
    check laser_hip_map_strided_unary_f64_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)
  elif T is int32:
    check laser_hip_map_strided_unary_i32_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)
  else:
    check laser_hip_map_strided_unary_i64_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)

proc mapStrided*[T: float32 or float64 or int32 or int64](op: MapOp, dst: DevicePtr[T], dstStrides: openarray[int],
                 a: DevicePtr[T], aStrides: openarray[int], b: DevicePtr[T], bStrides: openarray[int],
                 shape: openarray[int], alpha = T(1), beta = T(1), stream: pointer = nil) =
  ## `forEachStrided d in dst, x in a, y in b: d = f(x, y)` on device buffers.
  assert shape.len == dstStrides.len and shape.len == aStrides.len and shape.len == bStrides.len and shape.len <= 6 and ord(op) >= 32
  when T is float32:
    check laser_hip_map_strided_binary_f32_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, pointer(b), bStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)
  elif T is float64:
    check laser_hip_map_strided_binary_f64_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, pointer(b), bStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)
  elif T is int32:
    check laser_hip_map_strided_binary_i32_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, pointer(b), bStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)
  else:
    check laser_hip_map_strided_binary_i64_dev(cint(ord(op)), pointer(dst), dstStrides[0].unsafeAddr, pointer(a), aStrides[0].unsafeAddr, pointer(b), bStrides[0].unsafeAddr, shape[0].unsafeAddr, cint(shape.len), alpha, beta, stream)

# ---- the whole node behind an unchanged gemm_strided call, and pinned host memory ------------------------------------
# Laser parallelises one gemm_strided call over OpenMP threads by ic row blocks (gemm.nim:160-176); here the same row blocks
# go to the GPUs of the node: after `laserHipShardDevices(0)` (0 = every visible GPU, n = that many, 1 = off) the plain
# host-pointer gemm_strided above cuts large problems into one row range per GPU inside the library -- call sites unchanged.
proc laser_hip_set_shard_devices(ndev: cint): cint {.lh, importc: "laser_hip_set_shard_devices".}
proc laser_hip_get_shard_devices(): cint {.lh, importc: "laser_hip_get_shard_devices".}
proc laser_hip_host_alloc(hostPtr: ptr pointer, bytes: int): cint {.lh, importc: "laser_hip_host_alloc".}
proc laser_hip_host_free(hostPtr: pointer): cint {.lh, importc: "laser_hip_host_free".}
proc laser_hip_host_register(hostPtr: pointer, bytes: int): cint {.lh, importc: "laser_hip_host_register".}
proc laser_hip_host_unregister(hostPtr: pointer): cint {.lh, importc: "laser_hip_host_unregister".}

proc laserHipSetOption*(name: string, value: int) = check laser_hip_set_option(cstring(name), cint(value))
proc laserHipGetOption*(name: string): int =
  check laser_hip_get_option(cstring(name), result.addr)
proc laserHipShardDevices*(ndev: int) = check laser_hip_set_shard_devices(cint(ndev))
proc laserHipShardDevices*(): int = int(laser_hip_get_shard_devices())

# ---- one gemm_strided call over every GPU, operands resident in HBM, C all-gathered over xGMI ------------------------
# The device-resident form of the same partition: rows of C are dealt block-cyclically (`shardPlan`), device slot g holds
# its row panels of A, all of B, and the FULL C; with a gather mode every device ends up with all of C -- sub-panel s is
# sent (peer copies on every xGMI link at once, or RCCL's ncclAllGather) while sub-panel s+1 multiplies.  No K split, so
# every element is computed exactly as on one GPU (gemm.nim:160-176 partitions M the same way across threads).
type
  ShardGather* = enum
    gatherNone = 0, gatherPeer = 1, gatherRccl = 2
  ShardPlan* = object
    rowsPerPanel*: int   ## rows of one (sub-panel, device) block; a multiple of 256 when M allows
    panelsPerDev*: int   ## sub-panels per device actually used
    paddedM*: int        ## rows the per-device C buffers must hold for gatherRccl (whole panels)
const shardPinTile* = 1  ## flags: 128x128 tiles for the local products (RCCL's kernels hold CUs meanwhile)

proc laser_hip_shard_plan(M: int, ndev, panelsPerDev: cint, rowsPerPanel: ptr int, panelsPerDevUsed: ptr cint, paddedM: ptr int): cint {.lh, importc: "laser_hip_shard_plan".}
proc laser_hip_gemm_strided_f32_sharded_dev(ndev: cint, devices: ptr cint, M, N, K: int, alpha: float32, dA: ptr pointer, rsA, csA: int, dB: ptr pointer, rsB, csB: int, beta: float32, dC: ptr pointer, rsC: int, panelsPerDev, gather, flags: cint): cint {.lh, importc: "laser_hip_gemm_strided_f32_sharded_dev".}
proc laser_hip_gemm_strided_f64_sharded_dev(ndev: cint, devices: ptr cint, M, N, K: int, alpha: float64, dA: ptr pointer, rsA, csA: int, dB: ptr pointer, rsB, csB: int, beta: float64, dC: ptr pointer, rsC: int, panelsPerDev, gather, flags: cint): cint {.lh, importc: "laser_hip_gemm_strided_f64_sharded_dev".}
proc laser_hip_gemm_strided_i32_sharded_dev(ndev: cint, devices: ptr cint, M, N, K: int, alpha: int32, dA: ptr pointer, rsA, csA: int, dB: ptr pointer, rsB, csB: int, beta: int32, dC: ptr pointer, rsC: int, panelsPerDev, gather, flags: cint): cint {.lh, importc: "laser_hip_gemm_strided_i32_sharded_dev".}
proc laser_hip_gemm_strided_i64_sharded_dev(ndev: cint, devices: ptr cint, M, N, K: int, alpha: int64, dA: ptr pointer, rsA, csA: int, dB: ptr pointer, rsB, csB: int, beta: int64, dC: ptr pointer, rsC: int, panelsPerDev, gather, flags: cint): cint {.lh, importc: "laser_hip_gemm_strided_i64_sharded_dev".}

proc shardPlan*(M, ndev: int, panelsPerDev = 4): ShardPlan =
  var ppd: cint
  check laser_hip_shard_plan(M, cint(ndev), cint(panelsPerDev), result.rowsPerPanel.addr, ppd.addr, result.paddedM.addr)
  result.panelsPerDev = int(ppd)

# (The device-resident sharded call has no stream parameter: it works on the library's own streams, so every operand must be COMPLETE in
# memory when it is made -- a caller that fills its device tensors asynchronously synchronises that stream first.  flags = 1
# (LASER_HIP_SHARD_PIN_TILE): the hand-scheduled 128x128x16 assembly tile for the local float32 products, beside RCCL's kernels.)
proc gemm_strided_sharded*[T: float32 or float64 or int32 or int64](
      devices: openarray[cint],                 ## HIP ordinals, one per device slot
      M, N, K: int, alpha: T,
      A_panels: openarray[DevicePtr[T]],        ## per slot: its row panels of A, stacked in local order
      rowStrideA, colStrideA: int,
      B: openarray[DevicePtr[T]],               ## per slot: B (replicated)
      rowStrideB, colStrideB: int,
      beta: T,
      C: openarray[DevicePtr[T]],               ## per slot: the full row-major C
      rowStrideC: int,
      panelsPerDev = 4, gather = gatherPeer, flags = 0) =
  ## Same arithmetic as `gemm_strided` (bit-identical for every device count); synchronous.
  assert A_panels.len == devices.len and B.len == devices.len and C.len == devices.len
  let n = cint(devices.len)
  let dv = devices[0].unsafeAddr
  let a = cast[ptr pointer](A_panels[0].unsafeAddr)
  let b = cast[ptr pointer](B[0].unsafeAddr)
  let c = cast[ptr pointer](C[0].unsafeAddr)
  when T is float32:
    check laser_hip_gemm_strided_f32_sharded_dev(n, dv, M, N, K, alpha, a, rowStrideA, colStrideA, b, rowStrideB, colStrideB, beta, c, rowStrideC, cint(panelsPerDev), cint(ord(gather)), cint(flags))
  elif T is float64:
    check laser_hip_gemm_strided_f64_sharded_dev(n, dv, M, N, K, alpha, a, rowStrideA, colStrideA, b, rowStrideB, colStrideB, beta, c, rowStrideC, cint(panelsPerDev), cint(ord(gather)), cint(flags))
  elif T is int32:
    check laser_hip_gemm_strided_i32_sharded_dev(n, dv, M, N, K, alpha, a, rowStrideA, colStrideA, b, rowStrideB, colStrideB, beta, c, rowStrideC, cint(panelsPerDev), cint(ord(gather)), cint(flags))
  else:
    check laser_hip_gemm_strided_i64_sharded_dev(n, dv, M, N, K, alpha, a, rowStrideA, colStrideA, b, rowStrideB, colStrideB, beta, c, rowStrideC, cint(panelsPerDev), cint(ord(gather)), cint(flags))
proc allocPinned*[T](len: int): ptr UncheckedArray[T] =
  ## page-locked host memory for operands of the host-pointer calls (what an allocator would hand to Tensor[T])
  var p: pointer
  check laser_hip_host_alloc(p.addr, sizeof(T) * len)
  cast[ptr UncheckedArray[T]](p)
proc freePinned*(p: pointer) = check laser_hip_host_free(p)
proc registerPinned*(p: pointer, bytes: int) = check laser_hip_host_register(p, bytes)
proc unregisterPinned*(p: pointer) = check laser_hip_host_unregister(p)

# gemm_strided on device-resident operands: the SAME parameter list as gemm.nim:184-193 with DevicePtr[T]
# in place of ptr T (overload resolution keeps host and device pointers apart), asynchronous on `stream`.
proc gemm_strided*[T: SomeNumber](
      M, N, K: int,
      alpha: T,
      A: DevicePtr[T],
      rowStrideA, colStrideA: int,
      B: DevicePtr[T],
      rowStrideB, colStrideB: int,
      beta: T,
      C: DevicePtr[T],
      rowStrideC, colStrideC: int,
      stream: pointer = nil) =
  when T is float32:
    check laser_hip_gemm_strided_f32_dev(M, N, K, alpha, pointer(A), rowStrideA, colStrideA, pointer(B), rowStrideB, colStrideB, beta, pointer(C), rowStrideC, colStrideC, stream)
  elif T is float64:
    check laser_hip_gemm_strided_f64_dev(M, N, K, alpha, pointer(A), rowStrideA, colStrideA, pointer(B), rowStrideB, colStrideB, beta, pointer(C), rowStrideC, colStrideC, stream)
  elif T is int32:
    check laser_hip_gemm_strided_i32_dev(M, N, K, alpha, pointer(A), rowStrideA, colStrideA, pointer(B), rowStrideB, colStrideB, beta, pointer(C), rowStrideC, colStrideC, stream)
  elif T is uint32:
    check laser_hip_gemm_strided_i32_dev(M, N, K, cast[int32](alpha), pointer(A), rowStrideA, colStrideA, pointer(B), rowStrideB, colStrideB, cast[int32](beta), pointer(C), rowStrideC, colStrideC, stream)
  elif T is int64 or T is int or T is uint64 or T is uint:
    check laser_hip_gemm_strided_i64_dev(M, N, K, cast[int64](alpha), pointer(A), rowStrideA, colStrideA, pointer(B), rowStrideB, colStrideB, cast[int64](beta), pointer(C), rowStrideC, colStrideC, stream)
  elif T is int8 or T is uint8:
    check laser_hip_gemm_strided_i8_dev(M, N, K, int32(cast[int8](alpha)), pointer(A), rowStrideA, colStrideA, pointer(B), rowStrideB, colStrideB, int32(cast[int8](beta)), pointer(C), rowStrideC, colStrideC, stream)
  elif T is int16 or T is uint16:
    check laser_hip_gemm_strided_i16_dev(M, N, K, int32(cast[int16](alpha)), pointer(A), rowStrideA, colStrideA, pointer(B), rowStrideB, colStrideB, int32(cast[int16](beta)), pointer(C), rowStrideC, colStrideC, stream)
  else:
    {.error: "laser_hip: unsupported element type " & $T.}

# ---- forEach with a body (include/laser_hip.h "forEach with a body"): foreach.nim:192-264 on device buffers ----------
# The body is HIP C++ compiled at run time (Laser's `x += y * z` statements are valid C++).  Translating a Nim AST body
# to C++ is not done here: the body is a string.
proc laser_hip_foreach_source(body: cstring, nops: cint, names: ptr cstring, dtypes: ptr cint, writable: ptr cint, nparams: cint, paramNames: ptr cstring, paramDtypes: ptr cint, buf: pointer, cap: int64, len: ptr int64): cint {.lh, importc: "laser_hip_foreach_source".}
proc laser_hip_foreach_code(body: cstring, nops: cint, names: ptr cstring, dtypes: ptr cint, writable: ptr cint, nparams: cint, paramNames: ptr cstring, paramDtypes: ptr cint, arch: cstring, buf: pointer, cap: int64, len: ptr int64): cint {.lh, importc: "laser_hip_foreach_code".}
proc laser_hip_foreach_kernel(body: cstring, nops: cint, names: ptr cstring, dtypes: ptr cint, writable: ptr cint, nparams: cint, paramNames: ptr cstring, paramDtypes: ptr cint, handle: ptr int64): cint {.lh, importc: "laser_hip_foreach_kernel".}
proc laser_hip_foreach_dev(handle: int64, ptrs: ptr pointer, strides: ptr int64, shape: ptr int64, rank: cint, params: pointer, stream: pointer): cint {.lh, importc: "laser_hip_foreach_dev".}

type
  ForEachOperand* = object
    name*: string
    dtype*: cint                 # LASER_HIP_DT_*
    writable*: bool
    data*: pointer               # a device address
    strides*: seq[int]           # element strides over the iteration shape (0 = broadcast, read-only operands only)
  ForEachParam* = object
    name*: string
    dtype*: cint
    slot*: uint64                # the value in the low bytes

func dtypeCode*(T: typedesc): cint =
  when T is float32: 0
  elif T is float64: 1
  elif T is int8: 2
  elif T is int16: 3
  elif T is int32: 4
  elif T is int64 or T is int: 5
  elif T is uint8: 6
  elif T is uint16: 7
  elif T is uint32: 8
  elif T is uint64 or T is uint: 9
  else: {.error: "laser_hip: unsupported element type " & $T.}

func operand*[T](name: string, p: DevicePtr[T], strides: openarray[int], writable = false): ForEachOperand =
  ForEachOperand(name: name, dtype: dtypeCode(T), writable: writable, data: pointer(p), strides: @strides)

func param*[T: SomeNumber](name: string, value: T): ForEachParam =
  result = ForEachParam(name: name, dtype: dtypeCode(T))
  copyMem(result.slot.addr, value.unsafeAddr, sizeof(T))

proc forEachDevice*(body: string, operands: openarray[ForEachOperand], shape: openarray[int],
                    params: openarray[ForEachParam] = [], stream: pointer = nil) =
  ## `forEach x in a, y in b: <body>` over device buffers: every operand has one stride per dimension of `shape`.
  doAssert operands.len >= 1 and shape.len >= 1, "forEachDevice: at least one operand and one dimension"
  var names, pnames: seq[cstring]
  var dtypes, writable, pdtypes: seq[cint]
  var ptrs: seq[pointer]
  var strides: seq[int64]
  var slots: seq[uint64]
  for o in operands:
    doAssert o.strides.len == shape.len, "forEachDevice: operand " & o.name & " needs one stride per dimension"
    names.add cstring(o.name)
    dtypes.add o.dtype
    writable.add cint(ord(o.writable))
    ptrs.add o.data
    for s in o.strides: strides.add int64(s)
  for p in params:
    pnames.add cstring(p.name)
    pdtypes.add p.dtype
    slots.add p.slot
  pnames.add nil   # keeps [0] addressable without parameters
  pdtypes.add 0
  slots.add 0
  var handle: int64
  check laser_hip_foreach_kernel(cstring(body), cint(operands.len), names[0].addr, dtypes[0].addr, writable[0].addr,
                                 cint(params.len), pnames[0].addr, pdtypes[0].addr, handle.addr)
  var shp = newSeq[int64](shape.len)
  for i, s in shape: shp[i] = int64(s)
  check laser_hip_foreach_dev(handle, ptrs[0].addr, strides[0].addr, shp[0].addr, cint(shape.len), slots[0].addr, stream)

# ---- Reductions (include/laser_hip.h "Reductions"): reductions.nim:48-116 -----------------------------------------------
# The order of the operations is fixed -- a function of the element count alone -- so, unlike the reference's OpenMP sum,
# the same input gives the same bits on every run.  min / max: any NaN gives NaN, -0 ranks below +0.
proc laser_hip_reduce_sum_f32(data: ptr float32, len: int64, res: ptr float32): cint {.lh, importc: "laser_hip_reduce_sum_f32".}
proc laser_hip_reduce_min_f32(data: ptr float32, len: int64, res: ptr float32): cint {.lh, importc: "laser_hip_reduce_min_f32".}
proc laser_hip_reduce_max_f32(data: ptr float32, len: int64, res: ptr float32): cint {.lh, importc: "laser_hip_reduce_max_f32".}
# device views (asynchronous on `stream`, the result to the device address `res`)
proc laser_hip_reduce_sum_f32_dev*(src: ptr float32, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr float32, stream: pointer): cint {.lh, importc: "laser_hip_reduce_sum_f32_dev".}
proc laser_hip_reduce_min_f32_dev*(src: ptr float32, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr float32, stream: pointer): cint {.lh, importc: "laser_hip_reduce_min_f32_dev".}
proc laser_hip_reduce_max_f32_dev*(src: ptr float32, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr float32, stream: pointer): cint {.lh, importc: "laser_hip_reduce_max_f32_dev".}
proc laser_hip_reduce_sum_f64_dev*(src: ptr float64, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr float64, stream: pointer): cint {.lh, importc: "laser_hip_reduce_sum_f64_dev".}
proc laser_hip_reduce_min_f64_dev*(src: ptr float64, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr float64, stream: pointer): cint {.lh, importc: "laser_hip_reduce_min_f64_dev".}
proc laser_hip_reduce_max_f64_dev*(src: ptr float64, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr float64, stream: pointer): cint {.lh, importc: "laser_hip_reduce_max_f64_dev".}
proc laser_hip_reduce_sum_i32_dev*(src: ptr int32, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr int32, stream: pointer): cint {.lh, importc: "laser_hip_reduce_sum_i32_dev".}
proc laser_hip_reduce_min_i32_dev*(src: ptr int32, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr int32, stream: pointer): cint {.lh, importc: "laser_hip_reduce_min_i32_dev".}
proc laser_hip_reduce_max_i32_dev*(src: ptr int32, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr int32, stream: pointer): cint {.lh, importc: "laser_hip_reduce_max_i32_dev".}
proc laser_hip_reduce_sum_i64_dev*(src: ptr int64, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr int64, stream: pointer): cint {.lh, importc: "laser_hip_reduce_sum_i64_dev".}
proc laser_hip_reduce_min_i64_dev*(src: ptr int64, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr int64, stream: pointer): cint {.lh, importc: "laser_hip_reduce_min_i64_dev".}
proc laser_hip_reduce_max_i64_dev*(src: ptr int64, strides: ptr int64, shape: ptr int64, rank: cint, res: ptr int64, stream: pointer): cint {.lh, importc: "laser_hip_reduce_max_i64_dev".}

proc reduce_sum*(data: ptr (float32 or UncheckedArray[float32]), len: Natural): float32 =
  ## reductions.nim:91-96: sum of a contiguous range of float32 (host memory; the GPU computes it)
  check laser_hip_reduce_sum_f32(cast[ptr float32](data), int64(len), result.addr)

proc reduce_min*(data: ptr (float32 or UncheckedArray[float32]), len: Natural): float32 =
  ## reductions.nim:98-103 (+Inf when len = 0)
  check laser_hip_reduce_min_f32(cast[ptr float32](data), int64(len), result.addr)

proc reduce_max*(data: ptr (float32 or UncheckedArray[float32]), len: Natural): float32 =
  ## reductions.nim:105-110 (-Inf when len = 0)
  check laser_hip_reduce_max_f32(cast[ptr float32](data), int64(len), result.addr)

# ---- exp and row softmax (include/laser_hip.h "exp and row softmax"): simd_math/exp_log_*.nim ---------------------------
# exp is Laser's table-driven exp, bit for bit the exported SIMD forms; softmax sums in the fixed order of the reductions.
proc laser_hip_exp_f32(dst: ptr float32, src: ptr float32, len: int64): cint {.lh, importc: "laser_hip_exp_f32".}
# device views (asynchronous on `stream`): element strides, rank <= 6; dst may be src
proc laser_hip_exp_f32_dev*(dst: ptr float32, dstStrides: ptr int64, src: ptr float32, srcStrides: ptr int64, shape: ptr int64, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_exp_f32_dev".}
proc laser_hip_softmax_rows_f32_dev*(dst: ptr float32, dstRowStride: int64, src: ptr float32, srcRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_softmax_rows_f32_dev".}
proc laser_hip_softmax_axis_f32_dev*(dst: ptr float32, dstOuterStride: int64, dstAxisStride: int64, src: ptr float32, srcOuterStride: int64, srcAxisStride: int64, outer: int64, n: int64, inner: int64, stream: pointer): cint {.lh, importc: "laser_hip_softmax_axis_f32_dev".}
proc laser_hip_softmax_axis_plan*(outer: int64, n: int64, inner: int64, vec: cint, cus: cint, out4: ptr int64): cint {.lh, importc: "laser_hip_softmax_axis_plan".}

proc exp*(dst, src: ptr (float32 or UncheckedArray[float32]), len: Natural) =
  ## exp_log_avx2.nim:49-65 over a contiguous range of float32 (host memory; the GPU computes it): dst[i] = exp(src[i])
  check laser_hip_exp_f32(cast[ptr float32](dst), cast[ptr float32](src), int64(len))

proc softmax*(dst: DevicePtr[float32], dstRowStride: int, src: DevicePtr[float32], srcRowStride: int, rows, n: Natural, stream: pointer = nil) =
  ## softmax over the rows of a device matrix (row elements contiguous, row strides in elements); dst may be src
  check laser_hip_softmax_rows_f32_dev(cast[ptr float32](dst), int64(dstRowStride), cast[ptr float32](src), int64(srcRowStride), int64(rows), int64(n), stream)

proc softmaxAxis*(dst: DevicePtr[float32], dstOuterStride, dstAxisStride: int, src: DevicePtr[float32], srcOuterStride, srcAxisStride: int, outer, n, inner: Natural, stream: pointer = nil) =
  ## softmax along the middle axis of a device operand viewed as (outer, n, inner): element (o, k, i) at
  ## o * outerStride + k * axisStride + i (element strides); every column bit for bit what `softmax` gives it as a row
  check laser_hip_softmax_axis_f32_dev(cast[ptr float32](dst), int64(dstOuterStride), int64(dstAxisStride), cast[ptr float32](src), int64(srcOuterStride), int64(srcAxisStride), int64(outer), int64(n), int64(inner), stream)

# ---- log, logsumexp, log-softmax and cross-entropy (include/laser_hip.h, the section of that name) ------------------------
# log is llog of log_core.h: faithful and monotone over every positive float32.  The row procs use exactly the maximum and the
# sum of `softmax`.
proc laser_hip_log_f32(dst: ptr float32, src: ptr float32, len: int64): cint {.lh, importc: "laser_hip_log_f32".}
proc laser_hip_log_f32_dev*(dst: ptr float32, dstStrides: ptr int64, src: ptr float32, srcStrides: ptr int64, shape: ptr int64, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_log_f32_dev".}
proc laser_hip_logsumexp_rows_f32_dev*(dst: ptr float32, dstStride: int64, src: ptr float32, srcRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_logsumexp_rows_f32_dev".}
proc laser_hip_log_softmax_rows_f32_dev*(dst: ptr float32, dstRowStride: int64, src: ptr float32, srcRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_log_softmax_rows_f32_dev".}
proc laser_hip_softmax_xent_rows_f32_dev*(loss: ptr float32, lossStride: int64, grad: ptr float32, gradRowStride: int64, src: ptr float32, srcRowStride: int64, labels: ptr int32, rows: int64, n: int64, scale: float32, stream: pointer): cint {.lh, importc: "laser_hip_softmax_xent_rows_f32_dev".}
proc laser_hip_softmax_rows_plan*(rows: int64, n: int64, vec: cint, out3: ptr int64): cint {.lh, importc: "laser_hip_softmax_rows_plan".}

proc log*(dst, src: ptr (float32 or UncheckedArray[float32]), len: Natural) =
  ## dst[i] = ln(src[i]) over a contiguous range of float32 (host memory; the GPU computes it)
  check laser_hip_log_f32(cast[ptr float32](dst), cast[ptr float32](src), int64(len))

proc logsumexp*(dst: DevicePtr[float32], dstStride: int, src: DevicePtr[float32], srcRowStride: int, rows, n: Natural, stream: pointer = nil) =
  ## dst[row * dstStride] = max + ln(sum of exp(x - max)) of each row of a device matrix (row elements contiguous)
  check laser_hip_logsumexp_rows_f32_dev(cast[ptr float32](dst), int64(dstStride), cast[ptr float32](src), int64(srcRowStride), int64(rows), int64(n), stream)

proc logSoftmax*(dst: DevicePtr[float32], dstRowStride: int, src: DevicePtr[float32], srcRowStride: int, rows, n: Natural, stream: pointer = nil) =
  ## y = (x - max) - ln(sum) over the rows of a device matrix; dst may be src
  check laser_hip_log_softmax_rows_f32_dev(cast[ptr float32](dst), int64(dstRowStride), cast[ptr float32](src), int64(srcRowStride), int64(rows), int64(n), stream)

proc softmaxCrossEntropy*(loss: DevicePtr[float32], lossStride: int, grad: DevicePtr[float32], gradRowStride: int, src: DevicePtr[float32], srcRowStride: int, labels: DevicePtr[int32], rows, n: Natural, scale: float32 = 1'f32, stream: pointer = nil) =
  ## Arraymancer's sparse_softmax_cross_entropy and its gradient in one launch: loss per row and (softmax - onehot) * scale;
  ## loss or grad may be nil (not both); label -1 is ignored, any other label outside 0 ..< n gives NaN
  check laser_hip_softmax_xent_rows_f32_dev(cast[ptr float32](loss), int64(lossStride), cast[ptr float32](grad), int64(gradRowStride), cast[ptr float32](src), int64(srcRowStride), cast[ptr int32](labels), int64(rows), int64(n), scale, stream)

# ---- activations (include/laser_hip.h "Activations"): relu, tanh, sigmoid and their gradients from the output -----------
# tanh and sigmoid are ltanh and lsigmoid of act_core.h: faithful, monotone, tanh odd bit for bit, sigmoid(0) = 0.5; relu is the
# fused epilogue's rule (x > 0 ? x : +0).  `Activation` is the enum of the fused epilogue; actNone is not accepted here.
proc laser_hip_act_f32(act: cint, dst: ptr float32, src: ptr float32, len: int64): cint {.lh, importc: "laser_hip_act_f32".}
proc laser_hip_act_f32_dev*(act: cint, dst: ptr float32, dstStrides: ptr int64, src: ptr float32, srcStrides: ptr int64, shape: ptr int64, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_act_f32_dev".}
proc laser_hip_act_grad_f32_dev*(act: cint, dx: ptr float32, dxStrides: ptr int64, dy: ptr float32, dyStrides: ptr int64, y: ptr float32, yStrides: ptr int64, shape: ptr int64, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_act_grad_f32_dev".}

proc tanh*(dst, src: ptr (float32 or UncheckedArray[float32]), len: Natural) =
  ## dst[i] = tanh(src[i]) over a contiguous range of float32 (host memory; the GPU computes it)
  check laser_hip_act_f32(cint(ord(actTanh)), cast[ptr float32](dst), cast[ptr float32](src), int64(len))

proc sigmoid*(dst, src: ptr (float32 or UncheckedArray[float32]), len: Natural) =
  ## dst[i] = 1 / (1 + exp(-src[i])) over a contiguous range of float32 (host memory; the GPU computes it)
  check laser_hip_act_f32(cint(ord(actSigmoid)), cast[ptr float32](dst), cast[ptr float32](src), int64(len))

proc activation*(kind: Activation, dst, src: DevicePtr[float32], len: Natural, stream: pointer = nil) =
  ## dst[i] = kind(src[i]) over `len` contiguous device elements; dst may be src
  var stride = 1'i64
  var n = int64(len)
  check laser_hip_act_f32_dev(cint(ord(kind)), cast[ptr float32](dst), stride.addr, cast[ptr float32](src), stride.addr, n.addr, 1, stream)

proc activationGrad*(kind: Activation, dx, dy, y: DevicePtr[float32], len: Natural, stream: pointer = nil) =
  ## the gradient of `kind` from dy and the forward OUTPUT y over `len` contiguous device elements: relu y > 0 ? dy : 0,
  ## tanh dy * (1 - y * y), sigmoid dy * (y * (1 - y)), each float32 operation rounded on its own; dx may be dy or y
  var stride = 1'i64
  var n = int64(len)
  check laser_hip_act_grad_f32_dev(cint(ord(kind)), cast[ptr float32](dx), stride.addr, cast[ptr float32](dy), stride.addr, cast[ptr float32](y), stride.addr, n.addr, 1, stream)

# ---- dense-layer backward (include/laser_hip.h "Dense-layer backward"): dZ = dY * f'(Y) and the bias gradient in one pass --
# dz by activationGrad's rule (actNone: dz = dy, y may be nil), db[j] = reduce_sum of column j of dz; row-major (rows, n)
# device matrices with unit column stride, row strides in elements
proc laser_hip_bias_grad_f32_dev*(db: ptr float32, dbStride: int64, dz: ptr float32, dzRowStride: int64, dy: ptr float32, dyRowStride: int64, y: ptr float32, yRowStride: int64, rows: int64, n: int64, act: cint, stream: pointer): cint {.lh, importc: "laser_hip_bias_grad_f32_dev".}
proc laser_hip_bias_grad_plan*(rows: int64, n: int64, vec: cint, cus: cint, out4: ptr int64): cint {.lh, importc: "laser_hip_bias_grad_plan".}
proc laser_hip_bias_grad_last_kernel*(): cint {.lh, importc: "laser_hip_bias_grad_last_kernel".}

proc biasGrad*(kind: Activation, db: DevicePtr[float32], dbStride: int, dz: DevicePtr[float32], dzRowStride: int, dy: DevicePtr[float32], dyRowStride: int, y: DevicePtr[float32], yRowStride: int, rows, n: Natural, stream: pointer = nil) =
  ## dz[r, j] = the gradient of `kind` from dy[r, j] and the forward OUTPUT y[r, j] (activationGrad's bits) and
  ## db[j * dbStride] = the sum of dz[0 ..< rows, j] in the order of reduce_sum over that column; dz may be nil (only db),
  ## dy or y (equal row strides); rows <= 2^26
  check laser_hip_bias_grad_f32_dev(cast[ptr float32](db), int64(dbStride), cast[ptr float32](dz), int64(dzRowStride), cast[ptr float32](dy), int64(dyRowStride), cast[ptr float32](y), int64(yRowStride), int64(rows), int64(n), cint(ord(kind)), stream)

proc linearBackward*(kind: Activation, dx, dw, db, dz: DevicePtr[float32], x, w, dy, y: DevicePtr[float32], M, K, N: Natural, stream: pointer = nil) =
  ## the gradients of the layer Y = kind(X W + b) with row-major X (M, K), W (K, N), dY and Y (M, N): one biasGrad call writes
  ## dz (M, N; may be dy) and db (N), then dw (K, N) = X^T dZ and dx (M, K) = dZ W^T on gemm_strided, the transposes as
  ## strides; dx may be nil (the first layer of a network)
  biasGrad(kind, db, 1, dz, N, dy, N, y, N, M, N, stream)
  gemm_strided(K, N, M, 1'f32, x, 1, K, dz, N, 1, 0'f32, dw, N, 1, stream)
  if not pointer(dx).isNil:
    gemm_strided(M, K, N, 1'f32, dz, N, 1, w, 1, N, 0'f32, dx, K, 1, stream)

# ---- layer normalization (include/laser_hip.h "Layer normalization"): forward and backward over the rows of a matrix -------
# every float32 operation rounded on its own, every sum in reduce_sum's order; row-major (rows, n) device matrices with unit
# column stride, strides in elements; gamma, beta, mean and rstd may be nil where the header says so
proc laser_hip_layer_norm_f32_dev*(y: ptr float32, yRowStride: int64, mean: ptr float32, meanStride: int64, rstd: ptr float32, rstdStride: int64, x: ptr float32, xRowStride: int64, gamma: ptr float32, gammaStride: int64, beta: ptr float32, betaStride: int64, rows: int64, n: int64, eps: float32, stream: pointer): cint {.lh, importc: "laser_hip_layer_norm_f32_dev".}
proc laser_hip_layer_norm_grad_f32_dev*(dx: ptr float32, dxRowStride: int64, dgamma: ptr float32, dgammaStride: int64, dbeta: ptr float32, dbetaStride: int64, dy: ptr float32, dyRowStride: int64, x: ptr float32, xRowStride: int64, mean: ptr float32, meanStride: int64, rstd: ptr float32, rstdStride: int64, gamma: ptr float32, gammaStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_layer_norm_grad_f32_dev".}
proc laser_hip_layer_norm_plan*(rows: int64, n: int64, vec: cint, what: cint, outp: ptr int64): cint {.lh, importc: "laser_hip_layer_norm_plan".}
proc laser_hip_layer_norm_last_kernel*(what: cint): cint {.lh, importc: "laser_hip_layer_norm_last_kernel".}

proc layerNorm*(y, mean, rstd: DevicePtr[float32], x, gamma, beta: DevicePtr[float32], rows, n: Natural, eps: float32 = 1e-5'f32, stream: pointer = nil) =
  ## y[r, j] = ((x[r, j] - mean[r]) * rstd[r]) * gamma[j] + beta[j] with mean = rsum(x) / n and rstd = 1 / sqrt(var + eps) of
  ## row r; contiguous rows; mean and rstd (the statistics layerNormBackward needs), gamma and beta may be nil; y may be x
  check laser_hip_layer_norm_f32_dev(cast[ptr float32](y), int64(n), cast[ptr float32](mean), 1, cast[ptr float32](rstd), 1, cast[ptr float32](x), int64(n), cast[ptr float32](gamma), 1, cast[ptr float32](beta), 1, int64(rows), int64(n), eps, stream)

proc layerNormBackward*(dx, dgamma, dbeta: DevicePtr[float32], dy, x, mean, rstd, gamma: DevicePtr[float32], rows, n: Natural, stream: pointer = nil) =
  ## dx (rows, n), dgamma (n) and dbeta (n) from dy, the forward input x and the saved mean and rstd; each of the three may be
  ## nil (not wanted) but not all; gamma may be nil; dx may be dy or x; rows <= 2^26 with a parameter gradient
  check laser_hip_layer_norm_grad_f32_dev(cast[ptr float32](dx), int64(n), cast[ptr float32](dgamma), 1, cast[ptr float32](dbeta), 1, cast[ptr float32](dy), int64(n), cast[ptr float32](x), int64(n), cast[ptr float32](mean), 1, cast[ptr float32](rstd), 1, cast[ptr float32](gamma), 1, int64(rows), int64(n), stream)

# ---- the softmax gradient and attention (include/laser_hip.h "Softmax gradient", "Attention") -------------------------------
# the gradient of the row softmax from its OUTPUT; the fused attention forward O = softmax(scale * Q K^T) V with the scores
# never in global memory; and the backward composed from the forward's P, the softmax gradient and the batched GEMM
proc laser_hip_softmax_grad_rows_f32_dev*(dx: ptr float32, dxRowStride: int64, dy: ptr float32, dyRowStride: int64, y: ptr float32, yRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_softmax_grad_rows_f32_dev".}
proc laser_hip_softmax_grad_plan*(rows: int64, n: int64, vec: cint, out3: ptr int64): cint {.lh, importc: "laser_hip_softmax_grad_plan".}
proc laser_hip_softmax_grad_last_kernel*(): cint {.lh, importc: "laser_hip_softmax_grad_last_kernel".}
proc laser_hip_attention_f32_dev*(o: ptr float32, oStrides: ptr int64, q: ptr float32, qStrides: ptr int64, k: ptr float32, kStrides: ptr int64, v: ptr float32, vStrides: ptr int64, probs: ptr float32, probsStrides: ptr int64, rowMax: ptr float32, rowSum: ptr float32, batch: int64, heads: int64, tq: int64, tk: int64, d: int64, dv: int64, scale: float32, causal: cint, stream: pointer): cint {.lh, importc: "laser_hip_attention_f32_dev".}
proc laser_hip_attention_plan*(bh: int64, tq: int64, tk: int64, d: int64, dv: int64, causal: cint, vec: cint, out5: ptr int64): cint {.lh, importc: "laser_hip_attention_plan".}
proc laser_hip_attention_last_kernel*(): cint {.lh, importc: "laser_hip_attention_last_kernel".}
proc laser_hip_gemm_strided_batched_f32_dev(batch, M, N, K: int, alpha: float32, A: pointer, rsA, csA, bsA: int, B: pointer, rsB, csB, bsB: int, beta: float32, C: pointer, rsC, csC, bsC: int, stream: pointer): cint {.lh, importc: "laser_hip_gemm_strided_batched_f32_dev".}

proc softmaxBackward*(dx: DevicePtr[float32], dxRowStride: int, dy: DevicePtr[float32], dyRowStride: int, y: DevicePtr[float32], yRowStride: int, rows, n: Natural, stream: pointer = nil) =
  ## dx[r, j] = y[r, j] * (dy[r, j] - D[r]) with D[r] = the sum of the rounded products dy[r, :] * y[r, :] in the order of
  ## reduce_sum; y is the softmax's OUTPUT; dx may be dy or y (equal row strides); 1 <= n <= 2^26
  check laser_hip_softmax_grad_rows_f32_dev(cast[ptr float32](dx), int64(dxRowStride), cast[ptr float32](dy), int64(dyRowStride), cast[ptr float32](y), int64(yRowStride), int64(rows), int64(n), stream)

from std/math import sqrt
proc attentionDefaultScale*(d: Natural): float32 = float32(1.0 / sqrt(float64(d)))

proc attention*(o, probs, rowMax, rowSum: DevicePtr[float32], q, k, v: DevicePtr[float32], bh, tq, tk, d, dv: Natural, scale: float32, causal = false, stream: pointer = nil) =
  ## contiguous row-major slices: q (bh, tq, d), k (bh, tk, d), v (bh, tk, dv) -> o (bh, tq, dv), probs (bh, tq, tk), rowMax and
  ## rowSum (bh, tq); each output may be nil (not wanted) but not all; with o nil the P V sweep is skipped.  causal: row i sees
  ## keys [0, i + (tk - tq) + 1), tq <= tk.  1 <= d, dv <= 128, 1 <= tk <= 65536.  Views of other strides (slices of a fused
  ## (B, T, 3, H, d) projection) go through laser_hip_attention_f32_dev with their {batch, head, position} strides.
  var os = [int64(tq * dv), 0'i64, int64(dv)]
  var qs = [int64(tq * d), 0'i64, int64(d)]
  var ks = [int64(tk * d), 0'i64, int64(d)]
  var vs = [int64(tk * dv), 0'i64, int64(dv)]
  var ps = [int64(tq * tk), 0'i64, int64(tk)]
  check laser_hip_attention_f32_dev(cast[ptr float32](o), addr os[0], cast[ptr float32](q), addr qs[0], cast[ptr float32](k), addr ks[0], cast[ptr float32](v), addr vs[0], cast[ptr float32](probs), addr ps[0], cast[ptr float32](rowMax), cast[ptr float32](rowSum), int64(bh), 1, int64(tq), int64(tk), int64(d), int64(dv), scale, cint(ord(causal)), stream)

proc attentionBackward*(dq, dk, dvOut: DevicePtr[float32], probs, ds: DevicePtr[float32], dout, q, k, v: DevicePtr[float32], bh, tq, tk, d, dv: Natural, scale: float32, causal = false, stream: pointer = nil) =
  ## the gradients of `attention` for contiguous slices, as the header composes them: probs (bh, tq, tk) <- P from the forward
  ## kernel; dvOut = P^T dO; ds (bh, tq, tk) <- dO V^T, then softmaxBackward in place; dq = scale * (dS K); dk = scale * (dS^T Q)
  ## on gemm_strided_batched in the current float mode, the transposes as strides.  probs and ds are scratch of bh * tq * tk
  ## floats each; dq, dk and dvOut may each be nil (not wanted)
  attention(DevicePtr[float32](nil), probs, DevicePtr[float32](nil), DevicePtr[float32](nil), q, k, v, bh, tq, tk, d, dv, scale, causal, stream)
  if not pointer(dvOut).isNil:
    check laser_hip_gemm_strided_batched_f32_dev(bh, tk, dv, tq, 1'f32, pointer(probs), 1, tk, tq * tk, pointer(dout), dv, 1, tq * dv, 0'f32, pointer(dvOut), dv, 1, tk * dv, stream)
  if pointer(dq).isNil and pointer(dk).isNil: return
  check laser_hip_gemm_strided_batched_f32_dev(bh, tq, tk, dv, 1'f32, pointer(dout), dv, 1, tq * dv, pointer(v), 1, dv, tk * dv, 0'f32, pointer(ds), tk, 1, tq * tk, stream)
  softmaxBackward(ds, tk, ds, tk, probs, tk, bh * tq, tk, stream)
  if not pointer(dq).isNil:
    check laser_hip_gemm_strided_batched_f32_dev(bh, tq, d, tk, scale, pointer(ds), tk, 1, tq * tk, pointer(k), d, 1, tk * d, 0'f32, pointer(dq), d, 1, tq * d, stream)
  if not pointer(dk).isNil:
    check laser_hip_gemm_strided_batched_f32_dev(bh, tk, d, tq, scale, pointer(ds), 1, tk, tq * tk, pointer(q), d, 1, tq * d, 0'f32, pointer(dk), d, 1, tk * d, stream)

# ---- embedding (include/laser_hip.h "Embedding"): row gather by int32 ids, stable grouping, deterministic gradient --------
# row-major device matrices with unit column stride, contiguous rows; ids are int32 (-1: a row of +0 and no gradient; any
# other id outside [0, vocab): a row of NaN and no gradient)
proc laser_hip_embedding_f32_dev*(y: ptr float32, yRowStride: int64, w: ptr float32, wRowStride: int64, idx: ptr int32, tokens: int64, vocab: int64, dim: int64, stream: pointer): cint {.lh, importc: "laser_hip_embedding_f32_dev".}
proc laser_hip_embedding_group_i32_dev*(order: ptr int32, starts: ptr int32, idx: ptr int32, tokens: int64, vocab: int64, stream: pointer): cint {.lh, importc: "laser_hip_embedding_group_i32_dev".}
proc laser_hip_embedding_grad_f32_dev*(dw: ptr float32, dwRowStride: int64, dy: ptr float32, dyRowStride: int64, idx: ptr int32, order: ptr int32, starts: ptr int32, tokens: int64, vocab: int64, dim: int64, stream: pointer): cint {.lh, importc: "laser_hip_embedding_grad_f32_dev".}
proc laser_hip_embedding_plan*(tokens: int64, vocab: int64, dim: int64, vec: cint, cus: cint, out8: ptr int64): cint {.lh, importc: "laser_hip_embedding_plan".}
proc laser_hip_embedding_last_kernel*(what: cint): cint {.lh, importc: "laser_hip_embedding_last_kernel".}

proc embedding*(y: DevicePtr[float32], w: DevicePtr[float32], idx: DevicePtr[int32], tokens, vocab, dim: Natural, stream: pointer = nil) =
  ## y[t, :] = w[idx[t], :], a bit copy; y is (tokens, dim), w is (vocab, dim)
  check laser_hip_embedding_f32_dev(cast[ptr float32](y), int64(dim), cast[ptr float32](w), int64(dim), cast[ptr int32](idx), int64(tokens), int64(vocab), int64(dim), stream)

proc embeddingGroup*(order, starts: DevicePtr[int32], idx: DevicePtr[int32], tokens, vocab: Natural, stream: pointer = nil) =
  ## the stable grouping of the positions by id: order (tokens) and starts (vocab + 1); id v owns order[starts[v] ..< starts[v + 1]]
  check laser_hip_embedding_group_i32_dev(cast[ptr int32](order), cast[ptr int32](starts), cast[ptr int32](idx), int64(tokens), int64(vocab), stream)

proc embeddingBackward*(dw: DevicePtr[float32], dy: DevicePtr[float32], idx: DevicePtr[int32], order, starts: DevicePtr[int32], tokens, vocab, dim: Natural, stream: pointer = nil) =
  ## dw[v, :] = the sum of dy[t, :] over the tokens of id v in reduce_sum's order; order and starts are embeddingGroup's, or
  ## both nil (the call groups by itself)
  check laser_hip_embedding_grad_f32_dev(cast[ptr float32](dw), int64(dim), cast[ptr float32](dy), int64(dim), cast[ptr int32](idx), cast[ptr int32](order), cast[ptr int32](starts), int64(tokens), int64(vocab), int64(dim), stream)

# ---- optimizer steps (include/laser_hip.h "Optimizer steps"): multi-tensor SGD and Adam, the global gradient norm -----------
# the lists are host arrays of device pointers, tensor k is lens[k] contiguous floats; every float32 operation is rounded on
# its own (laser_amd/csrc/optim_core.h); the clip factor of gradNorm is read by the step kernels on the device
proc laser_hip_sgd_step_f32_dev*(w: ptr ptr float32, g: ptr ptr float32, m: ptr ptr float32, lens: ptr int64, count: cint, lr: float32, mu: float32, wd: float32, nesterov: cint, gscale: float32, clip: ptr float32, stream: pointer): cint {.lh, importc: "laser_hip_sgd_step_f32_dev".}
proc laser_hip_adam_step_f32_dev*(w: ptr ptr float32, g: ptr ptr float32, m: ptr ptr float32, v: ptr ptr float32, lens: ptr int64, count: cint, lr: float32, b1: float32, b2: float32, eps: float32, wd: float32, decoupled: cint, bc1: float32, bc2: float32, gscale: float32, clip: ptr float32, stream: pointer): cint {.lh, importc: "laser_hip_adam_step_f32_dev".}
proc laser_hip_grad_norm_f32_dev*(norm: ptr float32, clip: ptr float32, g: ptr ptr float32, lens: ptr int64, count: cint, maxNorm: float32, stream: pointer): cint {.lh, importc: "laser_hip_grad_norm_f32_dev".}
proc laser_hip_adam_bias_correction*(beta: float32, step: int64, outp: ptr float32): cint {.lh, importc: "laser_hip_adam_bias_correction".}
proc laser_hip_optim_plan*(what: cint, lens: ptr int64, count: cint, outp: ptr int64): cint {.lh, importc: "laser_hip_optim_plan".}

proc optimList(list: openArray[DevicePtr[float32]]): ptr ptr float32 =
  if list.len == 0: nil else: cast[ptr ptr float32](unsafeAddr list[0])

proc adamBiasCorrection*(beta: float32, step: int64): float32 =
  ## 1 - beta^step (step >= 1) as the float32 every mirror uses: no device needed
  check laser_hip_adam_bias_correction(beta, step, addr result)

proc sgdStep*(w, g: openArray[DevicePtr[float32]], m: openArray[DevicePtr[float32]], lens: openArray[int64], lr: float32, mu: float32 = 0, wd: float32 = 0, nesterov = false, gscale: float32 = 1, clip: DevicePtr[float32] = DevicePtr[float32](nil), stream: pointer = nil) =
  ## one SGD step on every tensor of the list, in place; m empty: no momentum (mu = 0 and no nesterov); clip: gradNorm's factor or nil
  doAssert w.len == lens.len and g.len == lens.len and (m.len == 0 or m.len == lens.len)
  check laser_hip_sgd_step_f32_dev(optimList(w), optimList(g), optimList(m), (if lens.len == 0: nil else: unsafeAddr lens[0]), cint(lens.len), lr, mu, wd, cint(ord(nesterov)), gscale, cast[ptr float32](clip), stream)

proc adamStep*(w, g, m, v: openArray[DevicePtr[float32]], lens: openArray[int64], step: int64, lr: float32, b1: float32 = 0.9, b2: float32 = 0.999, eps: float32 = 1e-8, wd: float32 = 0, decoupled = false, gscale: float32 = 1, clip: DevicePtr[float32] = DevicePtr[float32](nil), stream: pointer = nil) =
  ## one Adam step (step counts from 1; m and v start as zeros) on every tensor of the list, in place; decoupled: AdamW's decay
  doAssert w.len == lens.len and g.len == lens.len and m.len == lens.len and v.len == lens.len
  check laser_hip_adam_step_f32_dev(optimList(w), optimList(g), optimList(m), optimList(v), (if lens.len == 0: nil else: unsafeAddr lens[0]), cint(lens.len), lr, b1, b2, eps, wd, cint(ord(decoupled)), adamBiasCorrection(b1, step), adamBiasCorrection(b2, step), gscale, cast[ptr float32](clip), stream)

proc gradNorm*(norm, clip: DevicePtr[float32], g: openArray[DevicePtr[float32]], lens: openArray[int64], maxNorm: float32 = Inf, stream: pointer = nil) =
  ## norm = sqrt of the sum over the list of reduce_sum(g * g), clip = maxNorm / norm when norm > maxNorm, else 1: one device
  ## float each; either may be nil, not both
  doAssert g.len == lens.len
  check laser_hip_grad_norm_f32_dev(cast[ptr float32](norm), cast[ptr float32](clip), optimList(g), (if lens.len == 0: nil else: unsafeAddr lens[0]), cint(lens.len), maxNorm, stream)

# ---- sine and cosine (include/laser_hip.h "Sine and cosine"): lsin and lcos of sincos_core.h -----------------------------
# faithful for every finite float32, lsin odd and lcos even bit for bit, lsin(x) = x for tiny x, NaN for NaN and +-Inf
proc laser_hip_sin_f32(dst: ptr float32, src: ptr float32, len: int64): cint {.lh, importc: "laser_hip_sin_f32".}
proc laser_hip_cos_f32(dst: ptr float32, src: ptr float32, len: int64): cint {.lh, importc: "laser_hip_cos_f32".}
proc laser_hip_sin_f32_dev*(dst: ptr float32, dstStrides: ptr int64, src: ptr float32, srcStrides: ptr int64, shape: ptr int64, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_sin_f32_dev".}
proc laser_hip_cos_f32_dev*(dst: ptr float32, dstStrides: ptr int64, src: ptr float32, srcStrides: ptr int64, shape: ptr int64, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_cos_f32_dev".}
proc laser_hip_sincos_f32_dev*(sinDst: ptr float32, sinStrides: ptr int64, cosDst: ptr float32, cosStrides: ptr int64, src: ptr float32, srcStrides: ptr int64, shape: ptr int64, rank: cint, stream: pointer): cint {.lh, importc: "laser_hip_sincos_f32_dev".}

proc sin*(dst, src: ptr (float32 or UncheckedArray[float32]), len: Natural) =
  ## dst[i] = sin(src[i]) over a contiguous range of float32 (host memory; the GPU computes it)
  check laser_hip_sin_f32(cast[ptr float32](dst), cast[ptr float32](src), int64(len))

proc cos*(dst, src: ptr (float32 or UncheckedArray[float32]), len: Natural) =
  ## dst[i] = cos(src[i]) over a contiguous range of float32 (host memory; the GPU computes it)
  check laser_hip_cos_f32(cast[ptr float32](dst), cast[ptr float32](src), int64(len))

proc sin*(dst, src: DevicePtr[float32], len: Natural, stream: pointer = nil) =
  ## dst[i] = sin(src[i]) over `len` contiguous device elements; dst may be src
  var stride = 1'i64
  var n = int64(len)
  check laser_hip_sin_f32_dev(cast[ptr float32](dst), stride.addr, cast[ptr float32](src), stride.addr, n.addr, 1, stream)

proc cos*(dst, src: DevicePtr[float32], len: Natural, stream: pointer = nil) =
  ## dst[i] = cos(src[i]) over `len` contiguous device elements; dst may be src
  var stride = 1'i64
  var n = int64(len)
  check laser_hip_cos_f32_dev(cast[ptr float32](dst), stride.addr, cast[ptr float32](src), stride.addr, n.addr, 1, stream)

proc sincos*(sinDst, cosDst, src: DevicePtr[float32], len: Natural, stream: pointer = nil) =
  ## both from one argument reduction, the same bits as sin and cos; either destination may be src
  var stride = 1'i64
  var n = int64(len)
  check laser_hip_sincos_f32_dev(cast[ptr float32](sinDst), stride.addr, cast[ptr float32](cosDst), stride.addr, cast[ptr float32](src), stride.addr, n.addr, 1, stream)

# ---- F+tree weighted sampler (include/laser_hip.h "F+tree weighted sampler"): fenwicktree.nim over HipStorage -----------
# One tree image of 2 P float32 per row (P = the next power of two >= n; the reference's array shifted up by one slot).  The
# uniform numbers are the caller's, or come from a HipRng stream ("Random numbers" below): the overloads taking `rng`.
proc laser_hip_sampler_tree_elems*(n: int64, elems: ptr int64): cint {.lh, importc: "laser_hip_sampler_tree_elems".}
proc laser_hip_sampler_plan*(rows: int64, n: int64, out4: ptr int64): cint {.lh, importc: "laser_hip_sampler_plan".}
proc laser_hip_sampler_build_f32_dev*(tree: ptr float32, treeRowStride: int64, w: ptr float32, wRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_sampler_build_f32_dev".}
proc laser_hip_sampler_sample_f32_dev*(idx: ptr int32, tree: ptr float32, treeRowStride: int64, u01: ptr float32, rows: int64, n: int64, m: int64, stream: pointer): cint {.lh, importc: "laser_hip_sampler_sample_f32_dev".}
proc laser_hip_sampler_sample_remove_f32_dev*(idx: ptr int32, tree: ptr float32, treeRowStride: int64, u01: ptr float32, rows: int64, n: int64, k: int64, stream: pointer): cint {.lh, importc: "laser_hip_sampler_sample_remove_f32_dev".}
proc laser_hip_sampler_update_f32_dev*(tree: ptr float32, treeRowStride: int64, elem: ptr int32, weight: ptr float32, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_sampler_update_f32_dev".}

type
  Sampler* = object
    ## fenwicktree.nim:38 for `rows` rows of `n` weights on the device: `tree` holds rows images of `treeElems` float32
    tree*: HipStorage[float32]
    rows*, n*, treeElems*: int

proc newSampler*(weights: DevicePtr[float32], wRowStride: int, rows, n: Natural, stream: pointer = nil): Sampler =
  ## fenwicktree.nim:67-118 for every row of a device matrix (row elements contiguous, wRowStride >= n elements)
  var elems: int64
  check laser_hip_sampler_tree_elems(int64(n), elems.addr)
  result.rows = rows
  result.n = n
  result.treeElems = int(elems)
  allocHipStorage(result.tree, rows * int(elems))
  check laser_hip_sampler_build_f32_dev(cast[ptr float32](result.tree.raw_buffer), elems, cast[ptr float32](weights), int64(wRowStride), int64(rows), int64(n), stream)

proc sample*(s: Sampler, idx: DevicePtr[int32], u01: DevicePtr[float32], m: Natural = 1, stream: pointer = nil) =
  ## fenwicktree.nim:147-165: m independent draws per row; idx and u01 are (rows, m) row-major on the device, u01 in [0, 1)
  check laser_hip_sampler_sample_f32_dev(cast[ptr int32](idx), cast[ptr float32](s.tree.raw_buffer), int64(s.treeElems), cast[ptr float32](u01), int64(s.rows), int64(s.n), int64(m), stream)

proc sampleAndRemove*(s: var Sampler, idx: DevicePtr[int32], u01: DevicePtr[float32], k: Natural = 1, stream: pointer = nil) =
  ## fenwicktree.nim:186-199, k times per row: a drawn element's weight becomes 0 before the next draw; -1 once a row is empty
  check laser_hip_sampler_sample_remove_f32_dev(cast[ptr int32](idx), cast[ptr float32](s.tree.raw_buffer), int64(s.treeElems), cast[ptr float32](u01), int64(s.rows), int64(s.n), int64(k), stream)

proc update*(s: var Sampler, elem: DevicePtr[int32], weight: DevicePtr[float32], stream: pointer = nil) =
  ## fenwicktree.nim:175-184 with one (elem, weight) per row on the device; elem -1 leaves that row alone
  check laser_hip_sampler_update_f32_dev(cast[ptr float32](s.tree.raw_buffer), int64(s.treeElems), cast[ptr int32](elem), cast[ptr float32](weight), int64(s.rows), int64(s.n), stream)

# ---- Random numbers (include/laser_hip.h "Random numbers"): Philox4x32-10 streams, randomTensor over HipStorage -----------
# Word w of a stream is a function of (seed, subseq, w) alone; a HipRng holds (seed, subseq, offset) on the host and nothing
# lives on the device.  The three travel as int64 (the C-ABI has no unsigned parameters): the same 64 bits, read as unsigned.
proc laser_hip_random_plan*(n: int64, wordsPerElem: cint, offset: int64, dstMisaligned: cint, cus: cint, out4: ptr int64): cint {.lh, importc: "laser_hip_random_plan".}
proc laser_hip_random_bits_u32_dev*(dst: ptr uint32, n: int64, seed: int64, subseq: int64, offset: int64, stream: pointer): cint {.lh, importc: "laser_hip_random_bits_u32_dev".}
proc laser_hip_random_uniform_f32_dev*(dst: ptr float32, n: int64, lo: float32, hi: float32, seed: int64, subseq: int64, offset: int64, stream: pointer): cint {.lh, importc: "laser_hip_random_uniform_f32_dev".}
proc laser_hip_random_uniform_f64_dev*(dst: ptr float64, n: int64, lo: float64, hi: float64, seed: int64, subseq: int64, offset: int64, stream: pointer): cint {.lh, importc: "laser_hip_random_uniform_f64_dev".}
proc laser_hip_random_uniform_i32_dev*(dst: ptr int32, n: int64, lo: int32, hi: int32, seed: int64, subseq: int64, offset: int64, stream: pointer): cint {.lh, importc: "laser_hip_random_uniform_i32_dev".}
proc laser_hip_random_uniform_i64_dev*(dst: ptr int64, n: int64, lo: int64, hi: int64, seed: int64, subseq: int64, offset: int64, stream: pointer): cint {.lh, importc: "laser_hip_random_uniform_i64_dev".}
proc laser_hip_random_normal_f32_dev*(dst: ptr float32, n: int64, mean: float32, std: float32, seed: int64, subseq: int64, offset: int64, stream: pointer): cint {.lh, importc: "laser_hip_random_normal_f32_dev".}
proc laser_hip_sampler_sample_rng_f32_dev*(idx: ptr int32, tree: ptr float32, treeRowStride: int64, seed: int64, subseq: int64, offset: int64, rows: int64, n: int64, m: int64, stream: pointer): cint {.lh, importc: "laser_hip_sampler_sample_rng_f32_dev".}
proc laser_hip_sampler_sample_remove_rng_f32_dev*(idx: ptr int32, tree: ptr float32, treeRowStride: int64, seed: int64, subseq: int64, offset: int64, rows: int64, n: int64, k: int64, stream: pointer): cint {.lh, importc: "laser_hip_sampler_sample_remove_rng_f32_dev".}

type
  HipRng* = object
    ## the stream (seed, subseq) and the next unused word; every draw advances `offset` by the words it used (mod 2^64)
    seed*, subseq*, offset*: uint64

func initHipRng*(seed: uint64, subseq: uint64 = 0, offset: uint64 = 0): HipRng {.inline.} =
  HipRng(seed: seed, subseq: subseq, offset: offset)

proc randomTensor*[T](shape: openarray[int], valrange: Slice[T], rng: var HipRng): HipStorage[T] =
  ## randomTensor(shape, valrange) of the reference's benchmarks (bench_exp.nim:17) on the device: prod(shape) elements in
  ## row-major order, uniform on the closed interval valrange.a .. valrange.b; T is float32, float64, int32 or int64 (int)
  var size = 1
  for s in shape: size *= s
  allocHipStorage(result, size)
  let (sd, sq, off) = (cast[int64](rng.seed), cast[int64](rng.subseq), cast[int64](rng.offset))
  when T is float32:
    check laser_hip_random_uniform_f32_dev(cast[ptr float32](result.raw_buffer), int64(size), valrange.a, valrange.b, sd, sq, off, nil)
  elif T is float64:
    check laser_hip_random_uniform_f64_dev(cast[ptr float64](result.raw_buffer), int64(size), valrange.a, valrange.b, sd, sq, off, nil)
  elif T is int32:
    check laser_hip_random_uniform_i32_dev(cast[ptr int32](result.raw_buffer), int64(size), valrange.a, valrange.b, sd, sq, off, nil)
  elif T is int64 or T is int:
    check laser_hip_random_uniform_i64_dev(cast[ptr int64](result.raw_buffer), int64(size), int64(valrange.a), int64(valrange.b), sd, sq, off, nil)
  else:
    {.error: "randomTensor: float32, float64, int32 or int64".}
  rng.offset += uint64(size) * uint64(sizeof(T) div 4)

proc randomTensor*[T](shape: openarray[int], max: T, rng: var HipRng): HipStorage[T] =
  ## randomTensor(shape, max) (reduction_bench.nim:40): uniform on 0 .. max
  randomTensor(shape, T(0)..max, rng)

proc randomNormalTensor*(shape: openarray[int], mean, std: float32, rng: var HipRng): HipStorage[float32] =
  ## prod(shape) float32 normal draws in row-major order (Box-Muller on pairs of words of the stream, normal_core.h): element k
  ## from stream position rng.offset + k; the offset advances by the element count
  var size = 1
  for s in shape: size *= s
  allocHipStorage(result, size)
  check laser_hip_random_normal_f32_dev(cast[ptr float32](result.raw_buffer), int64(size), mean, std, cast[int64](rng.seed), cast[int64](rng.subseq), cast[int64](rng.offset), nil)
  rng.offset += uint64(size)

proc randomBits*(n: Natural, rng: var HipRng): HipStorage[uint32] =
  ## the next n words of the stream
  allocHipStorage(result, n)
  check laser_hip_random_bits_u32_dev(cast[ptr uint32](result.raw_buffer), int64(n), cast[int64](rng.seed), cast[int64](rng.subseq), cast[int64](rng.offset), nil)
  rng.offset += uint64(n)

proc sample*(s: Sampler, idx: DevicePtr[int32], rng: var HipRng, m: Natural = 1, stream: pointer = nil) =
  ## `sample` with u01[row, j] made in the kernel from word rng.offset + row * m + j; the rng advances by rows * m
  check laser_hip_sampler_sample_rng_f32_dev(cast[ptr int32](idx), cast[ptr float32](s.tree.raw_buffer), int64(s.treeElems), cast[int64](rng.seed), cast[int64](rng.subseq), cast[int64](rng.offset), int64(s.rows), int64(s.n), int64(m), stream)
  rng.offset += uint64(s.rows * m)

proc sampleAndRemove*(s: var Sampler, idx: DevicePtr[int32], rng: var HipRng, k: Natural = 1, stream: pointer = nil) =
  ## `sampleAndRemove` with the uniform numbers of the stream; the rng advances by rows * k
  check laser_hip_sampler_sample_remove_rng_f32_dev(cast[ptr int32](idx), cast[ptr float32](s.tree.raw_buffer), int64(s.treeElems), cast[int64](rng.seed), cast[int64](rng.subseq), cast[int64](rng.offset), int64(s.rows), int64(s.n), int64(k), stream)
  rng.offset += uint64(s.rows * k)

# ---- Row cumsum, searchsorted and the inverse-CDF sampler (include/laser_hip.h, the section of that name):
# cumsum, searchsorted and sample of bench_multinomial_samplers.nim:49-61, 143-214 over HipStorage --------------------------
proc laser_hip_cumsum_f32_dev*(dst: ptr float32, dstRowStride: int64, src: ptr float32, srcRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_cumsum_f32_dev".}
proc laser_hip_cumsum_f64_dev*(dst: ptr float64, dstRowStride: int64, src: ptr float64, srcRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_cumsum_f64_dev".}
proc laser_hip_cumsum_i32_dev*(dst: ptr int32, dstRowStride: int64, src: ptr int32, srcRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_cumsum_i32_dev".}
proc laser_hip_cumsum_i64_dev*(dst: ptr int64, dstRowStride: int64, src: ptr int64, srcRowStride: int64, rows: int64, n: int64, stream: pointer): cint {.lh, importc: "laser_hip_cumsum_i64_dev".}
proc laser_hip_searchsorted_f32_dev*(idx: ptr int32, a: ptr float32, aRowStride: int64, v: ptr float32, rows: int64, n: int64, m: int64, right: cint, stream: pointer): cint {.lh, importc: "laser_hip_searchsorted_f32_dev".}
proc laser_hip_searchsorted_f64_dev*(idx: ptr int32, a: ptr float64, aRowStride: int64, v: ptr float64, rows: int64, n: int64, m: int64, right: cint, stream: pointer): cint {.lh, importc: "laser_hip_searchsorted_f64_dev".}
proc laser_hip_searchsorted_i32_dev*(idx: ptr int32, a: ptr int32, aRowStride: int64, v: ptr int32, rows: int64, n: int64, m: int64, right: cint, stream: pointer): cint {.lh, importc: "laser_hip_searchsorted_i32_dev".}
proc laser_hip_searchsorted_i64_dev*(idx: ptr int32, a: ptr int64, aRowStride: int64, v: ptr int64, rows: int64, n: int64, m: int64, right: cint, stream: pointer): cint {.lh, importc: "laser_hip_searchsorted_i64_dev".}
proc laser_hip_cumsum_plan*(rows: int64, n: int64, elemSize: cint, cus: cint, out4: ptr int64): cint {.lh, importc: "laser_hip_cumsum_plan".}
proc laser_hip_cdf_sample_f32_dev*(idx: ptr int32, cdf: ptr float32, cdfRowStride: int64, u01: ptr float32, rows: int64, n: int64, m: int64, stream: pointer): cint {.lh, importc: "laser_hip_cdf_sample_f32_dev".}
proc laser_hip_cdf_sample_remove_f32_dev*(idx: ptr int32, w: ptr float32, wRowStride: int64, cdf: ptr float32, cdfRowStride: int64, u01: ptr float32, rows: int64, n: int64, k: int64, stream: pointer): cint {.lh, importc: "laser_hip_cdf_sample_remove_f32_dev".}
proc laser_hip_cdf_sample_rng_f32_dev*(idx: ptr int32, cdf: ptr float32, cdfRowStride: int64, seed: int64, subseq: int64, offset: int64, rows: int64, n: int64, m: int64, stream: pointer): cint {.lh, importc: "laser_hip_cdf_sample_rng_f32_dev".}
proc laser_hip_cdf_sample_remove_rng_f32_dev*(idx: ptr int32, w: ptr float32, wRowStride: int64, cdf: ptr float32, cdfRowStride: int64, seed: int64, subseq: int64, offset: int64, rows: int64, n: int64, k: int64, stream: pointer): cint {.lh, importc: "laser_hip_cdf_sample_remove_rng_f32_dev".}

proc cumsum*[T](t: HipStorage[T], rows, n: Natural, stream: pointer = nil): HipStorage[T] =
  ## cumsum(t) of bench_multinomial_samplers.nim:143-148 on the device: `rows` contiguous rows of n elements, the inclusive
  ## prefix sum of every row in the order of scan_core.h; T is float32, float64, int32 or int64 (int)
  allocHipStorage(result, rows * n)
  when T is float32:
    check laser_hip_cumsum_f32_dev(cast[ptr float32](result.raw_buffer), int64(n), cast[ptr float32](t.raw_buffer), int64(n), int64(rows), int64(n), stream)
  elif T is float64:
    check laser_hip_cumsum_f64_dev(cast[ptr float64](result.raw_buffer), int64(n), cast[ptr float64](t.raw_buffer), int64(n), int64(rows), int64(n), stream)
  elif T is int32:
    check laser_hip_cumsum_i32_dev(cast[ptr int32](result.raw_buffer), int64(n), cast[ptr int32](t.raw_buffer), int64(n), int64(rows), int64(n), stream)
  elif T is int64 or T is int:
    check laser_hip_cumsum_i64_dev(cast[ptr int64](result.raw_buffer), int64(n), cast[ptr int64](t.raw_buffer), int64(n), int64(rows), int64(n), stream)
  else:
    {.error: "cumsum: float32, float64, int32 or int64".}

proc searchsorted*[T](input: HipStorage[T], values: HipStorage[T], leftSide: bool, rows, n: Natural, m: Natural = 1, stream: pointer = nil): HipStorage[int32] =
  ## searchsorted(input, values, leftSide) of bench_multinomial_samplers.nim:162-170: `input` holds `rows` sorted rows of n
  ## elements, `values` m values per row; lowerBound (leftSide) or upperBound of every value in its row
  allocHipStorage(result, rows * m)
  let right = cint(if leftSide: 0 else: 1)
  when T is float32:
    check laser_hip_searchsorted_f32_dev(cast[ptr int32](result.raw_buffer), cast[ptr float32](input.raw_buffer), int64(n), cast[ptr float32](values.raw_buffer), int64(rows), int64(n), int64(m), right, stream)
  elif T is float64:
    check laser_hip_searchsorted_f64_dev(cast[ptr int32](result.raw_buffer), cast[ptr float64](input.raw_buffer), int64(n), cast[ptr float64](values.raw_buffer), int64(rows), int64(n), int64(m), right, stream)
  elif T is int32:
    check laser_hip_searchsorted_i32_dev(cast[ptr int32](result.raw_buffer), cast[ptr int32](input.raw_buffer), int64(n), cast[ptr int32](values.raw_buffer), int64(rows), int64(n), int64(m), right, stream)
  elif T is int64 or T is int:
    check laser_hip_searchsorted_i64_dev(cast[ptr int32](result.raw_buffer), cast[ptr int64](input.raw_buffer), int64(n), cast[ptr int64](values.raw_buffer), int64(rows), int64(n), int64(m), right, stream)
  else:
    {.error: "searchsorted: float32, float64, int32 or int64".}

proc sample*(probs: HipStorage[float32], rows, n: Natural, nbSamples: Natural, rng: var HipRng, stream: pointer = nil): HipStorage[int32] =
  ## sample(probs, nb_samples) of bench_multinomial_samplers.nim:172-214: nbSamples == 1 is one cumsum and one right-side search
  ## per row; more draws are made WITHOUT replacement on a private copy of the weights.  The uniform numbers are those of `rng`,
  ## which advances by rows * nbSamples.
  allocHipStorage(result, rows * nbSamples)
  var cdf: HipStorage[float32]
  allocHipStorage(cdf, rows * n)
  let (sd, sq, off) = (cast[int64](rng.seed), cast[int64](rng.subseq), cast[int64](rng.offset))
  if nbSamples == 1:
    check laser_hip_cumsum_f32_dev(cast[ptr float32](cdf.raw_buffer), int64(n), cast[ptr float32](probs.raw_buffer), int64(n), int64(rows), int64(n), stream)
    check laser_hip_cdf_sample_rng_f32_dev(cast[ptr int32](result.raw_buffer), cast[ptr float32](cdf.raw_buffer), int64(n), sd, sq, off, int64(rows), int64(n), 1, stream)
  else:
    var w: HipStorage[float32]
    allocHipStorage(w, rows * n)
    var shape = [int(rows), int(n)]
    var strides = [int(n), 1]
    check laser_hip_copy_strided_b32_dev(pointer(w.raw_buffer), strides[0].addr, pointer(probs.raw_buffer), strides[0].addr, shape[0].addr, 2, stream)
    check laser_hip_cdf_sample_remove_rng_f32_dev(cast[ptr int32](result.raw_buffer), cast[ptr float32](w.raw_buffer), int64(n), cast[ptr float32](cdf.raw_buffer), int64(n), sd, sq, off, int64(rows), int64(n), int64(nbSamples), stream)
  rng.offset += uint64(rows * nbSamples)

# ---- forEachReduce (include/laser_hip.h "forEachReduce"): foreach_staged.nim:318 on device buffers ------------------------
proc laser_hip_foreach_reduce_source(body: cstring, nops: cint, names: ptr cstring, dtypes: ptr cint, writable: ptr cint, nparams: cint, paramNames: ptr cstring, paramDtypes: ptr cint, accName: cstring, accDtype: cint, merge: cstring, buf: pointer, cap: int64, len: ptr int64): cint {.lh, importc: "laser_hip_foreach_reduce_source".}
proc laser_hip_foreach_reduce_code(body: cstring, nops: cint, names: ptr cstring, dtypes: ptr cint, writable: ptr cint, nparams: cint, paramNames: ptr cstring, paramDtypes: ptr cint, accName: cstring, accDtype: cint, merge: cstring, arch: cstring, buf: pointer, cap: int64, len: ptr int64): cint {.lh, importc: "laser_hip_foreach_reduce_code".}
proc laser_hip_foreach_reduce_kernel*(body: cstring, nops: cint, names: ptr cstring, dtypes: ptr cint, writable: ptr cint, nparams: cint, paramNames: ptr cstring, paramDtypes: ptr cint, accName: cstring, accDtype: cint, merge: cstring, handle: ptr int64): cint {.lh, importc: "laser_hip_foreach_reduce_kernel".}
proc laser_hip_foreach_reduce_dev*(handle: int64, ptrs: ptr pointer, strides: ptr int64, shape: ptr int64, rank: cint, params: pointer, init: pointer, res: pointer, stream: pointer): cint {.lh, importc: "laser_hip_foreach_reduce_dev".}
