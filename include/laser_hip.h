/* include/laser_hip.h -- C-ABI of liblaser_hip.so, the MI355X (gfx950) implementation of Laser's
 * packed-panel GEMM hot path, its physical transposes and the im2col->GEMM convolution.
 *
 * This is the drop-in boundary: plain pointers, sizes and element strides; no C++/torch types.
 * Every entry point names the reference proc it replaces (file:line relative to the mratsim/laser
 * tree).  The Nim side keeps its own signatures and forwards here with
 *   {.dynlib: "liblaser_hip.so", importc: "laser_hip_...", cdecl.}
 * (see INTEGRATION.md and nim/laser_hip.nim).  Nim `int` == int64_t on amd64, `float32` == float.
 *
 * Conventions
 *   - Return value: 0 on success, non-zero on failure (LASER_HIP_E_*); the message is available
 *     from laser_hip_last_error() (thread-local).  The reference procs return void and abort via
 *     doAssert on precondition violations; the Nim shim turns a non-zero return into doAssert.
 *   - Strides are in ELEMENTS, element X[r,c] lives at ptr[r*rowStride + c*colStride]
 *     (gemm_utils.nim:36-60).  Any strides are accepted, including transposed and negative.
 *   - Host-pointer entry points (no suffix) are synchronous: they stage operands to the GPU, run,
 *     and copy C back before returning -- exactly Laser's blocking call semantics.  Caller keeps
 *     ownership of every pointer; the library owns only cached device scratch (freed by
 *     laser_hip_finalize).
 *   - `_dev` entry points take DEVICE pointers and a hipStream_t (as void*; NULL = default stream)
 *     and are asynchronous on that stream: this is the path measured against the roofline.
 *   - Semantics preserved from the reference: beta == 0 never reads C (NaN / uninitialised safe,
 *     gemm_ukernel_generic.nim:53-76); K == 0 leaves C untouched even if beta != 1 (gemm.nim:150);
 *     alpha, beta have the element type (integers too); overlapping A/B/C is undefined.
 *   - fp32 arithmetic order (LASER_HIP_F32_LASER_ORDER, the default): for every C[i,j] an
 *     ascending-k fused-multiply-add chain restarted from +0 every kc = 512 values of k, the slice
 *     sums added into beta*C in ascending order -- bit-identical to Laser on an FMA host
 *     (gemm_ukernel_generator.nim:245-248, gemm.nim:150-158, gemm_tiling.nim:309-310).
 *     LASER_HIP_F32_FAST keeps one chain across all of K (within 1e-5 relative, not bit-equal
 *     for K > 512; launch plans that split K -- few tiles x long K, the rows of a badly filled
 *     last round -- add kc-slice chains in order instead: the same bound).  f64 follows the same
 *     rule with kc = 256.
 */
#ifndef LASER_HIP_H
#define LASER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LASER_HIP_OK 0
#define LASER_HIP_E_INVALID 1   /* bad argument (negative size, null pointer, misaligned pre-pack buffer ...) */
#define LASER_HIP_E_HIP 2       /* a HIP runtime call failed; see laser_hip_last_error() */
#define LASER_HIP_E_NODEVICE 3  /* no gfx950 device / library built without device code for this GPU */
#define LASER_HIP_E_HANDLE 4    /* pre-packed buffer handle is stale or corrupt */
#define LASER_HIP_E_COMPILE 5   /* a forEach body did not compile, or hiprtc could not be loaded (see "forEach with a body") */

/* ---- lifecycle ----------------------------------------------------------------------------- */
/* Lazy-initialised on first use; explicit init selects the device (-1 = current device). */
int laser_hip_init(int device);
int laser_hip_finalize(void);
const char *laser_hip_last_error(void);
const char *laser_hip_version(void);
/* Incremented whenever an exported prototype, an option name or an operation code changes incompatibly (round 3 changed the
 * alpha / beta types of map_strided and collapsed the setters into laser_hip_set_option: 2; round 4 only added names: still 2).
 * A caller built against another header should refuse to run. */
#define LASER_HIP_ABI_VERSION 3
int laser_hip_abi_version(void);
int laser_hip_device_count(void);
/* Diagnostics (touches no device): the kernel and launch plan the float32 launcher takes for a dense row-major M x N x K product on a
 * device of `cus` compute units -- the launch plans scale with the device's own CU count, so a partitioned MI355X (CPX 32 / QPX 64 /
 * DPX 128 CUs) keeps the hand-scheduled kernels.  out8[0] = 1 + kernel index (0: compiler-scheduled kernels), [1] = plan (0 one tile
 * per workgroup, 1 persistent with K-slice cuts, 2 strided whole tiles with pipelined transitions, 3 hybrid: 2 for the whole rounds + 1 for the remaining tiles), [2] = workgroups,
 * [3] = K slices per tile (hybrid: of the second launch), [4] = tiles, [5] / [6] = tile rows / columns, [7] = workgroup slots.  The GPU twin of reading gemm_tiling.nim:276-341's
 * `newTiles` for a shape: what partition will the library use. */
int laser_hip_plan_f32(int64_t M, int64_t N, int64_t K, int laser_order, int cus, int64_t *out8);
/* Name of the GPU architecture in use, e.g. "gfx950" (replaces the reference's cpuinfo ISA
 * dispatch, gemm.nim:228-247). */
const char *laser_hip_arch(void);

#define LASER_HIP_F32_LASER_ORDER 0
#define LASER_HIP_F32_FAST 1
int laser_hip_set_float_mode(int mode);
int laser_hip_get_float_mode(void);
/* Force one tile configuration of the f32 MFMA kernel (-1 = heuristic).  For tuning/benchmarks. */
int laser_hip_set_f32_config(int cfg);
int laser_hip_f32_config_count(void);
/* ---- options: one entry point for every tuning / A-B switch ------------------------------------------------------------
 * laser_hip_set_option(name, value); unknown names are LASER_HIP_E_INVALID.  In LASER_ORDER float mode (the default) every switch
 * leaves results bit-identical (it selects between implementations of the same arithmetic); in FAST mode the switches that change how
 * K is cut ("split_tail", "slice_parallel", "asm_plan" / "asm_slice" / "asm_wgs") change the rounding order of the sums, within the
 * 1e-5 mean relative error of that mode.  Defaults in brackets.
 *   "f32_asm"          [1] float32 gemm_strided with any element strides on A, B and C (MatrixView, gemm_utils.nim:36-60), any alpha /
 *                          beta, any K -- and 3x3 / stride-1 convolutions with any zero padding: the hand-scheduled assembly
 *                          kernels (accumulators in AGPRs; laser_amd/asmgen/) when the problem has at least ~100 tiles of 64x64;
 *                          0 = never (the compiler-scheduled kernels); 2 = whenever eligible, whatever the tile count (tests)
 *   "f64_asm"          [1] float64 twin of "f32_asm" (unit column strides on A and C, B row-major-like or passed transposed, any
 *                          alpha / beta, K even; laser_amd/asmgen/f64_kernel.py)
 *   "i32_asm"          [1] int32 / int64 limb GEMMs, any alpha / beta: the hand-scheduled kernels (laser_amd/asmgen/i8_kernel.py;
 *                          K > 8192 in chunks)
 *   "int_group_m"      [4] tile rows per raster group of those kernels' workgroup -> tile map (1 .. 64; a scheduling knob: same results)
 *   "f64_mfma" "i32_mfma" "i64_mfma"  [1] matrix-core kernels (f64 MFMA; int8-limb decomposition for the integers, the
 *                          reference's integer micro-kernels: gemm_ukernel_avx512.nim:40-74); 0 = the VALU kernels
 *   "narrow_mfma"      [1] int8 / int16 GEMMs on the int8 matrix cores (one / two digit planes); 0 = the VALU / streaming kernels
 *   "conv_implicit"    [1] im2col fused into the GEMM's B loader; 0 = explicit im2col workspace + batched GEMM, the
 *                          reference's literal structure (conv2d_im2col.nim:126-166)
 *   "conv_patch"       [1] implicit conv reads B from an LDS-resident input patch when it fits; 0 = per-element gather
 *   "conv_direct"      [1] convolutions with <= 32 output channels and C_in*kH*kW <= 256 (the reference's conv bench shape,
 *                          conv2d_bench.nim:130-170): the direct HBM-streaming kernels; 0 = the implicit-GEMM kernels; 2 = without
 *                          the scalar-filter forms of 3x3 filters (A/B switch: the matrix-core / LDS-filter forms everywhere); 3 = the scalar-filter forms
 *                          without the two-channel-group split of small launches (A/B switch)
 *   "conv_tail"        [1] the pixel tail behind the hand-scheduled 3x3 conv main launch (npix % 128 pixels per image) as ONE launch
 *                          of the latency-built direct kernel (a wave per 32x32 block and kc slice, ordered fold in LDS); 0 = the
 *                          compiler-scheduled tail forms
 *   "conv_walk"        [1] assembly convolution main launch as unit walkers (a workgroup runs units (image, tile) g, g + G, ... with
 *                          pipelined transitions) where there are more units than workgroup slots; 0 never, 2 whenever there are two units,
 *                          >= 3: that many workgroups (tests).  Same bits either way.
 *   "conv_1x1_implicit" [0] probes: 1x1 / stride 1 / no padding convolutions through the implicit-GEMM kernels instead of the reference's
 *                          GEMM shortcut (conv2d_im2col.nim:121-153; measured 0.6 % ahead to 40 % behind it: profiles/r06/conv_1x1_probe_ae.jsonl)
 *   "conv_cut_always"  [0] tests / probes: cut every 3x3 convolution at its last whole 128-pixel tile, whatever the launch model says
 *   "conv_kslice"      [1] laser-order conv tail as parallel kc slices (gemm.nim:150-158) + ordered combine
 *   "host_pipeline_2d" [1] large host-pointer calls with pinned B and C: row panels x column panels; 0 = row panels only
 *   "zero_copy_poll"   [1] small host-pointer calls poll completion flags in mapped memory; 0 = synchronise the stream
 *   "skinny"           [1] M <= 8 or N <= 8: the streaming kernel        "small_path" [1] the one-wave-per-block kernel
 *   "split_tail"       [1] launch plans that cut a problem: main + tail launches of the compiler-scheduled kernels, peeled rows /
 *                          columns of ragged-by-a-few shapes, and the assembly kernels' persistent plan (below); 0 = one plain launch
 *   "slice_parallel"   [1] few tiles x long K: kc slices as one batched launch + ordered combine
 *   "slice_parallel_min" / "slice_parallel_tiles"  tuning overrides of that rule (0 = built-in)
 *   "asm_plan"         [0] launch plan of the assembly GEMM kernels: 0 = the launcher's model decides; 1 = one tile per workgroup;
 *                          2 = the persistent plan whenever legal: every workgroup slot of the chip gets an equal share of K-slice
 *                          units (laser-order: kc slices), a tile that straddles two workgroups is handed over in-kernel, in slice
 *                          order (gemm.nim:150-158) -- laser-order results are the same bits under every plan; 3 = the strided
 *                          whole-tile plan whenever legal (round 6): one persistent workgroup per slot walks tiles v, v + G, ...
 *                          WITHOUT leaving its K loop -- the last K-tile bodies of a tile fetch the next tile's first K-tiles, the next
 *                          tile's first body stores this tile's C (beta == 0, plain epilogue, K a multiple of the K-tile); what the
 *                          model takes by itself when there are more tiles than workgroup slots.  Same bits as plan 1, both modes.
 *                          4 = the hybrid plan whenever legal (round 6): two launches of one kernel -- the whole rounds of the tile
 *                          raster under plan 3, the remaining tiles (a fraction of a round, >= 8) under plan 2 -- what the model takes
 *                          in one-chain mode when the fraction is small; laser-order results are the same bits as under every plan.
 *                          A K-cut launch whose hand-over times out (a receiver polls ~2 s for its predecessor's running sum; never in
 *                          a correct run) is REPORTED: the error word travels back behind the launch and the next call on that stream
 *                          fails with LASER_HIP_E_HIP, laser_hip_last_error() naming the stream -- never a silently wrong C
 *                          ("asm_test_giveup" = 1 makes every receiver give up at once: tests of that report)
 *   "asm_kernel" [-1] / "asm_wgs" [0] / "asm_slice" [0] / "asm_noseed" [0] / "asm_group_m" [0]  tuning / test overrides of that plan:
 *                          force an assembly kernel index, the number of workgroups, the K-tiles per slice of a one-chain cut, the
 *                          two-run receive path, the tile rows per raster group (which tiles share an XCD's L2)
 *   "asm_tile"        [-1] pin a tile CLASS of the f32 assembly GEMM kernels (accumulation mode / transposed-B variant still follow the
 *                          call): 0 = 256x128 (laser-order) / 256x256, 1 = 256x128 one chain, 2 = 128x128x16 (two workgroups per CU:
 *                          degrades gracefully when another library's kernels -- RCCL's -- hold some CUs), 3 = 128x128x32, 4 = 64x64,
 *                          5 = 96x96, 6 = 160x96, 7 = 128x96, 8 = 192x96, 9 = 160x160 on 16x16 blocks (v_mfma_f32_16x16x4_f32: K % 4 == 0,
 *                          no fused prologue);
 *                          one tile per workgroup, no minimum tile count; -1 = the launcher's model decides.
 *   "thread_asm_tile" [-2] the same pin for the launches made BY THE CALLING THREAD only (-2 = none: "asm_tile" applies; -1 = the
 *                          model decides whatever "asm_tile" says).  The per-GPU processes of laser_amd/distributed.py set 2 around
 *                          their local products on the thread that launches them -- other threads' GEMMs keep their own choice;
 *                          LASER_HIP_SHARD_PIN_TILE is the same pin per call and per worker thread inside the single-process
 *                          sharded entry points
 *   "im2col_band"      [0] output pixels per workgroup band of the explicit im2col kernel (0 = 256 sixteen-byte vectors; tuning sweeps)
 * laser_hip_get_option reads any of them back, plus the read-only diagnostics of the last launch:
 *   "last_f32_config"  tile configuration index (-1 none yet, -2 small-matrix kernel, -3 direct small-channel conv kernel)
 *   "last_f32_asm" / "last_f64_asm" / "last_i32_asm"  0 = compiler-scheduled kernel, else 1 + index of the assembly kernel (gemm_f32_asm.cpp)
 *   "last_narrow_mfma" 1 = the last int8 / int16 GEMM ran on the matrix cores, 0 = a VALU / streaming kernel
 *   "last_asm_wgs" / "last_asm_slices"  workgroups and K slices per tile of the last assembly launch (slices 1 = tiles never cut)
 *   "last_asm_rem"     tiles the last assembly launch left to the K-cut launch of a hybrid plan (0: one launch)
 *   "last_asm_group_m"  its raster group height in tile rows (which tiles share an XCD's L2), + 65536 when the workgroup ids were
 *                      chunked per XCD
 *   "asm_fixup_timeouts"  streams of the current device on which a workgroup of a cut launch gave up waiting for a hand-over (0 in a
 *                      correct run; reading it synchronises the device, and a stream reported here has its hand-over flags reset)
 *   "last_conv_tail"   how the last convolution's pixel tail ran: 0 no tail, 1 the direct tail kernel, 2 kc slices + combine, 3 one
 *                      compiler-kernel launch
 *   "last_split"       column where the last compiler-scheduled float GEMM / conv launch was cut into main + tail (0 = one launch)
 *   "foreach_compiles" hiprtc compiles of forEach and forEachReduce bodies made by this process
 *   "last_foreach_variant"  kernel of the last laser_hip_foreach_dev / foreach_reduce_dev launch: 0 contiguous vectorised, 1 contiguous
 *                      scalar, 2 strided
 *   "last_reduce_variant"  traversal of the last laser_hip_reduce_* call: 0 contiguous vectorised, 1 contiguous scalar, 2 strided
 *   "last_softmax_kernel"  kernel of the last laser_hip_softmax_rows_f32_dev / _axis_f32_dev call (0 - 2 rows, 8 - 9 column
 *                          strips, + 4 single-element accesses; see the softmax section below)
 *   "shard_rccl_ranks" ranks of the RCCL communicator the last GATHER_RCCL sharded call used, as the communicator reports it; 0 = none yet */
int laser_hip_set_option(const char *name, int value);
int laser_hip_get_option(const char *name, int64_t *value);
const char *laser_hip_f32_config_name(int cfg);

/* ---- gemm_strided -- laser/primitives/matrix_multiplication/gemm.nim:184-193 ------------------
 * proc gemm_strided*[T: SomeNumber](M, N, K: int, alpha: T, A: ptr T, rowStrideA, colStrideA: int,
 *        B: ptr T, rowStrideB, colStrideB: int, beta: T, C: ptr T, rowStrideC, colStrideC: int) */
#define LASER_HIP_DECL_GEMM(SFX, T)                                                               \
  int laser_hip_gemm_strided_##SFX(int64_t M, int64_t N, int64_t K, T alpha, const T *A,          \
                                   int64_t rowStrideA, int64_t colStrideA, const T *B,            \
                                   int64_t rowStrideB, int64_t colStrideB, T beta, T *C,          \
                                   int64_t rowStrideC, int64_t colStrideC);                       \
  int laser_hip_gemm_strided_##SFX##_dev(int64_t M, int64_t N, int64_t K, T alpha, const T *dA,   \
                                         int64_t rowStrideA, int64_t colStrideA, const T *dB,     \
                                         int64_t rowStrideB, int64_t colStrideB, T beta, T *dC,   \
                                         int64_t rowStrideC, int64_t colStrideC, void *stream);   \
  /* `batch` independent problems; operand b starts at ptr + b*batchStrideX (elements; 0 shares). \
   * Used by the convolution (one GEMM per image, conv2d_im2col.nim:126-166).                     \
   * The entries of A and of B may overlap or be shared, and any batch stride may be zero or      \
   * negative (entry 0 then lies at the far end); the elements of C the call addresses must be    \
   * pairwise distinct over the whole batch.  batch <= 65535 (more is LASER_HIP_E_INVALID, C      \
   * untouched); batch == 0 and K == 0 leave C untouched. */                                      \
  int laser_hip_gemm_strided_batched_##SFX##_dev(                                                 \
      int64_t batch, int64_t M, int64_t N, int64_t K, T alpha, const T *dA, int64_t rowStrideA,   \
      int64_t colStrideA, int64_t batchStrideA, const T *dB, int64_t rowStrideB,                  \
      int64_t colStrideB, int64_t batchStrideB, T beta, T *dC, int64_t rowStrideC,                \
      int64_t colStrideC, int64_t batchStrideC, void *stream);
LASER_HIP_DECL_GEMM(f32, float)
LASER_HIP_DECL_GEMM(f64, double)
LASER_HIP_DECL_GEMM(i32, int32_t)
LASER_HIP_DECL_GEMM(i64, int64_t)
#undef LASER_HIP_DECL_GEMM

/* ---- pre-packed GEMM -- gemm_prepacked.nim:63-292 ----------------------------------------------
 * gemm_prepackB_mem_required*(T, M, N, K): int            :76-85
 * gemm_prepackB*[T](dst_packedB, M, N, K, src_B, rowStrideB, colStrideB)   :111-135
 * gemm_prepackA_mem_required*, gemm_prepackA*             :157-218
 * gemm_packed*[T](M, N, K, alpha, packedA, packedB, beta, C, rowStrideC, colStrideC)  :275-292
 *
 * As in the reference the packed buffers are opaque, machine dependent and "unsafe to store or
 * serialize" (:120-123).  Host variant: the caller allocates `mem_required` bytes, 64-B aligned
 * (same doAssert as :125/:208 -> LASER_HIP_E_INVALID), and the buffer is SELF-CONTAINED like the
 * reference's (:111-135, Design.md:5-7): a 64-byte header followed by the tile-padded panel image.
 * It may be copied with memcpy and freed at will.  gemm_packed multiplies from a device-resident
 * copy of the image that the library caches (made by the prepack call; re-made from the caller's
 * buffer when it is missing; bounded -- least recently used first -- so freeing buffers without
 * telling the library cannot leak HBM).  laser_hip_gemm_prepack_release(dst) drops the cached copy
 * early and invalidates the buffer (optional); laser_hip_finalize() drops them all.
 * `_dev` variant: dst is a DEVICE buffer of `mem_required` bytes that receives the padded panel
 * image itself at offset 0 (no header, nothing cached).  Unlike the reference (whose prepackA
 * indexing is only right for K <= kc, :186/:265) these are valid for every K. */
#define LASER_HIP_DECL_PACK(SFX, T)                                                               \
  int64_t laser_hip_gemm_prepackA_mem_required_##SFX(int64_t M, int64_t N, int64_t K);            \
  int64_t laser_hip_gemm_prepackB_mem_required_##SFX(int64_t M, int64_t N, int64_t K);            \
  int laser_hip_gemm_prepackA_##SFX(void *dst_packedA, int64_t M, int64_t N, int64_t K,           \
                                    const T *src_A, int64_t rowStrideA, int64_t colStrideA);      \
  int laser_hip_gemm_prepackB_##SFX(void *dst_packedB, int64_t M, int64_t N, int64_t K,           \
                                    const T *src_B, int64_t rowStrideB, int64_t colStrideB);      \
  int laser_hip_gemm_packed_##SFX(int64_t M, int64_t N, int64_t K, T alpha, const void *packedA,  \
                                  const void *packedB, T beta, T *C, int64_t rowStrideC,          \
                                  int64_t colStrideC);                                            \
  int laser_hip_gemm_prepackA_##SFX##_dev(void *d_dst, int64_t M, int64_t N, int64_t K,           \
                                          const T *dA, int64_t rowStrideA, int64_t colStrideA,    \
                                          void *stream);                                          \
  int laser_hip_gemm_prepackB_##SFX##_dev(void *d_dst, int64_t M, int64_t N, int64_t K,           \
                                          const T *dB, int64_t rowStrideB, int64_t colStrideB,    \
                                          void *stream);                                          \
  int laser_hip_gemm_packed_##SFX##_dev(int64_t M, int64_t N, int64_t K, T alpha,                 \
                                        const void *d_packedA, const void *d_packedB, T beta,     \
                                        T *dC, int64_t rowStrideC, int64_t colStrideC,            \
                                        void *stream);
LASER_HIP_DECL_PACK(f32, float)
LASER_HIP_DECL_PACK(f64, double)
LASER_HIP_DECL_PACK(i32, int32_t)
LASER_HIP_DECL_PACK(i64, int64_t)
#undef LASER_HIP_DECL_PACK

/* ---- gemm_strided / pre-packed GEMM for int8 and int16 (gemm.nim:184-248: every SomeNumber) -----------------
 * The same entry points as above for the narrow integer types, uint8 / uint16 on the same bits (two's-complement
 * wrap-around mod 2^8 / 2^16, the reference's gemm.nim:239 treatment of int32 / uint32).  alpha and beta travel as
 * int32_t and are reduced mod 2^8 / 2^16.  No _sharded and no fused-epilogue (_ex) form. */
#define LASER_HIP_DECL_GEMM_NARROW(SFX, T)                                                        \
  int laser_hip_gemm_strided_##SFX(int64_t M, int64_t N, int64_t K, int32_t alpha, const T *A,    \
                                   int64_t rowStrideA, int64_t colStrideA, const T *B,            \
                                   int64_t rowStrideB, int64_t colStrideB, int32_t beta, T *C,    \
                                   int64_t rowStrideC, int64_t colStrideC);                       \
  int laser_hip_gemm_strided_##SFX##_dev(int64_t M, int64_t N, int64_t K, int32_t alpha,          \
                                         const T *dA, int64_t rowStrideA, int64_t colStrideA,     \
                                         const T *dB, int64_t rowStrideB, int64_t colStrideB,     \
                                         int32_t beta, T *dC, int64_t rowStrideC,                 \
                                         int64_t colStrideC, void *stream);                       \
  int laser_hip_gemm_strided_batched_##SFX##_dev(                                                 \
      int64_t batch, int64_t M, int64_t N, int64_t K, int32_t alpha, const T *dA,                 \
      int64_t rowStrideA, int64_t colStrideA, int64_t batchStrideA, const T *dB,                  \
      int64_t rowStrideB, int64_t colStrideB, int64_t batchStrideB, int32_t beta, T *dC,          \
      int64_t rowStrideC, int64_t colStrideC, int64_t batchStrideC, void *stream);                \
  int64_t laser_hip_gemm_prepackA_mem_required_##SFX(int64_t M, int64_t N, int64_t K);            \
  int64_t laser_hip_gemm_prepackB_mem_required_##SFX(int64_t M, int64_t N, int64_t K);            \
  int laser_hip_gemm_prepackA_##SFX(void *dst_packedA, int64_t M, int64_t N, int64_t K,           \
                                    const T *src_A, int64_t rowStrideA, int64_t colStrideA);      \
  int laser_hip_gemm_prepackB_##SFX(void *dst_packedB, int64_t M, int64_t N, int64_t K,           \
                                    const T *src_B, int64_t rowStrideB, int64_t colStrideB);      \
  int laser_hip_gemm_packed_##SFX(int64_t M, int64_t N, int64_t K, int32_t alpha,                 \
                                  const void *packedA, const void *packedB, int32_t beta, T *C,   \
                                  int64_t rowStrideC, int64_t colStrideC);                        \
  int laser_hip_gemm_prepackA_##SFX##_dev(void *d_dst, int64_t M, int64_t N, int64_t K,           \
                                          const T *dA, int64_t rowStrideA, int64_t colStrideA,    \
                                          void *stream);                                          \
  int laser_hip_gemm_prepackB_##SFX##_dev(void *d_dst, int64_t M, int64_t N, int64_t K,           \
                                          const T *dB, int64_t rowStrideB, int64_t colStrideB,    \
                                          void *stream);                                          \
  int laser_hip_gemm_packed_##SFX##_dev(int64_t M, int64_t N, int64_t K, int32_t alpha,           \
                                        const void *d_packedA, const void *d_packedB,             \
                                        int32_t beta, T *dC, int64_t rowStrideC,                  \
                                        int64_t colStrideC, void *stream);
LASER_HIP_DECL_GEMM_NARROW(i8, int8_t)
LASER_HIP_DECL_GEMM_NARROW(i16, int16_t)
#undef LASER_HIP_DECL_GEMM_NARROW
int laser_hip_gemm_prepack_release(void *packed);

/* ---- physical transposes -- laser/primitives/swapaxes.nim:16-112 --------------------------------
 * transpose2D_copy*[T](dst, src, NR, NC)        :16-54   dst[j][i] = src[i][j]
 * transpose2D_batched*[T](dst, src, N, NR, NC)  :56-84
 * nchw2nhwc*[T](dst, src, N, C, H, W)           :86-98   = transpose2D_batched(N, C, H*W)
 * nhwc2nchw*[T](dst, src, N, C, H, W)           :100-112 = transpose2D_batched(N, H*W, C)
 * Pure data movement, generic in T like the reference: one entry point per element SIZE (b32: float32 / int32, b64: float64 /
 * int64, b16: float16 / int16, b8: int8 / uint8). */
#define LASER_HIP_DECL_TR(SFX)                                                                    \
  int laser_hip_transpose2d_copy_##SFX(void *dst, const void *src, int64_t NR, int64_t NC);       \
  int laser_hip_transpose2d_batched_##SFX(void *dst, const void *src, int64_t N, int64_t NR,      \
                                          int64_t NC);                                            \
  int laser_hip_nchw2nhwc_##SFX(void *dst, const void *src, int64_t N, int64_t C, int64_t H,      \
                                int64_t W);                                                       \
  int laser_hip_nhwc2nchw_##SFX(void *dst, const void *src, int64_t N, int64_t C, int64_t H,      \
                                int64_t W);                                                       \
  int laser_hip_transpose2d_batched_##SFX##_dev(void *d_dst, const void *d_src, int64_t N,        \
                                                int64_t NR, int64_t NC, void *stream);
LASER_HIP_DECL_TR(b32)
LASER_HIP_DECL_TR(b64)
LASER_HIP_DECL_TR(b16)
LASER_HIP_DECL_TR(b8)
#undef LASER_HIP_DECL_TR

/* ---- im2col + GEMM convolution -- benchmarks/convolution/conv2d_im2col.nim -----------------------
 * TensorShape = (n, c, h, w), KernelShape = (c_out, c_in, kH, kW), Padding = (h, w),
 * Strides = (h, w) (conv2d_common.nim:6-13) are passed as separate scalars.
 * conv2d_out_shape                           conv2d_common.nim:15-45
 * im2col_workspace_size*(ishape, kshape, padding, strides): int      conv2d_im2col.nim:10-20
 * im2col*[T](pworkspace, oshape, pinput, ishape, kshape, padding, strides)     :42-88
 * conv2d_im2col*(output, oshape, input, ishape, kernel, kshape, padding, strides, pworkspace) :90-166 */
int laser_hip_conv2d_out_shape(int64_t iN, int64_t iC, int64_t iH, int64_t iW, int64_t c_out,
                               int64_t c_in, int64_t kH, int64_t kW, int64_t padH, int64_t padW,
                               int64_t strideH, int64_t strideW, int64_t *oN, int64_t *oC,
                               int64_t *oH, int64_t *oW);
/* number of ELEMENTS, like the reference */
int64_t laser_hip_im2col_workspace_size(int64_t iN, int64_t iC, int64_t iH, int64_t iW,
                                        int64_t c_out, int64_t c_in, int64_t kH, int64_t kW,
                                        int64_t padH, int64_t padW, int64_t strideH,
                                        int64_t strideW);
/* One image [iC, iH, iW] -> workspace [iC*kH*kW, oH*oW].  im2col*[T] is generic in the reference (conv2d_im2col.nim:42-50):
 * _f32 and _f64 here (pure data movement; integer tensors of the same element size can be passed through a cast). */
int laser_hip_im2col_f32(float *pworkspace, int64_t oH, int64_t oW, const float *pinput, int64_t iC,
                         int64_t iH, int64_t iW, int64_t kH, int64_t kW, int64_t padH, int64_t padW,
                         int64_t strideH, int64_t strideW);
int laser_hip_im2col_f32_dev(float *d_workspace, int64_t oH, int64_t oW, const float *d_input,
                             int64_t batch, int64_t iC, int64_t iH, int64_t iW, int64_t kH,
                             int64_t kW, int64_t padH, int64_t padW, int64_t strideH,
                             int64_t strideW, void *stream);
int laser_hip_im2col_f64(double *pworkspace, int64_t oH, int64_t oW, const double *pinput, int64_t iC,
                         int64_t iH, int64_t iW, int64_t kH, int64_t kW, int64_t padH, int64_t padW,
                         int64_t strideH, int64_t strideW);
int laser_hip_im2col_f64_dev(double *d_workspace, int64_t oH, int64_t oW, const double *d_input,
                             int64_t batch, int64_t iC, int64_t iH, int64_t iW, int64_t kH,
                             int64_t kW, int64_t padH, int64_t padW, int64_t strideH,
                             int64_t strideW, void *stream);
/* output [iN, c_out, oH, oW] = conv(input [iN, iC, iH, iW], kernel [c_out, c_in, kH, kW]).
 * `pworkspace` (host variant) may be NULL: the scratch lives on the device; if non-NULL it must
 * hold im2col_workspace_size elements and receives the last image's im2col matrix, as in the
 * reference.  LASER_HIP_E_INVALID if c_in != iC (the reference asserts oshape.c == kshape.c_out,
 * :109, and conv2d_required_ops doAsserts C_in == kernel.c_in, conv2d_common.nim:66). */
int laser_hip_conv2d_im2col_f32(float *output, const float *input, int64_t iN, int64_t iC,
                                int64_t iH, int64_t iW, const float *kernel, int64_t c_out,
                                int64_t c_in, int64_t kH, int64_t kW, int64_t padH, int64_t padW,
                                int64_t strideH, int64_t strideW, float *pworkspace);
/* Device variant.  The default strategy (implicit GEMM) materialises nothing and ignores d_workspace.  On the
 * explicit path (kernels larger than 8x8, laser_hip_set_conv_implicit(0)) a non-NULL d_workspace is taken to hold
 * ONE image's im2col matrix -- im2col_workspace_size elements, the reference's contract ("can be reused between
 * batches", conv2d_im2col.nim:99) -- and the images are processed one by one through it; NULL = stream-ordered
 * library scratch (hipMallocAsync on `stream`), all images expanded in one pass and multiplied by one batched GEMM. */
int laser_hip_conv2d_im2col_f32_dev(float *d_output, const float *d_input, int64_t iN, int64_t iC,
                                    int64_t iH, int64_t iW, const float *d_kernel, int64_t c_out,
                                    int64_t c_in, int64_t kH, int64_t kW, int64_t padH,
                                    int64_t padW, int64_t strideH, int64_t strideW,
                                    float *d_workspace, void *stream);

/* ---- fused epilogue ------------------------------------------------
 * The reference plans it but does not have it: "fusing unary operations (like max/relu, tanh or
 * sigmoid) and binary operations (like adding a bias) at the end of the matrix multiplication
 * kernels" (README.md:238-242; TODOs gemm.nim:196, gemm_ukernel_generic.nim:78-79,128-129).
 *   C[i,j] = act( alpha*A*B + beta*C  +  bias[i*rowStrideBias + j*colStrideBias] )
 * The GEMM part is exactly gemm_strided (same accumulation order, same K == 0 rule: nothing is
 * touched); the bias is added with one more rounding after the LAST accumulation slice, then the
 * activation is applied -- once, on the accumulator, before the only store of C.  `bias` is a strided
 * M x N view whose strides may be 0: (1,0) = one value per row of C (a convolution's per-channel
 * bias), (0,1) = one per column (a dense layer's), (ldb,1) = a full residual matrix; NULL = none.
 * float32 / float64 only (the activations are floating-point functions). */
/* Fused PROLOGUE (the other half of the reference's fusion roadmap, README.md:243-244: "fuse operations before the matrix
 * multiplication kernel, during the prepacking ... for backward propagation"): OR these bits into `activation` and the product is
 * taken of relu(A) and / or relu(B), elementwise x > 0 ? x : 0, applied as the operand tile travels from HBM into the LDS panel
 * image (float32: the assembly kernels' `_pre` variants, in the staging registers; other paths: in the one packing pass the
 * operand gets anyway, or one made for it).  C = act(alpha * pre(A) * pre(B) + beta * C + bias). */
#define LASER_HIP_PRE_RELU_A 0x100
#define LASER_HIP_PRE_RELU_B 0x200
#define LASER_HIP_ACT_NONE 0
#define LASER_HIP_ACT_RELU 1     /* x > 0 ? x : 0 */
#define LASER_HIP_ACT_TANH 2
#define LASER_HIP_ACT_SIGMOID 3  /* 1 / (1 + exp(-x)) */
#define LASER_HIP_DECL_GEMM_EX(SFX, T)                                                            \
  int laser_hip_gemm_strided_ex_##SFX(int64_t M, int64_t N, int64_t K, T alpha, const T *A,       \
                                      int64_t rowStrideA, int64_t colStrideA, const T *B,         \
                                      int64_t rowStrideB, int64_t colStrideB, T beta, T *C,       \
                                      int64_t rowStrideC, int64_t colStrideC, const T *bias,      \
                                      int64_t rowStrideBias, int64_t colStrideBias,               \
                                      int activation);                                            \
  int laser_hip_gemm_strided_ex_##SFX##_dev(int64_t M, int64_t N, int64_t K, T alpha, const T *dA, \
                                            int64_t rowStrideA, int64_t colStrideA, const T *dB,  \
                                            int64_t rowStrideB, int64_t colStrideB, T beta, T *dC, \
                                            int64_t rowStrideC, int64_t colStrideC,               \
                                            const T *d_bias, int64_t rowStrideBias,               \
                                            int64_t colStrideBias, int activation, void *stream);
LASER_HIP_DECL_GEMM_EX(f32, float)
LASER_HIP_DECL_GEMM_EX(f64, double)
#undef LASER_HIP_DECL_GEMM_EX
/* conv2d_im2col with a per-output-channel bias ([c_out] or NULL) and an activation fused into the
 * implicit GEMM's store (signature = laser_hip_conv2d_im2col_f32[_dev] + bias, activation). */
int laser_hip_conv2d_im2col_ex_f32(float *output, const float *input, int64_t iN, int64_t iC,
                                   int64_t iH, int64_t iW, const float *kernel, int64_t c_out,
                                   int64_t c_in, int64_t kH, int64_t kW, int64_t padH, int64_t padW,
                                   int64_t strideH, int64_t strideW, float *pworkspace,
                                   const float *bias, int activation);
int laser_hip_conv2d_im2col_ex_f32_dev(float *d_output, const float *d_input, int64_t iN, int64_t iC,
                                       int64_t iH, int64_t iW, const float *d_kernel, int64_t c_out,
                                       int64_t c_in, int64_t kH, int64_t kW, int64_t padH,
                                       int64_t padW, int64_t strideH, int64_t strideW,
                                       float *d_workspace, const float *d_bias, int activation,
                                       void *stream);

/* ---- device tensor storage -----------------------------------------
 * The device twin of CpuStorage / allocCpuStorage and of the data-moving procs of
 * laser/tensor/initialization.nim, so that a Tensor[T]-shaped object (shape, strides, offset,
 * storage -- laser/tensor/datatypes.nim:18-30) can keep its buffer in HBM and chains of
 * gemm_strided / transposes / conv never cross PCIe.  The Tensor object itself stays on the host
 * language's side (nim/laser_hip.nim, include/laser.hpp, laser_amd/tensor.py); only raw buffers and
 * strides cross this ABI, as for every other entry point.
 *   storage_alloc    allocCpuStorage (allocator.nim:17-29): `bytes` of device memory, aligned to at
 *                    least LASER_MEM_ALIGN = 64 and zero-filled (allocShared0)
 *   storage_free     the storage finalizer (allocator.nim:11-15)
 *   storage_upload   copyFromRaw (initialization.nim:112-128): host buffer -> device storage
 *   storage_download the reverse (reading results back)
 *   storage_set_zero setZero (initialization.nim:130-154) on a contiguous extent
 *   copy_strided     `forEachStrided d in dst, s in src: d = s` (deepCopy / copyFrom of views,
 *                    initialization.nim:42-110): rank <= 6 (LASER_MAXRANK), element strides, same shape */
int laser_hip_storage_alloc(void **d_raw_buffer, int64_t bytes);
int laser_hip_storage_free(void *d_raw_buffer);
/* freed storages are cached per size for reuse (a device allocation costs ~100 us); this releases the cache */
int laser_hip_storage_trim(void);
int laser_hip_storage_upload(void *d_dst, const void *host_src, int64_t bytes);
int laser_hip_storage_download(void *host_dst, const void *d_src, int64_t bytes);
int laser_hip_storage_set_zero(void *d_buffer, int64_t bytes, void *stream);
/* Stream-ordered forms.  The plain storage_alloc completes its zero fill before returning and the plain upload /
 * download run on the NULL stream, which does NOT wait for non-blocking streams (PyTorch's side streams, any
 * hipStreamNonBlocking stream): a caller that computes on its own stream uses these so that the zero fill precedes
 * the first kernel on that stream, an upload follows the last reader and a download follows the producer.  Upload and
 * download are complete when the call returns.  storage_alloc_stream and storage_set_zero never synchronise the host.
 * A storage belongs to the stream it was allocated on (the NULL stream for the plain storage_alloc): storage_free
 * records, on that stream, the point after which a cached block may be handed out again, and the next storage_alloc_stream
 * of the block is ordered behind that point on the device (on the same stream by stream order alone).  A caller that
 * also uses a storage on ANOTHER stream orders that use before the free itself (an event, or a host wait), as with any
 * stream-ordered allocator. */
int laser_hip_storage_alloc_stream(void **d_raw_buffer, int64_t bytes, void *stream);
int laser_hip_storage_upload_stream(void *d_dst, const void *host_src, int64_t bytes, void *stream);
int laser_hip_storage_download_stream(void *host_dst, const void *d_src, int64_t bytes, void *stream);
int laser_hip_copy_strided_b32_dev(void *d_dst, const int64_t *dst_strides, const void *d_src,
                                   const int64_t *src_strides, const int64_t *shape, int rank,
                                   void *stream);
int laser_hip_copy_strided_b64_dev(void *d_dst, const int64_t *dst_strides, const void *d_src,
                                   const int64_t *src_strides, const int64_t *shape, int rank,
                                   void *stream);

/* ---- elementwise map over strided device views: the device twin of forEach ----------------------------------------
 * Laser's forEach / forEachStrided (laser/strided_iteration/foreach.nim:192-264) is a host macro over raw pointers
 * (`unsafe_raw_data`) with an odometer over shape / strides (foreach_common.nim:102-120).  A tensor whose storage lives
 * in HBM must never be handed to it (the host would dereference a device address: the Nim shim gives device storage a
 * distinct pointer type and no unsafe_raw_data for exactly that reason).  These entry points are what such tensors use
 * instead:      dst[idx] = f(a[idx])      /      dst[idx] = f(a[idx], b[idx])       for every index of `shape`
 * rank <= 6 (LASER_MAXRANK), every operand with its own ELEMENT strides (0 = broadcast along that dimension), dst may
 * alias a or b element for element.  alpha / beta (of the ELEMENT type, like gemm_strided's) are parameters of SCALE /
 * FILL / AXPY / AXPBY.  Element types f32, f64, i32, i64.  The ops are the arithmetic ones tensor initialisation needs
 * (laser/tensor/initialization.nim:42-154); SIMD exp / log and friends are out of scope.  HBM-bound,
 * asynchronous on `stream`. */
#define LASER_HIP_MAP_COPY 0     /* a                     (= copy_strided) */
#define LASER_HIP_MAP_FILL 1     /* alpha                 (no operand read; `a` may be NULL) */
#define LASER_HIP_MAP_NEG 2
#define LASER_HIP_MAP_ABS 3
#define LASER_HIP_MAP_RELU 4     /* a > 0 ? a : 0 */
#define LASER_HIP_MAP_SCALE 5    /* alpha*a + beta        (two roundings) */
#define LASER_HIP_MAP_SQUARE 6
#define LASER_HIP_MAP_ADD 32     /* binary from here on */
#define LASER_HIP_MAP_SUB 33
#define LASER_HIP_MAP_MUL 34
#define LASER_HIP_MAP_MAX 36
#define LASER_HIP_MAP_MIN 37
#define LASER_HIP_MAP_AXPY 38    /* alpha*a + b */
#define LASER_HIP_MAP_AXPBY 39   /* alpha*a + beta*b */
#define LASER_HIP_DECL_MAP(SFX, T)                                                                \
  int laser_hip_map_strided_unary_##SFX##_dev(int op, T *d_dst, const int64_t *dst_strides,        \
                                              const T *d_a, const int64_t *a_strides,              \
                                              const int64_t *shape, int rank, T alpha, T beta,     \
                                              void *stream);                                       \
  int laser_hip_map_strided_binary_##SFX##_dev(int op, T *d_dst, const int64_t *dst_strides,       \
                                               const T *d_a, const int64_t *a_strides,             \
                                               const T *d_b, const int64_t *b_strides,             \
                                               const int64_t *shape, int rank, T alpha, T beta,    \
                                               void *stream);
LASER_HIP_DECL_MAP(f32, float)
LASER_HIP_DECL_MAP(f64, double)
LASER_HIP_DECL_MAP(i32, int32_t)
LASER_HIP_DECL_MAP(i64, int64_t)
#undef LASER_HIP_DECL_MAP

/* ---- forEach with a body: laser/strided_iteration/foreach.nim:192-264 --------------------------------------------
 *   forEach x in a, y in b, z in c:  x += y * z
 * over device views: for every index of `shape`, each named operand is bound to its element, the body runs, and the
 * writable operands are stored back.  The body is HIP C++ (Laser's statement syntax `x += y * z`, `x = y > 0 ? y : 0` is
 * valid C++; statements are separated by `;`, a trailing one is optional) and may call the device math library (expf,
 * logf, sqrtf, fmaxf, ...).  It is compiled at run time with hiprtc (libhiprtc.so is loaded on first use; this library
 * does not link it) with -O3 -std=c++17 -ffp-contract=off -fwrapv: no fast-math, no denormal flushing, so + - * / on
 * floats give the bits numpy or a host loop gives, integer arithmetic wraps mod 2^n like numpy, and sqrtf / divisions are
 * the device library's correctly rounded forms.  Casts are C++'s: float -> int truncates, out-of-range is undefined.
 *
 * The spec -- every entry point below takes it, and it identifies one compiled kernel:
 *   body                          HIP C++ statements
 *   nops, names[], dtypes[], writable[]
 *                                 1..8 operands: name, element type (LASER_HIP_DT_*), non-zero = written back.  Read-only
 *                                 operands are `const` locals: assigning to one is a compile error.
 *   nparams, param_names[], param_dtypes[]
 *                                 0..8 scalar parameters (`const` locals of their type); their VALUES are launch
 *                                 arguments, so changing them does not compile again
 *   Names are C identifiers, unique, not C++ keywords, not starting with `lh_` (the template's prefix) or `__`; anything
 *   else (and an unknown dtype code, too many operands or parameters) is LASER_HIP_E_INVALID.
 *
 * foreach_source   the generated HIP source (NUL-terminated) into buf; *len = bytes needed including the NUL; buf == NULL
 *                  asks for the size only; cap < *len is LASER_HIP_E_INVALID.  Host code only, needs no device.
 * foreach_code     compiles for `arch` (e.g. "gfx950") and returns the code object (an amdgcn ELF, same buffer rules).  Loads
 *                  nothing, needs no device.  An arch naming xnack+ is LASER_HIP_E_INVALID.
 * foreach_kernel   compiles for the current device (its gcnArchName as reported), loads the module and returns a handle.
 *                  Cached per (device, spec) for the life of the process: a second call with the same spec does not
 *                  compile, and concurrent first calls compile once.  No gfx950 device: LASER_HIP_E_NODEVICE.
 * foreach_dev      launches, asynchronous on `stream`, on the device the handle was made for (the current device).
 *                  ptrs[k]: operand k's device address; strides: nops x rank ELEMENT strides (row k = operand k, negative
 *                  allowed; 0 = broadcast, allowed on read-only operands only -- LASER_HIP_E_INVALID on a writable one);
 *                  rank <= 6 (LASER_MAXRANK); params: nparams 8-byte slots, parameter j's value in the low bytes of slot j.
 *                  A writable operand may alias a read operand element for element; partial overlap is undefined.  Size 0
 *                  is a no-op.  Kernels (get_option "last_foreach_variant"): 0 = every operand C-contiguous and aligned to
 *                  16 bytes of the widest operand's vector -> 16-byte loads / stores per lane; 1 = contiguous with an
 *                  unaligned base; 2 = strided (dimensions merged as map_strided does).
 * Errors: LASER_HIP_E_COMPILE when the body does not compile or hiprtc cannot be loaded -- laser_hip_last_error() holds the
 * compiler's log.  get_option "foreach_compiles": hiprtc compiles made by this process (forEachReduce's included). */
#define LASER_HIP_DT_F32 0
#define LASER_HIP_DT_F64 1
#define LASER_HIP_DT_I8 2
#define LASER_HIP_DT_I16 3
#define LASER_HIP_DT_I32 4
#define LASER_HIP_DT_I64 5
#define LASER_HIP_DT_U8 6
#define LASER_HIP_DT_U16 7
#define LASER_HIP_DT_U32 8
#define LASER_HIP_DT_U64 9
int laser_hip_foreach_source(const char *body, int nops, const char *const *names, const int *dtypes,
                             const int *writable, int nparams, const char *const *param_names,
                             const int *param_dtypes, char *buf, int64_t cap, int64_t *len);
int laser_hip_foreach_code(const char *body, int nops, const char *const *names, const int *dtypes,
                           const int *writable, int nparams, const char *const *param_names,
                           const int *param_dtypes, const char *arch, void *buf, int64_t cap, int64_t *len);
int laser_hip_foreach_kernel(const char *body, int nops, const char *const *names, const int *dtypes,
                             const int *writable, int nparams, const char *const *param_names,
                             const int *param_dtypes, int64_t *handle);
int laser_hip_foreach_dev(int64_t handle, void *const *ptrs, const int64_t *strides, const int64_t *shape, int rank,
                          const void *params, void *stream);

/* ---- Reductions: laser/primitives/reductions.nim:48-116 (reduce_sum / reduce_min / reduce_max) --------------------
 * One number from a strided device view.  Unlike the reference's OpenMP sum, which "can give different results depending
 * on thread timings", the order of the operations is fixed: it is a function of the element count alone, never of the
 * device, the CU count, the grid, the stream, the base alignment or the strides.  In words:
 *   x[0..n) are the elements in the row-major logical order of `shape`.  E = 16 / (bytes of the widest operand): 4 for f32
 *   and i32, 2 for f64 and i64, 16 for int8.  W = LASER_HIP_REDUCE_LANES, R = LASER_HIP_REDUCE_STEPS; a chunk is S = R*W*E
 *   elements.  In chunk c, lane t keeps E accumulators, each starting at `init`; for r = 0..R-1, then j = 0..E-1, it
 *   applies the body to element c*S + r*W*E + t*E + j and accumulator j; elements at or past n are skipped.  The E
 *   accumulators are folded by halving (the upper half merged onto the lower half, repeated), then the W lane results the
 *   same way (lane t with t + W/2, then t + W/4, ...): the chunk's partial.  More than one chunk: the array of partials is
 *   reduced by the same rule with E = 16 / (bytes of the accumulator) and `merge` as the body, until one value is left.
 *   n = 0 gives `init`.  No float atomics: partials are plain stores into stream-ordered scratch, one launch per level.
 * reduce_sum accumulates in the element type (no denormal flushing; integers wrap mod 2^n like numpy's sum with
 * dtype = the element type).  reduce_min / reduce_max do not depend on the order at all: any NaN gives NaN (payload
 * unspecified), -0 ranks below +0 (min {+0, -0} = -0, max = +0), otherwise the true min / max.  Empty: sum 0, min +Inf /
 * the integer type's max, max -Inf / its min.
 * _dev forms: asynchronous on `stream`, never synchronise the host; rank <= 6 ELEMENT strides, negative and 0 (broadcast)
 * allowed; the result goes to the device address d_out.  get_option "last_reduce_variant": 0 = C-contiguous, 16-byte
 * aligned (one 16-byte vector per lane and step), 1 = contiguous with an unaligned base, 2 = strided -- same bits all three.
 * Host form (f32): the reference's `reduce_*(data: ptr float32, len: Natural): float32` -- synchronous, result in *out,
 * the same bits as the _dev form on the same values.  No gfx950 device: LASER_HIP_E_NODEVICE. */
#define LASER_HIP_REDUCE_LANES 256
#define LASER_HIP_REDUCE_STEPS 8
#define LASER_HIP_DECL_REDUCE(SFX, T)                                                                                  \
  int laser_hip_reduce_sum_##SFX##_dev(const T *d_src, const int64_t *strides, const int64_t *shape, int rank,          \
                                       T *d_out, void *stream);                                                        \
  int laser_hip_reduce_min_##SFX##_dev(const T *d_src, const int64_t *strides, const int64_t *shape, int rank,          \
                                       T *d_out, void *stream);                                                        \
  int laser_hip_reduce_max_##SFX##_dev(const T *d_src, const int64_t *strides, const int64_t *shape, int rank,          \
                                       T *d_out, void *stream);
LASER_HIP_DECL_REDUCE(f32, float)
LASER_HIP_DECL_REDUCE(f64, double)
LASER_HIP_DECL_REDUCE(i32, int32_t)
LASER_HIP_DECL_REDUCE(i64, int64_t)
#undef LASER_HIP_DECL_REDUCE
int laser_hip_reduce_sum_f32(const float *data, int64_t len, float *out);
int laser_hip_reduce_min_f32(const float *data, int64_t len, float *out);
int laser_hip_reduce_max_f32(const float *data, int64_t len, float *out);

/* ---- exp and row softmax (f32): laser/primitives/simd_math/exp_log_{sse2,avx2,avx512}.nim --------------------------
 * lexp(x) is Laser's table-driven exp, bit for bit the exported SIMD `exp*` (not the unexported scalar fallback, which
 * truncates where the SIMD forms round).  One definition, laser_amd/csrc/exp_core.h, shared by every kernel below and by
 * the forEach bodies.  For a float32 x, every operation rounded to float32 on its own (no fused multiply-add anywhere):
 *   1. NaN gives NaN (payload unspecified; the one deviation: x86 minps turns NaN into 88).  c = max(min(x, 88), -88);
 *      +-Inf clamp like any other value.
 *   2. r = int32(round-to-nearest-even(c * ExpA)),  ExpA = bits 0x44b8aa3b = float32(1024 / ln 2).
 *   3. t = (c - float(r) * ExpB) + 1,  ExpB = bits 0x3a317218 = float32(ln 2 / 1024): a multiply, a subtract, an add.
 *   4. v = r & 1023;  u = ((r + (127 << 10)) >> 10) << 23  (r + (127 << 10) is never negative).
 *   5. lexp(x) = t * bitcast<float>(LUT[v] | u), one multiply.  LUT[i] = the low 23 bits of the correctly rounded float32
 *      of 2^(i/1024), i = 0..1023 (as little-endian uint32 words the table has CRC-32 0x0c4cd4ff).
 * For x below about -87.3369 the exponent field u is 0, the second factor is subnormal and the product is not an
 * exponential any more -- exactly as in Laser; no denormal is flushed.  Relative error elsewhere: about 1e-6 on [-30, 0],
 * 4e-6 on [-87, 88].
 * laser_hip_exp_f32_dev: dst[idx] = lexp(src[idx]) for every index of `shape`; rank <= 6, ELEMENT strides, negative
 *   strides allowed, stride 0 (broadcast) on src only, dst == src with equal strides allowed (any other overlap is not).
 *   Asynchronous on `stream`.  C-contiguous and 16-byte aligned on both sides: one 16-byte vector per lane and step.
 * laser_hip_exp_f32: host pointers, `len` contiguous elements, synchronous (the reference's benchmark loop).
 * laser_exp(x) is callable in forEach / forEachReduce bodies: the prelude of their generated source embeds exp_core.h
 *   (laser_hip_foreach_source shows it).  The name is reserved like the lh_ names.
 * laser_hip_softmax_rows_f32_dev: for each of `rows` rows x[0..n) at d_src + row * src_row_stride (elements of a row
 *   contiguous, row strides in elements and >= n):
 *   1. m = the maximum of the row under the rule of reduce_max ("Reductions": any NaN gives NaN).
 *   2. e[j] = lexp(x[j] - m), one rounded subtract.
 *   3. s = the sum of e[0..n) in the order of "Reductions" applied to the row as a 1-D array of n float32 (E = 4,
 *      init +0): s is reduce_sum of e.
 *   4. y[j] = e[j] / s, a correctly rounded division; y goes to d_dst + row * dst_row_stride.
 *   So a row's result is a function of its values and n alone, never of rows, the strides, the base alignment, the
 *   grid or the stream.  A NaN in a row makes the whole output row NaN; so does a row of all -Inf (x - m = NaN) and a
 *   row whose maximum is +Inf.  1 <= n <= 2^26, rows >= 0 (rows = 0: nothing happens), any base alignment, dst == src
 *   with equal row strides allowed; anything else LASER_HIP_E_INVALID.  Asynchronous on `stream`.
 *   get_option "last_softmax_kernel": 0 = one wave per row (n <= 1024), 1 = one workgroup per row (n <= 8192), 2 = long
 *   rows; + 4 when a base or a row stride is off its 16-byte alignment (single-element accesses) -- same bits all six.
 * laser_hip_softmax_axis_f32_dev: the same softmax along any axis.  The operand is viewed as (outer, n, inner): element
 *   x[o, k, i] is at d_src + o * src_outer_stride + k * src_axis_stride + i (ELEMENT strides; the inner index has stride 1),
 *   and for every (o, i) the 1-D array x[o, 0..n, i] gets exactly steps 1-4 above, the sum in the order of "Reductions"
 *   applied to that array as a 1-D array of n float32.  Bit for bit (any NaN equals any NaN)
 *     softmax_axis(X, axis) == moveaxis(softmax_rows(moveaxis(X, axis, -1) made contiguous), -1, axis):
 *   a column's bits never depend on its neighbours, on outer, inner, the strides, the base alignment, the strip width, the
 *   grid or the stream; a NaN column, an all -Inf column or a +Inf maximum makes that column NaN and no other.
 *   The sum tree in terms of k: within a chunk of 8192 elements, element k goes to leaf a = k mod 1024; a leaf starts at +0
 *   and takes its up to 8 elements in ascending k; the 1024 leaves are folded by adding the higher index into the lower for
 *   index pairs that differ in bit 1, then bit 0, then bit 9, 8, .., 2; the chunk partials (at most 128 here) are folded by
 *   the same rule as one more such array.
 *   Valid: outer >= 0 (0: nothing happens), n >= 1, inner >= 1, both axis strides >= inner and, for outer > 1, both outer
 *   strides >= (n - 1) * axis_stride + inner; dst == src with equal strides allowed (any other overlap is not); any base
 *   alignment.  inner == 1 with both axis strides 1 forwards to the row kernels (n <= 2^26); otherwise
 *   n <= LASER_HIP_SOFTMAX_AXIS_MAX_N (one workgroup walks a whole column; past that: LASER_HIP_E_INVALID, and the text says
 *   so).  Asynchronous on `stream`.  A workgroup owns a strip of CW consecutive inner positions of one outer index over all
 *   n, every access a run of CW * 4 contiguous bytes per row.
 *   get_option "last_softmax_kernel" after it: 8 = column strip, column resident (n <= 2048: one read, one write),
 *   9 = column strip, streaming (three reads, one write); + 4 for the single-element instance (a base or a stride off its
 *   16-byte alignment); 0 - 2 (+ 4) when it forwarded to the row kernels.
 * laser_hip_softmax_axis_plan: what the call above would launch for a shape, without a device: out4 = {kernel code, strip
 *   width CW (0 for the row kernels), workgroups, LDS bytes}.  vec: 1 when bases and strides allow 16-byte vectors; cus: the
 *   device's compute units, taken for symmetry with laser_hip_plan_f32: the grid is min(2048, strips) on every device and
 *   does not depend on it.  inner == 1 is planned with unit axis strides.  The logic is laser_amd/csrc/softmax_axis_plan.h, which has no HIP dependency.
 * Not built: float64, splitting one long column over several workgroups (few strips x long n keeps few compute units
 *   busy), backward.
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
#define LASER_HIP_SOFTMAX_MAX_N (1ll << 26)
#define LASER_HIP_SOFTMAX_AXIS_MAX_N (1ll << 20)   /* for inner > 1 */
int laser_hip_exp_f32_dev(float *d_dst, const int64_t *dst_strides, const float *d_src, const int64_t *src_strides,
                          const int64_t *shape, int rank, void *stream);
int laser_hip_exp_f32(float *dst, const float *src, int64_t len);
int laser_hip_softmax_rows_f32_dev(float *d_dst, int64_t dst_row_stride, const float *d_src, int64_t src_row_stride,
                                   int64_t rows, int64_t n, void *stream);
int laser_hip_softmax_axis_f32_dev(float *d_dst, int64_t dst_outer_stride, int64_t dst_axis_stride,
                                   const float *d_src, int64_t src_outer_stride, int64_t src_axis_stride,
                                   int64_t outer, int64_t n, int64_t inner, void *stream);
int laser_hip_softmax_axis_plan(int64_t outer, int64_t n, int64_t inner, int vec, int cus, int64_t *out4);

/* ---- log, logsumexp, log-softmax and cross-entropy (f32): from logits to a loss without leaving the device ---------------
 * The reference's simd_math files are named exp_log_* but hold no logarithm; llog is this library's own, defined the way
 * lexp is: one definition, laser_amd/csrc/log_core.h, shared by every kernel below and by the forEach bodies, built from
 * integer operations, bit casts, an exact float32 -> float64 conversion, float64 multiplies, adds and subtracts each rounded
 * on its own (no fused multiply-add, no division, no libm) and one float64 -> float32 rounding to nearest even.  For a
 * float32 x with bits b:
 *   1. NaN gives NaN (payload unspecified).  +-0 gives -Inf.  Any other x with the sign bit set, -Inf included, gives NaN.
 *      +Inf gives +Inf.
 *   2. A subnormal x is normalised in integers (shift its bits left until the exponent field reads 1 and count the shifts
 *      into the exponent), so no floating-point operation sees a subnormal and nothing depends on flushing.
 *   3. x = 2^k z with z in [0.69921875, 1.3984375): t = b - 0x3f330000 mod 2^32, k = int32(t) >> 23 (plus the count of
 *      step 2), i = (t >> 19) & 15, z = float64(bitcast<float>(b - (t & 0xff800000))).  The range is around 1, so next to 1
 *      nothing cancels: k = 0 there.
 *   4. r = z * INVC[i] - 1, INVC[i] = float64(1 / midpoint of the i-th sixteenth of the range); the sixteenth that holds 1
 *      has INVC = 1 and LOGC = +0, so there r = z - 1 exactly.  |r| < 0.02963.
 *   5. q = (((C6 r + C5) r + C4) r + C3) r + C2 with C_j = float64((-1)^(j+1) / j).
 *   6. y = ((float64(k) * LN2 + LOGC[i]) + r) + (r * r) * q, LOGC[i] = float64(-ln INVC[i]), LN2 = float64(ln 2).
 *   7. llog(x) = float32(y).   llog(1) = +0 exactly.
 * Two properties, proved over all 2^31 - 2^23 positive finite float32 on the CPU (tests/cpp/log_core_host.cpp "sweep"):
 *   faithful: llog(x) is one of the two float32 that bracket the true logarithm (error < 1 ulp; measured against
 *     (float)log((double)x): maximum 0.501403 ulp at x = bits 0x3f8301a3, mean 0.250000 ulp);
 *   monotone: non-decreasing over the positive float32 in increasing order.
 * laser_hip_log_f32_dev: dst[idx] = llog(src[idx]) for every index of `shape`; the contract of laser_hip_exp_f32_dev (rank
 *   <= 6, ELEMENT strides, negative strides allowed, stride 0 on src only, dst == src with equal strides allowed).
 * laser_hip_log_f32: host pointers, `len` contiguous elements, synchronous.
 * laser_log(x) is callable in forEach / forEachReduce bodies: the prelude embeds log_core.h after exp_core.h.  The name is
 *   reserved like laser_exp.
 * The three row entry points below see rows x[0..n) at d_src + row * src_row_stride, exactly as
 * laser_hip_softmax_rows_f32_dev does, and m and s are exactly that softmax's: m = the maximum of the row under the rule of
 * reduce_max, s = the sum of lexp(x[j] - m) in the order of "Reductions" applied to the row as a 1-D array of n float32.
 * s >= 1 (the maximal element adds lexp(0) = 1), so llog(s) >= 0 and nothing cancels.  A row's result is a function of its
 * values, n (and its label) alone.  1 <= n <= 2^26, rows >= 0 (0: nothing happens), row strides >= n, per-row strides >= 1,
 * any base alignment; anything else LASER_HIP_E_INVALID.  Asynchronous on `stream`.
 * laser_hip_logsumexp_rows_f32_dev: d_dst[row * dst_stride] = m + llog(s), one rounded add.  m = +Inf gives +Inf, m = -Inf
 *   (a row of all -Inf) gives -Inf, a NaN in the row gives NaN.  Reads the row once (n <= 8192) or twice, writes 4 bytes.
 * laser_hip_log_softmax_rows_f32_dev: y[j] = (x[j] - m) - llog(s): two separately rounded subtractions, never x[j] - lse
 *   (which loses the low bits when |m| is large).  No special cases: a NaN in the row, a row of all -Inf or a +Inf maximum
 *   give what IEEE gives (NaN where x[j] - m is NaN), as the softmax documents.  Every finite result is <= 0.  dst == src
 *   with equal row strides allowed.
 * laser_hip_softmax_xent_rows_f32_dev: the softmax cross-entropy with integer labels, d_labels[row] an int32 (the index type
 *   the samplers return), in one launch; d_loss or d_grad may be NULL (not both), and the loss-only form reads the logits and
 *   writes `rows` floats.
 *     loss = llog(s) - (x[label] - m)                 at d_loss + row * loss_stride; the bits of 0 - log_softmax[label]
 *     grad[j] = (lexp(x[j] - m) / s - [j == label]) * scale    at d_grad + row * grad_row_stride; the division is the
 *       softmax's correctly rounded one (so the quotient has the softmax's bits), the subtraction and the multiply are rounded
 *       separately.  scale: 1 for a sum over the batch, 1 / rows for a mean.
 *   label == -1 (the samplers' "no draw") means ignore: the loss is +0 and the gradient row +0.  Any other label outside
 *   [0, n) gives a NaN loss and a NaN gradient row: a wrong label never passes silently.  x[label] is one scalar load.
 *   d_grad may not be d_src.
 * laser_hip_softmax_rows_plan: what the three calls above launch for a shape, without a device: out3 = {kernel code,
 *   workgroups, LDS bytes}.  Code 0 = one wave per row, four rows per workgroup (n <= 1024), 1 = one workgroup per row, the
 *   row in registers (n <= 8192), 2 = long rows streamed, chunk partials in LDS; + 4 when vec == 0 (a base or a row stride off
 *   its 16-byte alignment: single-element accesses) -- same bits all six.  At most 2048 workgroups, which stride over the
 *   rows.  The logic is laser_amd/csrc/softmax_rows_plan.h, which has no HIP dependency.
 * Not built: float64, these along a strided axis (the column-strip kernels), dense (probability-vector) targets, a fused
 *   mean over the batch (reduce_sum over the loss vector does it).
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
int laser_hip_log_f32_dev(float *d_dst, const int64_t *dst_strides, const float *d_src, const int64_t *src_strides,
                          const int64_t *shape, int rank, void *stream);
int laser_hip_log_f32(float *dst, const float *src, int64_t len);
int laser_hip_logsumexp_rows_f32_dev(float *d_dst, int64_t dst_stride, const float *d_src, int64_t src_row_stride,
                                     int64_t rows, int64_t n, void *stream);
int laser_hip_log_softmax_rows_f32_dev(float *d_dst, int64_t dst_row_stride, const float *d_src, int64_t src_row_stride,
                                       int64_t rows, int64_t n, void *stream);
int laser_hip_softmax_xent_rows_f32_dev(float *d_loss, int64_t loss_stride, float *d_grad, int64_t grad_row_stride,
                                        const float *d_src, int64_t src_row_stride, const int32_t *d_labels,
                                        int64_t rows, int64_t n, float scale, void *stream);
int laser_hip_softmax_rows_plan(int64_t rows, int64_t n, int vec, int64_t *out3);

/* ---- Activations (f32): relu, tanh and sigmoid on a tensor, forward and backward, defined bit by bit ----------------------
 * The reference's README lists optimised tanh and sigmoid beside exp and log, and the derivatives of relu, tanh and sigmoid
 * for backward propagation.  ltanh and lsigmoid are defined the way lexp and llog are: one definition,
 * laser_amd/csrc/act_core.h, shared by the kernels below and by the forEach bodies, built from integer operations, bit
 * casts, one exact float32 -> float64 conversion, float64 + - x / each rounded on its own (no fused multiply-add in the
 * polynomial parts, no libm, no device transcendental instruction), exactly one float64 division per result (IEEE
 * correctly rounded) and one float64 -> float32 rounding to nearest even.
 * Constants (float64): INV = float64(64 / ln 2); HI = float64(ln 2 / 64) with its low 24 significand bits cleared (k * HI is
 *   exact); LO = float64(ln 2 / 64 - HI); T[j] = the correctly rounded float64 of 2^(j/64), j = 0..63; C2..C5 = float64(1/2,
 *   1/6, 1/24, 1/120); D3, D5, D7 = float64(-1/3, 2/15, -17/315); R = 1.5 x 2^52.
 * E(a) for a float64 a in [-208, 0]:
 *   1. kf = (a * INV + R) - R: a * INV rounded to the nearest integer, ties to even, by two additions; k = int(kf).
 *   2. r = (a - kf * HI) - kf * LO.
 *   3. q = ((C5 r + C4) r + C3) r + C2.
 *   4. p = r + (r * r) * q.
 *   5. e = T[k & 63] + T[k & 63] * p.
 *   6. E = e * bitcast<float64>(uint64((k >> 6) + 1023) << 52): an exact multiply by 2^(k >> 6) (arithmetic shift), never
 *      subnormal in float64.
 * lsigmoid(x) for a float32 x:
 *   1. NaN gives NaN (payload unspecified).
 *   2. c = min(float64(|x|), 104); +-Inf clamp like any other value.  e = E(-c), d = 1 + e.
 *   3. Sign bit clear (+0 too): float32(1 / d).  Sign bit set (-0 too): float32(e / d).
 *   lsigmoid(+-0) = 0.5.  For x in about [-103.97, -87.34] the result is a float32 subnormal, rounded once from the float64
 *   quotient; no denormal is flushed.
 * ltanh(x) for a float32 x:
 *   1. NaN gives NaN (payload unspecified).
 *   2. a = min(float64(|x|), 10).
 *   3. a < 2^-6: s = a * a, q = ((D7 s + D5) s + D3) s, y = a + a * q.  Otherwise: e = E(-2 a), y = (1 - e) / (1 + e).
 *   4. ltanh(x) = float32(y) with x's sign bit ORed into its bits: ltanh(-x) has the bits of -ltanh(x), ltanh(-0) = -0,
 *      ltanh(+-Inf) = +-1, ltanh(x) = x for subnormal and tiny x.
 * Properties, checked over every finite float32 on the CPU against tanhl / expl in 80-bit long double
 * (tests/cpp/act_core_host.cpp "sweep"; profiles/activation/README.md has the output):
 *   faithful: the result is one of the two float32 that bracket the true value, at every input (ltanh: the correctly rounded
 *     float32 at every input, maximum error 0.500000 ulp; lsigmoid: maximum 0.500000 ulp, 73 of 4278190080 results are the
 *     other neighbour of the true value instead of the nearest);
 *   monotone: non-decreasing over all finite float32 in increasing order;
 *   odd: ltanh(-x) has the bits of -ltanh(x);
 *   bounded: |ltanh| <= 1, 0 <= lsigmoid <= 1, lsigmoid(+-0) = 0.5; ltanh is 1 from bits 0x41102cb4 (9.010914), lsigmoid is 1
 *     from bits 0x418aa123 (17.32868) and 0 from bits 0xc2cff1b5 (-103.972084): where the true functions round to them.
 * The rules by `act`; the gradients take the forward OUTPUT y, and their float32 operations are rounded one by one, never
 * fused:
 *   LASER_HIP_ACT_RELU     y = x > 0 ? x : +0 (NaN and -0 give +0)     dx = y > 0 ? dy : +0
 *   LASER_HIP_ACT_TANH     y = ltanh(x)                                 t = y * y;  u = 1 - t;  dx = dy * u
 *   LASER_HIP_ACT_SIGMOID  y = lsigmoid(x)                              u = 1 - y;  v = y * u;  dx = dy * v
 *   Any other `act`, LASER_HIP_ACT_NONE and the PRE_ bits included, gives LASER_HIP_E_INVALID.
 * The fused GEMM and conv epilogue (the `act` of the _ex entry points) is a different code path: its relu is this same rule,
 *   so matmul(.., relu) has the bits of act(matmul(..), relu); its tanh and sigmoid stay the device math library's tanhf and
 *   1 / (1 + expf(-x)), whose bits nothing defines and which may differ from ltanh and lsigmoid in the last bit.
 * laser_hip_act_f32_dev: dst[idx] = act(src[idx]) for every index of `shape`; the contract of laser_hip_exp_f32_dev: rank
 *   <= 6, ELEMENT strides, negative strides allowed, stride 0 (broadcast) on src only, dst == src with equal strides allowed
 *   (any other overlap is not), a zero-size shape does nothing, any base alignment.  Asynchronous on `stream`.  C-contiguous
 *   and 16-byte aligned on both sides: one 16-byte vector per lane and step.
 * laser_hip_act_f32: host pointers, `len` contiguous elements, synchronous.
 * laser_hip_act_grad_f32_dev: dx[idx] = the gradient rule above of (dy[idx], y[idx]); the same contract with two inputs:
 *   stride 0 on dy and y only, dx may equal dy or y (or both) with equal strides.
 * laser_tanh(x) and laser_sigmoid(x) are callable in forEach / forEachReduce bodies: the prelude embeds act_core.h after
 *   log_core.h.  The names are reserved like laser_log.
 * Not built: these rules as new codes of the GEMM / conv epilogue (the float64 bodies would land in every fused-epilogue
 *   instantiation, their register and code-size cost there is unmeasured; profiles/activation/README.md has the per-element
 *   figures that decision needs); float64; softplus, log-sigmoid, binary cross-entropy, GELU and SiLU (the last two are
 *   one-line forEach bodies over the two names); reductions along an axis other than the bias gradient of "Dense-layer backward".
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
int laser_hip_act_f32_dev(int act, float *d_dst, const int64_t *dst_strides, const float *d_src, const int64_t *src_strides,
                          const int64_t *shape, int rank, void *stream);
int laser_hip_act_f32(int act, float *dst, const float *src, int64_t len);
int laser_hip_act_grad_f32_dev(int act, float *d_dx, const int64_t *dx_strides, const float *d_dy, const int64_t *dy_strides,
                               const float *d_y, const int64_t *y_strides, const int64_t *shape, int rank, void *stream);

/* ---- Dense-layer backward (f32): dZ = dY (.) f'(Y) and the bias gradient in one pass ------------------------------------------
 * For the layer Y = act(X W + b), backward propagation needs dZ = dY (.) f'(Y), db[j] = the sum of dZ[0..rows, j], dW = X^T dZ
 * and dX = dZ W^T.  The two products run on gemm_strided (transposed views are strides); this call is the rest.
 * laser_hip_bias_grad_f32_dev: row r of dy is the n contiguous floats at d_dy + r * dy_row_stride; y and dz are addressed the
 *   same way (ELEMENT strides, each >= n).  `act` is LASER_HIP_ACT_NONE, _RELU, _TANH or _SIGMOID.
 *   1. dz[r, j] = the gradient rule of "Activations" for `act` applied to (dy[r, j], y[r, j]): exactly what
 *      laser_hip_act_grad_f32_dev gives, every float32 operation rounded on its own, never fused.  LASER_HIP_ACT_NONE:
 *      dz = dy, and d_y is ignored and may be NULL.
 *   2. d_db[j * db_stride] = the sum of the 1-D array dz[0..rows, j] in the order of "Reductions" applied to that column as
 *      an array of `rows` float32 (E = 4, init +0): db[j] is reduce_sum of the column.  The sum tree in terms of the row
 *      index r: within a chunk of 8192 rows, row k of the chunk goes to leaf a = k mod 1024; a leaf starts at +0 and takes its
 *      up to 8 elements in ascending k; the 1024 leaves are folded by adding the higher index into the lower for index pairs
 *      that differ in bit 1, then bit 0, then bit 9, 8, .., 2; the chunk partials (at most 8192: one chunk) are folded by the
 *      same rule as one more such array.  rows = 0 gives db = +0; n = 0 does nothing.
 *   d_dz may be NULL: only db is written (with LASER_HIP_ACT_NONE the call is then a plain column sum).  d_dz may equal d_dy
 *   or d_y when the row strides are equal; no other overlap is allowed, and d_db may not overlap anything.
 *   Valid: 0 <= rows <= LASER_HIP_BIAS_GRAD_MAX_ROWS (the chunk partials of a column fit one chunk: two levels at most),
 *   n >= 0, any base alignment; anything else -- a row stride below n, an unknown `act`, a NULL d_db, a NULL d_dy, a NULL d_y
 *   with an activation -- gives LASER_HIP_E_INVALID before any pointer is touched.  (A buffer that is never touched may be
 *   NULL: all of them when n = 0, d_dy and d_y when rows = 0.)  Asynchronous on `stream`.
 *   A column's bits depend on its own values and `rows` alone: never on n, the neighbouring columns, the strides, the base
 *   alignment, the grid or the stream.  A NaN in a column makes that db[j] NaN and no other.
 *   A workgroup of 256 lanes owns a (chunk of 8192 rows, strip of 16 columns) unit: 64 contiguous bytes per row, read once;
 *   rows <= 8192 is one launch, longer columns write chunk partials to stream-ordered scratch and the same kernel folds
 *   them: two launches.  No atomics, no workgroup waits on another.
 * laser_hip_bias_grad_last_kernel: the plan's kernel code of the last laser_hip_bias_grad_f32_dev launch of this process:
 *   0 = the vector instance (16-byte accesses wherever 4 columns lie inside n; bases 16-byte aligned, row strides multiples
 *   of 4), 1 = single elements -- same bits both; -1 = none yet.  (A function of its own, not a name of laser_hip_get_option:
 *   the option table is a recorded set.)
 * laser_hip_bias_grad_plan: what the call above would launch for a shape, without a device: out4 = {kernel code, workgroups
 *   of the first launch = min(2048, chunks * strips), launches, scratch floats = chunks * n when there are two launches}.
 *   vec: 1 when bases and strides allow 16-byte vectors; cus: the device's compute units, taken for symmetry with
 *   laser_hip_plan_f32: the plan does not depend on it.  n = 0: {code, 0, 0, 0}.  The logic is
 *   laser_amd/csrc/bias_grad_plan.h, which has no HIP dependency.
 * Not built: float64; f' fused into the GEMM's loader; sums along other axes or of other types, mean, argmin and argmax;
 *   convolution backward; optimizers (forEach writes w -= lr * dw); weight layouts other than matmul's; batch and RMS
 *   normalization (layer normalization is the next section).
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
#define LASER_HIP_BIAS_GRAD_MAX_ROWS (1ll << 26)
int laser_hip_bias_grad_f32_dev(float *d_db, int64_t db_stride, float *d_dz, int64_t dz_row_stride, const float *d_dy,
                                int64_t dy_row_stride, const float *d_y, int64_t y_row_stride, int64_t rows, int64_t n, int act,
                                void *stream);
int laser_hip_bias_grad_plan(int64_t rows, int64_t n, int vec, int cus, int64_t *out4);
int laser_hip_bias_grad_last_kernel(void);

/* ---- Layer normalization (f32): forward and backward over the rows of a matrix, defined bit by bit --------------------------
 * The layer between two dense layers: every row of x is shifted to mean 0, scaled to variance 1, then scaled by gamma and
 * shifted by beta.  Every operation below is ONE float32 operation rounded on its own (+ - x, a correctly rounded division
 * and a correctly rounded square root), never fused, and every sum is a sum of "Reductions": no polynomial, no table.
 * Row r of x is the n contiguous floats at d_x + r * x_row_stride; y, dy and dx are addressed the same way (ELEMENT strides,
 * each >= n); mean[r] is d_mean[r * mean_stride], gamma[j] is d_gamma[j * gamma_stride], and so on.
 * Definitions, for a row x[0..n):  nf = (float)n;  rsum(.) = the sum of the row as a 1-D array of n float32 in the order of
 *   "Reductions" (E = 4, init +0; elements at or past n are skipped): what reduce_sum gives for it.
 * laser_hip_layer_norm_f32_dev, the forward pass:
 *     mean = rsum(x) / nf
 *     d[j] = x[j] - mean
 *     var  = rsum(d[j] * d[j]) / nf
 *     rstd = 1 / sqrt(var + eps)
 *     xhat[j] = d[j] * rstd
 *     y[j] = xhat[j] * gamma[j] + beta[j]          two roundings; d_gamma NULL: no multiply; d_beta NULL: no add
 *   d_mean and d_rstd receive the row's statistics for the backward pass; either may be NULL (inference).  d_y may equal d_x
 *   when the row strides are equal; no other overlap is allowed.
 * laser_hip_layer_norm_grad_f32_dev, the backward pass, from dy, x, the saved mean and rstd, and gamma:
 *     xhat[j] = (x[j] - mean) * rstd               the forward's bits
 *     g[j] = dy[j] * gamma[j]                      d_gamma NULL: g = dy
 *     a = rsum(g) / nf
 *     b = rsum(g[j] * xhat[j]) / nf
 *     dx[j] = ((g[j] - a) - xhat[j] * b) * rstd
 *     dbeta[j]  = the sum over the rows of dy[r, j]
 *     dgamma[j] = the sum over the rows of dy[r, j] * xhat[r, j]
 *   The two column sums run in the order "Dense-layer backward" documents for db (chunks of 8192 rows, row k of a chunk to
 *   leaf k mod 1024, and so on): dbeta has exactly the bits of laser_hip_bias_grad_f32_dev's db for dy with LASER_HIP_ACT_NONE,
 *   and dgamma[j] those of reduce_sum of column j of the matrix dy * xhat.  rows = 0 gives dgamma = dbeta = +0.
 *   Each of d_dx, d_dgamma and d_dbeta may be NULL (not wanted), but not all three; what is asked for has the same bits
 *   whatever else is asked for.  d_dx may equal d_dy or d_x when the row strides are equal; no other overlap is allowed.
 * Consequences: a row's y, mean, rstd and dx depend on that row's values, n and eps alone, and a column's dgamma and dbeta
 *   on that column's values (with the rows' mean and rstd) and `rows` alone: never on the grid, the stream, the base
 *   alignment or the strides.  A NaN or an Inf in one row touches no other row's y, mean, rstd or dx; in dy it does touch the
 *   columns of dgamma and dbeta it sits in, and only those (in x it reaches every column of dgamma, through its row's xhat).  A sum starts at +0 and adds its first element, so a row of -0 has
 *   mean +0 and xhat -0.  n = 1 gives mean = x, var = +0 and y = (0 * rstd) * gamma + beta.  eps = 0 is allowed and follows
 *   IEEE: a constant row gives var = +0, rstd = +Inf and y = 0 * Inf = NaN.
 * Valid: rows >= 0, 1 <= n <= LASER_HIP_LAYER_NORM_MAX_N, eps >= 0 (not NaN), any base alignment; with d_dgamma or d_dbeta
 *   also rows <= LASER_HIP_LAYER_NORM_MAX_ROWS (the chunk partials of a column fit one chunk).  Anything else -- a row stride
 *   below n, a stride below 1 of a statistic or parameter that is written, a NULL d_y, d_x, d_dy, d_mean or d_rstd where it is
 *   required, in-place operands with unequal row strides, no gradient asked for -- gives LASER_HIP_E_INVALID before a device
 *   is looked for.  (With rows = 0 nothing but dgamma and dbeta is touched and the other pointers may be NULL.)
 *   Asynchronous on `stream`.
 * Kernels (laser_amd/csrc/layer_norm.hip).  Forward and dx, three lane mappings chosen by n alone, as the row softmax has
 *   them: n <= 1024 one wave per row and four rows per workgroup, n <= 8192 one workgroup per row with the row in registers,
 *   longer rows one workgroup streaming the row's chunks (x is read once per pass: three passes forward, two backward); at
 *   most 2048 workgroups, which stride over the rows.  Each has a 16-byte-vector instance (every row operand, gamma and beta
 *   16-byte aligned, row strides multiples of 4, gamma and beta with unit stride) and a single-element one: same bits.
 *   dgamma and dbeta: a workgroup owns a (chunk of 8192 rows, strip of 8 columns) unit and produces both sums from one
 *   read of dy and x; rows <= 8192 is one launch, longer columns write chunk partials to stream-ordered scratch, which the
 *   bias gradient's launch folds ("the partials are one more such array").  No atomics, no workgroup waits on another.
 * laser_hip_layer_norm_plan: what the calls above would launch, without a device.  what: 0 = forward, 1 = dx, 2 = dgamma and
 *   dbeta together.  out4 = {kernel code, workgroups of the first launch, launches, scratch bytes}.  Codes for 0 and 1:
 *   0 / 1 / 2 = wave / workgroup / long-row mapping, + 4 for the single-element instance (vec = 0); workgroups =
 *   min(2048, ceil(rows / 4)) for code 0 and min(2048, rows) otherwise; one launch (none for rows = 0).  For 2: code 0 = vector,
 *   1 = single elements; workgroups = min(2048, chunks * strips); rows <= 8192: one launch; longer: three (one fold per sum)
 *   and 2 * chunks * n * 4 scratch bytes (one sum asked for alone: one launch and one matrix fewer).  The logic is
 *   laser_amd/csrc/layer_norm_plan.h, which has no HIP dependency.
 * laser_hip_layer_norm_last_kernel(what): the plan's kernel code of the last launch of that kind in this process; -1 = none
 *   yet or an unknown `what`.  (A function of its own: the option table is a recorded set.)
 * Not built: float64; batch and RMS normalization; normalization along an axis other than the last; the normalization fused
 *   into a GEMM prologue or epilogue; one very long row split over several workgroups (64 rows keep 64 compute units busy).
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
#define LASER_HIP_LAYER_NORM_MAX_N (1ll << 26)
#define LASER_HIP_LAYER_NORM_MAX_ROWS (1ll << 26)
int laser_hip_layer_norm_f32_dev(float *d_y, int64_t y_row_stride, float *d_mean, int64_t mean_stride, float *d_rstd,
                                 int64_t rstd_stride, const float *d_x, int64_t x_row_stride, const float *d_gamma,
                                 int64_t gamma_stride, const float *d_beta, int64_t beta_stride, int64_t rows, int64_t n, float eps,
                                 void *stream);
int laser_hip_layer_norm_grad_f32_dev(float *d_dx, int64_t dx_row_stride, float *d_dgamma, int64_t dgamma_stride, float *d_dbeta,
                                      int64_t dbeta_stride, const float *d_dy, int64_t dy_row_stride, const float *d_x,
                                      int64_t x_row_stride, const float *d_mean, int64_t mean_stride, const float *d_rstd,
                                      int64_t rstd_stride, const float *d_gamma, int64_t gamma_stride, int64_t rows, int64_t n,
                                      void *stream);
int laser_hip_layer_norm_plan(int64_t rows, int64_t n, int vec, int what, int64_t *out);
int laser_hip_layer_norm_last_kernel(int what);

/* ---- Embedding (f32): row gather by int32 ids and a deterministic gradient ------------------------------------------------------
 * The first layer of a model that starts from token ids: the ids that "F+tree weighted sampler" and the inverse-CDF sampler
 * return, and that the cross-entropy takes as labels, select rows of a weight table.  The gradient adds the rows of dY that
 * hit the same id; here it does so in the one documented order of "Reductions", so a scatter keeps the project's claim that a
 * column's bits depend on its values and the row count alone.
 * Operands.  W is (vocab, dim) float32: row v is the dim contiguous floats at d_w + v * w_row_stride (ELEMENT strides, each
 *   >= dim).  idx is `tokens` contiguous int32.  Y and dY are (tokens, dim) and dW is (vocab, dim), addressed like W.
 * laser_hip_embedding_f32_dev, the forward pass: Y[t, :] is a bit copy of W[idx[t], :] -- NaN payloads and -0 are preserved,
 *   no arithmetic is done.  idx[t] == -1 (the samplers' "no draw", the cross-entropy's "ignore") gives a row of +0; any other
 *   id outside [0, vocab) gives a row of quiet NaN (0x7fc00000), so a wrong id never passes silently.  Y may not overlap W.
 * laser_hip_embedding_group_i32_dev(d_order, d_starts, d_idx, tokens, vocab, stream), the grouping: order is `tokens` int32
 *   and starts is vocab + 1 int32.  order holds the positions t of the tokens with 0 <= idx[t] < vocab sorted by
 *   (idx[t], t) ascending, and after them the positions of all other tokens (-1 and out of range alike) in ascending t.
 *   starts[v] = the number of tokens with a valid id below v: starts[0] = 0, starts[vocab] = the number of valid tokens, and
 *   id v owns order[starts[v] .. starts[v + 1]).  This is the stable counting sort of the positions by id; its output is
 *   unique, so it is the same on every grid, stream and run.
 * laser_hip_embedding_grad_f32_dev, the backward pass.  d_order and d_starts are either both NULL or both the output of the
 *   grouping call for the same idx and vocab; when NULL the call groups by itself in stream-ordered scratch (the pre-grouped
 *   form exists so that one id vector feeding several tables is grouped once).  With c = starts[v + 1] - starts[v] and
 *   a[k] = dY[order[starts[v] + k], j], k = 0 .. c - 1:  dW[v, j] = the sum of the 1-D array a in the order of "Reductions"
 *   (E = 4, init +0) -- exactly the tree "Dense-layer backward" documents for db, with k in place of the row index: chunks
 *   of 8192 elements, element k of a chunk to leaf k mod 1024, the fold stated there, chunk partials folded by the same rule.
 *   The call writes every element of dW: an id that never occurs gets +0, and a single occurrence gives 0 + dY, so -0
 *   becomes +0.  Tokens whose id is outside [0, vocab), -1 included, contribute nothing: the forward pass has already put NaN
 *   (or, for -1, the agreed zeros) into that token's row of Y, so the error is visible where it is made and the table's
 *   gradient stays usable.  dW may not overlap dY, idx, order or starts.
 * Consequences.  With vocab = 1 and every id 0, dW[0, :] has the bits of laser_hip_bias_grad_f32_dev's db for dY with
 *   LASER_HIP_ACT_NONE.  dW[v, j] depends on the sequence dY[t, j] over the tokens of id v, in token order, and on nothing
 *   else: not on other tokens, vocab, dim, the neighbouring columns, the strides, the base alignment, the grid or the stream.
 *   A NaN or an Inf in dY[t, j] reaches dW[idx[t], j] and no other element (NaN positions are defined, NaN payloads are not).
 * Valid: 0 <= tokens <= LASER_HIP_EMBEDDING_MAX_TOKENS (positions fit int32 and the chunk partials of one id fit one chunk:
 *   two levels at most), 0 <= vocab <= LASER_HIP_EMBEDDING_MAX_VOCAB, dim >= 0, any base alignment.  Anything else -- a row
 *   stride below dim, a NULL buffer that would be touched, exactly one of d_order / d_starts NULL -- gives
 *   LASER_HIP_E_INVALID before any pointer is touched or a device is looked for.  A buffer that is never touched may be NULL
 *   (Y and W when tokens or dim is 0, W also when vocab is 0, idx and order when tokens is 0, dW and dY when vocab or dim is
 *   0, dY when tokens is 0).  All calls are asynchronous on `stream`.
 * Kernels (laser_amd/csrc/embedding.hip).  Gather: a lane loads its row's id once and walks the row in 16-byte vectors
 *   (bases 16-byte aligned, row strides multiples of 4) or single elements: same bits.  Grouping: a stable least-significant-
 *   digit radix sort of the positions by key (the id, or vocab for every invalid id), 8 bits a pass and only as many passes
 *   as the bit length of vocab needs (vocab <= 255: one; <= 65535: two; < 2^24: three; else four).  A pass is per-wave-tile
 *   digit histograms, the int32 row cumsum of "Row cumsum" over the (digit, tile) table, and a scatter whose rank among equal
 *   digits is a per-digit LDS counter plus wave ballots counted below the lane; starts is scan_core.h's lower-bound descent
 *   over the sorted keys.  Integer adds into counters only; nothing claims a slot atomically.  Sums: ids of at most 32
 *   occurrences (none included) are evaluated by one lane per four columns in registers -- every leaf is +0 + x, so no partial
 *   is ever -0, adding a +0 partner is exact, and the tree restricted to the occupied leaves has the same bits; longer
 *   segments take the workgroup form of the bias gradient, (8192 gathered rows, 16 columns) per chunk, the chunk partials
 *   folded by the same workgroup.  Two launches whatever the ids are.  No floating-point atomics, no workgroup waits on
 *   another.
 * laser_hip_embedding_plan(tokens, vocab, dim, vec, cus, out8): what the calls launch, without a device: out8 = {sort passes,
 *   sort positions of one wave's tile, workgroups of a pass, kernel code of the sums (0 = 16-byte vectors when vec is 1, 1 =
 *   single elements), launches of the grouping (3 per pass + 1; tokens = 0: 1), launches of the gradient given a group (2; 0
 *   when vocab or dim is 0), scratch bytes of the grouping, scratch bytes of the gradient that groups by itself}.  cus is
 *   taken for symmetry with laser_hip_plan_f32: the plan does not depend on it.  The logic is
 *   laser_amd/csrc/embedding_plan.h, which has no HIP dependency.
 * laser_hip_embedding_last_kernel(what): what the last call of this process launched: 0 = the gather's kernel code (0 vector,
 *   1 single elements), 1 = the sort passes of the last grouping, 2 = the sums' kernel code, 3 = the workgroups of a pass
 *   of the last grouping; -1 = none yet or an unknown `what`.  (A function of its own: the option table is a recorded set.)
 * Not built: int64 ids; float64; accumulation into an existing dW; a sparse (rows, values) gradient; scale_grad_by_freq and
 *   max_norm; a padding id other than -1; a public general-purpose sort; a fused optimizer step (forEach writes
 *   w -= lr * dw).
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
#define LASER_HIP_EMBEDDING_MAX_TOKENS (1ll << 26)
#define LASER_HIP_EMBEDDING_MAX_VOCAB (1ll << 30)
int laser_hip_embedding_f32_dev(float *d_y, int64_t y_row_stride, const float *d_w, int64_t w_row_stride, const int32_t *d_idx,
                                int64_t tokens, int64_t vocab, int64_t dim, void *stream);
int laser_hip_embedding_group_i32_dev(int32_t *d_order, int32_t *d_starts, const int32_t *d_idx, int64_t tokens, int64_t vocab,
                                      void *stream);
int laser_hip_embedding_grad_f32_dev(float *d_dw, int64_t dw_row_stride, const float *d_dy, int64_t dy_row_stride,
                                     const int32_t *d_idx, const int32_t *d_order, const int32_t *d_starts, int64_t tokens,
                                     int64_t vocab, int64_t dim, void *stream);
int laser_hip_embedding_plan(int64_t tokens, int64_t vocab, int64_t dim, int vec, int cus, int64_t *out8);
int laser_hip_embedding_last_kernel(int what);

/* ---- Optimizer steps (f32): multi-tensor SGD and Adam and the global gradient norm, defined bit by bit ----------------------------
 * The last link of a training step: one call updates a whole LIST of parameter tensors, and the clip factor of the global
 * gradient norm is computed, kept and used on the device.  Every + - x / sqrt below is ONE correctly rounded float32
 * operation, never fused; the arithmetic is defined once, in laser_amd/csrc/optim_core.h.
 * Lists: d_w, d_g, d_m, d_v are HOST arrays of `count` DEVICE pointers; tensor k is lens[k] contiguous floats at any base
 * alignment.  A tensor of length 0 is skipped and its pointers may be NULL.  Operands of one call may not overlap (not
 * detected).  For element i of tensor k, with w, g, m, v the loaded values:
 *     g1 = g * gscale                        (gscale == 1.0f: the same bits)
 *     g2 = g1 * c,  c = *d_clip              (d_clip NULL: no operation; c is one device float, read by the kernel)
 * laser_hip_sgd_step_f32_dev(lr, mu, wd, nesterov):
 *     g3 = g2 + wd * w                       two roundings; wd == 0: no operation, g3 = g2
 *     with a momentum list:  m' = mu * m + g3  (two roundings);  d = nesterov ? g3 + mu * m' : m'
 *     without (d_m NULL):    d = g3          (mu != 0 or nesterov without a list: LASER_HIP_E_INVALID)
 *     w' = w - lr * d                        two roundings
 * laser_hip_adam_step_f32_dev(lr, b1, b2, eps, wd, decoupled, bc1, bc2):
 *     g3 = (!decoupled && wd != 0) ? g2 + wd * w : g2
 *     m' = b1 * m + omb1 * g3                three roundings; omb1 = 1.0f - b1 in float32, on the host, once
 *     v' = b2 * v + (omb2 * g3) * g3         four roundings; omb2 = 1.0f - b2 likewise
 *     mh = m' / bc1;  vh = v' / bc2;  den = sqrt(vh) + eps;  u = mh / den
 *     w1 = (decoupled && wd != 0) ? w - lrwd * w : w          lrwd = lr * wd in float32, on the host, once
 *     w' = w1 - lr * u
 *   m and v start as zeros supplied by the caller; there is no "first step" case.  Hyper-parameters are not validated: NaN,
 *   Inf and eps = 0 follow IEEE (v = g = 0 with eps = 0 gives 0 / 0 = NaN).  bc1 and bc2 are plain floats:
 * laser_hip_adam_bias_correction(beta, step, out), host only, no device needed: for step >= 1 (else LASER_HIP_E_INVALID), in
 *   double, p = beta^step by square-and-multiply from the low bit (r = 1, b = beta; while step: if step & 1: r *= b; b *= b;
 *   step >>= 1), then *out = (float)(1.0 - p), the product and the difference rounded separately.  Every mirror calls it, so
 *   bc1 = 1 - b1^t and bc2 = 1 - b2^t are the same bits in every language.
 * laser_hip_grad_norm_f32_dev(d_norm, d_clip, d_g, lens, count, max_norm):
 *     s_k   = rsum(g_k[i] * g_k[i])          the product rounded to float32, summed in the order of "Reductions" (E = 4,
 *                                            init +0): the bits reduce_sum gives for the array g_k * g_k (+0 for length 0)
 *     total = ((+0 + s_0) + s_1) + ...       left to right in list order
 *     norm  = sqrt(total)
 *     clip  = norm > max_norm ? max_norm / norm : 1.0f        (a NaN norm gives 1: the NaN is already in g and travels on)
 *   d_norm and d_clip are one device float each; either may be NULL, not both.  count = 0 gives norm = +0 and clip = 1.
 *   Valid max_norm: >= 0 and not NaN; +Inf is allowed (clip = 1 unless the norm is NaN).
 * Consequences: an element's w', m', v' depend on that element's four values and the scalars alone: never on the grid, the
 *   stream, the base alignment, the tensor's position in the list or how the list is cut into calls and launches.  SGD with
 *   mu = 0, wd = 0, gscale = 1, no momentum list and no clip has exactly the bits of forEach("w -= lr * g").  A NaN in one
 *   element of g reaches no other element, except through c.  s_k depends on tensor k alone; total depends on the list order.
 * Valid: 0 <= count <= LASER_HIP_OPTIM_MAX_COUNT, 0 <= lens[k] <= LASER_HIP_OPTIM_MAX_LEN (a tensor's chunk partials fit one
 *   chunk of the order).  A negative length, a limit exceeded, a NULL list or NULL lens with count > 0, a NULL entry with
 *   lens[k] > 0 give LASER_HIP_E_INVALID before a device is looked for.  Asynchronous on `stream`: no host synchronisation,
 *   no copy of a table to the device, no allocation but grad_norm's stream-ordered scratch, so a call can be captured in a
 *   graph.  The host lists are read before the call returns.
 * Kernels (laser_amd/csrc/optim.hip).  A step launch serves up to 64 tensors: their table (base pointers, lengths, running
 *   chunk counts) travels BY VALUE in the kernel arguments; a longer list is cut into consecutive launches.  Work is cut into
 *   chunks of 4096 elements; min(2048, chunks) workgroups stride over the chunks of all tensors of the launch and find a
 *   chunk's tensor from the prefix with a wave-uniform index.  Per tensor the 16-byte-vector instance runs when all its bases
 *   are 16-byte aligned (the last len % 4 elements singly), else the single-element one: same bits.  Every input of a step is
 *   loaded before any store.  grad_norm: per group of 192 tensors one launch with a workgroup per (tensor, 8192-element
 *   reduction chunk) and one with a workgroup per tensor that folds its partials; then one lane does the list sum, the
 *   square root and the clip.  No atomics, no workgroup waits on another.
 * laser_hip_optim_plan(what, lens, count, out4): what the calls would launch, without a device.  what: 0 = SGD, 1 = Adam,
 *   2 = grad_norm.  out4 = {launches, workgroups of the first launch, chunks in all, scratch bytes}.  Steps: one launch per
 *   group of 64 consecutive tensors, ceil(count / 64) (a group of empty tensors launches nothing); chunks = the sum of
 *   ceil(len / 4096); no scratch.  grad_norm: 2 * ceil(count / 192) + 1 launches -- three up to 192 tensors, one for an empty
 *   list; chunks = the sum of max(1, ceil(len / 8192)); scratch = 4 bytes per chunk and per tensor, each array rounded up to
 *   16.  The logic is laser_amd/csrc/optim_plan.h, which has no HIP dependency.
 * Not built: float64 and mixed precision; AMSGrad, RMSprop and LAMB; strided or non-contiguous parameters; a learning rate
 *   read from the device; per-tensor norms returned to the caller; loss scaling with overflow skip; the update fused into
 *   dW's GEMM epilogue.
 * No gfx950 device: LASER_HIP_E_NODEVICE (the bias correction and the plan need none). */
#define LASER_HIP_OPTIM_MAX_LEN (1ll << 26)
#define LASER_HIP_OPTIM_MAX_COUNT 65536
int laser_hip_sgd_step_f32_dev(float *const *d_w, const float *const *d_g, float *const *d_m, const int64_t *lens, int count, float lr,
                               float mu, float wd, int nesterov, float gscale, const float *d_clip, void *stream);
int laser_hip_adam_step_f32_dev(float *const *d_w, const float *const *d_g, float *const *d_m, float *const *d_v, const int64_t *lens,
                                int count, float lr, float b1, float b2, float eps, float wd, int decoupled, float bc1, float bc2,
                                float gscale, const float *d_clip, void *stream);
int laser_hip_grad_norm_f32_dev(float *d_norm, float *d_clip, const float *const *d_g, const int64_t *lens, int count, float max_norm,
                                void *stream);
int laser_hip_adam_bias_correction(float beta, int64_t step, float *out);
int laser_hip_optim_plan(int what, const int64_t *lens, int count, int64_t *out4);

/* ---- Softmax gradient (f32): the backward of the row softmax from its output, defined bit by bit ---------------------------------
 * laser_hip_softmax_grad_rows_f32_dev: for each of `rows` rows, with y the softmax's OUTPUT row and dy the incoming gradient
 *   (elements of a row contiguous, row strides in elements and >= n):
 *   1. D = reduce_sum(dy (.) y): every product dy[j] * y[j] rounded to float32 on its own, the sum in the order of
 *      "Reductions" applied to the row of products as a 1-D array of n float32 (E = 4, init +0).
 *   2. dx[j] = y[j] * (dy[j] - D): a rounded subtraction, then a rounded multiplication; nothing is fused.
 *   A row's result is a function of its values and n alone.  Valid: rows >= 0 (0: nothing happens), 1 <= n <= 2^26, any base
 *   alignment; d_dx may be d_dy or d_y with equal row strides (any other overlap is not allowed); anything else
 *   LASER_HIP_E_INVALID.  Asynchronous on `stream`.
 * laser_hip_softmax_grad_plan: what the call would launch, without a device: out3 = {kernel code, workgroups, LDS bytes}.  The
 *   lane mappings, their thresholds, the codes and the grid are those of laser_hip_softmax_rows_plan (0 = one wave per row,
 *   n <= 1024; 1 = one workgroup per row, n <= 8192; 2 = long rows; + 4 for single-element accesses); only the LDS differs (no
 *   table).  The logic is lh_softmax_grad_rows_plan in laser_amd/csrc/softmax_rows_plan.h.
 * laser_hip_softmax_grad_last_kernel(): the plan's kernel code of the last launch in this process; -1 = none yet.
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
int laser_hip_softmax_grad_rows_f32_dev(float *d_dx, int64_t dx_row_stride, const float *d_dy, int64_t dy_row_stride, const float *d_y,
                                        int64_t y_row_stride, int64_t rows, int64_t n, void *stream);
int laser_hip_softmax_grad_plan(int64_t rows, int64_t n, int vec, int64_t *out3);
int laser_hip_softmax_grad_last_kernel(void);

/* ---- Attention (f32): O = softmax(scale * Q K^T) V, fused, defined bit by bit ----------------------------------------------------
 * Per (batch b, head h) slice: Q is (Tq, d), K is (Tk, d), V is (Tk, dv), O is (Tq, dv).  Element [b, h, t, c] of an operand is at
 * ptr + b * strides[0] + h * strides[1] + t * strides[2] + c: ELEMENT strides {batch, head, position}, unit stride along the
 * feature index -- so Q, K and V may be slices of one fused projection output (B, T, 3, H, d) with no copy.
 * Limits: 1 <= d, dv <= LASER_HIP_ATTENTION_MAX_D; 1 <= Tk <= LASER_HIP_ATTENTION_MAX_KEYS; Tq >= 0; B * H >= 0 (0: nothing
 * happens).  Anything past a limit is LASER_HIP_E_INVALID and the text says which limit.
 * The rule:
 *   1. Scores.  c[i,j] = the k-ascending fmaf chain over k = 0..d-1 of Q[i,k] * K[j,k], from +0: the GEMM's laser-order
 *      contract for K <= 512 (one chain; an f32 MFMA is bitwise that chain, and gfx950 has no xf32 path).  s[i,j] =
 *      scale * c[i,j], one rounded multiply, never fused into the chain.  (gemm_strided writes 0 + alpha*AB on full tiles and
 *      alpha*AB on edge tiles, so a score matrix composed from it may differ from s in the sign of a zero.  That sign never
 *      reaches P: lexp(+-0 - m) has the same bits.  Where products underflow so that a chain ends at -0, the sign of a zero
 *      row_max is the chain's.)
 *   2. Causal (causal != 0; needs Tq <= Tk, otherwise LASER_HIP_E_INVALID).  Row i sees keys [0, n_i), n_i = i + (Tk - Tq) + 1;
 *      without causal n_i = Tk.  A masked score is never used: a NaN in a K row reaches only the rows that see that row.
 *      There is no -Inf trick: lexp clamps at -88, so -Inf would not give 0.
 *   3. Probabilities.  P[i, 0:n_i] is exactly laser_hip_softmax_rows_f32_dev applied to s[i, 0:n_i] as a 1-D array of n_i
 *      elements: m_i = the maximum under reduce_max's rule, e = lexp(s - m_i), s_i = the sum of e in the order of "Reductions"
 *      (E = 4, init +0), P = e / s_i correctly rounded.  P[i, j >= n_i] = +0.  The softmax's NaN rules carry over: a NaN or a
 *      +Inf maximum in a row makes that row of P NaN, and hence that row of O.
 *   4. Output.  O = P V in laser-order over ALL Tk keys, the masked ones included with their +0: S_p[i,c] = the fmaf chain
 *      over j in [512 p, 512 (p + 1)) of P[i,j] * V[j,c], from +0, and O = ((S_0 + S_1) + S_2) + .., each addition rounded,
 *      nothing fused (a single slice is S_0 itself).  That is gemm_strided(P, V) in laser-order mode.  So a NaN or an Inf in a
 *      V row reaches every row of O (0 * NaN), as it does in the composition.
 * Every row i of every slice depends on Q[i,:], K, V, scale, n_i and Tk alone: never on B, H, Tq, the strides, the base
 * alignment, the grid, the stream or the kernel instance the plan picks.
 * Outputs, each optional (NULL: not written), but at least one:
 *   d_out            O, with its own strides
 *   d_probs          P in full, (B, H, Tq, Tk) with its own strides {batch, head, row}, the masked +0 included
 *   d_row_max/_sum   m_i and s_i, (B, H, Tq) contiguous
 * With d_out NULL the P V sweep is skipped.  What is asked for has the same bits whatever else is asked for.  Outputs may not
 * overlap inputs or each other.  Position strides must be >= the row length (d, dv or Tk) wherever there is more than one
 * position; no stride may be negative.  Arguments are judged before any pointer is dereferenced.  Asynchronous on `stream`.
 * laser_hip_attention_plan: what a call would launch, without a device: out5 = {BM (query rows of a workgroup), kernel code,
 *   workgroups, LDS bytes, units}.  bh = B * H; vec = 1 when the bases of Q and K are 16-byte aligned and all their strides are
 *   multiples of 4 elements (code 0, 16-byte loads), else code 1 (single-element loads): the same bits.  The units are the
 *   bh * ceil(Tq / BM) query blocks; at most 1024 workgroups stride over them.  One kernel form, streaming: no resident form is
 *   built.  The logic is laser_amd/csrc/attention_plan.h, which has no HIP dependency.
 * laser_hip_attention_last_kernel(): the kernel code of the last launch in this process; -1 = none yet.
 * The backward is a composition of defined steps, built in the mirrors (laser_amd.attention_backward, laser::attention_backward,
 * attentionBackward): P from this entry point (d_probs, d_out NULL); dV = P^T dO; dP = dO V^T; dS = softmax_grad(dP, P) over the
 * full Tk (masked positions give +-0); dQ = scale * (dS K); dK = scale * (dS^T Q) -- the four products on
 * gemm_strided_batched in the current float mode, the transposes as strides, scale as the GEMM's alpha.
 * Not built: float64 and 16-bit operands, a resident (scores in LDS) form, a fused backward, dropout, an additive mask or bias.
 * No gfx950 device: LASER_HIP_E_NODEVICE. */
#define LASER_HIP_ATTENTION_MAX_D 128
#define LASER_HIP_ATTENTION_MAX_KEYS 65536
int laser_hip_attention_f32_dev(float *d_out, const int64_t *out_strides, const float *d_q, const int64_t *q_strides, const float *d_k,
                                const int64_t *k_strides, const float *d_v, const int64_t *v_strides, float *d_probs,
                                const int64_t *probs_strides, float *d_row_max, float *d_row_sum, int64_t batch, int64_t heads,
                                int64_t tq, int64_t tk, int64_t d, int64_t dv, float scale, int causal, void *stream);
int laser_hip_attention_plan(int64_t bh, int64_t tq, int64_t tk, int64_t d, int64_t dv, int causal, int vec, int64_t *out5);
int laser_hip_attention_last_kernel(void);

/* ---- Sine and cosine (f32): lsin and lcos, defined bit by bit ------------------------------------------------------------
 * The reference's forEach material uses exactly these two (`o = x + y - sin z` in benchmarks/loop_iteration/iter_bench.nim,
 * `sin(s) + cos(s)` in examples/ex02 and ex03); through the device library's sinf their bits are nobody's.  lsin and lcos are
 * one definition, laser_amd/csrc/sincos_core.h, for the host, these kernels, the normal random fill below and forEach bodies;
 * tests/sincos_model.py is the numpy model and scripts/gen_sincos_constants.py makes the constants from integer arithmetic.
 * Inside: integer operations, bit casts, one exact float32 -> float64 conversion, float64 + - x each rounded on its own (no
 * fused multiply-add, no division, no library call) and one rounding to float32.  Reduction to a quadrant and an argument in
 * about [-pi/4, pi/4]: below 2^20 with pi/2 in three parts (24 + 24 + 53 bits; the first two products and subtractions are
 * exact), from 2^20 on by Payne-Hanek in integers on a 128-bit window of the bits of 2/pi (a 288-bit table; at least 43 guard
 * bits below the 53 that are kept).  Then a sine kernel (odd series to r^15) or a cosine kernel (even series to r^16), chosen
 * and signed by the quadrant.
 * The contract, for every float32 x:
 *   Faithful      the result is one of the two float32 that bracket the true value: the error is below one ulp for every
 *                 finite input, however large.
 *   Symmetry      lsin(-x) has the bits of -lsin(x); lcos(-x) has the bits of lcos(x).
 *   Zeros, tiny   lsin(+-0) = +-0, lcos(+-0) = 1.  lsin(x) = x exactly and lcos(x) = 1 wherever the true result rounds to that
 *                 (lsin: every |x| up to bits 0x39e89768, lcos: up to 2^-12, and beyond where rounding says so); this
 *                 includes every subnormal, and nothing is flushed.
 *   Range         |result| <= 1 always.
 *   Monotonicity  over the float32 values in [0, pi/2] lsin is non-decreasing and lcos non-increasing.
 *   Specials      +-Inf and NaN give the NaN with bits 0x7fc00000 (whatever the input's sign and payload).
 *   All of it is measured over every finite float32 against 80-bit sinl / cosl (profiles/sincos/README.md): maximum error 0.5
 *   ulp, and 2 (lsin) and 8 (lcos) of the 4278190080 results are not the nearest float32.
 * laser_hip_sin_f32_dev / laser_hip_cos_f32_dev: dst[idx] = lsin(src[idx]) / lcos(src[idx]) for every index of `shape`; the
 *   contract of laser_hip_act_f32_dev: rank <= 6, ELEMENT strides, negative strides allowed, stride 0 (broadcast) on src only,
 *   dst == src with equal strides allowed (any other overlap is not), a zero-size shape does nothing, any base alignment.
 *   Asynchronous on `stream`.  C-contiguous and 16-byte aligned on both sides: one 16-byte vector per lane and step.
 * laser_hip_sincos_f32_dev: both from one argument reduction, with the bits of the two calls above; either destination may be
 *   src (equal strides), the two destinations must not overlap each other (the same base pointer is LASER_HIP_E_INVALID).
 * laser_hip_sin_f32 / laser_hip_cos_f32: host pointers, `len` contiguous elements, synchronous.
 * LASER_HIP_E_INVALID as for the activations: rank outside 0 .. 6, null shape / strides, a negative extent, stride 0 on a
 *   destination; then the device is looked for (LASER_HIP_E_NODEVICE without a gfx950); then a zero-size shape does nothing;
 *   then a null buffer is LASER_HIP_E_INVALID.
 * laser_sin(x) and laser_cos(x) are callable in forEach / forEachReduce bodies (`o = x + y - laser_sin(z)`): the prelude
 *   embeds sincos_core.h after act_core.h when the body or the merge names one of them, and only then, so other bodies
 *   compile as fast as before.  The names are reserved like laser_log.
 * Not built: float64 sin and cos, tan, sinpi / cospi, gradients, these as fused-epilogue codes. */
int laser_hip_sin_f32_dev(float *d_dst, const int64_t *dst_strides, const float *d_src, const int64_t *src_strides,
                          const int64_t *shape, int rank, void *stream);
int laser_hip_cos_f32_dev(float *d_dst, const int64_t *dst_strides, const float *d_src, const int64_t *src_strides,
                          const int64_t *shape, int rank, void *stream);
int laser_hip_sincos_f32_dev(float *d_sin, const int64_t *sin_strides, float *d_cos, const int64_t *cos_strides,
                             const float *d_src, const int64_t *src_strides, const int64_t *shape, int rank, void *stream);
int laser_hip_sin_f32(float *dst, const float *src, int64_t len);
int laser_hip_cos_f32(float *dst, const float *src, int64_t len);

/* ---- F+tree weighted sampler (f32): benchmarks/random_sampling/fenwicktree.nim, bench_multinomial_samplers.nim --------
 * The reference's `Sampler` over device rows: from a row of weights (the softmax above, or anything non-negative) to drawn
 * indices without leaving the device.  All float32, every operation rounded to float32 on its own, no denormal flushed.
 * The caller supplies the uniform numbers, or names a stream of the library's counter-based generator ("Random numbers"
 * below; the _rng forms): either way every call is a pure function of its operands.
 * Tree image of one row of n weights w, 1 <= n <= LASER_HIP_SAMPLER_MAX_N = 2^24.  P = the next power of two >= n; a row is
 *   2 P elements:
 *     slot 0      +0
 *     slot P + i  w[i] for i < n, +0 for n <= i < P
 *     slot j      slot[2 j] + slot[2 j + 1]  for j = P - 1 .. 1   (one addition of exactly these two; slot 1 is the root)
 *   The order of summation is this balanced pairwise tree and nothing else, so an image is a function of the row's values and
 *   n alone, never of rows, the strides, the base alignment, the grid or the stream.  It is the reference's array
 *   (newSampler, fenwicktree.nim:67-118) shifted up by one slot, image[i + 1] == ref[i] -- the ONE layout deviation: with
 *   the shift every level and every (left, right) pair starts on an aligned boundary (children 2 j, 2 j + 1, parent j / 2).
 *   Rows are tree_row_stride elements apart, tree_row_stride >= 2 P; nothing is written past a row's 2 P elements.
 *   laser_hip_sampler_tree_elems(n, &elems): elems = 2 P.  Needs no device.
 * Draw for one row and one u01 in [0, 1):
 *     root = slot[1]; not finite or not > 0 (an all-zero row, a NaN, an Inf): the result is -1.
 *     u = u01 * root (one multiply); j = 1
 *     while j < P:  l = slot[2 j], r = slot[2 j + 1];  if u >= l && r > 0: u = u - l, j = 2 j + 1;  else j = 2 j
 *     the result is j - P.
 *   Without the `r > 0` test this is sampleImpl (fenwicktree.nim:126-145).  The test is needed: rounding can leave u >= l
 *   (u01 * root rounds up to the root; a parent rounded below the sum of its children's exact values) under a right subtree
 *   that sums to 0, and the reference then ends on a zero-weight or padding leaf.  With the test, non-negative finite weights
 *   and a root > 0: a node > 0 has a child > 0 (x + y > 0 needs x > 0 or y > 0), the descent enters the right child only when
 *   it is > 0, and the left child only when u < l (so l > 0) or r is not > 0 (so l = node > 0): every node on the path is > 0,
 *   the leaf too, so 0 <= index < n and w[index] > 0.  The two rules differ only where the reference returns such an
 *   impossible element (on the host, 460 800 draws over sparse rows scaled by 10^+-30, n in {1, 2, 3, 5, 63, 64, 65, 1000,
 *   1025, 4097}, u01 random, 0 and 1 - 2^-24: 0 bad results with the test, 128 without).  Negative weights with a finite positive root: whatever the rule reaches (it stays inside
 *   [0, P)); nothing is promised about it.
 * Update(row, idx, w): slot[P + idx] = w, then slot[j] = slot[2 j] + slot[2 j + 1] for j = (P + idx) / 2 .. 1 (halving):
 *   the bits a rebuild would give.  idx = -1 does nothing; any other idx outside [0, n) is skipped (the indices live on the
 *   device, the host cannot check them).
 * Draw and remove, k times: for s = 0 .. k - 1: idx = draw(u01[row, s]); store it; update(row, idx, +0) unless it is -1.  Once
 *   the root is 0 the remaining draws are -1 (sampleAndRemove, fenwicktree.nim:186-199).
 * laser_hip_sampler_build_f32_dev      d_w: `rows` rows of n weights, w_row_stride >= n elements apart, elements of a row
 *                                      contiguous, any base alignment; writes rows images.
 * laser_hip_sampler_sample_f32_dev     m independent draws per row with replacement; d_u01 and d_idx are (rows, m) row-major;
 *                                      the tree is only read.
 * laser_hip_sampler_sample_remove_f32_dev   k draws per row without replacement; d_u01 and d_idx are (rows, k) row-major;
 *                                      MUTATES the tree.  One lane owns a row for the whole launch (k * log2 P dependent
 *                                      accesses); a concurrent sample on the same tree from another stream is the caller's race.
 * laser_hip_sampler_update_f32_dev     one (d_elem[row], d_weight[row]) per row; mutates the tree; the same race rule.
 * laser_hip_sampler_sample_rng_f32_dev, laser_hip_sampler_sample_remove_rng_f32_dev   the two draws with u01[row, j] = the f32
 *                                      u01 of word offset + row * m + j (k for m) of the stream (seed, subseq) of "Random numbers",
 *                                      made in the kernel: no buffer of uniform numbers is written or read.  The indices (and,
 *                                      for remove, the trees afterwards) are exactly those of laser_hip_random_uniform_f32_dev
 *                                      (lo = 0, hi = 1) into a (rows, m) buffer followed by the call above.  The draws use
 *                                      rows * m words.
 * All asynchronous on `stream`; pointers are device pointers; indices are int32.  LASER_HIP_E_INVALID, in this order: n
 *   outside 1 .. 2^24, a negative rows / m / k, tree_row_stride < 2 P, w_row_stride < n; then the device is looked for
 *   (LASER_HIP_E_NODEVICE without a gfx950); then rows = 0 (or m = 0, k = 0) does nothing; then a null pointer is
 *   LASER_HIP_E_INVALID.
 * laser_hip_sampler_plan(rows, n, out4): what the build would launch, without a device: out4 = {kernel: 0 = whole rows in LDS
 *   (P <= 512), 1 = segments of 1024 leaves plus a second launch for the levels above them; leaves a workgroup owns in one
 *   step; workgroups of the first launch; workgroups of the second launch (0: none)}.  The logic is
 *   laser_amd/csrc/sampler_plan.h, which has no HIP dependency.
 * Not built: float64, weights along an axis other than the last, alias tables.  The benchmark's other sampler (cumsum +
 *   searchsorted) is the next section, "Row cumsum, searchsorted and the inverse-CDF sampler". */
#define LASER_HIP_SAMPLER_MAX_N (1ll << 24)
int laser_hip_sampler_tree_elems(int64_t n, int64_t *elems);
int laser_hip_sampler_plan(int64_t rows, int64_t n, int64_t *out4);
int laser_hip_sampler_build_f32_dev(float *d_tree, int64_t tree_row_stride, const float *d_w, int64_t w_row_stride,
                                    int64_t rows, int64_t n, void *stream);
int laser_hip_sampler_sample_f32_dev(int32_t *d_idx, const float *d_tree, int64_t tree_row_stride, const float *d_u01,
                                     int64_t rows, int64_t n, int64_t m, void *stream);
int laser_hip_sampler_sample_remove_f32_dev(int32_t *d_idx, float *d_tree, int64_t tree_row_stride, const float *d_u01,
                                            int64_t rows, int64_t n, int64_t k, void *stream);
int laser_hip_sampler_update_f32_dev(float *d_tree, int64_t tree_row_stride, const int32_t *d_elem, const float *d_weight,
                                     int64_t rows, int64_t n, void *stream);
int laser_hip_sampler_sample_rng_f32_dev(int32_t *d_idx, const float *d_tree, int64_t tree_row_stride, int64_t seed,
                                         int64_t subseq, int64_t offset, int64_t rows, int64_t n, int64_t m, void *stream);
int laser_hip_sampler_sample_remove_rng_f32_dev(int32_t *d_idx, float *d_tree, int64_t tree_row_stride, int64_t seed,
                                                int64_t subseq, int64_t offset, int64_t rows, int64_t n, int64_t k,
                                                void *stream);

/* ---- Row cumsum, searchsorted and the inverse-CDF sampler: bench_multinomial_samplers.nim:49-61, 143-214 ----------------
 * The other half of the reference's sampling benchmark: `cumsum` over the rows of a matrix, `searchsorted` (lowerBound /
 * upperBound) and `sample`, the classic inverse-CDF multinomial draw -- the baseline the F+tree above is measured against.
 * One definition, laser_amd/csrc/scan_core.h (no HIP dependency: a host program can include it); tests/scan_model.py is the
 * numpy model.
 * Scan order.  An inclusive prefix sum along the contiguous last axis, one row at a time.  R = LH_SCAN_RUN (scan_core.h; 32,
 *   the fastest of 8, 16 and 32 at 128 rows of 50 000: profiles/scan).
 *   Row x[0..n) is cut into runs, run r = [r R, min(n, (r + 1) R)).
 *     loc(i) = x[i] at the first element of a run, else fl(loc(i - 1) + x[i])       (a serial sum inside the run)
 *     run 0:       out[i] = loc(i)
 *     run r >= 1:  out[i] = fl(carry_r + loc(i)), one addition, carry_r = out[r R - 1]   (the value stored for the last
 *                  element of the previous run)
 *   Every addition is rounded on its own in the element type; no denormal is flushed, nothing is reassociated.  The result is
 *   a function of the row's values, n and R alone, never of rows, the strides, the base alignment, the grid or the stream.
 *   The integer types wrap mod 2^32 / 2^64, where any order gives the serial result.  A usual work-efficient parallel float
 *   scan is NOT monotone (a later prefix can round below an earlier one); this order is, by construction.  For non-negative
 *   finite input without overflow:
 *   (a) Monotone: out is non-decreasing.  Inside a run loc is a serial sum of non-negatives, so loc is non-decreasing, and
 *       c -> fl(c + .) is monotone; across a boundary out[r R] = fl(out[r R - 1] + x[r R]) >= out[r R - 1].
 *   (b) Zero steps: x[i] == 0 (either sign) gives out[i] == out[i - 1].  Inside a run loc(i) = fl(loc(i - 1) + 0) = loc(i - 1),
 *       so out does not move; at a run's first element out[i] = fl(carry + 0) = carry = out[i - 1].
 *   The price is a chain of ceil(n / R) - 1 dependent additions per row, carry_{r+1} = fl(carry_r + total_r); the R-element
 *   local sums and the final carry + loc are parallel across lanes, rows across workgroups.
 * Search.  The result of this exact descent on any input, sorted or not, NaN included: lo = 0, count = n; while count > 0:
 *   step = count / 2, pos = lo + step; go right (lo = pos + 1, count -= step + 1) iff a[pos] < v (left side, right = 0) or
 *   a[pos] <= v (right side, right != 0); otherwise count = step.  The result is lo, in [0, n].  A comparison with NaN is
 *   false, so NaN goes left: what the reference's lowerBound / upperBound do.  At most 25 steps for n <= 2^24.
 * CDF draw (f32) for one row and one u01 in [0, 1):
 *     total = cdf[n - 1]; not finite or not > 0: the result is -1 (the rule of the F+tree root).
 *     u = u01 * total, one multiply -- the documented deviation from the reference, which divides the whole CDF by its last
 *       element instead; it is the F+tree draw's.
 *     idx = the right-side search of u;  idx == n: idx = the left-side search of total.
 *   The last rule is needed when u01 * total rounds up to total; in float32 that happens only for denormal totals (the smallest
 *   denormal times 1 - 2^-24 rounds to itself).  With a CDF made by the scan above from non-negative finite weights w, every
 *   result has 0 <= idx < n and w[idx] > 0: by (a) the searches are those of a sorted row.  The right-side search gives the
 *   first idx with cdf[idx] > u >= 0 and, for idx > 0, cdf[idx - 1] <= u < cdf[idx]: the CDF moves at idx, so by (b) w[idx] is
 *   not 0 (idx = 0: w[0] = cdf[0] > 0).  idx == n means u >= total, so u == total, and the left-side search gives the first
 *   idx with cdf[idx] >= total, which exists (n - 1 qualifies) and again has cdf[idx - 1] < cdf[idx] or idx = 0.
 * Draw and remove, min(k, n) rounds: round s scans the weights into the CDF workspace, draws with u01[row, s], stores the index
 *   and sets w[row, idx] = +0 unless the index is -1 (the reference zeroes, recomputes the CDF and rescales it; here the
 *   multiply by the fresh total stands for the rescaling).  Columns s >= n are -1.  Two launches per round.  OVERWRITES the
 *   caller's weights; d_cdf is workspace of rows rows, cdf_row_stride >= n apart.
 * laser_hip_cumsum_{f32,f64,i32,i64}_dev   rows rows of n elements, row strides >= n elements, the elements of a row contiguous,
 *                                      any base alignment of the element type.  d_dst == d_src with equal strides (in place)
 *                                      works; any other overlap is the caller's error.  Nothing outside a row's n elements is
 *                                      written.
 * laser_hip_searchsorted_{f32,f64,i32,i64}_dev   d_v and d_idx are (rows, m) row-major; row i of d_v is searched in row i of d_a.
 * laser_hip_cdf_sample_f32_dev         m draws per row with replacement; d_u01 and d_idx are (rows, m) row-major.
 * laser_hip_cdf_sample_remove_f32_dev  k draws per row without replacement; d_u01 and d_idx are (rows, k) row-major.
 * laser_hip_cdf_sample_rng_f32_dev, laser_hip_cdf_sample_remove_rng_f32_dev   the two draws with u01[row, j] = the f32 u01 of
 *                                      word offset + row * m + j (k for m) of the stream (seed, subseq) of "Random numbers", made
 *                                      in the kernel: exactly the results of laser_hip_random_uniform_f32_dev (lo = 0, hi = 1)
 *                                      into a (rows, m) buffer followed by the buffer form.
 * All asynchronous on `stream`; pointers are device pointers; indices are int32.  LASER_HIP_E_INVALID, in this order: n
 *   outside 1 .. LASER_HIP_SCAN_MAX_N = 2^24, a negative rows / m / k, a row stride < n; then the device is looked for
 *   (LASER_HIP_E_NODEVICE without a gfx950); then rows = 0 (or m = 0, k = 0) does nothing; then a null pointer is
 *   LASER_HIP_E_INVALID.
 * Kernels (laser_amd/csrc/scan.hip).  cumsum: a workgroup of 256 lanes owns a row (n > 64 R) or four rows of a wave each, and
 *   walks the row in tiles of 256 R (64 R) elements.  A lane owns one run of the tile: R elements in registers (16-byte loads
 *   and stores where both bases and both row strides allow, element by element otherwise and for the row's last, partial
 *   run: same bits), the run's total into LDS.  ONE lane per row walks the tile's chain, the fewest that keep the order;
 *   meanwhile the other waves form the local sums of the next tile, whose loads were issued before the chain.  Then every
 *   lane adds its run's carry and stores.  No workgroup waits on another and nothing spins.  searchsorted and the draws: one
 *   lane per (row, value); a round of draw-and-remove: one lane per row.
 * laser_hip_cumsum_plan(rows, n, elem_size, cus, out4): what a cumsum would launch, without a device: out4 = {variant: 0 = a
 *   wave per row, 1 = a workgroup per row; rows a workgroup owns at a time (4 or 1: a tile is 256 / that * R elements);
 *   workgroups (at most 8 per compute unit; cus <= 0: 256 compute units, which is what the entry points plan for); tiles per
 *   row}.  elem_size 4 or 8.  The logic is laser_amd/csrc/scan_plan.h, which has no HIP dependency.
 * Not built: exclusive scans, scans along another axis, the other six element types, float64 draws, a scan across workgroups
 *   for one very long row (one workgroup walks it: the chain of n / R additions bounds it). */
#define LASER_HIP_SCAN_MAX_N (1ll << 24)
#define LASER_HIP_DECL_SCAN(SFX, T)                                                                                     \
  int laser_hip_cumsum_##SFX##_dev(T *d_dst, int64_t dst_row_stride, const T *d_src, int64_t src_row_stride,           \
                                   int64_t rows, int64_t n, void *stream);                                              \
  int laser_hip_searchsorted_##SFX##_dev(int32_t *d_idx, const T *d_a, int64_t a_row_stride, const T *d_v,             \
                                         int64_t rows, int64_t n, int64_t m, int right, void *stream);
LASER_HIP_DECL_SCAN(f32, float)
LASER_HIP_DECL_SCAN(f64, double)
LASER_HIP_DECL_SCAN(i32, int32_t)
LASER_HIP_DECL_SCAN(i64, int64_t)
#undef LASER_HIP_DECL_SCAN
int laser_hip_cumsum_plan(int64_t rows, int64_t n, int elem_size, int cus, int64_t *out4);
int laser_hip_cdf_sample_f32_dev(int32_t *d_idx, const float *d_cdf, int64_t cdf_row_stride, const float *d_u01,
                                 int64_t rows, int64_t n, int64_t m, void *stream);
int laser_hip_cdf_sample_remove_f32_dev(int32_t *d_idx, float *d_w, int64_t w_row_stride, float *d_cdf,
                                        int64_t cdf_row_stride, const float *d_u01, int64_t rows, int64_t n, int64_t k,
                                        void *stream);
int laser_hip_cdf_sample_rng_f32_dev(int32_t *d_idx, const float *d_cdf, int64_t cdf_row_stride, int64_t seed,
                                     int64_t subseq, int64_t offset, int64_t rows, int64_t n, int64_t m, void *stream);
int laser_hip_cdf_sample_remove_rng_f32_dev(int32_t *d_idx, float *d_w, int64_t w_row_stride, float *d_cdf,
                                            int64_t cdf_row_stride, int64_t seed, int64_t subseq, int64_t offset,
                                            int64_t rows, int64_t n, int64_t k, void *stream);

/* ---- Random numbers: Philox4x32-10, randomTensor's uniform fills and normal fills -- the `randomTensor(shape, valrange)` and
 * `randomTensor(shape, max)` that open the reference's benchmarks (bench_exp.nim:17, reduction_bench.nim:40, ...) ----------
 * A counter-based generator (Salmon, Moraes, Dror, Shaw, SC'11): word w of a stream is a function of (seed, subseq, w) and of
 * nothing else.  No state lives on the device; a call captured in a graph replays the same numbers; a result never depends on
 * the grid, the stream, the base alignment or on how a fill was cut into calls.  One definition, laser_amd/csrc/philox_core.h
 * (no HIP dependency: a host program can include it); tests/philox_model.py is the numpy model.
 * seed, subseq and offset are 64-bit patterns read as UNSIGNED (mod 2^64).  They travel as int64_t like every other 64-bit
 *   integer of this ABI: pass the same bits (a uint64_t converts implicitly).
 * Philox4x32-10: multipliers 0xD2511F53 and 0xCD9E8D57, Weyl key increments 0x9E3779B9 and 0xBB67AE85, ten rounds.  Word w of
 *   the stream (seed, subseq) is word w & 3 of the block with counter {lo32(b), hi32(b), lo32(subseq), hi32(subseq)}, b = w >> 2,
 *   and key {lo32(seed), hi32(seed)}.  Counter and key all 0 give 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 * Element i of a call uses word (offset + i) mod 2^64; a 64-bit element type uses the pair (offset + 2 i, offset + 2 i + 1),
 *   low word first: x = w0 | w1 << 32.  A fill of n elements uses n (2 n) words: the next call continues at offset + n (2 n).
 * Distributions; every float operation rounded on its own in the element type, no fused multiply-add:
 *   bits_u32         the word itself
 *   u01 f32          float(x >> 8) * 2^-24, in [0, 1), at most 1 - 2^-24;   u01 f64: double(x >> 11) * 2^-53 of the 64-bit x
 *   uniform_f32/f64  on the CLOSED interval [lo, hi] like Nim's rand(a..b): t = u01 * (hi - lo), v = lo + t, the result
 *                    min(v, hi) -- the min is needed: float32 (1, 2) and (0.1, 0.3) reach hi at the largest u01.  lo = 0,
 *                    hi = 1 returns u01's bits, so there is no separate u01 entry point.  Valid: lo, hi and hi - lo finite,
 *                    lo <= hi.
 *   uniform_i32      on [lo, hi]: span = hi - lo + 1 in 1 .. 2^32; lo + int32((uint64(x) * span) >> 32)
 *   uniform_i64      span = hi - lo + 1 mod 2^64; 0 is the full range: x as a signed value; else lo + mulhi64(x, span), wrapping
 *   The integer multiply-shift is biased: a value's probability is off by a factor of at most 1 +- span / 2^32 (i32) or
 *   span / 2^64 (i64).  No rejection loop: an element costs a fixed number of words.  lo <= hi is required.
 * The fills are asynchronous on `stream`; d_dst is a device pointer to n contiguous elements, any alignment of the element
 *   type.  LASER_HIP_E_INVALID, in this order: n outside 0 .. LASER_HIP_RANDOM_MAX_N = 2^60, bounds that are not valid; then
 *   the device is looked for (LASER_HIP_E_NODEVICE without a gfx950); then n = 0 does nothing; then a null pointer is
 *   LASER_HIP_E_INVALID.
 * Kernels: one lane computes one Philox block per step and stores the elements that start in it (four 32-bit, two 64-bit: 16
 *   contiguous bytes) with one 16-byte store; blocks partly outside [0, n) (the head when offset & 3 != 0, the tail) and
 *   destinations whose runs are off their 16-byte boundaries are stored element by element, same bits.  A 64-bit type at an odd
 *   offset has elements that straddle two blocks; the lane computes both (twice the arithmetic).
 * laser_hip_random_plan(n, words_per_elem, offset, dst_misaligned, cus, out4): what a fill would launch, without a device:
 *   out4 = {variant: 0 = 16-byte stores, 1 = single-element; workgroups of 256 lanes (at most 8 per compute unit; cus <= 0: 256
 *   compute units); the most blocks one lane walks; the index of the first block, offset >> 2}.  words_per_elem: 1 for the 32-bit
 *   types, 2 for the 64-bit ones.  The fills plan for 256 compute units on every device.  The logic is
 *   laser_amd/csrc/random_plan.h, which has no HIP dependency.
 * normal_f32: Box-Muller on the same streams, fixed so that a fill can be cut anywhere (laser_amd/csrc/normal_core.h;
 *   tests/normal_model.py is the numpy model).  One word per element: element i is stream position p = offset + i, offsets count
 *   elements as for the 32-bit uniform fills and the next call continues at offset + n.  Pair q = p >> 1 owns words w0 = word(2q)
 *   and w1 = word(2q + 1); an even p is the pair's cosine branch, an odd p its sine branch, and a fill that starts or ends inside
 *   a pair stores only its half.
 *     radius  u = float((w0 >> 8) + 1) * 2^-24 in (0, 1];  L = llog(u);  r = sqrt(|-2 L|), a correctly rounded float32 square root
 *             (u = 1 gives +0)
 *     angle   k = w1 >> 8, the angle is 2 pi k / 2^24: reduced exactly on the integer to a quadrant and a fraction f in
 *             [-2^21, 2^21), a = (float64(f) * 2^-22) * float64(pi/2) (one rounding), t = float32(lsin's / lcos' own float64 sine
 *             or cosine kernel at a, chosen and signed by the quadrant)
 *     result  z = r * t;  out = mean + std * z: three float32 roundings, never contracted.  |z| <= sqrt(48 ln 2) < 5.77, every
 *             result is finite.  Valid: mean finite, std finite and >= 0 (checked where the uniform fills check their bounds).
 *   The kernel is the uniform fills' and random_plan.h plans it with one word per element: with 16-byte stores a lane turns one
 *   Philox block into two pairs, four results, the radius and the angle reduction shared inside each pair.
 * Not built: float64 normals, other distributions, the other six element types, strided destinations, a laser_rand callable in
 *   forEach bodies. */
#define LASER_HIP_RANDOM_MAX_N (1ll << 60)
int laser_hip_random_plan(int64_t n, int words_per_elem, int64_t offset, int dst_misaligned, int cus, int64_t *out4);
int laser_hip_random_bits_u32_dev(uint32_t *d_dst, int64_t n, int64_t seed, int64_t subseq, int64_t offset, void *stream);
int laser_hip_random_uniform_f32_dev(float *d_dst, int64_t n, float lo, float hi, int64_t seed, int64_t subseq,
                                     int64_t offset, void *stream);
int laser_hip_random_uniform_f64_dev(double *d_dst, int64_t n, double lo, double hi, int64_t seed, int64_t subseq,
                                     int64_t offset, void *stream);
int laser_hip_random_uniform_i32_dev(int32_t *d_dst, int64_t n, int32_t lo, int32_t hi, int64_t seed, int64_t subseq,
                                     int64_t offset, void *stream);
int laser_hip_random_uniform_i64_dev(int64_t *d_dst, int64_t n, int64_t lo, int64_t hi, int64_t seed, int64_t subseq,
                                     int64_t offset, void *stream);
int laser_hip_random_normal_f32_dev(float *d_dst, int64_t n, float mean, float std, int64_t seed, int64_t subseq,
                                    int64_t offset, void *stream);

/* ---- forEachReduce: forEach with a private accumulator per lane, merged at the end ---------------------------------
 * The device form of forEachStaged (laser/strided_iteration/foreach_staged.nim:318), e.g. a dot product:
 *   forEachReduce acc (f64) in x, y:  body "acc += x * y",  merge "acc += other",  init 0
 * The spec is forEach's (body, operands, writability, parameters; the same rules) plus
 *   acc_name    the accumulator's name in the body and in `merge` (a C identifier under forEach's naming rules)
 *   acc_dtype   its element type, any LASER_HIP_DT_*
 *   merge       a C++ statement that merges the accumulator `other` into `acc_name`: "acc += other",
 *               "acc = fmaxf(acc, other)".  `other` is reserved: no operand, parameter or accumulator may be called so.
 * The body runs once per element of `shape` in the order of "Reductions" above (E from the widest OPERAND), with the
 * accumulator as a reference; writable operands are stored back as in forEach, so "y = expf(x - m); acc += y" writes y and
 * sums it in one pass.  `init` must be an identity of `merge` (every private accumulator starts from it, and the folds
 * merge accumulators that saw no element).  Empty merge, a clash with `other`, or an acc_name equal to an operand or
 * parameter name: LASER_HIP_E_INVALID.  Compiles are cached apart from forEach's and counted in "foreach_compiles".
 * foreach_reduce_source / _code / _kernel   as foreach_source / _code / _kernel
 * foreach_reduce_dev   as foreach_dev, plus `init` (one 8-byte slot like a parameter, the value in its low bytes: a new
 *                      value does not compile again) and d_out (device address of one accumulator).  Asynchronous;
 *                      size 0 writes init.  get_option "last_foreach_variant" tells its traversal as for foreach_dev. */
int laser_hip_foreach_reduce_source(const char *body, int nops, const char *const *names, const int *dtypes,
                                    const int *writable, int nparams, const char *const *param_names,
                                    const int *param_dtypes, const char *acc_name, int acc_dtype, const char *merge,
                                    char *buf, int64_t cap, int64_t *len);
int laser_hip_foreach_reduce_code(const char *body, int nops, const char *const *names, const int *dtypes,
                                  const int *writable, int nparams, const char *const *param_names,
                                  const int *param_dtypes, const char *acc_name, int acc_dtype, const char *merge,
                                  const char *arch, void *buf, int64_t cap, int64_t *len);
int laser_hip_foreach_reduce_kernel(const char *body, int nops, const char *const *names, const int *dtypes,
                                    const int *writable, int nparams, const char *const *param_names,
                                    const int *param_dtypes, const char *acc_name, int acc_dtype, const char *merge,
                                    int64_t *handle);
int laser_hip_foreach_reduce_dev(int64_t handle, void *const *ptrs, const int64_t *strides, const int64_t *shape,
                                 int rank, const void *params, const void *init, void *d_out, void *stream);

/* ---- row-panel sharded gemm_strided over the GPUs of one node, ONE process ---------------------------------------
 * Laser partitions M across its OpenMP threads with no cross-thread reduction (gemm.nim:160-176: `omp for` over the
 * ic row blocks), so rows of C are independent units: each GPU owns row panels of A, all of B, and produces the
 * matching rows of C.  No K split => no reduction => every element is computed exactly as on one GPU (bit-identical,
 * whatever the device count).  `devices`: ndev HIP ordinals, or NULL for 0..ndev-1; ndev <= 0 = every visible GPU.
 * Both forms are synchronous (return when every device is done); one host thread per GPU drives it.
 *
 * Host pointers (the drop-in form -- same parameter list as gemm_strided after the device list): the rows are cut
 * into one contiguous range per GPU, each GPU runs the ordinary host-pointer pipeline on its own PCIe link and writes
 * its rows of C straight back to host memory (no inter-GPU traffic).  laser_hip_set_shard_devices(n) makes the PLAIN
 * laser_hip_gemm_strided_* entry points route large problems here (n = 1: off, the default; 0: every GPU), so an
 * unchanged Nim gemm_strided call uses the node. */
int laser_hip_set_shard_devices(int ndev);
int laser_hip_get_shard_devices(void);
/* Device-resident form (operands already in HBM; what the roofline is measured on).  The call has no stream parameter: it works on
 * the library's own streams (one set per device slot), so every operand must be COMPLETE in memory when it is made -- a caller that
 * fills A / B / C asynchronously on its own stream synchronises that stream first (the Python mirror does).  Rows are dealt block-cyclically:
 * panel (s, g) -- sub-panel s of device slot g -- is rows [(s*ndev + g)*R, +R) of C, R = rows_per_panel from
 * laser_hip_shard_plan (a multiple of 256 when M allows; panels_per_dev is reduced if steps would be empty).
 *   dA_panels[g]  device slot g's panels of A stacked in local order: row s*R + i = global row (s*ndev + g)*R + i
 *                 (element strides rowStrideA / colStrideA)
 *   dB[g]         B, replicated on every device (strides rowStrideB / colStrideB)
 *   dC[g]         the FULL row-major C on every device (colStride 1, rowStrideC >= N): device g computes its panels in
 *                 place and, with a gather mode, receives everybody else's -- the all-gather of C over xGMI -- sub-panel
 *                 s being sent while sub-panel s+1 multiplies.  beta != 0 reads the device's own copy of its rows.
 *   gather        LASER_HIP_GATHER_NONE  every device keeps only its own rows;
 *                 LASER_HIP_GATHER_PEER  the owner pushes finished rows to every peer with hipMemcpyPeerAsync on one
 *                                        copy stream per peer (all xGMI links at once, SDMA engines, no CUs);
 *                 LASER_HIP_GATHER_RCCL  ncclAllGather per slab (librccl.so loaded on first use; needs
 *                                        rowStrideC == N and dC[g] sized for padded_M rows).
 *   flags         LASER_HIP_SHARD_PIN_TILE: the hand-scheduled 128x128x16 assembly tile (option "asm_tile" = 2) for the local f32
 *                 products of this call (RCCL's kernels hold CUs meanwhile); other dtypes ignore it.
 * On an error return the operand buffers must stay alive until the devices are idle (work queued by the failed call may still
 * name them); the library drops the streams it queued that work on and makes new ones for the next call. */
#define LASER_HIP_GATHER_NONE 0
#define LASER_HIP_GATHER_PEER 1
#define LASER_HIP_GATHER_RCCL 2
#define LASER_HIP_SHARD_PIN_TILE 1
int laser_hip_shard_plan(int64_t M, int ndev, int panels_per_dev, int64_t *rows_per_panel,
                         int *panels_per_dev_used, int64_t *padded_M);
#define LASER_HIP_DECL_SHARDED(SFX, T)                                                            \
  int laser_hip_gemm_strided_##SFX##_sharded(int ndev, const int *devices, int64_t M, int64_t N,  \
                                             int64_t K, T alpha, const T *A, int64_t rowStrideA,  \
                                             int64_t colStrideA, const T *B, int64_t rowStrideB,  \
                                             int64_t colStrideB, T beta, T *C, int64_t rowStrideC,\
                                             int64_t colStrideC);                                 \
  int laser_hip_gemm_strided_##SFX##_sharded_dev(                                                 \
      int ndev, const int *devices, int64_t M, int64_t N, int64_t K, T alpha,                     \
      const T *const *dA_panels, int64_t rowStrideA, int64_t colStrideA, const T *const *dB,      \
      int64_t rowStrideB, int64_t colStrideB, T beta, T *const *dC, int64_t rowStrideC,           \
      int panels_per_dev, int gather, int flags);
LASER_HIP_DECL_SHARDED(f32, float)
LASER_HIP_DECL_SHARDED(f64, double)
LASER_HIP_DECL_SHARDED(i32, int32_t)
LASER_HIP_DECL_SHARDED(i64, int64_t)
#undef LASER_HIP_DECL_SHARDED

/* ---- pinned host memory (optional) ---------------------------------------------------------------------------------
 * The host-pointer entry points accept ANY host memory.  From pageable memory the runtime stages or pins every copy on
 * the fly; a tensor allocator that wants the full PCIe rate allocates its buffers with host_alloc (64-byte aligned, as
 * LASER_MEM_ALIGN asks) or registers existing ones -- Laser leaves buffer management to the caller (Design.md:5-7).
 * The same entry points then move the operands by direct asynchronous DMA; results are identical. */
int laser_hip_host_alloc(void **host_ptr, int64_t bytes);
int laser_hip_host_free(void *host_ptr);
int laser_hip_host_register(void *host_ptr, int64_t bytes);
int laser_hip_host_unregister(void *host_ptr);

/* ---- cblas-shaped GEMM -- benchmarks/third_party/blas.nim:12-23 ---------------------------------
 * The call conv2d_im2col makes (conv2d_im2col.nim:161-166); ORDER 101 rowMajor / 102 colMajor,
 * TRANS 111 noTranspose / 112 transpose / 113 conjTranspose.  Mapped onto gemm_strided strides. */
int laser_hip_cblas_sgemm(int order, int transA, int transB, int64_t M, int64_t N, int64_t K,
                          float alpha, const float *A, int64_t lda, const float *B, int64_t ldb,
                          float beta, float *C, int64_t ldc);
int laser_hip_cblas_dgemm(int order, int transA, int transB, int64_t M, int64_t N, int64_t K,
                          double alpha, const double *A, int64_t lda, const double *B, int64_t ldb,
                          double beta, double *C, int64_t ldc);

#ifdef __cplusplus
}
#endif
#endif /* LASER_HIP_H */
