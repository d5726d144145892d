# laser_hip_select.nim -- the C-ABI of include/laser_hip_select.h ("Row top-k, argmax and top-k sampling") for Nim: the
# entry points of the same liblaser_hip.so that are declared in a header of their own.  nim/laser_hip.nim cannot carry these
# imports: every importc of that file is held against include/laser_hip.h.  `import laser_hip, laser_hip_select`.
#
# The order is one of bit patterns: key(x) = bits xor 0xFFFFFFFF with the sign bit set, bits xor 0x80000000 otherwise; largest
# ranks by descending key, elements of identical bits by ascending column.  A positive NaN is the largest element, -0 ranks
# below +0, and every bit and index of a result is a function of the row's bits, k and `largest` alone.

import laser_hip

{.pragma: lh, cdecl, dynlib: laserHip.}

proc laser_hip_topk_rows_f32_dev*(vals: ptr float32, valsRowStride: int64, idx: ptr int32, idxRowStride: int64, src: ptr float32, srcRowStride: int64, rows: int64, n: int64, k: int64, largest: cint, stream: pointer): cint {.lh, importc: "laser_hip_topk_rows_f32_dev".}
proc laser_hip_argmax_rows_f32_dev*(idx: ptr int32, idxStride: int64, val: ptr float32, valStride: int64, src: ptr float32, srcRowStride: int64, rows: int64, n: int64, largest: cint, stream: pointer): cint {.lh, importc: "laser_hip_argmax_rows_f32_dev".}
proc laser_hip_take_rows_i32_dev*(outp: ptr int32, outRowStride: int64, src: ptr int32, srcRowStride: int64, j: ptr int32, jRowStride: int64, rows: int64, m: int64, num: int64, stream: pointer): cint {.lh, importc: "laser_hip_take_rows_i32_dev".}
proc laser_hip_topk_plan*(rows: int64, n: int64, k: int64, vec: cint, out3: ptr int64): cint {.lh, importc: "laser_hip_topk_plan".}
proc laser_hip_topk_last_kernel*(): cint {.lh, importc: "laser_hip_topk_last_kernel".}

template check(rc: cint) =
  # as laser_hip.nim: the procs return nothing and doAssert on a refused call (the text: laser_hip_last_error of the library)
  let code = rc
  doAssert code == 0, "laser_hip error " & $code

proc topk*(vals: DevicePtr[float32], idx: DevicePtr[int32], src: DevicePtr[float32], rows, n, k: Natural, largest: bool = true, stream: pointer = nil) =
  ## the k first elements of each of `rows` contiguous rows of n float32 and their columns, rank 0 first, into contiguous rows
  ## of k; vals (bit copies) or idx may be nil, not both; 1 <= k <= min(n, 1024), n <= 2^24
  check laser_hip_topk_rows_f32_dev(cast[ptr float32](vals), int64(k), cast[ptr int32](idx), int64(k), cast[ptr float32](src), int64(n), int64(rows), int64(n), int64(k), cint(ord(largest)), stream)

proc argmax*(idx: DevicePtr[int32], src: DevicePtr[float32], rows, n: Natural, stream: pointer = nil) =
  ## idx[r] = the column of the largest element of row r (the lowest column among identical bits): topk with k = 1, one pass
  check laser_hip_argmax_rows_f32_dev(cast[ptr int32](idx), 1, nil, 1, cast[ptr float32](src), int64(n), int64(rows), int64(n), 1, stream)

proc argmin*(idx: DevicePtr[int32], src: DevicePtr[float32], rows, n: Natural, stream: pointer = nil) =
  ## idx[r] = the column of the smallest element of row r
  check laser_hip_argmax_rows_f32_dev(cast[ptr int32](idx), 1, nil, 1, cast[ptr float32](src), int64(n), int64(rows), int64(n), 0, stream)

proc takeRows*(outp, src, j: DevicePtr[int32], rows, m, num: Natural, stream: pointer = nil) =
  ## outp[r, c] = src[r, j[r, c]] over contiguous rows (src: m per row; j and outp: num per row); -1 where j is outside 0 ..< m
  check laser_hip_take_rows_i32_dev(cast[ptr int32](outp), int64(num), cast[ptr int32](src), int64(m), cast[ptr int32](j), int64(num), int64(rows), int64(m), int64(num), stream)
