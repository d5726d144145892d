"""Row selection on the device (include/laser_hip_select.h "Row top-k, argmax and top-k sampling"), float32:

    laser_amd.topk(x, k, largest=True, values=True, indices=True) -> (values, indices)
        the k first elements of every row in the key order with their columns; what is not asked for is None
    laser_amd.argmax(x), laser_amd.argmin(x) -> int32 Tensor of x's leading shape
    laser_amd.take_rows(src, j) -> out[r, c] = src[r, j[r, c]], -1 where j[r, c] is outside the row

The order is one of bit patterns: key(x) = bits ^ 0xFFFFFFFF with the sign bit set, bits ^ 0x80000000 otherwise; largest ranks
by descending key, elements of identical bits by ascending column.  So a positive NaN is the largest element, -0 ranks below
+0, and every bit and index of a result is a function of the row's bits, k and `largest` alone.  `x` is a 2-D (rows, n)
device tensor or view with unit column stride, or a contiguous tensor of higher rank taken as (prod(leading), n), as
layer_norm takes its operand.  Operands are laser_amd.Tensors or torch CUDA tensors; calls are asynchronous on the current
torch stream.  Top-k sampling built from these: laser_amd.sample_top_k (sampling.py).
"""
import ctypes as C

import numpy as np

from . import _lib
from .foreach import _View
from .tensor import _stream, newTensor

__all__ = ["topk", "argmax", "argmin", "take_rows", "topk_plan", "topk_last_kernel"]

SELECT_MAX_N = 1 << 24
SELECT_MAX_K = 1024


def _rows(fn, name, obj, dtype=np.float32):
    """(view, rows, n, row stride) of a row operand: a 2-D tensor or view whose columns have unit stride, or a C-contiguous
    tensor of higher rank, taken as (prod(leading), n)"""
    v = _View(name, obj)
    if v.dtype != dtype:
        raise TypeError(f"{fn}: {name} has element type {v.dtype} ({np.dtype(dtype)} only)")
    if v.rank < 2:
        raise ValueError(f"{fn}: {name} has rank {v.rank} (rows of a 2-D tensor or view, or a contiguous tensor of higher rank)")
    n = v.shape[-1]
    if n < 1 or n > SELECT_MAX_N:
        raise ValueError(f"{fn}: {name} has rows of {n} elements (1 <= n <= 2^24)")
    if v.rank == 2:
        rows = v.shape[0]
        if n > 1 and v.strides[1] != 1:
            raise ValueError(f"{fn}: {name} has column stride {v.strides[1]} (1 is needed: transposed views are not taken)")
        return v, rows, n, (v.strides[0] if rows > 1 else n)  # (the stride of a lone row is never applied)
    rows, acc = 1, 1
    for e, st in zip(reversed(v.shape), reversed(v.strides)):
        if e > 1 and st != acc:
            raise ValueError(f"{fn}: {name} of rank {v.rank} has strides {v.strides} (C-contiguous is needed above rank 2)")
        acc *= e
    for e in v.shape[:-1]:
        rows *= e
    return v, rows, n, n


def _k(fn, k, n):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= min(n, SELECT_MAX_K):
        raise ValueError(f"{fn}: k = {k!r} (1 <= k <= min(n, 1024) is needed; n = {n})")
    return int(k)


def topk(x, k, largest=True, values=True, indices=True):
    """(values, indices) of the k first elements of every row of `x`: float32 and int32 Tensors of x's leading shape + (k,),
    rank 0 first; values are bit copies.  values=False or indices=False: that result is None and is not computed (the other
    has the same bits either way); asking for neither raises."""
    v, rows, n, xs = _rows("topk", "x", x)
    k = _k("topk", k, n)
    if not values and not indices:
        raise ValueError("topk: neither values nor indices are asked for")
    lead = v.shape[:-1]
    vals = newTensor(np.float32, *lead, k) if values else None
    idx = newTensor(np.int32, *lead, k) if indices else None
    ptr = lambda t: C.c_void_p(t.unsafe_raw_data()) if t is not None else None
    _lib.check(_lib.lib().laser_hip_topk_rows_f32_dev(ptr(vals), k, ptr(idx), k, C.c_void_p(v.ptr), xs, rows, n, k, 1 if largest else 0,
                                                      _stream()))
    return vals, idx


def _arg(fn, x, largest):
    v, rows, n, xs = _rows(fn, "x", x)
    idx = newTensor(np.int32, *v.shape[:-1])
    _lib.check(_lib.lib().laser_hip_argmax_rows_f32_dev(C.c_void_p(idx.unsafe_raw_data()), 1, None, 1, C.c_void_p(v.ptr), xs, rows, n,
                                                        largest, _stream()))
    return idx


def argmax(x):
    """the column of the largest element of every row (a positive NaN is the largest; the lowest column among identical bits):
    topk(x, 1)'s index from a single pass; int32 Tensor of x's leading shape"""
    return _arg("argmax", x, 1)


def argmin(x):
    """the column of the smallest element of every row: topk(x, 1, largest=False)'s index"""
    return _arg("argmin", x, 0)


def take_rows(src, j):
    """out[r, c] = src[r, j[r, c]] for int32 `src` (rows, m) and `j` (rows, num), -1 where j[r, c] is outside [0, m): maps
    positions among a row's candidates (topk's indices) back to columns.  int32 Tensor of j's shape."""
    sv, rows, m, ss = _rows("take_rows", "src", src, np.int32)
    jv = _View("j", j)
    if jv.dtype != np.int32:
        raise TypeError(f"take_rows: j has element type {jv.dtype} (int32 only)")
    if jv.rank != 2 or jv.shape[0] != rows or sv.rank != 2:
        raise ValueError(f"take_rows: src {sv.shape} and j {jv.shape} (two matrices with the same number of rows are needed)")
    num = jv.shape[1]
    if num > 1 and jv.strides[1] != 1:
        raise ValueError(f"take_rows: j has column stride {jv.strides[1]} (1 is needed)")
    out = newTensor(np.int32, rows, num)
    if rows and num:
        _lib.check(_lib.lib().laser_hip_take_rows_i32_dev(C.c_void_p(out.unsafe_raw_data()), num, C.c_void_p(sv.ptr), ss, C.c_void_p(jv.ptr),
                                                          jv.strides[0] if rows > 1 else num, rows, m, num, _stream()))
    return out


def topk_plan(rows, n, k, vec=True):
    """(kernel code, workgroups, LDS bytes) of a top-k launch, without a device (laser_hip_topk_plan)"""
    out = (C.c_int64 * 3)()
    _lib.check(_lib.lib().laser_hip_topk_plan(int(rows), int(n), int(k), 1 if vec else 0, out))
    return tuple(out)


def topk_last_kernel():
    """the plan's kernel code of the last top-k launch in this process, + 8 after an argmax launch; -1: none yet"""
    return _lib.lib().laser_hip_topk_last_kernel()
