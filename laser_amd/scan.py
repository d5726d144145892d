"""Row prefix sums, sorted search and the inverse-CDF multinomial draw on the device: the `cumsum`, `searchsorted` and `sample`
of the reference's benchmarks/random_sampling/bench_multinomial_samplers.nim (include/laser_hip.h "Row cumsum, searchsorted
and the inverse-CDF sampler").

    laser_amd.cumsum(t)                                  inclusive prefix sum along the last axis -> Tensor of t's type and shape
    laser_amd.searchsorted(a, v, leftSide=True)          per row: where v would go in the sorted row -> int32 Tensor like v
    laser_amd.cdfSample(cdf, u=None, num=1, rng=None)    num draws per row with replacement from rows of CDFs -> int32 (rows, num)
    laser_amd.cdfSampleAndRemove(weights, u=None, num=1, rng=None)   num draws per row without replacement from rows of weights

Operands are laser_amd.Tensors or torch CUDA tensors of rank 1 (one row) or 2 whose rows are contiguous; float32, float64,
int32 and int64 for cumsum and searchsorted, float32 for the draws.  The order of the float sums is fixed (scan_core.h), so a
result is a function of the row alone, bit for bit, and a CDF made by `cumsum` from non-negative weights never lets a draw
return an element of weight 0.  `u`, `num` and `rng` are those of laser_amd.Sampler (sampling.py).  Calls are asynchronous on
the current torch stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from .foreach import _View
from .sampling import _count, _uniforms
from .tensor import _stream, newTensor

_SFX = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64", np.dtype(np.int32): "i32", np.dtype(np.int64): "i64"}


def _rows(name, obj, dtypes=None):
    """view of an operand of rank 2 (rank 1: one row) whose rows are contiguous: (view, rows, n, row stride)"""
    v = _View(name, obj)
    if v.dtype not in (dtypes or _SFX):
        raise TypeError(f"{name}: element type {v.dtype} ({', '.join(str(d) for d in (dtypes or _SFX))} only)")
    if v.rank not in (1, 2):
        raise ValueError(f"{name}: rank {v.rank} (a matrix, or a vector for one row, is needed)")
    shape, strides = ((1,) + v.shape, (0,) + v.strides) if v.rank == 1 else (v.shape, v.strides)
    rows, n = shape
    if n != 1 and strides[1] != 1:
        raise ValueError(f"{name}: last stride {strides[1]} (the elements of a row must be contiguous)")
    rs = strides[0] if rows > 1 else n     # a single row has no row stride to speak of
    if rows > 1 and rs < n:
        raise ValueError(f"{name}: row stride {rs} below the row length {n}")
    return v, rows, n, rs


def _f32(name, obj):
    return _rows(name, obj, (np.dtype(np.float32),))


def cumsum(t):
    """inclusive prefix sum along the last axis, in the order of scan_core.h (the integer types wrap)"""
    v, rows, n, rs = _rows("t", t)
    out = newTensor(v.dtype, *v.shape)
    if rows and n:
        entry = getattr(_lib.lib(), f"laser_hip_cumsum_{_SFX[v.dtype]}_dev")
        _lib.check(entry(C.c_void_p(out.unsafe_raw_data()), n, C.c_void_p(v.ptr), rs, rows, n, _stream()))
    return out


def searchsorted(a, v, leftSide=True):
    """searchsorted(input, values, leftSide) of bench_multinomial_samplers.nim:55-61, 162-170: for every value of row i of `v`
    (shape (rows,): one value per row, or (rows, m)) the index in row i of `a` before which it would be inserted, the first
    such place (leftSide, lowerBound) or the last (upperBound)"""
    av, rows, n, rs = _rows("a", a)
    vv = _View("v", v)
    if vv.dtype != av.dtype:
        raise TypeError(f"v: element type {vv.dtype}, a has {av.dtype}")
    if vv.rank not in (1, 2) or vv.shape[0] != rows:
        raise ValueError(f"v: shape {vv.shape}, ({rows},) or ({rows}, m) is needed")
    m = 1 if vv.rank == 1 else vv.shape[1]
    want = (1,) if vv.rank == 1 else (m, 1)
    if any(e > 1 and s != w for e, s, w in zip(vv.shape, vv.strides, want)):
        raise ValueError("v: a row-major array is needed")
    if n < 1:
        raise ValueError("searchsorted: empty rows")
    out = newTensor(np.int32, *vv.shape)
    if rows and m:
        entry = getattr(_lib.lib(), f"laser_hip_searchsorted_{_SFX[av.dtype]}_dev")
        _lib.check(entry(C.c_void_p(out.unsafe_raw_data()), C.c_void_p(av.ptr), rs, C.c_void_p(vv.ptr), rows, n, m,
                         0 if leftSide else 1, _stream()))
    return out


def _source(which, u, rows, num, rng):
    """(entry point, the arguments that name the uniform numbers, what keeps them alive)"""
    if rng is None:
        u = _uniforms(u, rows, num)
        return getattr(_lib.lib(), f"laser_hip_{which}_f32_dev"), (C.c_void_p(_View("u", u).ptr),), u
    from .random import Rng
    if u is not None:
        raise ValueError("give the uniform numbers `u` or the generator `rng`, not both")
    if not isinstance(rng, Rng):
        raise TypeError(f"rng: {type(rng).__name__} (a laser_amd.Rng is needed)")
    return getattr(_lib.lib(), f"laser_hip_{which}_rng_f32_dev"), (rng.seed, rng.subseq, rng.offset), None


def cdfSample(cdf, u=None, num=1, rng=None):
    """num independent draws per row of `cdf` (rows of cumulative weights, e.g. cumsum(probs)): the index of the first element
    above u * total; -1 on a row whose total is not positive and finite"""
    v, rows, n, rs = _f32("cdf", cdf)
    num = _count(num)
    if n < 1:
        raise ValueError("cdfSample: empty rows")
    entry, source, keep = _source("cdf_sample", u, rows, num, rng)
    out = newTensor(np.int32, rows, num)
    _lib.check(entry(C.c_void_p(out.unsafe_raw_data()), C.c_void_p(v.ptr), rs, *source, rows, n, num, _stream()))
    if rng is not None:
        rng.advance(rows * num)
    return out


def cdfSampleAndRemove(weights, u=None, num=1, rng=None):
    """num draws per row without replacement (bench_multinomial_samplers.nim:190-214): after every draw the drawn weight is
    set to 0 and the CDF is formed again.  Works on a private copy of `weights`; -1 once a row has nothing left."""
    v, rows, n, rs = _f32("weights", weights)
    num = _count(num)
    if n < 1:
        raise ValueError("cdfSampleAndRemove: empty rows")
    entry, source, keep = _source("cdf_sample_remove", u, rows, num, rng)
    L = _lib.lib()
    w, cdf = newTensor(np.float32, rows, n), newTensor(np.float32, rows, n)
    if rows:
        i64x2 = C.c_int64 * 2
        _lib.check(L.laser_hip_copy_strided_b32_dev(C.c_void_p(w.unsafe_raw_data()), i64x2(n, 1), C.c_void_p(v.ptr), i64x2(rs, 1),
                                                    i64x2(rows, n), 2, _stream()))
    out = newTensor(np.int32, rows, num)
    _lib.check(entry(C.c_void_p(out.unsafe_raw_data()), C.c_void_p(w.unsafe_raw_data()), n, C.c_void_p(cdf.unsafe_raw_data()), n,
                     *source, rows, n, num, _stream()))
    if rng is not None:
        rng.advance(rows * num)
    return out
