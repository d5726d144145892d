"""Weighted random sampling on the device: the reference's F+tree `Sampler` (benchmarks/random_sampling/fenwicktree.nim;
include/laser_hip.h "F+tree weighted sampler") over the rows of a float32 matrix.

    s = laser_amd.newSampler(weights)          one tree per row of the 2-D `weights` (1-D: one row)
    s.sample(u=None, num=1, rng=None)          num independent draws per row, with replacement  -> int32 Tensor (rows, num)
    s.sampleAndRemove(u=None, num=1, rng=None) num draws per row without replacement (mutates the trees; -1 once a row is empty)
    s.update(elem, weight)                     one (elem, weight) per row; elem = -1 leaves that row alone
    laser_amd.multinomial(probs, num_samples=1, replacement=False, u=None, rng=None, method="ftree")   build and draw in one call
    laser_amd.sample_top_k(logits, k, num_samples=1, u=None, rng=None)     draws among the k largest logits of every row

`weights` is a laser_amd.Tensor or a torch CUDA tensor whose rows are contiguous; the weights need not sum to 1.  The uniform
numbers come from one of three places.  `u` is a float32 array of shape (rows, num) with values in [0, 1) -- a device tensor,
or a host numpy array, which is checked and uploaded -- and every result is a function of the weights and `u` alone, bit for
bit.  `rng` is a laser_amd.Rng (laser_amd/random.py), the library's counter-based generator: the kernel makes
u[row, j] = the float32 u01 of word rng.offset + row * num + j itself, the result is a function of the weights and
(seed, subseq, offset), and the rng advances by rows * num.  Giving both raises ValueError.  With neither, the numbers are
drawn with torch.rand on the device: the one place where a result depends on state outside the call.  Calls are asynchronous
on the current torch stream.  Not built: float64, weights along another axis, alias tables.
"""
import ctypes as C

import numpy as np

from . import _lib
from .foreach import _View
from .tensor import Tensor, _stream, newTensor, toTensor


def _f32_rows(name, obj):
    """view of a float32 operand of rank 2 (rank 1: one row) whose rows are contiguous: (view, rows, n, row stride)"""
    v = _View(name, obj)
    if v.dtype != np.float32:
        raise TypeError(f"{name}: element type {v.dtype} (float32 only)")
    if v.rank not in (1, 2):
        raise ValueError(f"{name}: rank {v.rank} (a matrix, or a vector for one row, is needed)")
    shape, strides = ((1,) + v.shape, (0,) + v.strides) if v.rank == 1 else (v.shape, v.strides)
    rows, n = shape
    if n != 1 and strides[1] != 1:
        raise ValueError(f"{name}: last stride {strides[1]} (the elements of a row must be contiguous)")
    rs = strides[0] if rows > 1 else n     # a single row has no row stride to speak of
    return v, rows, n, rs


def tree_elems(n):
    """elements of one row's tree image: twice the next power of two >= n"""
    out = C.c_int64()
    _lib.check(_lib.lib().laser_hip_sampler_tree_elems(int(n), C.byref(out)))
    return out.value


def _count(num):
    if isinstance(num, bool) or not isinstance(num, (int, np.integer)) or num < 0:
        raise ValueError(f"num = {num!r} (a count >= 0 is needed)")
    return int(num)


def _uniforms(u, rows, num):
    """the (rows, num) float32 uniform numbers as a device operand; None: torch.rand on the device"""
    _count(num)
    if u is None:
        import torch
        return torch.rand((rows, int(num)), dtype=torch.float32, device="cuda")
    if isinstance(u, np.ndarray):
        if u.dtype != np.float32:
            raise TypeError(f"u: element type {u.dtype} (float32 only)")
        if u.shape != (rows, num):
            raise ValueError(f"u: shape {u.shape}, {(rows, num)} is needed")
        if not bool(np.all((u >= 0) & (u < 1))):
            raise ValueError("u: values outside [0, 1)")
        return toTensor(u, np.float32)
    v = _View("u", u)
    if v.dtype != np.float32:
        raise TypeError(f"u: element type {v.dtype} (float32 only)")
    if v.shape != (rows, num):
        raise ValueError(f"u: shape {v.shape}, {(rows, num)} is needed")
    if not (isinstance(u, Tensor) and u.is_C_contiguous()) and not (hasattr(u, "is_contiguous") and u.is_contiguous()):
        raise ValueError("u: a row-major device array is needed")
    if v.shape[0] * v.shape[1]:
        import torch
        t = u if isinstance(u, torch.Tensor) else torch.as_tensor(u, device="cuda")
        if not bool(((t >= 0) & (t < 1)).all()):
            raise ValueError("u: values outside [0, 1)")
    return u


class Sampler:
    """F+tree images of `rows` rows of `n` weights: `.tree` is the (rows, 2 P) float32 Tensor of include/laser_hip.h."""

    def __init__(self, tree, rows, n):
        self.tree, self.rows, self.n = tree, int(rows), int(n)

    def _draw(self, which, u, num, rng):
        """laser_hip_sampler_<which>_f32_dev on `u`, or its _rng form on the stream of `rng`, which then advances"""
        num = _count(num)
        if rng is None:
            u = _uniforms(u, self.rows, num)
            entry, source = getattr(_lib.lib(), f"laser_hip_sampler_{which}_f32_dev"), (C.c_void_p(_View("u", u).ptr),)
        else:
            from .random import Rng
            if u is not None:
                raise ValueError("give the uniform numbers `u` or the generator `rng`, not both")
            if not isinstance(rng, Rng):
                raise TypeError(f"rng: {type(rng).__name__} (a laser_amd.Rng is needed)")
            entry, source = getattr(_lib.lib(), f"laser_hip_sampler_{which}_rng_f32_dev"), (rng.seed, rng.subseq, rng.offset)
        out = newTensor(np.int32, self.rows, num)
        _lib.check(entry(C.c_void_p(out.unsafe_raw_data()), C.c_void_p(self.tree.unsafe_raw_data()), self.tree.shape[1], *source,
                         self.rows, self.n, num, _stream()))
        if rng is not None:
            rng.advance(self.rows * num)
        return out

    def sample(self, u=None, num=1, rng=None):
        """num independent draws per row with replacement; the trees are only read"""
        return self._draw("sample", u, num, rng)

    def sampleAndRemove(self, u=None, num=1, rng=None):
        """num draws per row, each drawn element's weight set to 0 before the next draw; -1 once nothing is left"""
        return self._draw("sample_remove", u, num, rng)

    def update(self, elem, weight):
        """per row: the weight of element elem[row] becomes weight[row] (elem -1: nothing).  Host sequences are checked
        (anything else outside [0, n) raises) and uploaded; device operands are taken as they are, and the kernel skips what
        lies outside the row."""
        if not hasattr(elem, "__cuda_array_interface__"):
            e = np.asarray(elem)
            if e.dtype.kind not in "iu" or e.shape != (self.rows,):
                raise ValueError(f"elem: {self.rows} integers are needed")
            if bool(np.any((e < -1) | (e >= self.n))):
                raise ValueError(f"elem: an index outside [0, {self.n}) that is not -1")
            elem = toTensor(e.astype(np.int32), np.int32)
        if not hasattr(weight, "__cuda_array_interface__"):
            w = np.asarray(weight, np.float32)
            if w.shape != (self.rows,):
                raise ValueError(f"weight: {self.rows} numbers are needed")
            weight = toTensor(w, np.float32)
        ev, wv = _View("elem", elem), _View("weight", weight)
        if ev.dtype != np.int32 or wv.dtype != np.float32:
            raise TypeError(f"elem / weight: element types {ev.dtype} / {wv.dtype} (int32 / float32 are needed)")
        for name, v in (("elem", ev), ("weight", wv)):
            if v.shape != (self.rows,) or (self.rows > 1 and v.strides[0] != 1):
                raise ValueError(f"{name}: a contiguous vector of {self.rows} elements is needed")
        _lib.check(_lib.lib().laser_hip_sampler_update_f32_dev(C.c_void_p(self.tree.unsafe_raw_data()), self.tree.shape[1],
                                                               C.c_void_p(ev.ptr), C.c_void_p(wv.ptr), self.rows, self.n, _stream()))
        return self


def newSampler(weights):
    """newSampler(weights) of fenwicktree.nim:67 for every row of `weights`"""
    v, rows, n, rs = _f32_rows("weights", weights)
    if n < 1:
        raise ValueError("newSampler: empty rows")
    tree = newTensor(np.float32, rows, tree_elems(n))
    _lib.check(_lib.lib().laser_hip_sampler_build_f32_dev(C.c_void_p(tree.unsafe_raw_data()), tree.shape[1], C.c_void_p(v.ptr), rs,
                                                          rows, n, _stream()))
    return Sampler(tree, rows, n)


def multinomial(probs, num_samples=1, replacement=False, u=None, rng=None, method="ftree"):
    """num_samples indices per row of `probs`, drawn in proportion to the weights: int32 Tensor (rows, num_samples).  Without
    replacement an element is drawn at most once, and a row with fewer positive weights than num_samples ends in -1.
    method: "ftree" builds the F+tree and draws from it; "cdf" is the reference's other sampler (laser_amd/scan.py): one
    cumsum and one search per draw with replacement, a fresh cumsum per draw without."""
    if u is not None and rng is not None:
        raise ValueError("give the uniform numbers `u` or the generator `rng`, not both")
    if method == "cdf":
        from . import scan
        if replacement:
            _f32_rows("probs", probs)
            return scan.cdfSample(scan.cumsum(probs), u, num_samples, rng)
        return scan.cdfSampleAndRemove(probs, u, num_samples, rng)
    if method != "ftree":
        raise ValueError(f"method = {method!r} (\"ftree\" or \"cdf\")")
    s = newSampler(probs)
    return s.sample(u, num_samples, rng) if replacement else s.sampleAndRemove(u, num_samples, rng)


def sample_top_k(logits, k, num_samples=1, u=None, rng=None):
    """num_samples column indices per row of the 2-D float32 `logits`, drawn among the row's k largest in proportion to their
    softmax: int32 Tensor (rows, num_samples).  A composition of calls with defined bits -- topk (laser_amd/select.py), softmax
    of the k values, cumsum, the inverse-CDF draw cdfSample (laser_amd/scan.py) with `u` or `rng` as Sampler.sample takes
    them, then take_rows on topk's indices -- so the ids are a function of the logits and the uniform numbers alone.  k = 1
    is argmax.  A row whose k largest hold a NaN or +Inf has a NaN softmax and draws -1."""
    from . import scan, select
    from .simd_math import softmax
    if u is not None and rng is not None:
        raise ValueError("give the uniform numbers `u` or the generator `rng`, not both")
    v = _View("logits", logits)
    if v.rank != 2:
        raise ValueError(f"sample_top_k: logits has rank {v.rank} (a matrix is needed)")
    vals, idx = select.topk(logits, k)
    pos = scan.cdfSample(scan.cumsum(softmax(vals)), u, num_samples, rng)
    return select.take_rows(idx, pos)
