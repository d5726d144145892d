"""Random numbers on the device: the library's counter-based generator, Philox4x32-10, and the reference's `randomTensor`
(include/laser_hip.h "Random numbers"; laser_amd/csrc/philox_core.h is the definition, tests/philox_model.py the numpy model).

    rng = laser_amd.Rng(seed, subseq=0)            names the stream (seed, subseq); holds (seed, subseq, offset) on the host
    rng.bits(n)                                    n raw 32-bit words -> int32 Tensor (n,) holding the bits (.view(np.uint32))
    rng.randomTensor(shape, valrange_or_max, dtype=np.float32)
                                                   randomTensor(shape, valrange) / randomTensor(shape, max) of the reference:
                                                   uniform on the closed interval (lo, hi), a bare max means (0, max);
                                                   dtype float32, float64, int32 or int64
    laser_amd.randomTensor(shape, valrange_or_max, dtype, *, seed, subseq=0, offset=0)      the same as a pure function
    rng.randomNormalTensor(shape, mean=0.0, std=1.0)
                                                   float32 normal draws: Box-Muller on pairs of words of the same stream
                                                   (laser_amd/csrc/normal_core.h; tests/normal_model.py is the numpy model),
                                                   one word per element: the offset advances by the element count
    laser_amd.randomNormalTensor(shape, mean, std, *, seed, subseq=0, offset=0)             the same as a pure function

Word w of a stream is a function of (seed, subseq, w) alone: no state lives on the device, every draw advances the host-side
offset by the words it used (one per 32-bit element, two per 64-bit element), so two successive draws are one draw of the
joint length cut in two, bit for bit, on any stream and any alignment.  Calls are asynchronous on the current torch stream.
Sampler.sample / sampleAndRemove / multinomial take such an `rng` (laser_amd/sampling.py).
"""
import ctypes as C

import numpy as np

from . import _lib
from .tensor import _stream, newTensor

_M64 = (1 << 64) - 1
_SFX = {"float32": "f32", "float64": "f64", "int32": "i32", "int64": "i64"}


def _u64(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{name} = {v!r} (an integer is needed)")
    v = int(v)
    if not -(1 << 63) <= v <= _M64:
        raise ValueError(f"{name} = {v} does not fit 64 bits")
    return v & _M64


def _shape(shape):
    if isinstance(shape, (int, np.integer)) and not isinstance(shape, bool):
        shape = (shape,)
    shape = tuple(int(s) for s in shape)
    if any(s < 0 for s in shape):
        raise ValueError("negative extent")
    return shape


def _range(valrange_or_max, dt):
    """(lo, hi) in the element type; a bare max means (0, max)"""
    if isinstance(valrange_or_max, slice):
        lo, hi = valrange_or_max.start, valrange_or_max.stop
    elif isinstance(valrange_or_max, (tuple, list)):
        lo, hi = valrange_or_max
    else:
        lo, hi = 0, valrange_or_max
    if dt.kind == "i":
        info = np.iinfo(dt)
        for v in (lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not info.min <= int(v) <= info.max:
                raise ValueError(f"randomTensor: bound {v!r} is not an {dt.name}")
        lo, hi = int(lo), int(hi)
    else:
        lo, hi = dt.type(lo), dt.type(hi)
        with np.errstate(over="ignore", invalid="ignore"):
            if not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(hi - lo)):
                raise ValueError(f"randomTensor: bounds {lo}, {hi}: lo, hi and hi - lo must be finite in {dt.name}")
        lo, hi = float(lo), float(hi)
    if not lo <= hi:
        raise ValueError(f"randomTensor: empty range {lo} .. {hi}")
    return lo, hi


class Rng:
    """The stream (seed, subseq) of Philox4x32-10 and the next unused word, `offset`; all three live on the host."""

    def __init__(self, seed, subseq=0, offset=0):
        self.seed, self.subseq, self.offset = _u64("seed", seed), _u64("subseq", subseq), _u64("offset", offset)

    def advance(self, words):
        """skip `words` words: the offset a draw of that many words would leave; returns the offset before"""
        before = self.offset
        self.offset = (self.offset + int(words)) & _M64
        return before

    def bits(self, n):
        """the next n words of the stream: an int32 Tensor (n,) whose bit patterns are the uint32 words"""
        (n,) = _shape(n)
        out = newTensor(np.int32, n)
        _lib.check(_lib.lib().laser_hip_random_bits_u32_dev(C.c_void_p(out.unsafe_raw_data()), n, self.seed, self.subseq, self.offset,
                                                            _stream()))
        self.advance(n)
        return out

    def randomTensor(self, shape, valrange_or_max, dtype=np.float32):
        """uniform on the closed interval: a row-major Tensor of `shape`, element k of the flat order from word offset + k
        (float32, int32) or the pair of words offset + 2 k, offset + 2 k + 1 (float64, int64)"""
        dt = np.dtype(dtype)
        if dt.name not in _SFX:
            raise TypeError(f"randomTensor: element type {dt} ({', '.join(_SFX)})")
        shape = _shape(shape)
        lo, hi = _range(valrange_or_max, dt)
        out = newTensor(dt, *shape)
        entry = getattr(_lib.lib(), f"laser_hip_random_uniform_{_SFX[dt.name]}_dev")
        _lib.check(entry(C.c_void_p(out.unsafe_raw_data()), out.size, lo, hi, self.seed, self.subseq, self.offset, _stream()))
        self.advance(out.size * (dt.itemsize // 4))
        return out

    def randomNormalTensor(self, shape, mean=0.0, std=1.0):
        """normal with the given mean and standard deviation: a row-major float32 Tensor of `shape`, element k of the flat order
        from stream position offset + k (even positions are the cosine branch of their Box-Muller pair, odd ones the sine
        branch); the offset advances by the element count, so a following draw of any kind continues the stream"""
        shape = _shape(shape)
        mean, std = np.float32(mean), np.float32(std)
        if not (np.isfinite(mean) and np.isfinite(std) and std >= 0):
            raise ValueError(f"randomNormalTensor: mean {mean}, std {std}: mean must be finite, std finite and >= 0 in float32")
        out = newTensor(np.float32, *shape)
        _lib.check(_lib.lib().laser_hip_random_normal_f32_dev(C.c_void_p(out.unsafe_raw_data()), out.size, float(mean), float(std),
                                                              self.seed, self.subseq, self.offset, _stream()))
        self.advance(out.size)
        return out

    def __repr__(self):
        return f"Rng(seed={self.seed:#x}, subseq={self.subseq:#x}, offset={self.offset})"


def randomTensor(shape, valrange_or_max, dtype=np.float32, *, seed, subseq=0, offset=0):
    """randomTensor as a pure function of its arguments: Rng(seed, subseq, offset).randomTensor(shape, valrange_or_max, dtype)"""
    return Rng(seed, subseq, offset).randomTensor(shape, valrange_or_max, dtype)


def randomNormalTensor(shape, mean=0.0, std=1.0, *, seed, subseq=0, offset=0):
    """randomNormalTensor as a pure function of its arguments: Rng(seed, subseq, offset).randomNormalTensor(shape, mean, std)"""
    return Rng(seed, subseq, offset).randomNormalTensor(shape, mean, std)
