"""numpy model of the normal random fill (include/laser_hip.h "Random numbers"; laser_amd/csrc/normal_core.h): Box-Muller on
pairs of words of a Philox stream, written from the header's words.  The words are philox_model's, the logarithm is
log_model's llog, the sine and cosine kernels and float64(pi/2) are sincos_model's; every float operation is a numpy
operation rounded on its own in its type."""
import numpy as np

from tests import log_model, philox_model, sincos_model

M64 = (1 << 64) - 1
Z_MAX = 5.77                                            # sqrt(2 * 24 * ln 2) = 5.7684...


def radius(w0):
    """r of a pair from its first word: float32"""
    w0 = np.asarray(w0, np.uint32)
    u = ((w0 >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)      # in (0, 1], both steps exact
    t = np.float32(-2.0) * log_model.llog(u)                                                    # exact
    return np.sqrt(np.abs(t)).astype(np.float32)                                                # correctly rounded


def angle(w1):
    """(quadrant, reduced float64 argument) of a pair's angle 2 pi k / 2^24, k = w1 >> 8, reduced on the integer"""
    k = (np.asarray(w1, np.uint32) >> np.uint32(8)).astype(np.int64)
    j = (k + (1 << 21)) >> 22
    f = k - (j << 22)                                                                           # in [-2^21, 2^21)
    frac = f.astype(np.float64) * np.float64(2.0 ** -22)                                        # exact
    return j & 3, frac * sincos_model.K["PIO2"]


def z_pair(w0, w1):
    """(cosine branch, sine branch) of the pairs: float32 each"""
    q, a = angle(w1)
    r = radius(w0)
    tc = sincos_model.pick(q, a, 1).astype(np.float32)
    ts = sincos_model.pick(q, a, 0).astype(np.float32)
    return (r * tc).astype(np.float32), (r * ts).astype(np.float32)


def scale(z, mean, std):
    mean, std = np.float32(mean), np.float32(std)
    t = (std * np.asarray(z, np.float32)).astype(np.float32)
    return (mean + t).astype(np.float32)


def z_fill(n, seed, subseq, offset):
    """z of the stream positions offset .. offset + n - 1 (mod 2^64): even positions are cosine branches, odd ones sine"""
    offset = int(offset) & M64
    if n == 0:
        return np.zeros(0, np.float32)
    head = offset & 1
    first = (offset - head) & M64                       # the first pair's first word
    count = (head + n + 1) // 2 * 2
    w = philox_model.words(seed, subseq, first, count)
    zc, zs = z_pair(w[0::2], w[1::2])
    z = np.empty(count, np.float32)
    z[0::2], z[1::2] = zc, zs
    return z[head:head + n].copy()


def fill(n, mean, std, seed, subseq, offset):
    """the array laser_hip_random_normal_f32_dev(n, mean, std, seed, subseq, offset) gives"""
    return scale(z_fill(n, seed, subseq, offset), mean, std)


def params_ok(mean, std):
    mean, std = np.float32(mean), np.float32(std)
    return bool(np.isfinite(mean) and np.isfinite(std) and std >= 0)


same_bits = philox_model.same_bits
