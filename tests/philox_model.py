"""numpy model of the library's random numbers (include/laser_hip.h "Random numbers"; laser_amd/csrc/philox_core.h):
Philox4x32-10, the stream layout and the uniform distributions, in uint64 arithmetic with every float step rounded on its own
in the element type.  Written from the header's words, not from the C code."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
M64 = (1 << 64) - 1


def philox4x32_10(counter, key):
    """counter: (..., 4) words, key: (2,) words -> (..., 4) uint32"""
    c = [np.asarray(counter, np.uint64)[..., i] & MASK32 for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, -1).astype(np.uint32)


def words(seed, subseq, offset, n):
    """words offset .. offset + n - 1 (mod 2^64) of the stream (seed, subseq): uint32 (n,)"""
    seed, subseq, offset = int(seed) & M64, int(subseq) & M64, int(offset) & M64
    if n == 0:
        return np.zeros(0, np.uint32)
    first, last = offset >> 2, ((offset + n - 1) & M64) >> 2
    if first <= last:
        blocks = np.arange(first, last + 1, dtype=np.uint64)
    else:                                                  # the word index wraps: block 2^62 - 1 is followed by block 0
        blocks = np.concatenate([np.arange(first, 1 << 62, dtype=np.uint64), np.arange(0, last + 1, dtype=np.uint64)])
    ctr = np.stack([blocks & MASK32, blocks >> S32, np.full_like(blocks, subseq & 0xFFFFFFFF), np.full_like(blocks, subseq >> 32)], -1)
    out = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)
    head = offset & 3
    return out[head:head + n].copy()


def words64(seed, subseq, offset, n):
    """x = w0 | w1 << 32 of the pairs (offset + 2 i, offset + 2 i + 1): uint64 (n,)"""
    w = words(seed, subseq, offset, 2 * n).astype(np.uint64)
    return w[0::2] | (w[1::2] << S32)


def u01_f32(x):
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def u01_f64(x):
    return (np.asarray(x, np.uint64) >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)


def _uniform(u, lo, hi, ft):
    lo, hi = ft(lo), ft(hi)
    d = ft(hi - lo)
    t = (u * d).astype(ft)
    v = (lo + t).astype(ft)
    return np.minimum(v, hi).astype(ft)


def uniform_f32(x, lo, hi):
    return _uniform(u01_f32(x), lo, hi, np.float32)


def uniform_f64(x, lo, hi):
    return _uniform(u01_f64(x), lo, hi, np.float64)


def uniform_i32(x, lo, hi):
    span = int(hi) - int(lo) + 1                            # 1 .. 2^32
    r = (np.asarray(x, np.uint64) * np.uint64(span)) >> S32   # < 2^32 * 2^32: no overflow
    return ((r + np.uint64(int(lo) & 0xFFFFFFFF)) & MASK32).astype(np.uint32).view(np.int32)


def mulhi64(a, b):
    a = np.asarray(a, np.uint64)
    b = np.uint64(b)
    al, ah, bl, bh = a & MASK32, a >> S32, b & MASK32, b >> S32
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> S32) + (lh & MASK32) + (hl & MASK32)
    return hh + (lh >> S32) + (hl >> S32) + (mid >> S32)


def uniform_i64(x, lo, hi):
    x = np.asarray(x, np.uint64)
    span = (int(hi) - int(lo) + 1) & M64
    if span == 0:
        return x.view(np.int64)
    with np.errstate(over="ignore"):
        return (mulhi64(x, span) + np.uint64(int(lo) & M64)).view(np.int64)


# the five outputs of the C-ABI by name: fill(kind, n, lo, hi, seed, subseq, offset) -> the array a fill of n elements gives
KINDS = {"bits_u32": np.uint32, "uniform_f32": np.float32, "uniform_f64": np.float64, "uniform_i32": np.int32, "uniform_i64": np.int64}


def fill(kind, n, lo, hi, seed, subseq, offset):
    if kind == "bits_u32":
        return words(seed, subseq, offset, n)
    if kind == "uniform_f32":
        return uniform_f32(words(seed, subseq, offset, n), lo, hi)
    if kind == "uniform_i32":
        return uniform_i32(words(seed, subseq, offset, n), lo, hi)
    if kind == "uniform_f64":
        return uniform_f64(words64(seed, subseq, offset, n), lo, hi)
    if kind == "uniform_i64":
        return uniform_i64(words64(seed, subseq, offset, n), lo, hi)
    raise KeyError(kind)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
