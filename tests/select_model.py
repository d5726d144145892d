"""The numpy model of row selection (include/laser_hip_select.h "Row top-k, argmax and top-k sampling"): integer comparisons
of bit patterns only, so a result is compared by exact equality, values as uint32 bits.

    key(x) = bits ^ 0xFFFFFFFF when the sign bit is set, bits ^ 0x80000000 otherwise
    largest: descending key, identical bits by ascending column; smallest: ascending key, the same tie rule

and the fixtures the CPU and GPU suites share.
"""
import numpy as np

MAX_K = 1024


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def key(x):
    b = bits(x)
    return np.where(b >> 31 != 0, b ^ np.uint32(0xFFFFFFFF), b ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    """the float32 whose key is k"""
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32).view(np.float32)


def topk(x, k, largest=True, ties_by_highest_index=False):
    """(values, indices) of the k first elements of every row of the 2-D float32 x: float32 (bit copies) and int32, (rows, k).
    ties_by_highest_index: the deliberately WRONG tie rule, to show that a fixture discriminates."""
    x = np.ascontiguousarray(x, np.float32)
    rows, n = x.shape
    assert 1 <= k <= n
    kk = key(x)
    if largest:
        kk = ~kk
    col = np.arange(n, dtype=np.int64)
    idx = np.empty((rows, k), np.int32)
    for r in range(rows):
        idx[r] = np.lexsort((-col if ties_by_highest_index else col, kk[r]))[:k]
    return np.take_along_axis(x, idx.astype(np.int64), axis=1), idx


def argmax(x, largest=True):
    return topk(x, 1, largest)[1][:, 0]


def take_rows(src, j):
    src, j = np.asarray(src, np.int32), np.asarray(j, np.int32)
    ok = (j >= 0) & (j < src.shape[1])
    return np.where(ok, np.take_along_axis(src, np.where(ok, j, 0).astype(np.int64), axis=1), -1).astype(np.int32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
def f32(words):
    return np.array(words, np.uint32).view(np.float32)


# +-0, +-Inf, subnormals and NaNs of both signs with assorted payloads, in the order of ascending key
SPECIALS = f32([0xFFFFFFFF, 0xFFC00001, 0xFF800001, 0xFF800000, 0xFF7FFFFF, 0xBF800000, 0x80800000, 0x807FFFFF, 0x80000001, 0x80000000,
                0x00000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000, 0x7F800001, 0x7FC00000, 0x7FFFFFFF])
POS_NAN = f32([0x7FC00000])[0]


def data(kind, rows, n, seed=0):
    """a (rows, n) float32 matrix of one data class"""
    rng = np.random.default_rng([seed, rows, n, sum(kind.encode())])
    if kind == "normal":
        return rng.normal(0, 1, (rows, n)).astype(np.float32)
    if kind == "three":                                       # three distinct values: ties everywhere
        return rng.choice(np.float32([-1.5, 0.25, 3.0]), (rows, n)).astype(np.float32)
    if kind == "one":                                         # one value: pure tie picking
        return np.full((rows, n), np.float32(2.5))
    if kind == "low_byte":                                    # keys that differ only in their lowest byte
        return (np.uint32(0x3F800000) + rng.integers(0, 256, (rows, n)).astype(np.uint32)).view(np.float32)
    if kind == "high_byte":                                   # keys that differ only in their highest byte (NaN and Inf included)
        return unkey((rng.integers(0, 256, (rows, n)).astype(np.uint32) << 24) | np.uint32(0x00345678))
    if kind == "ascending":
        return np.sort(rng.normal(0, 1, (rows, n)).astype(np.float32), axis=1)
    if kind == "descending":
        return np.sort(rng.normal(0, 1, (rows, n)).astype(np.float32), axis=1)[:, ::-1].copy()
    if kind == "special":
        return rng.choice(SPECIALS, (rows, n)).astype(np.float32)
    raise ValueError(kind)


KINDS = ("normal", "three", "one", "low_byte", "high_byte", "ascending", "descending", "special")


def straddle(n, k, at, seed=0):
    """one row of n: k - 5 elements above a tie group of 9 equal elements whose columns lie on both sides of `at` (a multiple
    of a chunk size), the rest below: the group straddles the k-th rank (5 of the 9 are taken: 3 before `at`, 2 from it on)
    and the chunk boundary"""
    assert k >= 6 and n >= at + 8 and at >= 8 and n >= k + 9
    rng = np.random.default_rng([seed, n, k, at])
    x = rng.uniform(-2.0, -1.0, n).astype(np.float32)
    tie = np.array([at - 5, at - 2, at - 1, at, at + 1, at + 3, at + 4, at + 6, at + 7])
    free = np.setdiff1d(np.arange(n), tie)
    x[rng.choice(free, k - 5, replace=False)] = rng.uniform(2.0, 3.0, k - 5).astype(np.float32)
    x[tie] = np.float32(1.0)
    return x[None, :]
