"""Batched GEMM operands in every layout the strided-batched entry point accepts, each operand inside a flat arena of its own
with guard elements around it.  Used by tests/test_batched_views_cpu.py (the geometry and the references, no device) and
tests/test_gpu_batched.py.

A view is (offset, (bs, rs, cs)) in elements: element [p][r][c] of the operand lies at offset + p * bs + r * rs + c * cs of its
arena.  A case is

    (layout, element type, batch, M, N, K, view of A, view of B, view of C, alpha, beta)

The placement rule.  A view's addressed elements span [offset + lo, offset + hi]; the arena reaches slack(view) = batch * |bs| +
one matrix span further on BOTH sides.  A kernel that takes a batch index, a batch stride's sign or an entry's base wrong by up
to a whole batch lands on a guard element of the same allocation: the A and B arenas hold seeded data everywhere, so a wrong read
gives a wrong number, and the C arena holds a sentinel (one NaN bit pattern for the float types, 7 for the integers) on every
element the view does not address, so a wrong write is seen.  Nothing the catalogue can provoke leaves the allocation.

The batched call is well defined when the addressed elements of C are pairwise distinct over the whole batch (entries of A and
B may overlap, be shared, or run backwards); tests/test_batched_views_cpu.py checks that on every case.

Layouts (all of them at every shape of the element type):
  dense             row-major, bs = the matrix size
  share_a / share_b / share_ab    bsA = 0 / bsB = 0 / both; C distinct per entry
  padded            leading dimensions + 3 / + 5 / + 7, odd batch strides (the padded matrix + a gap of 3 or 4), bases 1 / 3 / 5
                    elements past a 64-byte boundary of a 64-byte-aligned arena: no 16-byte vector load is legal
  transposed        A column-major (rsA = 1, csA = M + 1), B k-contiguous (rsB = 1, csB = K + 4), C column-major (rsC = 1, csC = M + 2)
  reversed_batches  bsA, bsB, bsC negative: entry 0 lies at the far end
  negative_inner    k reversed on A and on B, A's rows reversed, C with csC = -2 (the gaps hold sentinels)
  interleaved       batch stride 1, the inner strides multiplied by batch: A[p][i][k] at i * K * batch + k * batch + p
  sliding           overlapping reads: A[p] = rows p * s .. p * s + M of one tall matrix (s < M), B[p] = columns p * t .. p * t + N
                    of one wide matrix; C dense
  b_transposed      B alone k-contiguous (rsB = 1, csB = K + 4), A and C row-major: the one layout with a batch that the
                    hand-scheduled kernels' transposed-B variants take (`transposed` has a column-major A, which they decline)
"""
import collections
import zlib

import numpy as np

DTYPES = [np.float32, np.float64, np.int32, np.int64, np.int8, np.uint8, np.int16, np.uint16, np.uint32, np.uint64]
BASE = [np.float32, np.float64, np.int32, np.int64]           # the CPU oracle's element types
REQUIRED_LAYOUTS = ["dense", "share_a", "share_b", "share_ab", "padded", "transposed", "reversed_batches", "negative_inner",
                    "interleaved", "sliding"]
LAYOUTS = REQUIRED_LAYOUTS + ["b_transposed"]

# (batch, M, N, K): the smallest shapes at which each kernel family can still be wrong (kc = 512 for f32, 256 for f64)
SMALL_SHAPES = [(5, 7, 33, 50), (3, 64, 64, 128)]                                  # the small-matrix kernel (floats)
TILED_SHAPES = [(3, 130, 70, 517),         # ragged everywhere, K > kc
                (3, 200, 136, 260),        # K <= kc for f32, two slices for f64
                (2, 260, 136, 1028)]       # 4-aligned but ragged: the EDGE vector loaders
MATVEC_SHAPES = [(3, 300, 1, 600), (3, 4, 300, 600), (4, 1, 1, 1)]                 # one-column / one-row tiles of the tiled kernels
FLOAT_SHAPES = SMALL_SHAPES + TILED_SHAPES + MATVEC_SHAPES
INT_SHAPES = [(4, 65, 67, 33), (3, 130, 1, 257), (2, 200, 136, 516)]

FLOAT_SCALARS = [(1, 0), (1, 1), (0.5, 0.25)]
INT_SCALARS = [(1, 0), (1, 1), (2, 3), (-3, 1)]              # (-3, 1): wrap-around

INT_SENTINEL = 7
NAN_SENTINEL = {4: 0x7fc5a5a5, 8: 0x7ff85a5a5a5a5a5a}        # the one bit pattern of every non-addressed float element of a C arena

View = collections.namedtuple("View", "offset strides")       # strides = (bs, rs, cs), everything in elements
Case = collections.namedtuple("Case", "layout dtype batch M N K A B C alpha beta")


def shapes(dtype):
    return FLOAT_SHAPES if np.dtype(dtype).kind == "f" else INT_SHAPES


def scalars(dtype):
    return FLOAT_SCALARS if np.dtype(dtype).kind == "f" else INT_SCALARS


# ---- geometry -----------------------------------------------------------------------------------------------------------
def dims(c, which):
    """(rows, cols) of operand "A" / "B" / "C" of the case"""
    return {"A": (c.M, c.K), "B": (c.K, c.N), "C": (c.M, c.N)}[which]


def matrix_span(strides, rows, cols):
    """elements from the lowest to the highest address of ONE entry, inclusive"""
    return (rows - 1) * abs(strides[1]) + (cols - 1) * abs(strides[2]) + 1


def reach(strides, batch, rows, cols):
    """(lo, hi): the lowest and highest element offset the view addresses, relative to its base (lo <= 0 <= hi)"""
    ext = [(n - 1) * s for n, s in zip((batch, rows, cols), strides)]
    return sum(min(0, e) for e in ext), sum(max(0, e) for e in ext)


def slack(strides, batch, rows, cols):
    """guard elements on each side of the view: one whole batch span plus one matrix span"""
    return batch * abs(strides[0]) + matrix_span(strides, rows, cols)


def arena_len(v, batch, rows, cols):
    return v.offset + reach(v.strides, batch, rows, cols)[1] + 1 + slack(v.strides, batch, rows, cols)


def element_offsets(v, batch, rows, cols):
    """int64 [batch][rows][cols]: the arena index of every element of the view (a stride-0 axis repeats)"""
    bs, rs, cs = v.strides
    return (v.offset + np.arange(batch, dtype=np.int64)[:, None, None] * bs + np.arange(rows, dtype=np.int64)[None, :, None] * rs +
            np.arange(cols, dtype=np.int64)[None, None, :] * cs)


def _place(strides, batch, rows, cols, odd=0):
    """the view at the lowest offset that leaves the slack below it, its base on a 64-element boundary (+ `odd`)"""
    lo, _ = reach(strides, batch, rows, cols)
    first = slack(strides, batch, rows, cols) - lo
    return View(-(-first // 64) * 64 + odd, tuple(int(s) for s in strides))


def _layout(layout, batch, M, N, K):
    """strides of A, B, C and the odd base offsets (padded only)"""
    a, b, c = (M * K, K, 1), (K * N, N, 1), (M * N, N, 1)
    odd = (0, 0, 0)
    if layout == "dense":
        pass
    elif layout == "share_a":
        a = (0, K, 1)
    elif layout == "share_b":
        b = (0, N, 1)
    elif layout == "share_ab":
        a, b = (0, K, 1), (0, N, 1)
    elif layout == "padded":
        lda, ldb, ldc = K + 3, N + 5, N + 7
        a, b, c = ((M * lda + 3) | 1, lda, 1), ((K * ldb + 3) | 1, ldb, 1), ((M * ldc + 3) | 1, ldc, 1)
        odd = (1, 3, 5)
    elif layout == "transposed":
        a, b, c = (K * (M + 1), 1, M + 1), (N * (K + 4), 1, K + 4), (N * (M + 2), 1, M + 2)
    elif layout == "reversed_batches":
        a, b, c = (-M * K, K, 1), (-K * N, N, 1), (-M * N, N, 1)
    elif layout == "negative_inner":
        a, b, c = (M * K, -K, -1), (K * N, -N, 1), (M * 2 * N, 2 * N, -2)
    elif layout == "interleaved":
        a, b, c = (1, K * batch, batch), (1, N * batch, batch), (1, N * batch, batch)
    elif layout == "sliding":
        s, t = M // 2, max(1, N // 3)          # s < M; M = 1 slides by 0 (every entry the same row)
        ldb = (batch - 1) * t + N
        a, b = (s * K, K, 1), (t, ldb, 1)
    elif layout == "b_transposed":
        b = (N * (K + 4), 1, K + 4)
    else:
        raise ValueError(layout)
    return a, b, c, odd


def make_case(layout, dtype, shape, alpha, beta):
    batch, M, N, K = shape
    a, b, c, odd = _layout(layout, batch, M, N, K)
    return Case(layout, np.dtype(dtype), batch, M, N, K, _place(a, batch, M, K, odd[0]), _place(b, batch, K, N, odd[1]),
                _place(c, batch, M, N, odd[2]), alpha, beta)


def cases(dtype, shape_list=None, layouts=None, scalar_list=None):
    """the catalogue of one element type, grouped by (layout, shape) so that the alpha / beta variants share their arenas"""
    return [make_case(lay, dtype, sh, al, be)
            for lay in (layouts or LAYOUTS) for sh in (shape_list or shapes(dtype)) for al, be in (scalar_list or scalars(dtype))]


def all_cases():
    return [c for dt in DTYPES for c in cases(dt)]


def describe(c):
    return (f"{c.layout} {c.dtype} batch={c.batch} M={c.M} N={c.N} K={c.K} alpha={c.alpha} beta={c.beta} "
            f"A={tuple(c.A)} B={tuple(c.B)} C={tuple(c.C)}")


# ---- values -------------------------------------------------------------------------------------------------------------
def _draw(rng, n, dtype):
    if dtype.kind == "f":
        return rng.uniform(-0.5, 0.5, n).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)      # the full range: wrap-around arithmetic


def nan_patterns(n, dtype):
    """quiet and signalling NaNs of both signs with varying payloads, none of them the sentinel"""
    size = np.dtype(dtype).itemsize
    u = np.dtype(f"u{size}")
    heads = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001] if size == 4 else
                     [0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001], dtype=np.uint64)
    pay = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0x1ffffe)      # (even: the sentinels' payloads are odd)
    return (heads[np.arange(n) % 4] | pay).astype(u).view(dtype)


def sentinel(dtype, n):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return np.full(n, NAN_SENTINEL[dt.itemsize], dtype=f"u{dt.itemsize}").view(dt)
    return np.full(n, INT_SENTINEL, dtype=dt)


def bits(x):
    """floats as their bit patterns (NaN payloads compare), integers as they are"""
    return x.view(np.dtype(f"u{x.dtype.itemsize}")) if x.dtype.kind == "f" else x


_ARENAS = collections.OrderedDict()


def arenas(c, nan_c=False):
    """(A arena, B arena, C arena, addressed) of the case, read-only: A and B seeded data everywhere; C seeded C0 (or, with
    nan_c, NaN patterns) on the addressed elements and the sentinel elsewhere; addressed = bool mask over the C arena.  Depends on
    the layout, shape and element type only, not on alpha / beta.  The last few are kept."""
    key = (c.layout, c.dtype.name, c.batch, c.M, c.N, c.K, bool(nan_c))
    if key in _ARENAS:
        _ARENAS.move_to_end(key)
        return _ARENAS[key]
    rng = np.random.default_rng(zlib.crc32(repr(key[:-1]).encode()))
    a = _draw(rng, arena_len(c.A, c.batch, c.M, c.K), c.dtype)
    b = _draw(rng, arena_len(c.B, c.batch, c.K, c.N), c.dtype)
    n = arena_len(c.C, c.batch, c.M, c.N)
    off = element_offsets(c.C, c.batch, c.M, c.N).ravel()
    cbuf = sentinel(c.dtype, n)
    cbuf[off] = nan_patterns(off.size, c.dtype) if nan_c else _draw(rng, off.size, c.dtype)
    mask = np.zeros(n, dtype=bool)
    mask[off] = True
    for x in (a, b, cbuf, mask):
        x.setflags(write=False)
    _ARENAS[key] = (a, b, cbuf, mask)
    while len(_ARENAS) > 6:
        _ARENAS.popitem(last=False)
    return _ARENAS[key]


def as_view(arena, v, batch, rows, cols):
    """the numpy view [batch][rows][cols] of the arena (negative and zero strides as they are)"""
    size = arena.dtype.itemsize
    base = arena[v.offset:v.offset + 1]
    return np.lib.stride_tricks.as_strided(base, (batch, rows, cols), tuple(s * size for s in v.strides), writeable=False)


def operands(c, nan_c=False):
    """A [batch][M][K], B [batch][K][N], C0 [batch][M][N]: numpy views of the case's arenas"""
    a, b, cbuf, _ = arenas(c, nan_c)
    return as_view(a, c.A, c.batch, c.M, c.K), as_view(b, c.B, c.batch, c.K, c.N), as_view(cbuf, c.C, c.batch, c.M, c.N)


def gather(arena, v, batch, rows, cols):
    """a dense copy [batch][rows][cols] of the view's elements, by index"""
    return arena[element_offsets(v, batch, rows, cols)]


# ---- references ---------------------------------------------------------------------------------------------------------
def wrap_u64(x):
    """every element sign-extended to 64 bits, as uint64 (mod 2^n the extension does not matter)"""
    return x.astype(np.int64).view(np.uint64)


def wrap_reference(A, B, alpha, beta, C0):
    """alpha * A @ B + beta * C0 mod 2^n for any integer element type: wrapping 64-bit arithmetic (numpy's integer @ wraps),
    truncated to the element width.  beta = 0 does not read C0."""
    dt = A.dtype
    with np.errstate(over="ignore"):
        v = np.uint64(int(alpha) % 2 ** 64) * (wrap_u64(A) @ wrap_u64(B))
        if int(beta) != 0:
            v = v + np.uint64(int(beta) % 2 ** 64) * wrap_u64(C0)
    return v.astype(np.dtype(f"u{dt.itemsize}")).view(dt)


def reference(A, B, alpha, beta, C0):
    """one entry: the CPU oracle for float32 / float64 / int32 / int64 (on the views as they are: it takes any strides), the
    wrapping integer reference for the narrow and unsigned types.  beta = 0 never reads C0 (the oracle is handed zeros)."""
    dt = A.dtype
    if dt in [np.dtype(t) for t in BASE]:
        from oracle import oracle
        c0 = np.array(C0, order="C", copy=True) if beta != 0 else np.zeros(C0.shape, dtype=dt)
        return oracle.matmul(A, B, alpha, beta, c0, isa=oracle.fused_isa(dt))
    return wrap_reference(A, B, alpha, beta, C0)


_EXPECTED = {}


def expected(c):
    """[batch][M][N], read-only, computed once per (layout, shape, element type, alpha, beta) and shared by every route"""
    key = (c.layout, c.dtype.name, c.batch, c.M, c.N, c.K, c.alpha, c.beta)
    if key not in _EXPECTED:
        A, B, C0 = operands(c)
        want = np.stack([reference(A[p], B[p], c.alpha, c.beta, C0[p]) for p in range(c.batch)])
        want.setflags(write=False)
        _EXPECTED[key] = want
    return _EXPECTED[key]


# ---- the batch-count limit ----------------------------------------------------------------------------------------------
LIMIT_BATCH, LIMIT_SHAPE = 65535, (2, 3, 4)


def limit_operands(dtype, batch=LIMIT_BATCH, seed=9):
    """A [M][K] shared by the batch, B [batch][K][N], C0 [batch][M][N], integer values in [-8, 8] (every order of operations gives
    the same bits), and the expected alpha * A @ B[p] + beta * C0[p] for (alpha, beta) = (2, 1) by one einsum"""
    dt = np.dtype(dtype)
    M, N, K = LIMIT_SHAPE
    rng = np.random.default_rng(seed)
    A = rng.integers(-8, 8, (M, K), endpoint=True).astype(dt)
    B = rng.integers(-8, 8, (batch, K, N), endpoint=True).astype(dt)
    C0 = rng.integers(-8, 8, (batch, M, N), endpoint=True).astype(dt)
    wide = np.float64 if dt.kind == "f" else np.int64
    want = (2 * np.einsum("ik,pkj->pij", A.astype(wide), B.astype(wide)) + C0.astype(wide)).astype(dt)
    return A, B, C0, 2, 1, want
