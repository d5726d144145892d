"""GEMM operands whose spans reach and pass 2^31 and 2^32 bytes, laid out inside ONE device buffer (the arena), and the
catalogue of cases that straddle every hand-written 32-bit guard of the GEMM launchers.  Used by tests/test_far_views_cpu.py
(the geometry, no device) and tests/test_gpu_far_views.py.

A view is (shape, element strides, element offset) into the arena seen as an array of the case's element type: 2-D for a
matrix, 3-D (batch first) for a batched operand.  cases(dtype) yields

    (name, element type, M, N, K, view of A, view of B, view of C, guard, side, extra)

guard names an entry of GUARDS (or "" for the cases beyond the pairs), side is "inside" (the guarded kernel still takes the
view) or "past" (it must decline, and whichever kernel comes next must do the 64-bit arithmetic); extra holds what only some
cases have (bias view, batch count, kind, alpha / beta, whether the spans pass 2^32 bytes).

The placement rule.  Every far view lies at least FAR0 = 2^31 bytes into the arena.  A kernel gets the 64-bit address of a
view's first element and adds byte offsets to it.  An offset computed in 32 bits is the true one minus a multiple of 2^32
when it is truncated, and at worst 2^31 below zero when it is sign-extended, so with non-negative strides the wrong address lies
in [view - 2^31, true address): inside the arena.  The one view with negative strides (neg_rsA) has true offsets in (-2^32, 0];
truncated they become positive, below 2^32, and arena_bytes() keeps the arena longer than that view's base + 2^32.  Either way
a 32-bit slip gives a wrong number, which the comparison and the arena checksum report, not an access outside the allocation.
Rows of the far operands interleave inside one row pitch -- a pitch is megabytes, a row a few hundred elements -- and the
dense operands of a pair sit in the gap of the first pitch, so a 4-8 GB span for all three costs one buffer.

Each guard is written as the expression the launcher uses, with the function that holds it next to it.

Guards that cannot be straddled under the 12 GiB cap:
  * bias strides above 0x3fffffff elements (asm_plan.h choose_gemm_f32_asm): a 2-row bias at that stride is 4 GiB and fits, but the span
    limit on the same line declines first for any M, N >= 2, so the stride limit alone is unreachable with a real view;
  * gemm_small's K >= 2^30 (gemm_small.hip:203): the kernel is only offered K <= 128 (gemm_small_takes);
  * the tile-count limits `t * 8 * tn >= 4e9` (asm_plan.h consider_kernel, gemm_f32_asm.cpp launch_gemm_int_asm): they need ~10^4 x 10^4 tiles, a C of
    terabytes;
  * a batch stride past 2^31 ELEMENTS on 8-byte types (16 GiB).  Batch strides of 2^29 elements (2 and 4 GiB) are covered.
"""
import collections

import numpy as np

FAR0 = 2 ** 31                      # bytes: where far views start
CAP = 12 * 2 ** 30                  # bytes: the most the GPU module may hold in the arena
M, N, K = 300, 260, 520             # ragged against every tile (256, 192, 160, 128, 96, 64, 32), K % 4 == 0, one ragged kc slice
PITCH = 15_200_000                  # bytes: row pitch of the cases beyond the pairs (300 rows: 4.5e9 bytes > 2^32)
COL = (0, 8192, 16384)              # byte column of an A / B / C row inside a shared pitch (a row is at most 520 * 8 bytes)
DENSE = (1 << 16, (1 << 16) + (3 << 19), (1 << 16) + (6 << 19))      # byte offsets past FAR0 of the dense operands of a pair
DTYPES = [np.float32, np.float64, np.int32, np.int64, np.int8, np.int16]

View = collections.namedtuple("View", "shape strides offset")
Case = collections.namedtuple("Case", "name dtype M N K A B C guard side extra")


def _f(x):
    return float(x)


# ---- the guards, as the launchers write them: inside(...) is True where the guarded kernel still takes the view ----------
def f32_asm_A(rsA):          # asm_plan.h gemm_operands_fit<float>  (double)a.rsA * el * rows >= 4.0e9, el = 4, rows = 256
    return not (_f(rsA) * 4.0 * 256 >= 4.0e9)


def f32_asm_B(ldb, K=K):     # gemm_operands_fit<float>  (double)a.K * (double)ldb * el >= 4.0e9   (B row-major)
    return not (_f(K) * _f(ldb) * 4.0 >= 4.0e9)         # == gemm_mfma.hip:50-51 small() on a row-major B: ld * K * 4 < 4.0e9


def f32_asm_Bt(ldb):         # gemm_operands_fit<float>  (double)ldb * el * rows >= 4.0e9          (B passed transposed)
    return not (_f(ldb) * 4.0 * 256 >= 4.0e9)


def f32_asm_C(rsC, csC=1, M=M, N=N):      # gemm_operands_fit<float>  ((M-1) * rsC + (N-1) * csC + 1.0) * el > 2147483648.0
    return not ((_f(M - 1) * _f(rsC) + _f(N - 1) * _f(csC) + 1.0) * 4.0 > 2147483648.0)


def f32_asm_bias(rs, cs=1, M=M, N=N):     # asm_plan.h choose_gemm_f32_asm: the bias view
    return not (rs < 0 or cs < 0 or rs > 0x3fffffff or cs > 0x3fffffff or
                (_f(M - 1) * rs + _f(N - 1) * cs + 1.0) * 4.0 >= 2147483648.0)


def f64_asm_A(rsA):          # gemm_operands_fit<double>  (double)a.rsA * el * rows >= 4.0e9, el = 8, rows = 128
    return not (_f(rsA) * 8.0 * 128 >= 4.0e9)


def f64_asm_B(ldb, K=K):     # gemm_operands_fit<double>  (double)a.K * (double)ldb * el >= 4.0e9
    return not (_f(K) * _f(ldb) * 8.0 >= 4.0e9)


def f64_asm_Bt(ldb):         # gemm_operands_fit<double>  (double)ldb * el * rows >= 4.0e9
    return not (_f(ldb) * 8.0 * 128 >= 4.0e9)


def f64_asm_C(rsC, M=M, N=N):             # gemm_operands_fit<double>  ((M-1) * rsC + (N-1) * csC + 1.0) * el > 2147483648.0 with csC = 1
    return not ((_f(M - 1) * _f(rsC) + _f(N)) * 8.0 > 2147483648.0)


def int_asm_C(rsC, limbs, M=M, N=N):      # gemm_f32_asm.cpp launch_gemm_int_asm  ((M-1) * rsC + N) * limbs > 2147483648.0
    return not ((_f(M - 1) * _f(rsC) + _f(N)) * _f(limbs) > 2147483648.0)


def mfma_small_A(ld, size, M=M):          # gemm_mfma.hip:50-51  ld > 0 && (double)ld * (double)(sk == 1 ? X : K) * sizeof(E) < 4.0e9
    return ld > 0 and _f(ld) * _f(M) * size < 4.0e9      # A: sk = csA = 1, X = M


def mfma_small_B(ld, size, K=K):          # the same line for a row-major B: sx = csB = 1, so the factor is K
    return ld > 0 and _f(ld) * _f(K) * size < 4.0e9


def small_kstride(st, size):              # gemm_small.hip:202  st * sizeof(E) < (1ll << 31) && st * sizeof(E) > -(1ll << 31)
    return -(1 << 31) < st * size < (1 << 31)


def edge(inside, guess):
    """(ld_in, ld_past): the largest multiple of 4 that `inside` accepts and the next multiple of 4, found from `guess`"""
    ld = int(guess) // 4 * 4
    while not inside(ld):
        ld -= 4
    while inside(ld + 4):
        ld += 4
    assert inside(ld) and not inside(ld + 4)
    return ld, ld + 4


def _far(dtype, col=0):
    """element offset of a far view's first element"""
    return (FAR0 + col) // np.dtype(dtype).itemsize


def _dense(dtype, slot, rows, cols):
    return View((rows, cols), (cols, 1), (FAR0 + DENSE[slot]) // np.dtype(dtype).itemsize)


def _pair(dtype, guard, inside, guess, build):
    """the two cases of a guard: build(ld) -> (A, B, C, extra) with one operand far at leading dimension ld"""
    out = []
    for side, ld in zip(("inside", "past"), edge(inside, guess)):
        A, B, C, extra = build(ld)
        out.append(Case(f"{guard}-{side}", np.dtype(dtype), extra.pop("M", M), extra.pop("N", N), extra.pop("K", K), A, B, C, guard, side, extra))
    return out


def _gemm_views(dtype, far, ld, transposed_b=False):
    """A, B, C with operand `far` ("A" / "B" / "C") at leading dimension ld, the others dense in the gap of its first pitch"""
    A = View((M, K), (ld, 1), _far(dtype)) if far == "A" else _dense(dtype, 0, M, K)
    if far == "B":
        B = View((K, N), (1, ld), _far(dtype)) if transposed_b else View((K, N), (ld, 1), _far(dtype))
    else:
        B = _dense(dtype, 1, K, N)
    C = View((M, N), (ld, 1), _far(dtype)) if far == "C" else _dense(dtype, 2, M, N)
    return A, B, C


# inside(view strides...) of a case, by guard name: the CPU test evaluates it on the catalogue's own views
GUARDS = {
    "f32_asm_A": lambda c: f32_asm_A(c.A.strides[0]),
    "f32_asm_B": lambda c: f32_asm_B(c.B.strides[0], c.K) and mfma_small_B(c.B.strides[0], 4, c.K),
    "f32_asm_Bt": lambda c: f32_asm_Bt(c.B.strides[1]),
    "f32_asm_C": lambda c: f32_asm_C(c.C.strides[0], c.C.strides[1], c.M, c.N),
    "f32_asm_bias": lambda c: f32_asm_bias(c.extra["bias"].strides[0], c.extra["bias"].strides[1], c.M, c.N),
    "f32_mfma_small_A": lambda c: mfma_small_A(c.A.strides[0], 4, c.M),
    "f64_asm_A": lambda c: f64_asm_A(c.A.strides[0]),
    "f64_asm_B": lambda c: f64_asm_B(c.B.strides[0], c.K) and mfma_small_B(c.B.strides[0], 8, c.K),
    "f64_asm_Bt": lambda c: f64_asm_Bt(c.B.strides[1]),
    "f64_asm_C": lambda c: f64_asm_C(c.C.strides[0], c.M, c.N),
    "f64_mfma_small_A": lambda c: mfma_small_A(c.A.strides[0], 8, c.M),
    "int_asm_C": lambda c: int_asm_C(c.C.strides[0], c.dtype.itemsize, c.M, c.N),
    "gemm_small_kA": lambda c: small_kstride(c.A.strides[2], c.dtype.itemsize),
    "gemm_small_kB": lambda c: small_kstride(c.B.strides[1], c.dtype.itemsize),
}
# guards of the hand-scheduled kernels: on their "inside" case, with those kernels forced, the launch must be theirs
ASM_GUARDS = {"f32_asm_A", "f32_asm_B", "f32_asm_Bt", "f32_asm_C", "f32_asm_bias", "f64_asm_A", "f64_asm_B", "f64_asm_Bt",
              "f64_asm_C", "int_asm_C"}


def _small_pairs(dtype):
    """gemm_small (batches of matrices up to 64 x 64, K <= 128): K = 4 with a k-stride just under / at 2^31 bytes, on A (its
    column stride) and on B (its row stride); 2 problems"""
    size = np.dtype(dtype).itemsize
    m, n, k, b = 40, 36, 4, 2
    lim = (1 << 31) // size

    def on_a(cs):            # A[p][i][kk] at p * 512 + i * 8 + kk * cs
        return (View((b, m, k), (512, 8, cs), _far(dtype)), View((b, k, n), (k * n, n, 1), (FAR0 + DENSE[1]) // size),
                View((b, m, n), (m * n, n, 1), (FAR0 + DENSE[2]) // size), dict(M=m, N=n, K=k, kind="batched", batch=b))

    def on_b(rs):            # B[p][kk][j] at p * 64 + kk * rs + j
        return (View((b, m, k), (m * k, k, 1), (FAR0 + DENSE[0]) // size), View((b, k, n), (64, rs, 1), _far(dtype)),
                View((b, m, n), (m * n, n, 1), (FAR0 + DENSE[2]) // size), dict(M=m, N=n, K=k, kind="batched", batch=b))

    return (_pair(dtype, "gemm_small_kA", lambda st: small_kstride(st, size), lim - 4, on_a) +
            _pair(dtype, "gemm_small_kB", lambda st: small_kstride(st, size), lim - 4, on_b))


def _beyond(dtype):
    """the cases beyond the pairs, for any element type"""
    dt = np.dtype(dtype)
    size = dt.itemsize
    P = PITCH // size
    out = []

    def add(name, A, B, C, m=M, n=N, k=K, **extra):
        out.append(Case(name, dt, m, n, k, A, B, C, "", "", extra))

    far = lambda i: _far(dtype, COL[i])
    # all three far, interleaved in one pitch, every span past 2^32 bytes; beta = 0 over a C full of NaN patterns
    add("all_far_2p32", View((M, K), (P, 1), far(0)), View((K, N), (P, 1), far(1)), View((M, N), (P, 1), far(2)), p32=True, nan_c=True)
    # a large negative row stride on A, base at the far end
    Pn = P // 2              # (300 rows: 2.27e9 bytes > 2^31; the arena has to reach 2^32 past the base, see the module docstring)
    add("neg_rsA", View((M, K), (-Pn, 1), far(0) + (M - 1) * Pn), _dense(dtype, 1, K, N), _dense(dtype, 2, M, N))
    # C with a column stride of 2 and a far row stride
    add("C_cs2_far", _dense(dtype, 0, M, K), _dense(dtype, 1, K, N), View((M, N), (P, 2), far(2)), p32=True)
    # batched: 3 problems, batch strides of 2^29 elements (and at least 2 GiB: more elements for the 1- and 2-byte types) on B
    # and on C, A shared
    bs = max(2 ** 29, 2 ** 31 // size)
    add("batched_bs_2p29", View((3, M, K), (0, K, 1), (FAR0 + DENSE[0]) // size), View((3, K, N), (bs, N, 1), far(1) + (1 << 21) // size),
        View((3, M, N), (bs, N, 1), far(2) + (1 << 22) // size), kind="batched", batch=3, p32=size * bs * 2 >= 2 ** 32)
    # skinny: the long operand's slow stride at 2^28 elements (and at least 1 GiB)
    ss = max(2 ** 28, 2 ** 30 // size)
    add("skinny_M4", View((4, K), (ss, 1), far(0)), _dense(dtype, 1, K, N), _dense(dtype, 2, 4, N), m=4, p32=size * ss * 3 >= 2 ** 32)
    add("skinny_N4", _dense(dtype, 0, M, K), View((K, 4), (1, ss), far(1)), _dense(dtype, 2, M, 4), n=4, p32=size * ss * 3 >= 2 ** 32)
    # pre-packed: gemm_prepackA / B from far strided sources, gemm_packed into a far C
    add("prepacked", View((M, K), (P, 1), far(0)), View((K, N), (P, 1), far(1)), View((M, N), (P, 1), far(2)), kind="prepacked", p32=True)
    return out


def cases(dtype):
    """the catalogue for one element type"""
    dt = np.dtype(dtype)
    size = dt.itemsize
    out = []
    gv = lambda far, tb=False: (lambda ld: _gemm_views(dt, far, ld, tb) + (dict(),))
    if dt == np.float32:
        out += _pair(dt, "f32_asm_A", f32_asm_A, 4.0e9 / 1024, gv("A"))
        out += _pair(dt, "f32_asm_B", f32_asm_B, 4.0e9 / (4 * K), gv("B"))
        out += _pair(dt, "f32_asm_Bt", f32_asm_Bt, 4.0e9 / 1024, gv("B", True))
        out += _pair(dt, "f32_asm_C", f32_asm_C, 2 ** 29 / (M - 1), gv("C"))
        out += _pair(dt, "f32_mfma_small_A", lambda ld: mfma_small_A(ld, 4), 4.0e9 / (4 * M), gv("A"))

        def with_bias(ld):      # every GEMM operand dense, the bias view of the fused epilogue far; beta = 0 (the one-chain
            A, B, C = _gemm_views(dt, "", 0)      # assembly kernels' fused epilogue has no C read)
            return A, B, C, dict(bias=View((M, N), (ld, 1), _far(dt)), beta=0)
        out += _pair(dt, "f32_asm_bias", f32_asm_bias, 2 ** 29 / (M - 1), with_bias)
        out += _small_pairs(dt)
    elif dt == np.float64:
        out += _pair(dt, "f64_asm_A", f64_asm_A, 4.0e9 / 1024, gv("A"))
        out += _pair(dt, "f64_asm_B", f64_asm_B, 4.0e9 / (8 * K), gv("B"))
        out += _pair(dt, "f64_asm_Bt", f64_asm_Bt, 4.0e9 / 1024, gv("B", True))
        out += _pair(dt, "f64_asm_C", f64_asm_C, 2 ** 28 / (M - 1), gv("C"))
        out += _pair(dt, "f64_mfma_small_A", lambda ld: mfma_small_A(ld, 8), 4.0e9 / (8 * M), gv("A"))
        out += _small_pairs(dt)
    elif dt in (np.dtype(np.int32), np.dtype(np.int64)):
        out += _pair(dt, "int_asm_C", lambda ld: int_asm_C(ld, size), 2 ** 31 / size / (M - 1), gv("C"))
    return out + _beyond(dt)


def all_cases():
    return [c for dt in DTYPES for c in cases(dt)]


# ---- geometry on the CPU ---------------------------------------------------------------------------------------------
def operands(c):
    """[(what, view)] of every operand view of the case, the bias included"""
    ops = [("A", c.A), ("B", c.B), ("C", c.C)]
    if "bias" in c.extra:
        ops.append(("bias", c.extra["bias"]))
    return ops


def element_offsets(v):
    """true element offsets of every element of the view, int64, in the view's shape (a stride-0 axis is kept: repeats)"""
    off = np.full((), v.offset, dtype=np.int64)
    for ax, (n, s) in enumerate(zip(v.shape, v.strides)):
        shape = [1] * len(v.shape)
        shape[ax] = n
        off = off + (np.arange(n, dtype=np.int64) * np.int64(s)).reshape(shape)
    return off


def byte_span(v, size):
    """[lo, hi) in bytes"""
    lo = v.offset + sum(min(0, (n - 1) * s) for n, s in zip(v.shape, v.strides))
    hi = v.offset + sum(max(0, (n - 1) * s) for n, s in zip(v.shape, v.strides)) + 1
    return lo * size, hi * size


def is_far(v, size):
    """the dense operands are at most 1.3 MB"""
    lo, hi = byte_span(v, size)
    return hi - lo > (64 << 20)


def arena_bytes(case_list):
    """bytes of the arena that holds every case of the list: past the last byte used, rounded up to 64 MiB, and above 2^32 so
    that a truncated 32-bit offset stays inside"""
    end = max(byte_span(v, c.dtype.itemsize)[1] for c in case_list for _, v in operands(c))
    for c in case_list:
        for _, v in operands(c):
            if min(v.strides) < 0:
                end = max(end, v.offset * c.dtype.itemsize + 2 ** 32 + (1 << 20))
    return max(-(-end // (64 << 20)) * (64 << 20), 2 ** 32 + (64 << 20))


def has_teeth(v, size):
    """(uint32 differs, int32 differs): does a byte offset from the view's base, accumulated in 32 bits, differ from the true
    one for some element?  The offset is what a kernel adds to the 64-bit base pointer of the view."""
    rel = (element_offsets(v) - np.int64(v.offset)) * np.int64(size)
    u = rel.astype(np.uint32).astype(np.int64)
    i = rel.astype(np.int32).astype(np.int64)
    return bool((u != rel).any()), bool((i != rel).any())


# ---- host operands ------------------------------------------------------------------------------------------------------
def scalars(c, fast=False):
    """(alpha, beta): beta != 0 reads the far C; the nan_c case and the bias pair run beta = 0"""
    if c.dtype.kind == "f":
        alpha, beta = (2.0, -1.0) if fast else (0.75, -0.5)
    else:
        alpha, beta = 3, -2
    if c.extra.get("nan_c") or c.extra.get("beta") == 0:
        beta = type(beta)(0)
    return alpha, beta


def _gen(c, rng, shape, fast):
    if c.dtype.kind != "f":
        info = np.iinfo(c.dtype)
        return rng.integers(info.min, info.max, shape, dtype=c.dtype, endpoint=True)
    if fast:
        return rng.integers(-8, 8, shape, endpoint=True).astype(c.dtype)
    return rng.uniform(-1, 1, shape).astype(c.dtype)


def _operands(c, fast):
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{c.dtype}-{c.name}-{int(fast)}".encode()))
    out = []
    for _, v in operands(c):
        x = _gen(c, rng, v.shape, fast)
        if len(v.shape) == 3 and v.strides[0] == 0:      # one matrix shared by the batch
            x[:] = x[0]
        out.append(x)
    return tuple(out) + ((None,) if len(out) == 3 else ())


def fast_operands(c):
    """A, B, C0, bias (or None) in the shapes of the views: small integers stored as floats, |v| <= 8"""
    assert c.dtype.kind == "f"
    return _operands(c, True)


def laser_operands(c):
    """A, B, C0, bias (or None): uniform in (-1, 1) for the float types, full range for the integer types"""
    return _operands(c, False)


def nan_patterns(shape, dtype):
    """quiet and signalling NaNs of both signs with varying payloads"""
    n = int(np.prod(shape))
    if np.dtype(dtype) == np.float32:
        heads = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001], dtype=np.uint32)
        bits = heads[np.arange(n) % 4] | (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) & np.uint32(0x003ffffe))
        return bits.view(np.float32).reshape(shape)
    heads = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001], dtype=np.uint64)
    bits = heads[np.arange(n) % 4] | (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) & np.uint64(0x0007fffffffffffe))
    return bits.view(np.float64).reshape(shape)
