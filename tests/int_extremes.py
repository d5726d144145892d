"""Coherent integer GEMM operands that drive the limb kernels' int32 accumulators to their documented bound, and an exact
closed-form reference for them (used by tests/test_int_extremes_cpu.py and tests/test_gpu_int_extremes.py).

The limb kernels (gemm_i32_mfma.hip, gemm_i64_mfma.hip, gemm_narrow_mfma.hip, asmgen/i8_kernel.py) write every element as
balanced base-256 digits s_p in [-128, 127] and accumulate, per power s of 256, G_s = sum_{p+q=s} sum_k s_p(a_ik) s_q(b_kj) in
int32.  What keeps G_s inside int32 is a limit on the K summed between two folds (CHUNK below); with uniformly random operands
the digit products cancel and |G_s| stays near sqrt(K) * 2^13, a thousand times below the bound, so only same-sign extreme
digits on BOTH operands over a whole chunk show that the chunk is short enough.

Operands.  A[i, k] = u[i] for k < K1, else w[i];  B[k, j] = v[j] for k < K1, else x[j], so that

    (A B)[i, j] = K1 u_i v_j + (K - K1) w_i x_j        C = alpha (A B) + beta C0   (mod 2^n)

is evaluated in Python integers -- independent of the oracle and of numpy's wrap-around.  u, v (and w, x, C0, shifted) cycle
through extremes(n), whose head is

    NEG = 0x7f..7f80   every balanced digit is -128 (the top digit after the carry: (a + 0x0080..80) ^ 0x0080..80 = 0x80..80)
    POS = 0x7f..7f     every balanced digit is +127

followed by min, max, -1, 0, 1, 0x0080..80 and the values of tests/test_gpu_parity.py's "extreme digits" loops.  Rows and
columns repeat with period len(extremes(n)) <= M, N, so every pair of extremes meets in some (i, j).  With u = NEG and v = NEG
every digit product is +2^14 and G_{L-1} (L = n / 8 digits) is L * K * 2^14: exactly the documented bound at K = CHUNK --
2^29 for int32 and int16, 2^30 for int64 (2^28 for int8, whose single digit has one product).  With v = POS it is
-L * K * 128 * 127, the most negative value there is.
"""
import numpy as np

# K summed into one int32 accumulator group between two folds
CHUNK = {8: 16384,      # gemm_narrow_mfma.hip:25 NARROW_MAX_K (gemm_route.cpp run_gemm_int cuts longer K with int_gemm_k_chunks)
         16: 16384,
         32: 8192,      # gemm_i32_mfma.hip:49 IFOLD_K (folded inside the kernel); asmgen/i8_kernel.py:18 K <= 8192 per launch
         64: 8192}      # gemm_i64_mfma.hip:13-14 (chunks cut by the launcher); gemm_route.cpp int_gemm_k_chunks kChunk
BOUND = {8: 2 ** 28, 16: 2 ** 29, 32: 2 ** 29, 64: 2 ** 30}      # L * CHUNK * 2^14
M = N = 160     # ragged against the 128 and 64 tiles; 160 * 160 * K is above the matrix-core work threshold (gemm_route.cpp: 64^3 * 8)
DTYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64]


def bits(dtype):
    return np.dtype(dtype).itemsize * 8


def k_list(n):
    c = CHUNK[n]
    # 64-bit: at 4 chunks G_3 = 4 * 32768 * 2^14 = 2^31 wraps in an unsplit int32 accumulator and changes the product (below
    # that only G_4..7 pass 2^31, whose high bits the shift by 8 s drops anyway: tests/test_int_extremes_cpu.py)
    return [c - 1, c, c + 1, 2 * c, 2 * c + 37, 3 * c - 1] + ([4 * c] if n == 64 else [])


def k1_list(n, K):
    """Where the operands change value: at the last chunk seam <= K (K itself below one chunk: no change at all), 5
    elements before it, so that the value change does not coincide with the chunk change, and never (K1 = K: every chunk
    and the ragged tail carry the same values)."""
    c = CHUNK[n]
    seam = K // c * c if K >= c else K
    return [seam, seam - 5] + ([K] if K != seam else [])


def neg_digits_value(n):
    return (int("7f" * (n // 8 - 1), 16) << 8 | 0x80) if n > 8 else 0x80


def pos_digits_value(n):
    return int("7f" * (n // 8), 16)


def extremes(n):
    """The n-bit patterns (unsigned Python ints), NEG and POS first, no value twice."""
    mask = (1 << n) - 1
    lo80 = int("80" * (n // 8 - 1), 16) if n > 8 else 0x80            # 0x0080..80
    vals = [neg_digits_value(n), pos_digits_value(n), 1 << (n - 1), (1 << (n - 1)) - 1, -1, 0, 1, lo80,
            # tests/test_gpu_parity.py:231 and :267-268
            -int("7f" * (n // 8 - 1) + "80", 16), 128, 127, -128, -129, 1 << 32, (1 << 32) - 1, -(1 << 56)]
    out = []
    for v in vals:
        if v & mask not in out:
            out.append(v & mask)
    return out


def signed(v, n):
    v &= (1 << n) - 1
    return v - (1 << n) if v >> (n - 1) else v


def balanced_digits(v, n):
    """The n / 8 digits the packing passes produce for the n-bit pattern v (limb_planes.h:26 and :31, gemm_i32_mfma.hip:15-17,
    gemm_narrow_mfma.hip:11): byte p of (v + 0x0080..80) ^ 0x0080..80 read as int8; the int8 digit is the byte itself."""
    mask = (1 << n) - 1
    c = int("80" * (n // 8 - 1), 16) if n > 8 else 0
    d = (((v & mask) + c) & mask) ^ c
    return [signed(d >> (8 * p), 8) for p in range(n // 8)]


def scalars(n):
    """(alpha, beta) pairs: the issue's three and one full-range pair (fixed odd constants cut to n bits)."""
    return [(1, 0), (-1, 1), (signed(1 << (n - 1), n), -1),
            (signed(0x9e3779b97f4a7c15, n), signed(0xc2b2ae3d27d4eb4f, n))]


class Case:
    """One product: the four value vectors as indices into extremes(n) (row i uses index i % L), K, K1 and C0."""

    def __init__(self, dtype, K, K1, same=False):
        self.dtype = np.dtype(dtype)
        self.n = bits(dtype)
        self.K, self.K1 = K, K1
        self.E = extremes(self.n)
        self.L = L = len(self.E)
        assert L <= M and L <= N and 0 <= K1 <= K
        # index of u, w (by i % L) and v, x (by j % L); `same`: w = u and x = v (the bound in every chunk)
        self.iu = list(range(L))
        self.iv = list(range(L))
        self.iw = self.iu if same else [(a + 1) % L for a in range(L)]
        self.ix = self.iv if same else [(b + 2) % L for b in range(L)]

    def _np(self, patterns):
        u = np.array(patterns, dtype=np.dtype(f"u{self.n // 8}"))
        return u.view(self.dtype) if self.dtype.kind == "i" else u

    def _col(self, idx, count):
        return self._np([self.E[idx[i % self.L]] for i in range(count)])

    def A(self):
        a = np.empty((M, self.K), dtype=self.dtype)
        a[:, :self.K1] = self._col(self.iu, M)[:, None]
        a[:, self.K1:] = self._col(self.iw, M)[:, None]
        return a

    def B(self):
        b = np.empty((self.K, N), dtype=self.dtype)
        b[:self.K1] = self._col(self.iv, N)[None, :]
        b[self.K1:] = self._col(self.ix, N)[None, :]
        return b

    def c0_index(self, a, b):
        return (3 * a + b + 1) % self.L

    def C0(self):
        L = self.L
        return self._np([[self.E[self.c0_index(i % L, j % L)] for j in range(N)] for i in range(M)])

    def closed_form(self, alpha, beta):
        """alpha (K1 u_i v_j + (K - K1) w_i x_j) + beta C0[i, j] mod 2^n, in Python integers on the signed (or unsigned)
        values; one evaluation per (i % L, j % L), spread over M x N."""
        L, n, E = self.L, self.n, self.E
        val = (lambda p: signed(p, n)) if self.dtype.kind == "i" else (lambda p: p)
        T = [[(alpha * (self.K1 * val(E[self.iu[a]]) * val(E[self.iv[b]])
                        + (self.K - self.K1) * val(E[self.iw[a]]) * val(E[self.ix[b]]))
               + beta * val(E[self.c0_index(a, b)])) % (1 << n) for b in range(L)] for a in range(L)]
        return self._np([[T[i % L][j % L] for j in range(N)] for i in range(M)])


def digit_planes(X, n):
    """balanced_digits of every element of the integer array X: float64 planes [n / 8][...] (exact: |digit| <= 128)."""
    u = X.view(np.dtype(f"u{n // 8}")).astype(np.uint64)
    mask = np.uint64((1 << n) - 1)
    c = np.uint64(int("80" * (n // 8 - 1), 16) if n > 8 else 0)
    with np.errstate(over="ignore"):
        d = ((u + c) & mask) ^ c          # (uint64 wraps mod 2^64: the carry out of the top digit is dropped, as on the GPU)
    planes = []
    for p in range(n // 8):
        byte = ((d >> np.uint64(8 * p)) & np.uint64(0xff)).astype(np.int64)
        planes.append(np.where(byte >= 128, byte - 256, byte).astype(np.float64))
    return planes


def group_sums(A, B, n, k0=0, k1=None):
    """G_s[i, j] = sum_{p+q=s} sum_{k0 <= k < k1} s_p(A[i, k]) s_q(B[k, j]) as exact int64 (float64 products of digits: every
    partial sum is an integer below 2^53), s = 0 .. n / 8 - 1."""
    k1 = A.shape[1] if k1 is None else k1
    pa, pb = digit_planes(A[:, k0:k1], n), digit_planes(B[k0:k1], n)
    nl = n // 8
    return [sum(pa[p] @ pb[s - p] for p in range(s + 1)).astype(np.int64) for s in range(nl)]


def recombine(G, n):
    """sum_s G_s << 8 s mod 2^n as Python integers (the kernels' epilogues before alpha / beta)."""
    out = np.zeros(G[0].shape, dtype=object)
    for s, g in enumerate(G):
        out = (out + g.astype(object) * 256 ** s) % (1 << n)
    return out
