"""tests/int_extremes.py checked on the CPU: the chosen values have the digits the docstring says, the operands of the GPU test
drive the accumulator groups exactly to the documented bound at K = one chunk, a missing split would show, and the closed form
is the product."""
import numpy as np
import pytest

from tests import int_extremes as X

WIDTHS = [8, 16, 32, 64]


@pytest.mark.parametrize("n", WIDTHS)
def test_balanced_digits_of_the_chosen_values(n):
    nl = n // 8
    assert X.balanced_digits(X.neg_digits_value(n), n) == [-128] * nl
    assert X.balanced_digits(X.pos_digits_value(n), n) == [127] * nl
    assert X.neg_digits_value(n) == {8: 0x80, 16: 0x7f80, 32: 0x7f7f7f80, 64: 0x7f7f7f7f7f7f7f80}[n]
    E = X.extremes(n)
    assert E[0] == X.neg_digits_value(n) and E[1] == X.pos_digits_value(n) and len(set(E)) == len(E) <= min(X.M, X.N)
    for want in (1 << (n - 1), (1 << (n - 1)) - 1, (1 << n) - 1, 0, 1):      # min, max, -1, 0, 1
        assert want in E
    for v in E:
        d = X.balanced_digits(v, n)
        assert all(-128 <= x <= 127 for x in d)
        assert sum(x * 256 ** p for p, x in enumerate(d)) % (1 << n) == v      # the digits recompose the value mod 2^n
    # the vectorised form agrees with the scalar one
    dt = np.dtype(f"i{nl}")
    planes = X.digit_planes(np.array(E, dtype=np.dtype(f"u{nl}")).view(dt), n)
    assert [[int(planes[p][i]) for p in range(nl)] for i in range(len(E))] == [X.balanced_digits(v, n) for v in E]


def _slice(case):
    """The first L rows of A and L columns of B: rows and columns repeat with period L (checked), so these hold every value."""
    A, B, L = case.A(), case.B(), case.L
    assert np.array_equal(A[L:2 * L], A[:L]) and np.array_equal(B[:, L:2 * L], B[:, :L])
    assert np.array_equal(A[X.M - X.M % L - L:X.M - X.M % L], A[:L])
    return A[:L], B[:, :L]


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64, np.uint16, np.uint64])
def test_accumulator_groups_reach_the_documented_bound_at_one_chunk(dtype):
    n = X.bits(dtype)
    chunk = X.CHUNK[n]
    assert X.BOUND[n] == (n // 8) * chunk * 2 ** 14 == {8: 2 ** 28, 16: 2 ** 29, 32: 2 ** 29, 64: 2 ** 30}[n]
    for K1 in X.k1_list(n, chunk):
        A, B = _slice(X.Case(dtype, chunk, K1))
        G = X.group_sums(A, B, n)
        top = max(int(np.abs(g).max()) for g in G)
        if K1 == chunk:
            assert top == X.BOUND[n] and int(G[-1][0, 0]) == X.BOUND[n]                 # NEG x NEG
            assert int(G[-1][0, 1]) == -(n // 8) * chunk * 128 * 127                    # NEG x POS: the negative end
        assert top <= X.BOUND[n] < 2 ** 31
    # one element more than a chunk, unsplit, is past the bound; split at the chunk it is not
    A, B = _slice(X.Case(dtype, chunk + 1, chunk + 1))
    assert max(int(np.abs(g).max()) for g in X.group_sums(A, B, n)) > X.BOUND[n]
    for k0 in (0, chunk):
        assert max(int(np.abs(g).max()) for g in X.group_sums(A, B, n, k0, min(k0 + chunk, chunk + 1))) <= X.BOUND[n]


def _fold(G, saturate):
    if saturate:
        return [np.clip(g, -2 ** 31, 2 ** 31 - 1) for g in G]
    return [(g + 2 ** 31) % 2 ** 32 - 2 ** 31 for g in G]


def test_int64_without_the_split_would_show():
    """What an int32 accumulator that is never folded does to the int64 product of the GPU test's operands.
    Two chunks: G_4..7 pass 2^31 - 1.  Of G_s, s >= 4, only the low 64 - 8 s <= 32 bits survive the shift, so a WRAPPING
    accumulator still gives the right product there; a saturating one does not.  Four chunks: G_3 = 4 * 32768 * 2^14 = 2^31
    wraps, and that changes the product.  So the GPU cases at 2 * chunk .. 3 * chunk - 1 pin "no saturation, or a split", and
    the int64 case at 4 * chunk fails for any int32 accumulator without the split."""
    n, chunk = 64, X.CHUNK[64]
    case = X.Case(np.int64, 2 * chunk, 2 * chunk)
    A, B = _slice(case)
    G = X.group_sums(A, B, n)
    assert max(int(g.max()) for g in G) > 2 ** 31 - 1 and max(int(np.abs(g).max()) for g in G[:4]) < 2 ** 31
    true = X.recombine(G, n)
    want = case.closed_form(1, 0)[:case.L, :case.L].view(np.uint64).astype(object)
    assert (true == want).all()
    assert (X.recombine(_fold(G, False), n) == true).all()
    assert X.recombine(_fold(G, True), n)[0, 0] != true[0, 0]
    # chunk by chunk the groups stay in range and the sum of the recombined chunks is the product
    parts = [X.group_sums(A, B, n, k0, k0 + chunk) for k0 in (0, chunk)]
    assert all(int(np.abs(g).max()) <= 2 ** 30 for part in parts for g in part)
    assert (((X.recombine(parts[0], n) + X.recombine(parts[1], n)) % (1 << n)) == want).all()
    # four chunks, the extra K of the 64-bit types
    assert X.k_list(64)[-1] == 4 * chunk
    case = X.Case(np.int64, 4 * chunk, 4 * chunk)
    A, B = _slice(case)
    G = X.group_sums(A, B, n)
    assert int(G[3][0, 0]) == 2 ** 31
    true = X.recombine(G, n)
    assert (true == case.closed_form(1, 0)[:case.L, :case.L].view(np.uint64).astype(object)).all()
    for saturate in (False, True):
        assert X.recombine(_fold(G, saturate), n)[0, 0] != true[0, 0]


@pytest.mark.parametrize("n", [8, 16, 32])
def test_narrower_types_do_not_depend_on_the_split(n):
    """n <= 32: even unsplit, the longest K of the list keeps every group below 2^31 (L * (3 * chunk - 1) * 2^14 < 2^31), and a
    wrap would vanish mod 2^n anyway; what those cases pin is the seam handling (beta = 1 from the second chunk on, the
    in-kernel fold) on coherent data and the bound itself."""
    dtype = np.dtype(f"i{n // 8}")
    K = X.k_list(n)[-1]
    case = X.Case(dtype, K, K)
    A, B = _slice(case)
    G = X.group_sums(A, B, n)
    assert X.BOUND[n] < max(int(np.abs(g).max()) for g in G) < 2 ** 31
    assert (X.recombine(_fold(G, False), n) == X.recombine(G, n)).all()


@pytest.mark.parametrize("dtype", X.DTYPES)
def test_closed_form_equals_numpys_wrapping_product_on_small_k(dtype):
    n = X.bits(dtype)
    for K, K1 in ((37, 37), (37, 32), (64, 0), (5, 3)):
        for same in (False, True):
            case = X.Case(dtype, K, K1, same)
            A, B, C0 = case.A(), case.B(), case.C0()
            assert A.dtype == np.dtype(dtype) and A.shape == (X.M, K) and B.shape == (K, X.N) and C0.shape == (X.M, X.N)
            for alpha, beta in X.scalars(n):
                with np.errstate(over="ignore"):
                    al, be = np.array(alpha % (1 << n), dtype=f"u{n // 8}").astype(dtype), np.array(beta % (1 << n), dtype=f"u{n // 8}").astype(dtype)
                    want = al * (A @ B) + be * C0
                assert want.dtype == np.dtype(dtype)
                assert np.array_equal(case.closed_form(alpha, beta), want), (dtype, K, K1, same, alpha, beta)


@pytest.mark.parametrize("n", WIDTHS)
def test_shapes_and_seams(n):
    c = X.CHUNK[n]
    assert X.k_list(n)[:6] == [c - 1, c, c + 1, 2 * c, 2 * c + 37, 3 * c - 1]
    for K in X.k_list(n):
        k1s = X.k1_list(n, K)
        assert all(0 < k1 <= K for k1 in k1s)
        assert k1s[0] - k1s[1] == 5 and (k1s[0] % c == 0 or K < c)
    assert any(b != 0 for _, b in X.scalars(n)) and (1, 0) in X.scalars(n) and (-1, 1) in X.scalars(n)
    assert X.scalars(n)[2] == (-(1 << (n - 1)), -1)
