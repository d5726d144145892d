"""The catalogue of tests/far_views.py checked without a device: every view is inside the arena and apart from the other
operands of its case, far views obey the 2^31-byte placement rule, every pair lies on its two sides of the mirrored guard, a
kernel that did the view's address arithmetic in 32 bits would touch another address, and the integer-valued operands of the
one-chain (FAST) mode keep every partial sum exact."""
import numpy as np
import pytest

from tests import far_views as FV

ALL = FV.all_cases()
IDS = [f"{c.dtype}-{c.name}" for c in ALL]


def test_catalogue_covers_what_it_should():
    names = {(str(c.dtype), c.name) for c in ALL}
    assert len(names) == len(ALL)
    for dt in FV.DTYPES:
        have = {c.name for c in FV.cases(dt)}
        assert {"all_far_2p32", "neg_rsA", "C_cs2_far", "batched_bs_2p29", "skinny_M4", "skinny_N4", "prepacked"} <= have
    f32 = {c.guard for c in FV.cases(np.float32)}
    assert {"f32_asm_A", "f32_asm_B", "f32_asm_Bt", "f32_asm_C", "f32_asm_bias", "f32_mfma_small_A", "gemm_small_kA", "gemm_small_kB"} <= f32
    f64 = {c.guard for c in FV.cases(np.float64)}
    assert {"f64_asm_A", "f64_asm_B", "f64_asm_Bt", "f64_asm_C", "f64_mfma_small_A", "gemm_small_kA", "gemm_small_kB"} <= f64
    for dt in (np.int32, np.int64):
        assert "int_asm_C" in {c.guard for c in FV.cases(dt)}
    assert (FV.M, FV.N, FV.K) == (300, 260, 520)
    for tile in (32, 64, 96, 128, 160, 192, 256):
        assert FV.M % tile and FV.N % tile
    assert FV.K % 4 == 0 and FV.K % 512


@pytest.mark.parametrize("dtype", FV.DTYPES, ids=[str(np.dtype(d)) for d in FV.DTYPES])
def test_the_arena_fits_under_the_cap(dtype):
    n = FV.arena_bytes(FV.cases(dtype))
    assert 2 ** 32 < n <= FV.CAP and n % 4 == 0


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_views_in_bounds_apart_and_far(c):
    size = c.dtype.itemsize
    arena = FV.arena_bytes(FV.cases(c.dtype))
    ops = FV.operands(c)
    spans = {}
    for what, v in ops:
        lo, hi = FV.byte_span(v, size)
        assert 0 <= lo < hi <= arena, (what, lo, hi, arena)
        off = FV.element_offsets(v)
        assert int(off.min()) * size == lo and (int(off.max()) + 1) * size == hi
        spans[what] = off
        if FV.is_far(v, size):
            assert lo >= FV.FAR0, f"{what} starts {lo} bytes into the arena: the placement rule wants 2^31"
            assert (v.offset * size) % 16 == 0                                   # the vector loaders stay eligible
            assert all(s % 4 == 0 or abs(s) <= 2 for s in v.strides), v.strides
            if min(v.strides) < 0:
                assert v.offset * size + 2 ** 32 <= arena
    # shapes agree with M, N, K
    assert c.A.shape[-2:] == (c.M, c.K) and c.B.shape[-2:] == (c.K, c.N) and c.C.shape[-2:] == (c.M, c.N)
    # no operand shares an element with another, and C (written) has no element twice
    flat = {w: np.unique(o.ravel()) for w, o in spans.items()}
    assert flat["C"].size == int(np.prod(c.C.shape))
    names = sorted(flat)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert np.intersect1d(flat[a], flat[b]).size == 0, (a, b)
    assert any(FV.is_far(v, size) for _, v in ops)
    if c.guard:          # one operand far, the others dense
        assert sum(FV.is_far(v, size) for _, v in ops) == 1


@pytest.mark.parametrize("c", [c for c in ALL if c.guard], ids=[i for i, c in zip(IDS, ALL) if c.guard])
def test_pairs_straddle_the_mirrored_guard(c):
    inside = FV.GUARDS[c.guard](c)
    assert inside == (c.side == "inside"), (c.name, inside)
    twin = [o for o in FV.cases(c.dtype) if o.guard == c.guard and o.side != c.side]
    assert len(twin) == 1
    # the two sides differ by one step of 4 elements in one stride of one operand
    diffs = [(abs(s - t)) for (_, v), (_, w) in zip(FV.operands(c), FV.operands(twin[0])) for s, t in zip(v.strides, w.strides) if s != t]
    assert diffs == [4], diffs


def test_guard_edges_by_hand():
    """the mirrored expressions at values worked out from the source lines"""
    assert FV.f32_asm_A(3906248) and not FV.f32_asm_A(3906250) and not FV.f32_asm_A(3906252)       # 4e9 / 1024 = 3906250
    assert FV.f32_asm_Bt(3906248) and not FV.f32_asm_Bt(3906252)
    assert FV.f32_asm_B(1923076) and not FV.f32_asm_B(1923077)                                   # 4e9 / (520 * 4) = 1923076.9
    assert FV.f32_asm_C(1795552) and not FV.f32_asm_C(1795556)                                   # (2^29 - 260) / 299 = 1795553.7
    assert FV.f64_asm_A(3906248) and not FV.f64_asm_A(3906250)                                   # 4e9 / (8 * 128)
    assert FV.f64_asm_C(897776) and not FV.f64_asm_C(897780)                                     # (2^28 - 260) / 299 = 897776.4
    assert FV.int_asm_C(1795552, 4) and not FV.int_asm_C(1795556, 4) and FV.int_asm_C(897776, 8) and not FV.int_asm_C(897780, 8)
    assert FV.mfma_small_A(3333332, 4) and not FV.mfma_small_A(3333336, 4)                       # 4e9 / (300 * 4) = 3333333.3
    assert FV.small_kstride(2 ** 29 - 4, 4) and not FV.small_kstride(2 ** 29, 4) and not FV.small_kstride(-2 ** 29, 4)


@pytest.mark.parametrize("c", ALL, ids=IDS)
def test_every_far_view_has_teeth(c):
    """Byte offsets from the view's first element, recomputed in 32 bits, differ from the true ones for some element: in int32
    for every far view (so a kernel with an `int` in its address arithmetic touches another address), in uint32 as well where
    the case is labelled 2^32.  The one exception is by construction: the `inside` cases of the guards that sit AT 2^31 bytes
    (the C and bias spans) end within one row step below 2^31, where 32-bit offsets are still exact -- that is the limit
    the hand-scheduled kernels rely on, and their `past` twins have teeth."""
    size = c.dtype.itemsize
    at_2p31 = c.guard in ("f32_asm_C", "f32_asm_bias", "f64_asm_C", "int_asm_C")
    for what, v in FV.operands(c):
        if not FV.is_far(v, size):
            continue
        u32, i32 = FV.has_teeth(v, size)
        if at_2p31 and c.side == "inside":
            lo, hi = FV.byte_span(v, size)
            assert not i32 and 2 ** 31 - 4 * (c.M - 1) * size - 16 <= hi - lo <= 2 ** 31
        else:
            assert i32, (c.name, what)
        if c.extra.get("p32"):
            assert u32, (c.name, what)
        # and from the arena's base every element of a far view is past 2^31: int32 differs everywhere
        assert int(FV.element_offsets(v).min()) * size >= 2 ** 31
    if c.name == "all_far_2p32":
        assert c.extra["p32"] and all(FV.byte_span(v, size)[1] - FV.byte_span(v, size)[0] > 2 ** 32 for _, v in FV.operands(c))


def test_fast_mode_operands_stay_exact():
    """small integers stored as floats, |v| <= 8: every partial sum of alpha * A B + beta * C0 (+ bias), in any order, is an
    integer below 2^24, so float32 (and float64) arithmetic is exact and the bar is equality with the float64 product"""
    for c in ALL:
        if c.dtype.kind != "f":
            continue
        A, B, C0, bias = FV.fast_operands(c)
        for x in (A, B, C0) + (() if bias is None else (bias,)):
            assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 8 and x.dtype == c.dtype
        alpha, beta = FV.scalars(c, fast=True)
        assert alpha == int(alpha) and beta == int(beta)
        # the largest partial sum any order can reach: sum of absolute values, exactly, in Python integers via int64
        worst = np.abs(A).astype(np.int64) @ np.abs(B).astype(np.int64) if A.ndim == 2 else \
            np.einsum("bik,bkj->bij", np.abs(A).astype(np.int64), np.abs(B).astype(np.int64))
        worst = abs(int(alpha)) * worst + abs(int(beta)) * np.abs(C0).astype(np.int64) + (0 if bias is None else np.abs(bias).astype(np.int64))
        assert int(worst.max()) < 2 ** 24, (c.name, int(worst.max()))
