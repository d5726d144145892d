"""The batched-GEMM case generator (tests/batched_views.py) checked on its own, without a device: the geometry of every view,
the properties each layout class exists for, and the cached references against independent computations on gathered dense
copies."""
import numpy as np
import pytest

from tests import batched_views as BV

INTS = [dt for dt in BV.DTYPES if np.dtype(dt).kind != "f"]
FLOATS = [np.float32, np.float64]


def _ops(c):
    return [(w, getattr(c, w)) + BV.dims(c, w) for w in "ABC"]


def test_every_view_lies_inside_its_arena_with_the_slack():
    """at least one whole batch span plus one matrix span of the arena on both sides of every view"""
    for c in BV.all_cases():
        for w, v, rows, cols in _ops(c):
            lo, hi = BV.reach(v.strides, c.batch, rows, cols)
            sl = BV.slack(v.strides, c.batch, rows, cols)
            assert sl >= c.batch * abs(v.strides[0]) + BV.matrix_span(v.strides, rows, cols) >= 1
            n = BV.arena_len(v, c.batch, rows, cols)
            assert v.offset + lo - sl >= 0 and v.offset + hi + sl < n, (BV.describe(c), w)
            off = BV.element_offsets(v, c.batch, rows, cols)
            assert off.min() == v.offset + lo and off.max() == v.offset + hi, (BV.describe(c), w)
    # the arenas have that length, and the C arena holds the sentinel exactly where the view does not address it
    for dt in (np.float32, np.int16):
        for c in BV.cases(dt, scalar_list=[(1, 0)]):
            a, b, cbuf, mask = BV.arenas(c)
            assert (a.size, b.size, cbuf.size) == tuple(BV.arena_len(v, c.batch, r, k) for _, v, r, k in _ops(c))
            assert mask.sum() == c.batch * c.M * c.N
            assert np.array_equal(BV.bits(cbuf)[~mask], BV.bits(BV.sentinel(dt, int((~mask).sum()))))
            assert not (BV.bits(cbuf)[mask] == BV.bits(BV.sentinel(dt, 1))[0]).all()
            if np.dtype(dt).kind == "f":
                assert np.isnan(cbuf[~mask]).all() and not np.isnan(cbuf[mask]).any()
                assert np.isnan(BV.arenas(c, nan_c=True)[2]).all()


def test_addressed_elements_of_c_are_pairwise_distinct():
    """The condition that makes the batched call well defined: no two addressed elements of C alias, within an entry or across
    entries (A and B may overlap or be shared)."""
    for c in BV.all_cases():
        off = BV.element_offsets(c.C, c.batch, c.M, c.N).ravel()
        assert np.unique(off).size == off.size == c.batch * c.M * c.N, BV.describe(c)


def test_all_layouts_types_shapes_and_scalars_appear():
    every = BV.all_cases()
    assert {c.layout for c in every} == set(BV.LAYOUTS) >= set(BV.REQUIRED_LAYOUTS) and len(set(BV.REQUIRED_LAYOUTS)) == 10
    assert {c.dtype for c in every} == {np.dtype(t) for t in BV.DTYPES} and len(BV.DTYPES) == 10
    for dt in BV.DTYPES:
        got = BV.cases(dt)
        flo = np.dtype(dt).kind == "f"
        want_shapes = ([(5, 7, 33, 50), (3, 64, 64, 128), (3, 130, 70, 517), (3, 200, 136, 260), (2, 260, 136, 1028), (3, 300, 1, 600),
                        (3, 4, 300, 600), (4, 1, 1, 1)] if flo else [(4, 65, 67, 33), (3, 130, 1, 257), (2, 200, 136, 516)])
        want_scalars = [(1, 0), (1, 1), (0.5, 0.25)] if flo else [(1, 0), (1, 1), (2, 3), (-3, 1)]
        assert {(c.layout, (c.batch, c.M, c.N, c.K), (c.alpha, c.beta)) for c in got} == \
            {(lay, sh, ab) for lay in BV.LAYOUTS for sh in want_shapes for ab in want_scalars}
    from laser_amd import primitives
    assert {np.dtype(t).name for t in BV.DTYPES} == set(primitives._SFX)


def test_layout_classes_are_what_they_claim():
    for c in BV.all_cases():
        (bsA, rsA, csA), (bsB, rsB, csB), (bsC, rsC, csC) = c.A.strides, c.B.strides, c.C.strides
        what = BV.describe(c)
        if c.layout == "dense":
            assert (c.A.strides, c.B.strides, c.C.strides) == ((c.M * c.K, c.K, 1), (c.K * c.N, c.N, 1), (c.M * c.N, c.N, 1))
            assert all(v.offset % 64 == 0 for v in (c.A, c.B, c.C))
        elif c.layout.startswith("share"):
            assert (bsA == 0) == (c.layout in ("share_a", "share_ab")) and (bsB == 0) == (c.layout in ("share_b", "share_ab")) and bsC > 0
        elif c.layout == "padded":
            assert (rsA, rsB, rsC) == (c.K + 3, c.N + 5, c.N + 7) and (csA, csB, csC) == (1, 1, 1)
            for (w, v, rows, cols), odd in zip(_ops(c), (1, 3, 5)):
                bs = v.strides[0]
                assert bs % 4 != 0 and bs % 2 != 0 and bs >= BV.matrix_span(v.strides, rows, cols) + 3, what
                assert v.offset % 64 == odd and (v.offset * c.dtype.itemsize) % 16 != 0, what        # the arena itself is 64-byte aligned
        elif c.layout == "transposed":
            assert (rsA, csA, rsB, csB, rsC, csC) == (1, c.M + 1, 1, c.K + 4, 1, c.M + 2)
        elif c.layout == "b_transposed":
            assert (rsA, csA, rsB, csB, rsC, csC) == (c.K, 1, 1, c.K + 4, c.N, 1) and min(bsA, bsB, bsC) > 0
        elif c.layout == "reversed_batches":
            assert bsA < 0 and bsB < 0 and bsC < 0, what
            for w, v, rows, cols in _ops(c):       # entry 0 at the far end
                off = BV.element_offsets(v, c.batch, rows, cols)
                assert off[0].min() > off[-1].max()
        elif c.layout == "negative_inner":
            assert csA == -1 and rsB < 0 and rsA < 0 and csC == -2 and rsC == 2 * c.N
            _, _, cbuf, mask = BV.arenas(c)
            if c.N > 1:                              # the elements between C's columns are sentinels
                assert not mask[BV.element_offsets(c.C, c.batch, c.M, c.N)[:, :, 1:] + 1].any()
        elif c.layout == "interleaved":
            assert (bsA, bsB, bsC) == (1, 1, 1) and (rsA, csA) == (c.K * c.batch, c.batch) and (rsB, csB) == (c.N * c.batch, c.batch) \
                and (rsC, csC) == (c.N * c.batch, c.batch)
        elif c.layout == "sliding":
            assert bsA == (c.M // 2) * rsA and bsA < c.M * rsA and (bsB < c.N or c.N == 1) and csB == 1
            offA = BV.element_offsets(c.A, c.batch, c.M, c.K)
            offB = BV.element_offsets(c.B, c.batch, c.K, c.N)
            overlaps = np.intersect1d(offA[0], offA[1]).size > 0, np.intersect1d(offB[0], offB[1]).size > 0
            assert overlaps[0] or c.M == 1 and bsA == 0, what
            assert overlaps[1] or c.N == 1, what
            assert any(overlaps) or (c.M, c.N) == (1, 1), what
        else:
            raise AssertionError(c.layout)


def _dense(c):
    a, b, cbuf, _ = BV.arenas(c)
    return BV.gather(a, c.A, c.batch, c.M, c.K), BV.gather(b, c.B, c.batch, c.K, c.N), BV.gather(cbuf, c.C, c.batch, c.M, c.N)


def test_views_and_gathered_copies_hold_the_same_values():
    for dt in (np.float64, np.uint8):
        for c in BV.cases(dt, scalar_list=[(1, 0)]):
            for x, y in zip(BV.operands(c), _dense(c)):
                assert np.array_equal(x, y), BV.describe(c)


@pytest.mark.parametrize("dtype", INTS, ids=[np.dtype(t).name for t in INTS])
def test_integer_references_equal_a_wrapping_einsum_on_dense_copies(oracle, dtype):
    """int32 / int64: the oracle on the views against numpy; the narrow and unsigned types: the wrapping reference on the views
    against the same arithmetic written as an einsum on gathered copies"""
    u = np.dtype(f"u{np.dtype(dtype).itemsize}")
    for c in BV.cases(dtype):
        A, B, C0 = (BV.wrap_u64(x) for x in _dense(c))
        with np.errstate(over="ignore"):
            v = np.uint64(c.alpha % 2 ** 64) * np.einsum("pik,pkj->pij", A, B) + np.uint64(c.beta % 2 ** 64) * C0
        assert np.array_equal(BV.expected(c), v.astype(u).view(c.dtype)), BV.describe(c)


def test_wrapping_reference_agrees_with_the_limb_reference():
    """tests/test_gpu_narrow_int.py's reference() (float64 products of 16-bit limbs) on one case of every type it serves: not two
    unverified models"""
    from tests.test_gpu_narrow_int import reference
    for dt in INTS:
        c = BV.make_case("padded", dt, (4, 65, 67, 33), -3, 1)
        A, B, C0 = BV.operands(c)
        for p in range(c.batch):
            assert np.array_equal(BV.expected(c)[p], reference(np.ascontiguousarray(A[p]), np.ascontiguousarray(B[p]), -3, 1,
                                                               np.ascontiguousarray(C0[p]))), (dt, p)


@pytest.mark.parametrize("dtype", FLOATS, ids=["float32", "float64"])
def test_float_references_do_not_depend_on_the_view(oracle, dtype):
    """the oracle on dense copies of the same values gives the same bits as on the strided, reversed or overlapping views"""
    for c in BV.cases(dtype):
        A, B, C0 = _dense(c)
        want = np.stack([oracle.matmul(A[p], B[p], c.alpha, c.beta, C0[p].copy() if c.beta else np.zeros_like(C0[p]),
                                       isa=oracle.fused_isa(dtype)) for p in range(c.batch)])
        assert np.array_equal(BV.bits(BV.expected(c)), BV.bits(want)), BV.describe(c)


def test_limit_operands_are_exact_in_any_order():
    for dt in (np.float32, np.float64, np.int32):
        A, B, C0, alpha, beta, want = BV.limit_operands(dt, batch=300)
        assert np.abs(A).max() <= 8 and np.abs(B).max() <= 8 and np.abs(C0).max() <= 8
        for p in (0, 299):
            assert np.array_equal(want[p], (alpha * (A.astype(np.float64)[:, ::-1] @ B[p].astype(np.float64)[::-1]) + beta * C0[p]).astype(dt))
