"""tests/poison_views.py itself, no device: the poisoned arenas differ from the clean ones exactly where they should, no clean
value is a zero (a NaN x 0 would then enter the expected classes), the expected classes are whole rows and columns, and at least
60 % of every case stays finite and therefore compared bit for bit."""
import numpy as np
import pytest

from tests import batched_views as BV
from tests import poison_views as PV

FLOATS = [np.float32, np.float64]


def _groups(dtype):
    """one case per (layout, shape): the arenas do not depend on alpha / beta"""
    return BV.cases(dtype, scalar_list=[(1, 0)])


@pytest.mark.parametrize("dtype", FLOATS, ids=["float32", "float64"])
def test_poison_values_are_all_non_finite_and_of_every_kind(dtype):
    p = PV.poison(600, dtype)
    assert not np.isfinite(p).any()
    assert np.isposinf(p).sum() == 100 and np.isneginf(p).sum() == 100
    heads = BV.bits(p[np.isnan(p)]) >> (23 if np.dtype(dtype).itemsize == 4 else 52)
    assert len(set(heads.tolist())) == 2 and len(set(BV.bits(p).tolist())) > 100      # both signs, many payloads
    sent = BV.NAN_SENTINEL[np.dtype(dtype).itemsize]
    assert not (BV.bits(p) == sent).any()
    assert PV.classify(np.array([1.0, np.nan, np.inf, -np.inf], dtype)).tolist() == [PV.FINITE, PV.NAN, PV.PINF, PV.NINF]


@pytest.mark.parametrize("dtype", FLOATS, ids=["float32", "float64"])
def test_gap_poison_is_the_complement_of_the_addressed_elements(dtype):
    for c in _groups(dtype):
        a, b, _, _ = BV.arenas(c)
        ga, gb = PV.gap_poisoned(c)
        for clean, got, v, which in ((a, ga, c.A, "A"), (b, gb, c.B, "B")):
            rows, cols = BV.dims(c, which)
            mask = PV.addressed_mask(v, c.batch, rows, cols, clean.size)
            what = f"{which} of {BV.describe(c)}"
            assert got.dtype == clean.dtype and got.shape == clean.shape, what
            assert np.array_equal(BV.bits(got)[mask], BV.bits(clean)[mask]), what
            assert not np.isfinite(got[~mask]).any(), what
            assert (~mask).sum() >= 2 * BV.matrix_span(v.strides, rows, cols), what      # the slack on both sides, at the least
            kinds = set(PV.classify(got[~mask]).tolist())
            assert kinds == {PV.NAN, PV.PINF, PV.NINF}, what
            assert (clean[mask] != 0).all(), f"{what}: an addressed clean value is a zero"
            assert not got.flags.writeable


def test_gap_poison_fills_the_gaps_each_layout_has():
    """padded: the leading-dimension gap after every row; b_transposed / transposed: the K + 4 pitch; interleaved and
    negative_inner address a dense block of A, so their poison is the slack at both ends"""
    sh = (3, 130, 70, 517)
    c = BV.make_case("padded", np.float32, sh, 1, 0)
    ga, gb = PV.gap_poisoned(c)
    assert not np.isfinite(ga[c.A.offset + c.K:c.A.offset + c.K + 3]).any() and np.isfinite(ga[c.A.offset + c.K + 3])
    assert not np.isfinite(gb[c.B.offset + c.N:c.B.offset + c.N + 5]).any() and np.isfinite(gb[c.B.offset + c.N + 5])
    for lay in ("transposed", "b_transposed"):
        c = BV.make_case(lay, np.float32, sh, 1, 0)
        _, gb = PV.gap_poisoned(c)
        assert not np.isfinite(gb[c.B.offset + c.K:c.B.offset + c.K + 4]).any() and np.isfinite(gb[c.B.offset + c.K + 4])
    c = BV.make_case("interleaved", np.float32, sh, 1, 0)
    ga, _ = PV.gap_poisoned(c)
    assert np.isfinite(ga[c.A.offset:c.A.offset + c.batch]).all()            # batch stride 1: the entries fill the gaps themselves
    assert not np.isfinite(ga[c.A.offset - 1]) and not np.isfinite(ga[c.A.offset + c.batch * c.M * c.K])
    c = BV.make_case("negative_inner", np.float32, sh, 1, 0)
    ga, _ = PV.gap_poisoned(c)
    top = c.A.offset + (c.batch - 1) * c.M * c.K                            # rows and k run downwards from each entry's base
    assert np.isfinite(ga[c.A.offset - c.M * c.K + 1:top + 1]).all()
    assert not np.isfinite(ga[c.A.offset - c.M * c.K]) and not np.isfinite(ga[top + 1])


@pytest.mark.parametrize("dtype", FLOATS, ids=["float32", "float64"])
def test_element_poison_touches_the_chosen_elements_only_and_rows_and_columns_follow(dtype):
    for c in BV.cases(dtype, scalar_list=[(1, 0), (0.5, 0.25)]):
        what = BV.describe(c)
        a, b, _, _ = BV.arenas(c)
        ea, eb, special = PV.element_poisoned(c)
        pa, pb = PV.element_positions(c)
        assert bool(pa) == (c.M >= 8) and bool(pb) == (c.N >= 8), what
        for clean, got, v, which, pos in ((a, ea, c.A, "A", pa), (b, eb, c.B, "B", pb)):
            rows, cols = BV.dims(c, which)
            off = BV.element_offsets(v, c.batch, rows, cols)
            hit = np.zeros(clean.size, dtype=bool)
            for (r, k) in pos:
                hit[off[:, r, k]] = True
            assert np.array_equal(BV.bits(got)[~hit], BV.bits(clean)[~hit]), what
            assert not np.isfinite(got[hit]).any(), what
            assert hit.sum() <= 2 * c.batch
        A, B = BV.gather(ea, c.A, c.batch, c.M, c.K), BV.gather(eb, c.B, c.batch, c.K, c.N)
        nan_row, nan_col = np.isnan(A).any(axis=2), np.isnan(B).any(axis=1)          # [batch][M], [batch][N]
        inf_col = np.isinf(B).any(axis=1) & ~nan_col
        want_nan = nan_row[:, :, None] | nan_col[:, None, :]
        assert special.shape == (c.batch, c.M, c.N) and not special.flags.writeable
        assert np.array_equal(special == PV.NAN, want_nan), what
        # a +Inf of B times a non-zero finite A[i, K - 1]: the column is an infinity of that element's sign wherever it is not NaN
        inf = (special == PV.PINF) | (special == PV.NINF)
        assert np.array_equal(inf, inf_col[:, None, :] & ~want_nan), what
        if pb and pa:
            sign = np.where(A[:, :, c.K - 1] > 0, PV.PINF, PV.NINF)
            col = special[:, :, c.N - 1]
            assert np.array_equal(col[col != PV.NAN], sign[col != PV.NAN]), what
        assert PV.finite_share(special) >= PV.CAP, f"{what}: {PV.finite_share(special):.3f} of C expected finite"
        if c.M < 8 and c.N < 8:
            assert (special == PV.FINITE).all(), what
        elif c.M >= 8 and c.N >= 8:
            assert nan_row.sum(axis=1).min() >= 2 and nan_col.sum(axis=1).min() >= 1 and inf_col.sum(axis=1).min() >= 1, what


def test_check_result_sees_each_kind_of_deviation():
    clean = np.arange(1, 7, dtype=np.float32).reshape(2, 3)
    special = np.array([[PV.FINITE, PV.NAN, PV.PINF], [PV.NINF, PV.FINITE, PV.FINITE]], dtype=np.int8)
    good = clean.copy()
    good[0, 1], good[0, 2], good[1, 0] = np.nan, np.inf, -np.inf
    assert PV.check_result(good, clean, special) is None
    for at, value in (((0, 0), np.nan), ((1, 1), 5.0000005), ((0, 1), 2.0), ((0, 2), -np.inf), ((0, 2), np.nan), ((1, 0), np.inf)):
        bad = good.copy()
        bad[at] = value
        assert PV.check_result(bad, clean, special) is not None, (at, value)
    neg = good.copy()
    neg[1, 2] = -0.0
    zero = clean.copy()
    zero[1, 2] = 0.0
    assert PV.check_result(neg, zero, special) is not None          # bit patterns, not values


@pytest.mark.parametrize("geometry", PV.CONV_GEOMETRIES, ids=[f"{g[0]}-{g[1]}".replace(" ", "") for g in PV.CONV_GEOMETRIES])
def test_conv_poison(geometry):
    ishape, kshape, pad, st = geometry
    n, C, H, W = ishape
    p = PV.conv_poison(ishape, kshape, pad, st, seed=5)
    assert p.x.dtype == p.w.dtype == p.bias.dtype == np.float32
    assert (p.x != 0).all() and (p.w != 0).all() and (p.bias != 0).all()
    assert np.isfinite(p.x).all() and np.isfinite(p.w).all()
    hit = ~np.isfinite(p.x_poison)
    assert 4 <= hit.sum() <= 5 and np.array_equal(BV.bits(p.x_poison)[~hit], BV.bits(p.x)[~hit])
    assert np.isnan(p.x_poison[0, 0, 0, 0]) and np.isnan(p.x_poison[n - 1, C - 1, H - 1, W - 1]) and np.isposinf(p.x_poison).sum() == 1
    assert n == 1 or np.isnan(p.x_poison[1, 0, 0, 0])
    oH, oW = (H + 2 * pad[0] - kshape[2]) // st[0] + 1, (W + 2 * pad[1] - kshape[3]) // st[1] + 1
    assert p.special.shape == (n, kshape[0], oH, oW)
    assert (PV.classify(PV.conv_reference(p.x, p.w, pad, st, p.bias)) == PV.FINITE).all()
    # a poisoned pixel reaches an output pixel of every channel or of none: the classes' NaN map is the same over c_out
    assert (p.special != PV.FINITE).any() and ((p.special == PV.NAN) == (p.special[:, :1] == PV.NAN)).all()
    assert p.special[0, :, 0, 0].tolist() == [PV.NAN] * kshape[0]
    assert PV.finite_share(p.special) >= PV.CAP, PV.finite_share(p.special)
    if pad == (0, 0):
        assert np.isnan(p.w_poison).sum() == 1 and np.isnan(p.w_poison[p.w_channel, C - 1, kshape[2] - 1, kshape[3] - 1])
        want = np.zeros(p.w_special.shape, dtype=bool)
        want[:, p.w_channel] = True
        assert np.array_equal(p.w_special == PV.NAN, want) and (p.w_special[~want] == PV.FINITE).all()
        assert PV.finite_share(p.w_special) >= PV.CAP
    else:
        assert p.w_poison is None and p.w_special is None
    buf, start = PV.guarded(p.x)
    assert start % 64 == 0 and start == PV.GUARD and buf.size == p.x.size + 2 * PV.GUARD
    assert np.array_equal(BV.bits(buf[start:start + p.x.size]), BV.bits(p.x.ravel()))
    assert not np.isfinite(buf[:start]).any() and not np.isfinite(buf[start + p.x.size:]).any()
