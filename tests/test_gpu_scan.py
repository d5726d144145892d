"""The row cumsum, searchsorted and the inverse-CDF sampler on an MI355X (laser_amd.cumsum / searchsorted / cdfSample /
cdfSampleAndRemove / multinomial(method="cdf") / laser_hip_cumsum_* ...; include/laser_hip.h "Row cumsum, searchsorted and the
inverse-CDF sampler"), bit for bit against the numpy model of tests/scan_model.py: sums compared as integer views, indices with
==.  cumsum at every row length where the kernel changes path (the run, the tile, the switch between a wave and a workgroup
per row) over 1, 3 and 67 rows and four types, in padded, offset and in-place layouts with sentinels; searchsorted on both
sides; draws from a buffer and from the generator; softmax -> cumsum -> cdfSample end to end; the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import scan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

TOP = np.float32(1) - np.float32(2.0 ** -24)      # the largest float32 below 1
KINDS = 6                                          # uniform, 60 % zeros, x 1e30, x 1e-30, denormals, all zero
DTYPES = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i64": np.int64}
BITS = {4: np.uint32, 8: np.uint64}
R = M.run()


def L():
    return laser_amd.lib()


def plan(rows, n, elem=4):
    out = (C.c_int64 * 4)()
    assert L().laser_hip_cumsum_plan(rows, n, elem, 0, out) == 0
    return list(out)


def plan_constant(name):
    import re
    text = open(os.path.join(ROOT, "laser_amd", "csrc", "scan_plan.h")).read()
    return int(re.search(r"#define " + name + r" (\d+)", text).group(1))


# read from scan_plan.h so that collecting this file needs no library; the first test holds them against the library's plan
T = plan_constant("LH_SCAN_LANES") * R             # the tile of the long-row kernel, in elements
SWITCHES = [plan_constant("LH_SCAN_WAVE") * R]     # the last n of every variant but the last one
N_GRID = sorted({1, 2, R - 1, R, R + 1, 2 * R + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 50000, 65537} |
                {n + d for n in SWITCHES for d in (-1, 0, 1)})
# (at most 67 rows and 64 draws a row here; more rows, values and draws than the capped grids hold are in test_gpu_grid_stride.py)


def test_the_grid_covers_the_kernels_bounds():
    assert R in (8, 16, 32) and T == 256 // plan(1, 1 << 24)[1] * R
    for n in (1, 2, R - 1, R, R + 1, 2 * R + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 50000, 65537):
        assert n in N_GRID
    for elem in (4, 8):             # every variant switch the plan reports, the same for both widths, is bracketed
        assert [n for n in range(1, 2 * T + 2) if plan(1, n, elem)[0] != plan(1, n + 1, elem)[0]] == SWITCHES
        assert plan(1, 2 * T + 2, elem)[0] == plan(1, 1 << 24, elem)[0] == plan(1, 1 << 20, elem)[0]
    for n in SWITCHES:
        assert n - 1 in N_GRID and n in N_GRID and n + 1 in N_GRID
    assert {plan(1, n)[0] for n in N_GRID} == {0, 1}                                           # every variant is run
    assert plan(1, T)[3] == 1 and plan(1, T + 1)[3] == 2 and plan(1, 2 * T + 1)[3] == 3        # tiles per row
    assert plan(67, 5)[1] == 4 and plan(67, 5)[2] == 17 and plan(67, T)[1:3] == [1, 67]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(BITS[a.dtype.itemsize]), b.view(BITS[b.dtype.itemsize]))


def rows_of(dtype, rows, n, seed=0):
    rng = np.random.default_rng(1000 * n + rows + seed)
    dt = np.dtype(dtype)
    if dt.kind == "i":
        info = np.iinfo(dt)
        return rng.integers(info.min, info.max, (rows, n), dtype=dt, endpoint=True)               # full range: the sums wrap
    w = rng.uniform(0, 1, (rows, n)).astype(dt)
    for r in range(rows):
        kind = r % KINDS if rows > 1 else n % (KINDS - 1)        # a lone row is never the all-zero one
        if kind == 1:
            w[r][rng.random(n) < 0.6] = 0
        elif kind == 2:
            w[r] *= dt.type(1e30)
        elif kind == 3:
            w[r] *= dt.type(1e-30)
        elif kind == 4:                                             # denormals (and some zeros)
            w[r] = rng.integers(0, 1 << 20, n).astype(BITS[dt.itemsize]).view(dt)
        elif kind == 5:
            w[r] = 0
    return w


_cases = {}


def case(sfx, rows, n):
    """rows and the model's sums, computed once per (type, rows, n) and never written again"""
    key = (sfx, rows, n)
    if key not in _cases:
        x = rows_of(DTYPES[sfx], rows, n)
        want = M.cumsum(x)
        x.setflags(write=False)
        want.setflags(write=False)
        _cases[key] = (x, want)
    return _cases[key]


def dev(a):
    return laser_amd.toTensor(np.ascontiguousarray(a), a.dtype)


def ptr(t, off=0):
    return C.c_void_p(t.unsafe_raw_data() + off * t.dtype.itemsize)


def stream():
    from laser_amd.tensor import _stream
    return _stream()


def sentinel(dt):
    return np.dtype(dt).type(-12345)


def gpu_cumsum(sfx, x, s_off=0, ss=None, d_off=0, ds=None, in_place=False):
    """the sums of `x` through the C entry point in the given layout (offsets and row strides in elements); checks that
    nothing outside a row's n elements was written"""
    rows, n = x.shape
    dt = x.dtype
    ss = n if ss is None else ss
    ds = n if ds is None else ds
    S = sentinel(dt)
    sbuf = np.full(s_off + rows * ss + 4, S, dt)
    for r in range(rows):
        sbuf[s_off + r * ss:s_off + r * ss + n] = x[r]
    dsrc = dev(sbuf)
    if in_place:
        ddst, d_off, ds = dsrc, s_off, ss
    else:
        ddst = dev(np.full(d_off + rows * ds + 4, S, dt))
    rc = getattr(L(), f"laser_hip_cumsum_{sfx}_dev")(ptr(ddst, d_off), ds, ptr(dsrc, s_off), ss, rows, n, stream())
    assert rc == 0, L().laser_hip_last_error()
    out = ddst.to_numpy()
    body = out[d_off:d_off + rows * ds].reshape(rows, ds)
    assert np.all(out[:d_off] == S) and np.all(out[d_off + rows * ds:] == S), "wrote outside the rows"
    assert np.all(body[:, n:] == S), "wrote into the gap between two rows"
    if not in_place:
        assert same_bits(dsrc.to_numpy(), sbuf), "wrote into the source"
    return np.ascontiguousarray(body[:, :n])


@pytest.mark.parametrize("sfx", list(DTYPES))
@pytest.mark.parametrize("n", N_GRID)
def test_cumsum_matches_the_model(n, sfx):
    e = 16 // np.dtype(DTYPES[sfx]).itemsize            # elements of 16 bytes
    pad = (n + e - 1) // e * e + e                      # a row stride that keeps every row on a 16-byte boundary
    for rows in ((1, 3, 67) if n <= 4097 else (1, 3)):
        x, want = case(sfx, rows, n)
        # contiguous; bases off 16 bytes with odd strides; aligned rows with a gap; only the source or only the destination
        # off its boundary; in place, aligned and not
        layouts = [dict(), dict(s_off=1, ss=n + 3, d_off=1, ds=n + 5), dict(ss=pad, ds=pad + e)]
        if rows < 67:
            layouts += [dict(s_off=1, ss=n + 1), dict(d_off=e + 1, ds=pad + 1), dict(in_place=True, ss=pad),
                        dict(in_place=True, s_off=1, ss=n + 3)]
        for lay in layouts:
            got = gpu_cumsum(sfx, x, **lay)
            assert same_bits(got, want), (sfx, n, rows, lay)


def test_cumsum_on_float_rows_is_monotone_and_zero_weights_do_not_move_it():
    for n in (R + 1, T + 1, 50000):
        x, _ = case("f32", 3, n)
        got = laser_amd.cumsum(dev(x)).to_numpy()
        assert np.all(got[:, 1:] >= got[:, :-1]) and np.all((got[:, 1:] == got[:, :-1]) | (x[:, 1:] != 0)), n


def test_cumsum_of_a_row_with_nan_and_inf():
    for sfx in ("f32", "f64"):
        x = rows_of(DTYPES[sfx], 2, 2 * T + 1, seed=5).copy()
        x[0] = np.abs(x[0]) + 1
        x[0, T // 2], x[0, T + 7] = np.inf, np.nan
        x[1, 3], x[1, R], x[1, 2 * T] = -np.inf, np.inf, -0.0
        with np.errstate(invalid="ignore"):
            want = M.cumsum(x)
        got = gpu_cumsum(sfx, x)
        assert np.isinf(want[0, T]) and np.isnan(want[0, -1]) and np.isnan(want[1, -1])
        assert same_bits(got, want), sfx


def test_python_cumsum_takes_tensors_torch_tensors_vectors_and_strided_rows():
    import torch
    x, want = case("f32", 3, 2 * R + 1)
    assert same_bits(laser_amd.cumsum(dev(x)).to_numpy(), want)
    assert same_bits(laser_amd.cumsum(torch.from_numpy(np.array(x)).cuda()).to_numpy(), want)
    one = laser_amd.cumsum(dev(x[1]))                                              # 1-D: one row
    assert one.shape == (2 * R + 1,) and same_bits(one.to_numpy(), want[1])
    wide = torch.from_numpy(np.concatenate([x, x], 1)).cuda()
    assert same_bits(laser_amd.cumsum(wide[:, :2 * R + 1]).to_numpy(), want)      # a row stride above n
    xi, wi = case("i64", 3, R + 1)
    got = laser_amd.cumsum(dev(xi))
    assert got.dtype == np.int64 and np.array_equal(got.to_numpy(), wi) and np.array_equal(wi, np.cumsum(xi, axis=1, dtype=np.int64))
    with pytest.raises(TypeError):
        laser_amd.cumsum(np.array(x))                  # a host array
    with pytest.raises(ValueError):
        laser_amd.cumsum(dev(np.zeros((8, 6), np.float32)).T)                     # the elements of a row must be contiguous
    with pytest.raises(ValueError):
        laser_amd.cumsum(dev(np.zeros((2, 3, 4), np.float32)))


@pytest.mark.parametrize("sfx", list(DTYPES))
def test_searchsorted_matches_the_model(sfx):
    dt = np.dtype(DTYPES[sfx])
    rng = np.random.default_rng(11)
    for n in (1, 2, 5, 64, 1000, 50000):
        for m in (1, 5):
            a = np.sort(rng.integers(-40, 40, (3, n)), axis=1).astype(dt)           # many equal neighbours
            v = rng.integers(-40, 40, (3, m)).astype(dt)
            v[0, 0], v[1, 0], v[2, 0] = a[0, 0] - 1, a[1, -1] + 1, a[2, n // 2]      # below, above, equal
            if m > 1:
                v[0, 1], v[1, 1] = a[0, 0], a[1, -1]
                if dt.kind == "f":
                    v[2, 1], v[2, 2] = a[2, n // 2] + 0.5, np.nan                    # inside a gap; NaN goes left
            for left in (True, False):
                got = laser_amd.searchsorted(dev(a), dev(v), leftSide=left).to_numpy()
                assert got.dtype == np.int32 and got.shape == (3, m)
                assert np.array_equal(got, M.searchsorted(a, v, right=not left)), (sfx, n, m, left)
                ok = ~np.isnan(v.astype(np.float64))
                for r in range(3):
                    assert np.array_equal(got[r][ok[r]], np.searchsorted(a[r], v[r][ok[r]], "left" if left else "right"))
    # one value per row as a vector; an unsorted row: the descent's result, whatever it means
    a = rng.permutation(30).reshape(3, 10).astype(dt)
    v = np.array([4, 15, 29], dt)
    got = laser_amd.searchsorted(dev(a), dev(v)).to_numpy()
    assert got.shape == (3,) and np.array_equal(got, M.searchsorted(a, v))
    # a padded row stride through the C entry point
    n, m = 7, 5
    a = np.sort(rng.integers(0, 9, (3, n)), axis=1).astype(dt)
    v = rng.integers(-1, 10, (3, m)).astype(dt)
    buf = np.full(1 + 3 * (n + 2), sentinel(dt), dt)
    for r in range(3):
        buf[1 + r * (n + 2):1 + r * (n + 2) + n] = a[r]
    da, dv, di = dev(buf), dev(v), laser_amd.newTensor(np.int32, 3, m)
    assert getattr(L(), f"laser_hip_searchsorted_{sfx}_dev")(ptr(di), ptr(da, 1), n + 2, ptr(dv), 3, n, m, 1, stream()) == 0
    assert np.array_equal(di.to_numpy(), M.searchsorted(a, v, right=True))


@pytest.mark.parametrize("sfx", ["i32", "i64"])
def test_searchsorted_passes_the_references_checks(sfx):
    """sanityChecks, bench_multinomial_samplers.nim:63-82"""
    dt = DTYPES[sfx]
    p = dev(np.array([1, 2, 3, 4, 5], dt))
    assert laser_amd.searchsorted(p, dev(np.array([[3]], dt))).to_numpy().tolist() == [[2]]
    assert laser_amd.searchsorted(p, dev(np.array([[3]], dt)), leftSide=False).to_numpy().tolist() == [[3]]
    assert laser_amd.searchsorted(p, dev(np.array([[-10, 10, 2, 3]], dt))).to_numpy().tolist() == [[0, 5, 1, 2]]
    a = dev(np.array([[0, 3, 9, 9, 10], [1, 2, 3, 4, 5]], dt))
    v = dev(np.array([[2, 4, 9], [0, 2, 6]], dt))
    assert laser_amd.searchsorted(a, v).to_numpy().tolist() == [[1, 2, 2], [0, 1, 5]]
    assert laser_amd.searchsorted(a, v, leftSide=False).to_numpy().tolist() == [[1, 2, 4], [0, 2, 5]]


def special_rows(n):
    """the KINDS kinds, a NaN row, an Inf row and a sparse row; which rows must give -1"""
    w = rows_of(np.float32, KINDS + 3, n, seed=7).copy()
    w[KINDS, n // 2] = np.nan
    w[KINDS + 1, n - 1] = np.inf
    w[KINDS + 2][np.random.default_rng(n).random(n) < 0.9] = 0
    with np.errstate(invalid="ignore"):
        total = M.cumsum(w)[:, -1]
    dead = ~(np.isfinite(total) & (total > 0))
    assert dead[5] and dead[KINDS] and dead[KINDS + 1]
    return w, dead


def uniforms(rows, m, seed):
    u = np.random.default_rng(seed).random((rows, m), dtype=np.float32)
    if m >= 2:
        u[:, 0], u[:, -1] = 0, TOP
    else:
        u[0::2, 0], u[1::2, 0] = 0, TOP
    return u


@pytest.mark.parametrize("n", [1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 1000, 1025, 4097, 50000])
def test_cdf_sample_matches_the_model(n):
    w, dead = special_rows(n)
    rows = w.shape[0]
    with np.errstate(invalid="ignore"):
        want_cdf = M.cumsum(w)
    cdf = laser_amd.cumsum(dev(w))
    assert same_bits(cdf.to_numpy(), want_cdf)
    live = np.flatnonzero(~dead)
    for m in (1, 7, 64):
        u = uniforms(rows, m, 31 * n + m)
        idx = laser_amd.cdfSample(cdf, u, num=m).to_numpy()
        assert idx.dtype == np.int32 and idx.shape == (rows, m)
        assert np.array_equal(idx, M.draw(want_cdf, u)), (n, m)
        assert np.all(idx[dead] == -1) and np.all(idx[~dead] >= 0) and np.all(idx[~dead] < n)
        assert np.all(np.take_along_axis(w[live], idx[live].astype(np.int64), 1) > 0), (n, m)
    assert same_bits(cdf.to_numpy(), want_cdf), "the draw wrote into the CDF"


def test_cdf_sample_at_a_denormal_total_takes_the_last_branch():
    tiny = np.float32(2.0 ** -149)
    w = np.array([[0, tiny, 0, 0, 0], [tiny, 0, tiny, 0, 0]], np.float32)
    u = np.array([[TOP, 0, 0.5], [TOP, 0, 0.25]], np.float32)
    want, past = M.draw(M.cumsum(w), u, branch=True)
    assert past[:, 0].all()
    got = laser_amd.cdfSample(laser_amd.cumsum(dev(w)), u, num=3).to_numpy()
    assert np.array_equal(got, want) and got[:, 0].tolist() == [1, 2]


def test_cdf_sample_from_a_padded_offset_cdf():
    n = 1025
    w, dead = special_rows(n)
    rows = w.shape[0]
    with np.errstate(invalid="ignore"):
        cdf = M.cumsum(w)
    buf = np.full(1 + rows * (n + 3), np.float32(-1), np.float32)
    for r in range(rows):
        buf[1 + r * (n + 3):1 + r * (n + 3) + n] = cdf[r]
    u = uniforms(rows, 16, 5)
    dc, du, di = dev(buf), dev(u), laser_amd.newTensor(np.int32, rows, 16)
    assert L().laser_hip_cdf_sample_f32_dev(ptr(di), ptr(dc, 1), n + 3, ptr(du), rows, n, 16, stream()) == 0
    assert np.array_equal(di.to_numpy(), M.draw(cdf, u))


def test_rng_forms_equal_a_fill_followed_by_the_buffer_forms():
    n = 1000
    w, dead = special_rows(n)
    rows = w.shape[0]
    dw = dev(w)
    cdf = laser_amd.cumsum(dw)
    for m, offset in ((1, 0), (5, 3), (64, (1 << 40) + 1)):
        rng = laser_amd.Rng(9, 2, offset)
        ubuf = laser_amd.newTensor(np.float32, rows, m)
        assert L().laser_hip_random_uniform_f32_dev(ptr(ubuf), rows * m, 0.0, 1.0, 9, 2, offset, stream()) == 0
        host_u = ubuf.to_numpy()
        got = laser_amd.cdfSample(cdf, rng=rng, num=m).to_numpy()
        assert rng.offset == offset + rows * m
        assert np.array_equal(got, laser_amd.cdfSample(cdf, ubuf, num=m).to_numpy())
        with np.errstate(invalid="ignore"):
            assert np.array_equal(got, M.draw(M.cumsum(w), host_u)), (m, offset)
        rng = laser_amd.Rng(9, 2, offset)
        rem = laser_amd.cdfSampleAndRemove(dw, rng=rng, num=m).to_numpy()
        assert rng.offset == offset + rows * m
        assert np.array_equal(rem, laser_amd.cdfSampleAndRemove(dw, ubuf, num=m).to_numpy())
        with np.errstate(invalid="ignore"):
            assert np.array_equal(rem, M.draw_remove(w.copy(), host_u)), (m, offset)
    with pytest.raises(ValueError):
        laser_amd.cdfSample(cdf, uniforms(rows, 2, 1), num=2, rng=laser_amd.Rng(1))      # u xor rng
    with pytest.raises(TypeError):
        laser_amd.cdfSample(cdf, num=2, rng=np.random.default_rng(1))


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 1025])
def test_cdf_sample_and_remove_matches_the_model(n):
    w = rows_of(np.float32, 7, n, seed=3)
    for k in (1, 10, n + 2) if n <= 65 else (10,):
        u = uniforms(7, k, 17 * n + k)
        dw = dev(w)
        idx = laser_amd.cdfSampleAndRemove(dw, u, num=k).to_numpy()
        assert same_bits(dw.to_numpy(), w), "the caller's weights were written"
        assert np.array_equal(idx, M.draw_remove(w.copy(), u)), (n, k)
        for r in range(7):
            drawn = idx[r][idx[r] >= 0]
            assert len(set(drawn.tolist())) == drawn.size and np.all(w[r, drawn] > 0)
        assert np.all(idx[:, n:] == -1)                                             # columns s >= n
        if k == n + 2:
            pos = (w > 0).sum(1)
            for r in range(7):          # every positive element once, then -1
                assert sorted(idx[r, :pos[r]].tolist()) == np.flatnonzero(w[r] > 0).tolist() and np.all(idx[r, pos[r]:] == -1)


def test_ten_draws_from_four_positive_weights_end_in_six_minus_ones():
    w = np.zeros((2, 2 * T + 1), np.float32)
    w[0, [3, R, T, 2 * T]] = [0.5, 2, 0.25, 1]
    w[1, [0, 1, 2, 3]] = 1
    keep = w.copy()
    dw = dev(w)
    idx = laser_amd.cdfSampleAndRemove(dw, uniforms(2, 10, 3), num=10).to_numpy()
    assert sorted(idx[0, :4].tolist()) == [3, R, T, 2 * T] and sorted(idx[1, :4].tolist()) == [0, 1, 2, 3]
    assert np.all(idx[:, 4:] == -1)
    assert same_bits(dw.to_numpy(), keep), "the caller's array was changed"
    # the C entry point overwrites the weights it is given: the drawn elements become +0
    cdf, di, du = laser_amd.newTensor(np.float32, 2, 2 * T + 1), laser_amd.newTensor(np.int32, 2, 10), dev(uniforms(2, 10, 3))
    n = 2 * T + 1
    assert L().laser_hip_cdf_sample_remove_f32_dev(ptr(di), ptr(dw), n, ptr(cdf), n, ptr(du), 2, n, 10, stream()) == 0
    assert np.array_equal(di.to_numpy(), idx)
    after = dw.to_numpy()
    assert np.all(after == 0) and not np.signbit(after).any()


def test_softmax_to_cumsum_to_cdf_sample_end_to_end():
    import torch
    rng = np.random.default_rng(11)
    logits = rng.uniform(-8, 8, (3, 1000)).astype(np.float32)
    p = laser_amd.softmax(dev(logits))
    host_p = p.to_numpy()
    u = uniforms(3, 4, 12)
    cdf = laser_amd.cumsum(p)
    assert same_bits(cdf.to_numpy(), M.cumsum(host_p))
    want = M.draw(M.cumsum(host_p), u)
    assert np.array_equal(laser_amd.cdfSample(cdf, u, num=4).to_numpy(), want)
    assert np.array_equal(laser_amd.multinomial(p, 4, replacement=True, u=u, method="cdf").to_numpy(), want)
    got = laser_amd.multinomial(p, num_samples=4, u=u, method="cdf").to_numpy()
    assert np.array_equal(got, M.draw_remove(host_p.copy(), u)) and all(len(set(r.tolist())) == 4 for r in got)
    assert same_bits(p.to_numpy(), host_p)
    # the default method is the F+tree, as before; both draw in proportion to the same weights
    tp = torch.from_numpy(host_p).cuda()
    assert np.array_equal(laser_amd.multinomial(tp, 4, u=u).to_numpy(), laser_amd.multinomial(tp, 4, u=u, method="ftree").to_numpy())
    drawn = laser_amd.multinomial(tp, 4, method="cdf").to_numpy()
    assert drawn.shape == (3, 4) and drawn.min() >= 0 and drawn.max() < 1000 and all(len(set(r.tolist())) == 4 for r in drawn)
    assert laser_amd.multinomial(tp, 0, method="cdf").to_numpy().shape == (3, 0)
    with pytest.raises(ValueError):
        laser_amd.multinomial(tp, 1, method="alias")


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "scan_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "scan_mirror.cpp"), "-o", exe, "-L", lib, "-llaser_hip",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
