"""llog, logsumexp, log-softmax and the softmax cross-entropy on an MI355X (laser_amd.log / logsumexp / log_softmax /
softmax_cross_entropy, laser_log in forEach bodies; include/laser_hip.h "log, logsumexp, log-softmax and cross-entropy"), bit
for bit against the numpy model of tests/log_model.py: every row length at which the kernels change path, for 1, 3, 4, 5 and 9
rows, two grid-stride cases, an offset base, odd and padded row strides, in place; rows with a wide spread, ties for the
maximum, one +Inf, all -Inf and a NaN first, in the middle and last; labels 0, n - 1, the argmax, another one, -1, -2 and n.
The model of the nine rows of a length is computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import laser_amd
from tests import exp_model as E
from tests import log_model as G

pytestmark = pytest.mark.gpu

NS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 16385]
ROWS = [1, 3, 4, 5, 9]      # (past the cap of 2048 workgroups: the two cases below; the long-row kernel's: test_gpu_grid_stride.py)
SENTINEL = np.float32(-12345.0)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the shared rows are read-only


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not E.same_bits(got, want):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


@functools.lru_cache(maxsize=None)
def rows_of(n):
    """nine rows of length n: 0 plain (+-80), 1 ties for the maximum, 2 one +Inf, 3 all -Inf, 4 - 6 a NaN first, in the middle,
    last, 7 - 8 plain; read-only"""
    rng = np.random.default_rng(1000 + n)
    x = rng.uniform(-80, 80, (9, n)).astype(np.float32)
    x[1, :: max(1, n // 3)] = np.float32(80)
    x[2, n // 2] = np.inf
    x[3] = -np.inf
    x[4, 0] = np.nan
    x[5, n // 2] = np.nan
    x[6, n - 1] = np.nan
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def labels_of(n, which):
    """nine labels: the argmax, n - 1, 0, one that is not the argmax, -1, -2, n, 0, n - 1; `which` rotates them over the rows"""
    x = rows_of(n)
    with np.errstate(all="ignore"):
        am = int(np.argmax(np.where(np.isnan(x[0]), -np.inf, x[0])))
    base = np.array([am, n - 1, 0, (am + 1) % n, -1, -2, n, 0, n - 1], np.int32)
    lab = np.roll(base, which)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def model(n):
    x = rows_of(n)
    return G.logsumexp_rows(x), G.log_softmax_rows(x)


@functools.lru_cache(maxsize=None)
def model_xent(n, which, scale=1.0):
    return G.xent_rows(rows_of(n), labels_of(n, which), scale)


def strided(x, stride, offset, fill=None):
    """a device view (rows, n) with row stride `stride` whose base is `offset` elements into a fresh buffer filled with the
    sentinel (then with x, or left when fill is False); returns (buffer, view)"""
    import torch
    rows, n = x.shape
    buf = torch.full((offset + rows * stride,), float(SENTINEL), device="cuda")
    view = buf[offset:].view(rows, stride)[:, :n]
    if fill is not False:
        view.copy_(torch.from_numpy(np.array(x)))
    return buf, view


def untouched(buf, offset, rows, stride, n):
    """everything of the buffer outside the view still holds the sentinel"""
    b = buf.cpu().numpy()
    m = np.ones(b.size, bool)
    for r in range(rows):
        m[offset + r * stride: offset + r * stride + n] = False
    return bool((b[m] == SENTINEL).all())


def run_all(x, lab, src, what, lsm_out=None, grad_view=None):
    """the three row calls on the device view `src` of x against the model of its rows"""
    rows, n = x.shape
    lse, lsm = (a[:rows] for a in model(n))
    assert_bits(laser_amd.logsumexp(src).to_numpy(), lse, f"logsumexp {what}")
    if lsm_out is None:
        assert_bits(laser_amd.log_softmax(src).to_numpy(), lsm, f"log_softmax {what}")
    else:
        laser_amd.log_softmax(src, out=lsm_out)
        assert_bits(lsm_out.cpu().numpy(), lsm, f"log_softmax {what}")
    for which in lab:
        labels = labels_of(n, which)[:rows]
        wl, wg = (a[:rows] for a in model_xent(n, which))
        loss, grad = laser_amd.softmax_cross_entropy(src, dev(labels), grad=True)
        assert_bits(loss.to_numpy(), wl, f"loss {what}, labels {labels}")
        assert_bits(grad.to_numpy(), wg, f"grad {what}, labels {labels}")
        assert_bits(laser_amd.softmax_cross_entropy(src, dev(labels)).to_numpy(), wl, f"loss alone {what}")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", NS)
def test_rows_match_the_model(n, rows):
    x = rows_of(n)[:rows]
    run_all(x, (0, 4, 5), dev(x), f"n={n} rows={rows}")


@pytest.mark.parametrize("n", NS)
def test_offset_base_odd_and_padded_strides_and_in_place(n):
    x = rows_of(n)[:5]
    rows = 5
    odd = n + 1 + (n % 2)                 # an odd row stride: single-element accesses
    pad = (n + 3) // 4 * 4 + 4            # a multiple of 4 past n: vectors, with a gap between the rows
    for stride, offset, name in ((n, 1, "base off by one element"), (odd, 0, "odd row stride"), (pad, 0, "padded row stride"),
                                 (pad, 4, "padded, base 16 bytes in")):
        sbuf, src = strided(x, stride, offset)
        obuf, out = strided(x, stride, offset, fill=False)
        run_all(x, (0,), src, f"n={n} {name}", lsm_out=out)
        assert untouched(obuf, offset, rows, stride, n), f"log_softmax wrote outside its rows: n={n} {name}"
        assert_bits(src.cpu().numpy(), x, f"the source is left alone: n={n} {name}")
        laser_amd.log_softmax(src, out=src)
        assert_bits(src.cpu().numpy(), model(n)[1][:rows], f"dst == src: n={n} {name}")
        assert untouched(sbuf, offset, rows, stride, n), f"in place wrote outside its rows: n={n} {name}"


def test_gradient_and_loss_alone_through_the_c_abi_with_strides_and_scale():
    """d_loss or d_grad NULL, a loss stride of 3, a padded gradient, scale = 1 / rows"""
    import torch
    L = laser_amd.lib()
    for n in (5, 1025, 8193):
        x = rows_of(n)
        rows = 9
        labels = labels_of(n, 2)
        scale = np.float32(1.0) / np.float32(rows)
        wl, wg = G.xent_rows(x, labels, scale)
        src, lab = dev(x), dev(labels)
        gs = n + 3
        gbuf = torch.full((rows * gs,), float(SENTINEL), device="cuda")
        lbuf = torch.full((rows * 3,), float(SENTINEL), device="cuda")
        vp = C.c_void_p
        assert L.laser_hip_softmax_xent_rows_f32_dev(None, 0, vp(gbuf.data_ptr()), gs, vp(src.data_ptr()), n, vp(lab.data_ptr()), rows,
                                                     n, float(scale), None) == 0
        assert L.laser_hip_softmax_xent_rows_f32_dev(vp(lbuf.data_ptr()), 3, None, 0, vp(src.data_ptr()), n, vp(lab.data_ptr()), rows,
                                                     n, float(scale), None) == 0
        g = gbuf.cpu().numpy().reshape(rows, gs)
        assert_bits(g[:, :n], wg, f"grad alone, n={n}")
        assert (g[:, n:] == SENTINEL).all()
        lo = lbuf.cpu().numpy().reshape(rows, 3)
        assert_bits(lo[:, 0], wl, f"loss alone, n={n}")
        assert (lo[:, 1:] == SENTINEL).all()
        assert L.laser_hip_softmax_xent_rows_f32_dev(None, 0, None, 0, vp(src.data_ptr()), n, vp(lab.data_ptr()), rows, n, 1.0,
                                                     None) == laser_amd._lib.E_INVALID


@pytest.mark.parametrize("rows,n", [(4 * 2048 + 5, 5), (2048 + 2, 1025)])
def test_more_rows_than_the_grid_has_workgroups(rows, n):
    """workgroups stride over the rows: 13 distinct rows (13 is coprime to 4 and 2048) repeated, so the model runs 13 times"""
    period = 13
    rng = np.random.default_rng(rows)
    base = rng.uniform(-80, 80, (period, n)).astype(np.float32)
    lab13 = rng.integers(-1, n + 1, period).astype(np.int32)
    idx = np.arange(rows) % period
    x, labels = base[idx], lab13[idx]
    lse, lsm = G.logsumexp_rows(base), G.log_softmax_rows(base)
    wl, wg = G.xent_rows(base, lab13)
    plan = (C.c_int64 * 3)()
    assert laser_amd.lib().laser_hip_softmax_rows_plan(rows, n, 1, plan) == 0 and plan[1] == 2048
    src = dev(x)
    assert_bits(laser_amd.logsumexp(src).to_numpy(), lse[idx], "logsumexp")
    assert_bits(laser_amd.log_softmax(src).to_numpy(), lsm[idx], "log_softmax")
    loss, grad = laser_amd.softmax_cross_entropy(src, dev(labels), grad=True)
    assert_bits(loss.to_numpy(), wl[idx], "loss")
    assert_bits(grad.to_numpy(), wg[idx], "grad")


# ---- properties -----------------------------------------------------------------------------------------------------------
def test_log_softmax_survives_where_log_of_softmax_does_not():
    """log_softmax([0, -200]) is [0, -200]; the log of the existing softmax of the same row is not.  (lexp clamps its
    argument at -88 as Laser's does, so that softmax is a subnormal 3.5e-40, not 0, and its log is -90.8355, not -Inf: the
    naive route is wrong by 109, and has the bits the models of softmax and llog give it.)"""
    x = np.float32([[0, -200]])
    y = laser_amd.log_softmax(dev(x)).to_numpy()
    assert y[0, 0] == 0 and y[0, 1] == np.float32(-200)
    naive = laser_amd.log(laser_amd.softmax(dev(x))).to_numpy()
    assert_bits(naive, G.llog(E.softmax_rows(x)), "log of softmax")
    assert naive[0, 0] == 0 and naive[0, 1] > -91 and naive[0, 1] != y[0, 1]
    assert laser_amd.logsumexp(dev(x)).to_numpy()[0] == 0


def test_every_finite_log_softmax_value_is_at_most_zero():
    rng = np.random.default_rng(7)
    for n in (3, 700, 5000, 20000):
        x = (rng.uniform(-1, 1, (16, n)) * rng.choice([1e-3, 1.0, 30.0, 1e4], (16, 1))).astype(np.float32)
        y = laser_amd.log_softmax(dev(x)).to_numpy()
        assert np.isfinite(y).all() and (y <= 0).all(), n
    for n in NS:
        y = laser_amd.log_softmax(dev(rows_of(n))).to_numpy()
        f = np.isfinite(y)
        assert (y[f] <= 0).all(), n


def test_gradient_off_the_label_has_the_bits_of_softmax_and_loss_is_minus_log_softmax():
    """with scale = 1 every non-label element of grad is softmax's, bit for bit; the loss has the bits of 0 - log_softmax[label]
    (the negation taken as a subtraction from +0, so that a row whose sum is 1 keeps its +0)"""
    for n in (4, 257, 1025, 8193):
        x = rows_of(n)[[0, 1, 7, 8]]
        labels = np.array([0, n - 1, n // 2, 1 % n], np.int32)
        src = dev(x)
        sm = laser_amd.softmax(src).to_numpy()
        lsm = laser_amd.log_softmax(src).to_numpy()
        loss, grad = laser_amd.softmax_cross_entropy(src, dev(labels), grad=True, scale=1.0)
        loss, grad = loss.to_numpy(), grad.to_numpy()
        off = np.ones(x.shape, bool)
        off[np.arange(4), labels] = False
        assert np.array_equal(grad.view(np.uint32)[off], sm.view(np.uint32)[off]), n
        on = (sm[np.arange(4), labels] - np.float32(1)).astype(np.float32)
        assert np.array_equal(grad[np.arange(4), labels].view(np.uint32), on.view(np.uint32)), n
        want = (np.float32(0) - lsm[np.arange(4), labels]).astype(np.float32)
        assert np.array_equal(loss.view(np.uint32), want.view(np.uint32)), (n, loss, want)
    one = laser_amd.softmax_cross_entropy(dev(np.float32([[3.5]])), dev(np.int32([0]))).to_numpy()
    assert one.view(np.uint32)[0] == 0                       # a row of one element: the loss is +0


# ---- log ------------------------------------------------------------------------------------------------------------------
def values():
    rng = np.random.default_rng(31)
    bits = rng.integers(0, 2 ** 32, 20001, dtype=np.uint64).astype(np.uint32).view(np.float32)
    near = (1 + rng.uniform(-0.3, 0.4, 5000)).astype(np.float32)
    return np.concatenate([G.edges(), bits, near, np.abs(bits[:5000])])


def test_log_edges_random_bit_patterns_and_the_host_form():
    x = values()
    want = G.llog(x)
    got = laser_amd.log(dev(x)).to_numpy()
    assert_bits(got, want, "device")
    assert got[x == 1].view(np.uint32).tolist() == [0] * int((x == 1).sum())        # llog(1) = +0
    assert (got[x == 0] == -np.inf).all() and np.isnan(got[x < 0]).all() and (got[x == np.inf] == np.inf).all()
    assert_bits(laser_amd.log(x), want, "host pointers")
    for n in (1, 3, 4, 5, 1023):
        d = dev(x[: n + 1])
        assert_bits(laser_amd.log(d[1:]).to_numpy(), want[1: n + 1], f"n={n}, base off by one element")


def test_log_on_strided_views_and_laser_log_in_foreach_bodies():
    rng = np.random.default_rng(32)
    x = np.abs(rng.integers(0, 2 ** 31, (37, 53), dtype=np.int64).astype(np.uint32).view(np.float32))
    x[3, 4], x[5, 6], x[7, 8] = 0, -1, np.inf
    want = G.llog(x)
    t = laser_amd.toTensor(x)
    assert_bits(laser_amd.log(t.T).to_numpy(), want.T, "transposed source")
    assert_bits(laser_amd.log(t[::-1, ::-1]).to_numpy(), want[::-1, ::-1], "negative strides")
    assert_bits(laser_amd.log(t[::2, 1::3]).to_numpy(), want[::2, 1::3], "steps")
    out = laser_amd.newTensor(np.float32, 53, 37)
    laser_amd.log(t, out=out.T)
    assert_bits(out.to_numpy(), want.T, "transposed destination")
    row = laser_amd.toTensor(x[3])
    out = laser_amd.newTensor(np.float32, 5, 53)
    laser_amd.log(row, out=out)
    assert_bits(out.to_numpy(), np.broadcast_to(want[3], (5, 53)), "broadcast source")
    ty = laser_amd.newTensor(np.float32, 37, 53)
    laser_amd.forEach("y = laser_log(x)", y=ty, x=t)
    assert_bits(ty.to_numpy(), want, "forEach body = the model")
    laser_amd.forEach("y = laser_log(x)", y=ty.T, x=t.T)
    assert_bits(ty.to_numpy(), want, "forEach body on strided views")
    v = values()
    tv = laser_amd.toTensor(v)
    s = laser_amd.forEachReduce("acc = fmaxf(acc, laser_log(x))", merge="acc = fmaxf(acc, other)", init=np.float32(-np.inf), x=tv)
    with np.errstate(all="ignore"):
        assert np.float32(s) == np.nanmax(G.llog(v))
    laser_amd.log(t, out=t)
    assert_bits(t.to_numpy(), want, "dst == src")


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_axis_is_taken_only_where_the_rows_are_contiguous():
    x = rows_of(257)[[0, 1, 7, 8]]
    lse, lsm = (a[[0, 1, 7, 8]] for a in model(257))
    d = dev(x)
    assert_bits(laser_amd.logsumexp(d, axis=1).to_numpy(), lse, "axis = 1")
    assert_bits(laser_amd.log_softmax(d, axis=-1).to_numpy(), lsm, "axis = -1")
    # the transposed view (257, 4) with strides (1, 257): its axis 0 is the contiguous one
    assert_bits(laser_amd.logsumexp(d.T, axis=0).to_numpy(), lse, "a transposed view whose axis is contiguous")
    c = dev(x.reshape(2, 2, 257))
    assert_bits(laser_amd.logsumexp(c, axis=2).to_numpy(), lse.reshape(2, 2), "rank 3, last axis")
    assert_bits(laser_amd.log_softmax(c, axis=2).to_numpy(), lsm.reshape(2, 2, 257), "rank 3, last axis")
    for fn in (laser_amd.logsumexp, laser_amd.log_softmax):
        with pytest.raises(ValueError, match="transpose2D_batched"):
            fn(d, axis=0)
        with pytest.raises(ValueError):
            fn(d, axis=2)
        with pytest.raises(ValueError):
            fn(d.T)
    with pytest.raises(TypeError):
        laser_amd.softmax_cross_entropy(d, dev(np.zeros(4, np.int64)))
    with pytest.raises(ValueError):
        laser_amd.softmax_cross_entropy(d, dev(np.zeros(3, np.int32)))
    with pytest.raises(TypeError):
        laser_amd.log(dev(x.astype(np.float64)))
    L = laser_amd.lib()
    p = C.c_void_p(d.data_ptr())
    assert L.laser_hip_log_softmax_rows_f32_dev(p, 257, p, 257, 0, 257, None) == 0                     # rows = 0: nothing happens
    assert L.laser_hip_softmax_xent_rows_f32_dev(p, 1, p, 257, p, 257, p, 4, 257, 1.0, None) == laser_amd._lib.E_INVALID   # grad == src
