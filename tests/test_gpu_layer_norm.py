"""Layer normalization on an MI355X (laser_amd.layer_norm / layer_norm_backward; include/laser_hip.h "Layer
normalization"), bit for bit (any NaN equals any NaN) against the numpy model tests/layer_norm_model.py: plain float32
operations and reduce_model.model_sum for every sum.  The inputs are drawn once and sliced; a row's results depend on that
row alone and a column's on that column alone, so one model result per n (per rows) serves every smaller shape."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import laser_amd
from laser_amd import _lib
from tests import layer_norm_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 8191, 8192, 8193, 16389]    # vector, leaf, wave, chunk, long-row edges
ROWS = [0, 1, 3, 4, 5, 9]                                                            # the four-rows-per-workgroup edge
PROWS = [0, 1, 5, 1023, 1025, 8191, 8192, 8193, 16389]                               # leaf, chunk and partial boundaries
PCOLS = [1, 3, 4, 15, 16, 17, 37]                                                    # strip and vector edges
# (no shape here reaches the cap of 2048 workgroups: rows and units past it are in test_gpu_grid_stride.py)
SENTINEL = np.float32(-12345.0)
EPS = 1e-5
FWD, DX, PARAMS = 0, 1, 2


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not M.same_bits(got, want):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    if t is None:
        return None
    return t.to_numpy() if hasattr(t, "to_numpy") else t.cpu().numpy()


def last_kernel(what):
    return _lib.lib().laser_hip_layer_norm_last_kernel(what)


def plan_code(rows, n, vec, what):
    out = (C.c_int64 * 4)()
    assert _lib.lib().laser_hip_layer_norm_plan(rows, n, vec, what, out) == 0
    return out[0]


# ---- the row operands: drawn once ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_draws():
    """(x, dy, gamma, beta) of the largest row shape, read-only; x holds a few exact zeros and -0"""
    rng = np.random.default_rng(2026)
    x = rng.normal(3, 2, (max(ROWS), max(NS))).astype(np.float32)
    dy = rng.normal(0, 1, x.shape).astype(np.float32)
    gamma = rng.normal(1, 0.5, max(NS)).astype(np.float32)
    beta = rng.normal(0, 1, max(NS)).astype(np.float32)
    x[2, 1::97] = 0.0
    x[2, 2::101] = -0.0
    dy[1, ::89] = -0.0
    for a in (x, dy, gamma, beta):
        a.setflags(write=False)
    return x, dy, gamma, beta


@functools.lru_cache(maxsize=None)
def row_model(n, eps=EPS):
    """the model of the 9 rows of width n: {(has gamma, has beta): (y, mean, rstd)}, {has gamma: dx}; row r of each is the
    model of that row alone"""
    x, dy, gamma, beta = (a[..., :n] for a in row_draws())
    fwd = {(g, b): M.forward(x, gamma if g else None, beta if b else None, eps) for g in (0, 1) for b in (0, 1)}
    mean, rstd = fwd[1, 1][1:]
    for k in fwd:
        assert M.same_bits(fwd[k][1], mean) and M.same_bits(fwd[k][2], rstd)
    dx = {g: M.dx_of(dy, x, mean, rstd, gamma if g else None) for g in (0, 1)}
    return fwd, dx


# ---- 1. forward and dx over the shape sweep --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_forward_and_dx_sweep(n):
    x, dy, gamma, beta = (np.ascontiguousarray(a[..., :n]) for a in row_draws())
    fwd, dxm = row_model(n)
    dgamma, dbeta = dev(gamma), dev(beta)
    mean, rstd = fwd[1, 1][1:]
    kernel = 0 if n <= 1024 else 1 if n <= 8192 else 2
    for rows in ROWS:
        dx_, ddy = dev(x[:rows]), dev(dy[:rows])
        for g in (0, 1):
            for b in (0, 1):
                y, m, r = laser_amd.layer_norm(dx_, dgamma if g else None, dbeta if b else None, eps=EPS)
                same_bits(host(y), fwd[g, b][0][:rows], f"y {rows}x{n} gamma {g} beta {b}")
                same_bits(host(m), mean[:rows], f"mean {rows}x{n}")
                same_bits(host(r), rstd[:rows], f"rstd {rows}x{n}")
                if rows:
                    assert last_kernel(FWD) % 4 == kernel
        y, m, r = laser_amd.layer_norm(dx_, dgamma, dbeta, eps=EPS, stats=False)
        assert m is None and r is None
        same_bits(host(y), fwd[1, 1][0][:rows], f"y without statistics {rows}x{n}")
        dm, dr = dev(mean[:rows]), dev(rstd[:rows])
        for g in (0, 1):
            dx, dg, db = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, dgamma if g else None, need_params=False)
            assert dg is None and db is None
            same_bits(host(dx), dxm[g][:rows], f"dx {rows}x{n} gamma {g}")
            if rows:
                assert last_kernel(DX) % 4 == kernel
        assert np.array_equal(host(dx_).view(np.uint32), x[:rows].view(np.uint32))           # inputs untouched
        assert np.array_equal(host(ddy).view(np.uint32), dy[:rows].view(np.uint32))


def test_one_element_rows_and_the_edges_the_header_names():
    """n = 1: mean = x, var = +0, y = (0 * rstd) * gamma + beta"""
    x = np.float32([[5.0], [-2.5], [-0.0]])
    g, b = np.float32([3.0]), np.float32([0.25])
    y, m, r = laser_amd.layer_norm(dev(x), dev(g), dev(b), eps=EPS)
    rstd = np.float32(1) / np.sqrt(np.float32(0) + np.float32(EPS))
    same_bits(host(m), np.float32([5.0, -2.5, 0.0]), "mean")                                 # (+0 + -0 = +0)
    same_bits(host(r), np.float32([rstd] * 3), "rstd")
    same_bits(host(y), np.float32([[0.25]] * 3), "y")
    same_bits(host(y), M.forward(x, g, b, EPS)[0], "y is the model's")


# ---- 2. the parameter gradients ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def param_draws():
    """(dy, x, mean, rstd) of the largest column shape: a column sum takes any mean and rstd, so they are drawn, not computed"""
    rng = np.random.default_rng(99)
    rows, n = max(PROWS), max(PCOLS)
    dy = rng.normal(0, 3, (rows, n)).astype(np.float32)
    x = rng.normal(3, 2, (rows, n)).astype(np.float32)
    mean = rng.normal(3, 0.2, rows).astype(np.float32)
    rstd = rng.uniform(0.3, 0.8, rows).astype(np.float32)
    dy[::7, 2] = -0.0
    for a in (dy, x, mean, rstd):
        a.setflags(write=False)
    return dy, x, mean, rstd


@functools.lru_cache(maxsize=None)
def param_model(rows):
    """(dgamma, dbeta) of the first `rows` rows, all 37 columns: column j of each is the model of that column alone"""
    dy, x, mean, rstd = param_draws()
    return M.param_grads(dy[:rows], x[:rows], mean[:rows], rstd[:rows])


@pytest.mark.parametrize("rows", PROWS)
def test_parameter_gradients_sweep(rows):
    dy, x, mean, rstd = param_draws()
    want_g, want_b = param_model(rows)
    dm, dr = dev(mean[:rows]), dev(rstd[:rows])
    for n in PCOLS:
        ddy, dx_ = dev(dy[:rows, :n]), dev(x[:rows, :n])
        none, dg, db = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, need_dx=False)
        assert none is None
        same_bits(host(dg), want_g[:n], f"dgamma {rows}x{n}")
        same_bits(host(db), want_b[:n], f"dbeta {rows}x{n}")
        same_bits(host(db), host(laser_amd.bias_grad(ddy, dz=False)[0]), f"dbeta is bias_grad's {rows}x{n}")
        assert last_kernel(PARAMS) == plan_code(rows, n, 1 if n % 4 == 0 or rows <= 1 else 0, PARAMS)
        if rows == 0:
            assert not host(dg).view(np.uint32).any() and not host(db).view(np.uint32).any()      # +0
    # dgamma[j] is reduce_sum of column j of dy * xhat, on the device
    t = dev(dy[:rows] * M.xhat_of(x[:rows], mean[:rows], rstd[:rows]))
    if rows:
        for j in (0, 16, 36):
            s = laser_amd.reduce_sum(t[:, j])
            assert np.float32(s).view(np.uint32) == want_g[j:j + 1].view(np.uint32)[0], j


# ---- 3. alignment and strides ------------------------------------------------------------------------------------------------------
def padded(a, off, stride):
    """a device buffer filled with the sentinel, and the (rows, n) view of it that starts `off` elements in with the given
    row stride, holding a"""
    rows, n = a.shape
    buf = torch.full((off + rows * stride + 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
    view = torch.as_strided(buf, (rows, n), (stride, 1), off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, view


def padding_untouched(buf, off, rows, n, stride):
    h = buf.cpu().numpy()
    body = h[off:off + rows * stride].reshape(rows, stride)
    return (h[:off] == SENTINEL).all() and (body[:, n:] == SENTINEL).all() and (h[off + rows * stride:] == SENTINEL).all()


@pytest.mark.parametrize("n", [37, 1024, 1025, 8193])
def test_offset_bases_and_row_strides_give_the_same_bits(n):
    """a row stride that is a multiple of 4 above n (the vector instances), the same with the base one element off its
    alignment, a row stride of n + 1 (the single-element instances), of n + 4, and contiguous rows three elements off give the
    bits of the aligned contiguous call; the sentinel between the rows and after the last survives"""
    rows = 5
    x, dy, gamma, beta = (np.ascontiguousarray(a[..., :n]) for a in row_draws())
    x, dy = x[:rows], dy[:rows]
    fwd, dxm = row_model(n)
    want_y, mean, rstd = (a[:rows] for a in fwd[1, 1])
    want_dx = dxm[1][:rows]
    want_g, want_b = M.param_grads(dy, x, mean, rstd)
    kernel = 0 if n <= 1024 else 1 if n <= 8192 else 2
    zeros = np.zeros_like(x)
    vs = n + 4 - n % 4                                           # the next multiple of 4 above n
    for off, stride in ((0, vs), (1, vs), (0, n + 1), (4, n + 4), (3, n)):
        vec = 1 if off % 4 == 0 and stride % 4 == 0 else 0
        bx, vx = padded(x, off, stride)
        bdy, vdy = padded(dy, off, stride)
        by, vy = padded(zeros, off, stride)
        bdx, vdx = padded(zeros, off, stride)
        gbuf = torch.full((n + 9,), float(SENTINEL), dtype=torch.float32, device="cuda")
        vg = gbuf[4 * (1 - vec) + off % 4:][:n]                 # gamma as aligned as the rows are
        vg.copy_(torch.from_numpy(np.array(gamma)))
        dbeta_ = dev(beta)
        sbuf = torch.full((2 * rows + 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
        assert vx.data_ptr() % 16 == 4 * (off % 4)
        y, m, r = laser_amd.layer_norm(vx, vg, dbeta_, eps=EPS, out=vy)
        assert y is vy and last_kernel(FWD) == plan_code(rows, n, vec, FWD) == kernel + 4 * (1 - vec), (off, stride)
        same_bits(host(vy), want_y, f"y off {off} stride {stride}")
        same_bits(host(m), mean, "mean")
        same_bits(host(r), rstd, "rstd")
        assert padding_untouched(by, off, rows, n, stride) and padding_untouched(bx, off, rows, n, stride)
        sm = sbuf[3:3 + 2 * rows:2]                                # the statistics read with a stride of 2
        sm.copy_(torch.from_numpy(np.array(mean)))
        dx, dg, db = laser_amd.layer_norm_backward(vdy, vx, sm, dev(rstd), vg, need_dx=vdx)
        assert dx is vdx and last_kernel(DX) == plan_code(rows, n, vec, DX) == kernel + 4 * (1 - vec), (off, stride)
        assert last_kernel(PARAMS) == 1 - vec
        same_bits(host(vdx), want_dx, f"dx off {off} stride {stride}")
        same_bits(host(dg), want_g, f"dgamma off {off} stride {stride}")
        same_bits(host(db), want_b, f"dbeta off {off} stride {stride}")
        assert padding_untouched(bdx, off, rows, n, stride) and padding_untouched(bdy, off, rows, n, stride)
        assert np.array_equal(host(vx).view(np.uint32), x.view(np.uint32)) and np.array_equal(host(vdy).view(np.uint32), dy.view(np.uint32))
        assert (gbuf.cpu().numpy()[n + 8:] == SENTINEL).all()


def test_strided_gamma_and_beta_take_the_single_element_instance():
    rows, n = 4, 1025
    x, dy, gamma, beta = (np.ascontiguousarray(a[..., :n]) for a in row_draws())
    fwd, dxm = row_model(n)
    g2 = torch.zeros(2 * n, device="cuda")[::2]
    g2.copy_(torch.from_numpy(np.array(gamma)))
    y, m, r = laser_amd.layer_norm(dev(x[:rows]), g2, dev(beta), eps=EPS)
    assert last_kernel(FWD) == 5
    same_bits(host(y), fwd[1, 1][0][:rows], "y, gamma with a stride of 2")
    dx, _, _ = laser_amd.layer_norm_backward(dev(dy[:rows]), dev(x[:rows]), m, r, g2, need_params=False)
    assert last_kernel(DX) == 5
    same_bits(host(dx), dxm[1][:rows], "dx, gamma with a stride of 2")
    x3 = dev(np.stack([x[:4], x[4:8]]))                             # a contiguous rank-3 tensor is (prod(leading), n)
    y3, m3, r3 = laser_amd.layer_norm(x3, dev(gamma), dev(beta), eps=EPS)
    assert host(y3).shape == (2, 4, n) and host(m3).shape == (2, 4)
    same_bits(host(y3).reshape(8, n), fwd[1, 1][0][:8], "rank 3")
    same_bits(host(r3).reshape(8), fwd[1, 1][2][:8], "rank 3 rstd")


# ---- 4. aliasing and options -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 4099, 8193])
def test_in_place_and_each_gradient_alone(n):
    rows = 9
    x, dy, gamma, beta = (np.ascontiguousarray(a[..., :n]) for a in row_draws())
    fwd, dxm = row_model(n)
    want_y, mean, rstd = fwd[1, 1]
    want_g, want_b = M.param_grads(dy, x, mean, rstd)
    dgamma, dbeta, dm, dr = dev(gamma), dev(beta), dev(mean), dev(rstd)
    xin = dev(x)
    y, _, _ = laser_amd.layer_norm(xin, dgamma, dbeta, eps=EPS, out=xin)
    assert y is xin
    same_bits(host(xin), want_y, "y over x")
    # dx over dy and over x, the parameter gradients asked for in the same call: they see dy and x as they came
    for over in ("dy", "x"):
        ddy, dx_ = dev(dy), dev(x)
        dx, dg, db = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, dgamma, need_dx=ddy if over == "dy" else dx_)
        same_bits(host(dx), dxm[1], f"dx over {over}")
        same_bits(host(dg), want_g, f"dgamma, dx over {over}")
        same_bits(host(db), want_b, f"dbeta, dx over {over}")
    ddy, dx_ = dev(dy), dev(x)
    dx, dg, db = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, dgamma, need_params=False)
    assert dg is None and db is None
    same_bits(host(dx), dxm[1], "dx alone")
    dx, dg, db = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, dgamma, need_dx=False, need_params="gamma")
    assert dx is None and db is None
    same_bits(host(dg), want_g, "dgamma alone")
    dx, dg, db = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, dgamma, need_dx=False, need_params="beta")
    assert dx is None and dg is None
    same_bits(host(db), want_b, "dbeta alone")


def test_each_parameter_gradient_alone_past_one_chunk_of_rows():
    rows, n = 8193, 17
    dy, x, mean, rstd = param_draws()
    want_g, want_b = param_model(rows)
    ddy, dx_, dm, dr = dev(dy[:rows, :n]), dev(x[:rows, :n]), dev(mean[:rows]), dev(rstd[:rows])
    _, dg, none = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, need_dx=False, need_params="gamma")
    assert none is None
    same_bits(host(dg), want_g[:n], "dgamma alone")
    _, none, db = laser_amd.layer_norm_backward(ddy, dx_, dm, dr, need_dx=False, need_params="beta")
    assert none is None
    same_bits(host(db), want_b[:n], "dbeta alone")
    before = _lib.lib().laser_hip_bias_grad_last_kernel()
    laser_amd.layer_norm_backward(ddy, dx_, dm, dr, need_dx=False)
    assert _lib.lib().laser_hip_bias_grad_last_kernel() == before          # the fold launches leave bias_grad's record alone


# ---- 5. special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 1025, 8193])
def test_nan_inf_constant_and_negative_zero_rows_touch_no_other_row(n):
    rows = 9
    x0, dy0, gamma, beta = (np.ascontiguousarray(a[..., :n]) for a in row_draws())
    x, dy = np.array(x0), np.array(dy0)
    x[1, n // 2] = np.nan
    x[3, n - 1] = np.inf
    x[5, :] = 2.5                      # a constant row
    x[7, :] = -0.0
    dy[2, 0] = np.nan                  # in dy: one row of dx, one column of dgamma and dbeta
    dy[6, n - 1] = -np.inf
    dgamma, dbeta = dev(gamma), dev(beta)
    clean = [0, 2, 4, 6, 8]
    for eps in (0.0, EPS):
        want = M.forward(x, gamma, beta, eps)
        ref = M.forward(x0, gamma, beta, eps)
        y, m, r = (host(t) for t in laser_amd.layer_norm(dev(x), dgamma, dbeta, eps=eps))
        for got, w, c, name in zip((y, m, r), want, ref, ("y", "mean", "rstd")):
            same_bits(got, w, f"{name} eps {eps}")
            same_bits(got[clean], c[clean], f"{name} of the other rows, eps {eps}")
            assert np.isfinite(got[clean]).all()
        assert np.isnan(y[1]).all() and np.isnan(m[1]) and np.isnan(r[1])
        assert np.isnan(y[3]).all() and m[3] == np.inf and np.isnan(r[3])
        assert m[5] == np.float32(2.5) and m[7:8].view(np.uint32)[0] == 0                    # the row of -0 has mean +0
        if eps == 0.0:
            assert r[5] == np.inf and r[7] == np.inf and np.isnan(y[5]).all() and np.isnan(y[7]).all()       # 0 * Inf
        else:
            rstd = np.float32(1) / np.sqrt(np.float32(eps))
            assert r[5] == rstd and r[7] == rstd
            same_bits(y[5], beta, "a constant row is +0 * rstd * gamma + beta")
            same_bits(y[7], (np.float32(-0.0) * rstd) * gamma + beta, "a row of -0 is -0 * rstd * gamma + beta")
    # backward, with the statistics of the run with eps > 0
    mean, rstd = want[1], want[2]
    want_dx = M.dx_of(dy, x, mean, rstd, gamma)
    ref_dx = M.dx_of(dy0, x0, mean, rstd, gamma)
    want_g, want_b = M.param_grads(dy, x, mean, rstd)
    dx, dg, db = (host(t) for t in laser_amd.layer_norm_backward(dev(dy), dev(x), dev(mean), dev(rstd), dgamma))
    same_bits(dx, want_dx, "dx")
    same_bits(dg, want_g, "dgamma")
    same_bits(db, want_b, "dbeta")
    untouched = [0, 4, 8]                                        # rows with nothing special in x or dy
    same_bits(dx[untouched], ref_dx[untouched], "dx of the other rows")
    assert np.isfinite(dx[untouched]).all() and np.isnan(dx[2]).all() and np.isnan(dx[1]).all()
    assert np.isnan(db[0]) and db[n - 1] == -np.inf if n > 1 else True
    assert np.isfinite(db[1:n - 1]).all()                        # a NaN or Inf in dy reaches its own column of dbeta alone
    # ... and of dgamma, when x holds none (a NaN in x reaches every column of dgamma through its row's xhat)
    xc = np.array(x0)
    m0, r0 = M.forward(xc, None, None, EPS)[1:]
    g2, b2 = (host(t) for t in laser_amd.layer_norm_backward(dev(dy), dev(xc), dev(m0), dev(r0), need_dx=False)[1:])
    wg, wb = M.param_grads(dy, xc, m0, r0)
    cg, cb = M.param_grads(dy0, xc, m0, r0)
    same_bits(g2, wg, "dgamma, clean x")
    same_bits(b2, wb, "dbeta, clean x")
    assert np.isnan(g2[0]) and np.isinf(g2[n - 1])
    same_bits(g2[1:n - 1], cg[1:n - 1], "the other columns of dgamma are those of the clean dy")
    same_bits(b2[1:n - 1], cb[1:n - 1], "the other columns of dbeta are those of the clean dy")
    assert np.isfinite(g2[1:n - 1]).all()


# ---- 6. streams --------------------------------------------------------------------------------------------------------------------
def test_a_side_stream_gives_the_same_bits():
    rows = 9
    for n in (257, 4099, 16389):
        x, dy, gamma, beta = (np.ascontiguousarray(a[..., :n]) for a in row_draws())
        fwd, dxm = row_model(n)
        want_y, mean, rstd = fwd[1, 1]
        want_g, want_b = M.param_grads(dy, x, mean, rstd)
        ops = [dev(a) for a in (x, dy, gamma, beta)]
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            y, m, r = laser_amd.layer_norm(ops[0], ops[2], ops[3], eps=EPS)
            dx, dg, db = laser_amd.layer_norm_backward(ops[1], ops[0], m, r, ops[2])
            s.synchronize()
        for got, want, name in ((y, want_y, "y"), (m, mean, "mean"), (r, rstd, "rstd"), (dx, dxm[1], "dx"), (dg, want_g, "dgamma"),
                                (db, want_b, "dbeta")):
            same_bits(host(got), want, f"{name} on a side stream, n {n}")
    dyp, xp, mp, rp = param_draws()
    want_g, want_b = param_model(8193)
    ops = [dev(a) for a in (dyp[:8193], xp[:8193], mp[:8193], rp[:8193])]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                   # two levels: the scratch is ordered on the same stream
        _, dg, db = laser_amd.layer_norm_backward(*ops, need_dx=False)
        s.synchronize()
    same_bits(host(dg), want_g, "dgamma on a side stream")
    same_bits(host(db), want_b, "dbeta on a side stream")


# ---- 7. a small network ------------------------------------------------------------------------------------------------------------
def train(steps=20, lr=0.5):
    """softmax(tanh(layer_norm(X W1 + b1)) W2 + b2): 64 samples of 32 features, 24 hidden units, 4 classes, labels from a fixed
    linear rule; SGD on the device.  Returns the per-sample losses of every step and the final parameters."""
    S, F, H, Cn = 64, 32, 24, 4
    rng = np.random.default_rng(2027)
    x = rng.normal(0, 1, (S, F)).astype(np.float32)
    rule = rng.normal(0, 1, (F, Cn))
    labels = np.argmax(x.astype(np.float64) @ rule, axis=1).astype(np.int32)
    X, lab = laser_amd.toTensor(x), laser_amd.toTensor(labels)
    T = laser_amd.toTensor
    P = {"w1": T(rng.normal(0, 0.5, (F, H)).astype(np.float32)), "b1": T(np.zeros(H, np.float32)),
         "gamma": T(np.ones(H, np.float32)), "beta": T(np.zeros(H, np.float32)),
         "w2": T(rng.normal(0, 0.5, (H, Cn)).astype(np.float32)), "b2": T(np.zeros(Cn, np.float32))}
    lr = np.float32(lr)
    losses = []
    for _ in range(steps):
        z = laser_amd.matmul(X, P["w1"], bias=P["b1"])
        a, mean, rstd = laser_amd.layer_norm(z, P["gamma"], P["beta"])
        h = laser_amd.tanh(a, out=a)
        logits = laser_amd.matmul(h, P["w2"], bias=P["b2"])
        loss, g = laser_amd.softmax_cross_entropy(logits, lab, grad=True, scale=1.0 / S)
        dh, dw2, db2 = laser_amd.linear_backward(h, P["w2"], g)
        da = laser_amd.activation_grad(dh, h, "tanh", out=dh)
        dz, dgamma, dbeta = laser_amd.layer_norm_backward(da, z, mean, rstd, P["gamma"], need_dx=da)
        _, dw1, db1 = laser_amd.linear_backward(X, P["w1"], dz, need_dx=False)
        for name, grad in (("w1", dw1), ("b1", db1), ("gamma", dgamma), ("beta", dbeta), ("w2", dw2), ("b2", db2)):
            laser_amd.forEach("w -= lr * g", w=P[name], g=grad, params={"lr": lr})
        losses.append(loss.to_numpy())
    return np.stack(losses), {k: v.to_numpy() for k, v in P.items()}


def test_a_network_with_a_normalized_layer_trains_on_the_device_and_repeats_bit_for_bit():
    l1, p1 = train()
    l2, p2 = train()
    assert l1.shape == (20, 64) and np.isfinite(l1).all()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32))
    for k in p1:
        assert np.array_equal(p1[k].view(np.uint32), p2[k].view(np.uint32)), k
    assert not np.array_equal(p1["gamma"], np.ones(24, np.float32)) and p1["beta"].any()         # they were trained
    mean = l1.astype(np.float64).mean(axis=1)
    print("mean loss, first and last step:", mean[0], mean[-1])
    assert mean[-1] < mean[0]


# ---- the C++ mirror ----------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "layer_norm_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "laser_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "layer_norm_mirror.cpp"),
                    "-o", exe, "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
