"""The dense-layer backward pass on an MI355X (laser_amd.bias_grad / linear_backward; include/laser_hip.h "Dense-layer
backward"), bit for bit (any NaN equals any NaN) against the numpy models the library already has: dz is
act_model.activation_grad(dy, y, kind) (dy itself without an activation) and db[j] is reduce_model.model_sum(dz[:, j]), the
canonical reduction order applied to the column alone.  The inputs are drawn once and sliced; a model result is computed
once per (rows, n, kind)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import laser_amd
from laser_amd import _lib
from oracle import oracle
from tests import act_model as A
from tests import reduce_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [None, "relu", "tanh", "sigmoid"]
ROWS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 8191, 8192, 8193, 16389, 40961]     # leaf, chunk and partial boundaries; 2, 3, 6 chunks
COLS = [1, 3, 4, 15, 16, 17, 37]                                             # strip and vector edges
# (at most 6 chunks x 3 strips here; more units than the cap of 2048 workgroups are in test_gpu_grid_stride.py)
SENTINEL = np.float32(-12345.0)
EPS = 2.0 ** -23


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not A.same_bits(got, want):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


@functools.lru_cache(maxsize=None)
def draws():
    """(dy, y) of the largest shape, read-only: normal draws, and y values of exactly 0, 1, -1 and -0"""
    rng = np.random.default_rng(77)
    dy = rng.normal(0, 3, (max(ROWS), max(COLS))).astype(np.float32)
    y = rng.normal(0, 0.6, dy.shape).astype(np.float32)
    flat = y.reshape(-1)
    for i, v in enumerate((0.0, 1.0, -1.0, -0.0)):
        flat[3 + 11 * i::97] = np.float32(v)
    y[:5, :3] = np.float32([[0.0, 1.0, -1.0], [-0.0, 0.5, 0.0], [1.0, -0.0, -1.0], [0.25, 1.0, 0.0], [-1.0, -0.0, 1.0]])
    dy.setflags(write=False)
    y.setflags(write=False)
    return dy, y


def operands(rows, n):
    dy, y = draws()
    return np.ascontiguousarray(dy[:rows, :n]), np.ascontiguousarray(y[:rows, :n])


def model_of(dy, y, kind):
    dz = np.array(dy) if kind is None else A.activation_grad(dy, y, kind)
    db = np.array([R.model_sum(dz[:, j]) for j in range(dz.shape[1])], np.float32).reshape(dz.shape[1])
    return dz, db


@functools.lru_cache(maxsize=None)
def model(rows, n, kind):
    dz, db = model_of(*operands(rows, n), kind)
    dz.setflags(write=False)
    db.setflags(write=False)
    return dz, db


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.to_numpy() if hasattr(t, "to_numpy") else t.cpu().numpy()


def plan_code(rows, n, vec):
    out = (C.c_int64 * 4)()
    assert _lib.lib().laser_hip_bias_grad_plan(rows, n, vec, 256, out) == 0
    return out[0]


def last_kernel():
    return _lib.lib().laser_hip_bias_grad_last_kernel()


# ---- 1. the shape sweep ------------------------------------------------------------------------------------------------------
SWEEP = ([(r, 17, "tanh") for r in ROWS] + [(r, 1, None) for r in ROWS] + [(8193, n, "sigmoid") for n in COLS] +
         [(8193, 37, k) for k in KINDS] + [(5, 3, k) for k in KINDS])


@pytest.mark.parametrize("rows,n,kind", SWEEP)
def test_shape_sweep(rows, n, kind):
    dy, y = operands(rows, n)
    want_dz, want_db = model(rows, n, kind)
    ddy, dyy = dev(dy), dev(y)
    db, dz = laser_amd.bias_grad(ddy, dyy if kind else None, kind)
    same_bits(host(dz), want_dz, f"dz {rows}x{n} {kind}")
    same_bits(host(db), want_db, f"db {rows}x{n} {kind}")
    db2, none = laser_amd.bias_grad(ddy, dyy if kind else None, kind, dz=False)
    assert none is None
    same_bits(host(db2), want_db, f"db alone {rows}x{n} {kind}")
    assert np.array_equal(host(ddy), dy) and np.array_equal(host(dyy).view(np.uint32), y.view(np.uint32))   # inputs untouched
    if rows == 0:
        assert np.array_equal(host(db).view(np.uint32), np.zeros(n, np.uint32))                             # +0


# ---- 2. NaN, Inf and -0 columns ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, "sigmoid"])
def test_a_nan_an_inf_and_an_all_negative_zero_column_touch_no_other(kind):
    rows, n = 8193, 37
    dy, y = operands(rows, n)
    dy = np.array(dy)
    dy[5000, 3] = np.nan
    dy[8192, 7] = np.inf
    dy[:, 11] = -0.0
    if kind:
        y = np.array(y)
        y[:, 7] = 0.5                       # f' > 0 there: the +Inf stays +Inf
        y[:, 11] = 0.25                     # -0 * f' = -0
    want_dz, want_db = model_of(dy, y, kind)
    db, dz = laser_amd.bias_grad(dev(dy), dev(y) if kind else None, kind)
    got = host(db)
    same_bits(host(dz), want_dz, "dz")
    same_bits(got, want_db, "db")
    assert np.isnan(got[3]) and got[7] == np.inf and got[11:12].view(np.uint32)[0] == 0      # the all -0 column sums to +0
    others = np.delete(got, [3, 7])
    assert np.isfinite(others).all()
    clean_dz, clean_db = model(rows, n, kind)
    keep = [j for j in range(n) if j not in (3, 7, 11)]
    same_bits(got[keep], clean_db[keep], "the other columns are those of the clean input")


# ---- 3. layout ---------------------------------------------------------------------------------------------------------------
def padded(a, off, stride):
    """a device buffer filled with the sentinel, and the (rows, n) view of it that starts `off` elements in with the given
    row stride, holding a"""
    rows, n = a.shape
    buf = torch.full((off + rows * stride + 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
    view = torch.as_strided(buf, (rows, n), (stride, 1), off)
    view.copy_(torch.from_numpy(a))
    return buf, view


def padding_untouched(buf, off, rows, n, stride):
    h = buf.cpu().numpy()
    body = h[off:off + rows * stride].reshape(rows, stride)
    return (h[:off] == SENTINEL).all() and (body[:, n:] == SENTINEL).all() and (h[off + rows * stride:] == SENTINEL).all()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("kind", ["tanh", None])
def test_strided_rows_offset_bases_and_in_place(off, kind):
    """row strides of n + 3 = 40 (a multiple of 4: the vector instance when the base is aligned, with its last strip partial),
    the same one element off the 16-byte alignment (the single-element instance), dz in place over dy and over y, and no dz"""
    rows, n = 8193, 37
    stride = n + 3
    dy, y = operands(rows, n)
    want_dz, want_db = model(rows, n, kind)
    vec = 1 if off == 0 else 0
    bdy, vdy = padded(dy, off, stride)
    by, vy = padded(y, off, stride)
    bdz, vdz = padded(np.zeros_like(dy), off, stride)
    assert vdy.data_ptr() % 16 == 4 * off
    dbuf = torch.full((2 * n + 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
    out = dbuf[4:4 + 2 * n:2]                                        # db with a stride of 2
    laser_amd.bias_grad(vdy, vy if kind else None, kind, dz=vdz, out=out)
    assert last_kernel() == plan_code(rows, n, vec) == 1 - vec
    same_bits(host(vdz), want_dz, "dz")
    h = dbuf.cpu().numpy()
    same_bits(h[4:4 + 2 * n:2], want_db, "db")
    assert (h[:4] == SENTINEL).all() and (h[5:4 + 2 * n:2] == SENTINEL).all() and (h[4 + 2 * n - 1:] == SENTINEL).all()
    assert padding_untouched(bdz, off, rows, n, stride) and padding_untouched(bdy, off, rows, n, stride)
    assert np.array_equal(host(vdy), dy)
    # no dz
    db, none = laser_amd.bias_grad(vdy, vy if kind else None, kind, dz=False)
    assert none is None and last_kernel() == 1 - vec
    same_bits(host(db), want_db, "db alone")
    # in place over y, then over dy
    if kind:
        db, dz = laser_amd.bias_grad(vdy, vy, kind, dz=vy)
        assert dz is vy
        same_bits(host(vy), want_dz, "dz over y")
        same_bits(host(db), want_db, "db, dz over y")
        assert padding_untouched(by, off, rows, n, stride)
        by, vy = padded(y, off, stride)
    db, dz = laser_amd.bias_grad(vdy, vy if kind else None, kind, dz=vdy)
    assert dz is vdy
    same_bits(host(vdy), want_dz, "dz over dy")
    same_bits(host(db), want_db, "db, dz over dy")
    assert padding_untouched(bdy, off, rows, n, stride)


def test_both_instances_give_the_same_bits_on_contiguous_operands():
    """n = 16: whole strips, 16-byte rows -> the vector instance; the same values one element further -> single elements"""
    rows, n = 16389, 16
    dy, y = operands(rows, n)
    want_dz, want_db = model(rows, n, "relu")
    for off in (0, 1):
        _, vdy = padded(dy, off, n)
        _, vy = padded(y, off, n)
        db, dz = laser_amd.bias_grad(vdy, vy, "relu")
        assert last_kernel() == plan_code(rows, n, 1 - off) == off
        same_bits(host(dz), want_dz, f"dz off {off}")
        same_bits(host(db), want_db, f"db off {off}")


# ---- 4. independence ---------------------------------------------------------------------------------------------------------
def test_a_column_is_reduce_sum_of_itself_whatever_surrounds_it():
    rows, n = 8193, 37
    dy, y = operands(rows, n)
    ddy, dyy = dev(dy), dev(y)
    db, dz = laser_amd.bias_grad(ddy, dyy, "tanh")
    got = host(db)
    for j in (0, 16, 36):
        s = laser_amd.reduce_sum(dz[:, j])                               # the strided column view, on the device
        assert np.float32(s).view(np.uint32) == got[j:j + 1].view(np.uint32)[0], j
        alone, _ = laser_amd.bias_grad(ddy[:, j:j + 1], dyy[:, j:j + 1], "tanh")      # the same column called with n = 1
        assert host(alone).view(np.uint32)[0] == got[j:j + 1].view(np.uint32)[0], j


# ---- 5. linear_backward --------------------------------------------------------------------------------------------------------
def test_linear_backward_is_bias_grad_and_two_oracle_products():
    """(M, K, N) = (200, 24, 17), tanh.  db and dz are the model's; dw and dx are the oracle's products of the same operands
    (laser-order GEMM: bit for bit).  Against float64: a product of contraction length L computed in float32 in any order
    is within (L + 2) * 2^-23 * (|A| |B|) of the exact one (L - 1 additions and one multiplication per term, each within
    2^-24 relative, first order, with slack for the rounding of the float64 reference and second-order terms); db is such a
    product with a column of ones (L = M); dz = dy * (1 - y * y) has three roundings, so |dz - ref| <= 3 * 2^-23 *
    |dy| * (1 + y * y)."""
    assert laser_amd.get_float_mode() == _lib.F32_LASER_ORDER
    M, K, N = 200, 24, 17
    rng = np.random.default_rng(5)
    x = rng.normal(0, 1, (M, K)).astype(np.float32)
    w = rng.normal(0, 0.3, (K, N)).astype(np.float32)
    dy = rng.normal(0, 1, (M, N)).astype(np.float32)
    y = np.tanh(rng.normal(0, 1, (M, N))).astype(np.float32)
    dx_, dw_, dy_, y_ = dev(x), dev(w), dev(dy), dev(y)
    dx, dw, db = laser_amd.linear_backward(dx_, dw_, dy_, y_, "tanh")
    dz, want_db = model_of(dy, y, "tanh")
    gdx, gdw, gdb = host(dx), host(dw), host(db)
    same_bits(gdb, want_db, "db")
    same_bits(gdw, oracle.matmul(x.T, dz), "dw")
    same_bits(gdx, oracle.matmul(dz, w.T), "dx")
    _, gdz = laser_amd.bias_grad(dy_, y_, "tanh")
    same_bits(host(gdz), dz, "dz")
    f8 = np.float64
    ref_dz = dy.astype(f8) * (1 - y.astype(f8) ** 2)
    assert (np.abs(dz - ref_dz) <= 3 * EPS * np.abs(dy.astype(f8)) * (1 + y.astype(f8) ** 2)).all()
    z8 = dz.astype(f8)
    assert (np.abs(gdb - z8.sum(0)) <= (M + 2) * EPS * np.abs(z8).sum(0)).all()
    assert (np.abs(gdw - x.T.astype(f8) @ z8) <= (M + 2) * EPS * (np.abs(x.T.astype(f8)) @ np.abs(z8))).all()
    assert (np.abs(gdx - z8 @ w.T.astype(f8)) <= (N + 2) * EPS * (np.abs(z8) @ np.abs(w.T.astype(f8)))).all()
    for t, a in ((dx_, x), (dw_, w), (dy_, dy), (y_, y)):
        assert np.array_equal(host(t).view(np.uint32), a.view(np.uint32))                # operands unchanged
    none, dw2, db2 = laser_amd.linear_backward(dx_, dw_, dy_, y_, "tanh", need_dx=False)
    assert none is None
    same_bits(host(dw2), gdw, "dw without dx")
    same_bits(host(db2), gdb, "db without dx")


# ---- 6. a training loop ---------------------------------------------------------------------------------------------------------
def train(steps=30, lr=0.5):
    """Y = softmax(tanh(X W1 + b1) W2 + b2): 64 samples, 8 features, 16 hidden units, 4 classes, labels from a fixed linear
    rule; SGD on the device.  Returns the per-sample losses of every step and the final parameters."""
    S, F, H, Cn = 64, 8, 16, 4
    rng = np.random.default_rng(2024)
    x = rng.normal(0, 1, (S, F)).astype(np.float32)
    rule = rng.normal(0, 1, (F, Cn))
    labels = np.argmax(x.astype(np.float64) @ rule, axis=1).astype(np.int32)
    X, lab = laser_amd.toTensor(x), laser_amd.toTensor(labels)
    P = {"w1": laser_amd.toTensor(rng.normal(0, 0.5, (F, H)).astype(np.float32)), "b1": laser_amd.toTensor(np.zeros(H, np.float32)),
         "w2": laser_amd.toTensor(rng.normal(0, 0.5, (H, Cn)).astype(np.float32)), "b2": laser_amd.toTensor(np.zeros(Cn, np.float32))}
    lr = np.float32(lr)
    losses = []
    for _ in range(steps):
        h = laser_amd.matmul(X, P["w1"], bias=P["b1"])
        laser_amd.tanh(h, out=h)
        logits = laser_amd.matmul(h, P["w2"], bias=P["b2"])
        loss, g = laser_amd.softmax_cross_entropy(logits, lab, grad=True, scale=1.0 / S)
        dh, dw2, db2 = laser_amd.linear_backward(h, P["w2"], g)
        _, dw1, db1 = laser_amd.linear_backward(X, P["w1"], dh, h, "tanh", need_dx=False)
        for name, grad in (("w1", dw1), ("b1", db1), ("w2", dw2), ("b2", db2)):
            laser_amd.forEach("w -= lr * g", w=P[name], g=grad, params={"lr": lr})
        losses.append(loss.to_numpy())
    return np.stack(losses), {k: v.to_numpy() for k, v in P.items()}


def test_a_two_layer_network_trains_on_the_device_and_repeats_bit_for_bit():
    l1, p1 = train()
    l2, p2 = train()
    assert l1.shape == (30, 64) and np.isfinite(l1).all()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32))
    for k in p1:
        assert np.array_equal(p1[k].view(np.uint32), p2[k].view(np.uint32)), k
    mean = l1.astype(np.float64).mean(axis=1)
    print("mean loss, first and last step:", mean[0], mean[-1])
    assert mean[-1] < mean[0]                                     # a sanity condition, not a measurement


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "dense_grad_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "laser_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "dense_grad_mirror.cpp"),
                    "-o", exe, "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
