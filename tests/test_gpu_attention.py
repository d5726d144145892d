"""The fused attention forward, the softmax gradient and the composed attention backward on an MI355X (laser_amd.attention,
softmax_backward, attention_backward; include/laser_hip.h "Attention", "Softmax gradient"), bit for bit (any NaN equals any
NaN) against the numpy model tests/attention_model.py.  The inputs are drawn once and sliced; outputs are pre-filled with a
sentinel and the gaps of strided outputs must keep it; the model runs on at most 64 query rows wherever Tk > 1025."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import laser_amd
from laser_amd import _lib
from tests import attention_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(-12345.0)
MAX_D = 128
DS = [1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 128, MAX_D]
TKS = [1, 2, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 8191, 8192, 8193, 16389]
GRAD_NS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 8191, 8192, 8193, 16389]
GRAD_ROWS = [0, 1, 3, 4, 5, 9]


def plan(bh, tq, tk, d, dv, causal=0, vec=1):
    out = (C.c_int64 * 5)()
    assert _lib.lib().laser_hip_attention_plan(bh, tq, tk, d, dv, causal, vec, out) == 0
    return list(out)


BM = plan(1, 1, 1, 1, 1)[0]
TQS = [0, 1, BM - 1, BM, BM + 1, 2 * BM + 3]


def same_bits(got, want, what="", zeros_equal=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not M.same_bits(got, want, zeros_equal):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    if t is None:
        return None
    return t.to_numpy() if hasattr(t, "to_numpy") else t.cpu().numpy()


def last_kernel():
    return _lib.lib().laser_hip_attention_last_kernel()


@functools.lru_cache(maxsize=None)
def draws():
    """(q, k, v) of the largest shapes, read-only: (4, 100, MAX_D), (4, 16389, MAX_D), (4, 16389, MAX_D); q and k are scaled
    so that scores stay within lexp's stated range"""
    rng = np.random.default_rng(2027)
    q = rng.normal(0, 1, (4, 100, MAX_D)).astype(np.float32)
    k = rng.normal(0, 1, (4, 16389, MAX_D)).astype(np.float32)
    v = rng.normal(0, 1, (4, 16389, MAX_D)).astype(np.float32)
    q[1, 3, 1::7] = 0.0
    v[0, 5, ::3] = -0.0
    for a in (q, k, v):
        a.setflags(write=False)
    return q, k, v


def take(bh, tq, tk, d, dv):
    q, k, v = draws()
    return q[:bh, :tq, :d], k[:bh, :tk, :d], v[:bh, :tk, :dv]


def model(q, k, v, scale=None, causal=False, rows=None):
    """(O, P, m, s) stacked over the slices of 3-D operands"""
    res = [M.forward(q[i], k[i], v[i], scale, causal, rows) for i in range(q.shape[0])]
    return tuple(np.stack([r[j] for r in res]) if res else None for j in range(4))


def run(q, k, v, scale=None, causal=False, probs=True):
    """the device result (O, P, m, s) of 3-D host operands, O and P written into sentinel-filled buffers"""
    bh, tq, dv, tk = q.shape[0], q.shape[1], v.shape[2], k.shape[1]
    o = torch.full((bh, tq, dv), float(SENTINEL), dtype=torch.float32, device="cuda")
    p = torch.full((bh, tq, tk), float(SENTINEL), dtype=torch.float32, device="cuda") if probs else None
    r = laser_amd.attention(dev(q), dev(k), dev(v), scale=scale, causal=causal, out=o, probs=p, stats=True)
    assert r[0] is o and r[1] is p
    return host(o), host(p), host(r[2]), host(r[3])


def check(q, k, v, scale=None, causal=False, rows=None, what="", probs=True):
    got = run(q, k, v, scale, causal, probs)
    want = model(q, k, v, scale, causal, rows)
    sel = slice(None) if rows is None else np.asarray(rows)
    for name, g, w in zip(("O", "P", "row_max", "row_sum"), got, want):
        if g is None:
            continue
        if q.shape[0] * q.shape[1] == 0:
            assert g.size == 0
            continue
        same_bits(g[:, sel], w, f"{what} {name}")
    return got


# ---- 1. the shape sweeps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", sorted(set(DS)))
def test_feature_widths(d):
    check(*take(2, 37, 70, d, d), what=f"d={d}")
    check(*take(2, 37, 70, d, d), causal=True, what=f"causal d={d}")


@pytest.mark.parametrize("d,dv", [(64, 5), (3, 128)])
def test_value_width_differs(d, dv):
    check(*take(2, 37, 70, d, dv), what=f"d={d} dv={dv}")


@pytest.mark.parametrize("tk", TKS)
def test_key_counts(tk):
    """the MFMA tile edges, the P V slice fold (512), a leaf's second element (1024), the chunk partials (8192, 16384)"""
    check(*take(2, 3, tk, 5, 6), what=f"Tk={tk}", probs=tk <= 1025)
    if tk <= 1025:
        check(*take(1, 3, tk, 32, 33), what=f"Tk={tk} d=32")


@pytest.mark.parametrize("tq", TQS)
def test_query_counts(tq):
    check(*take(2, tq, 40, 16, 16), what=f"Tq={tq}")
    if 0 < tq <= 40:
        check(*take(2, tq, 40, 16, 16), causal=True, what=f"causal Tq={tq}")


# ---- 2. causal -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 33, 130, 600])
def test_causal_square(t):
    q, k, v = take(2, 100, t, 8, 8)
    rng = np.random.default_rng(t)
    q = rng.normal(0, 1, (2, t, 8)).astype(np.float32)
    got = check(q, k, v, causal=True, what=f"causal T={t}")
    assert (got[1][:, np.triu_indices(t, 1)[0], np.triu_indices(t, 1)[1]].view(np.uint32) == 0).all()      # masked: +0


def test_causal_decoding_step():
    check(*take(3, 1, 100, 16, 16), causal=True, what="decoding")
    q, k, v = take(3, 1, 100, 16, 16)
    full = run(q, k, v, causal=False)
    dec = run(q, k, v, causal=True)
    for a, b in zip(full, dec):
        same_bits(a, b, "Tq = 1 sees every key")


def test_causal_rows_straddle_the_chunk_boundary():
    """Tq = Tk = 8193 + BM: the rows around n_i = 8192 | 8193 (the last one-chunk row and the first two-chunk rows), and
    Tq = 40 against Tk = 8210: n_i = i + 8171 crosses the chunk boundary inside one query block"""
    t = 8193 + BM
    rng = np.random.default_rng(5)
    q = rng.normal(0, 1, (1, t, 4)).astype(np.float32)
    _, k, v = take(1, 1, t, 4, 4)
    rows = np.arange(8192 - BM, 8192 + BM)
    assert len(rows) <= 64
    check(q, k, v, causal=True, rows=rows, what="T=8193+BM", probs=False)
    q, k, v = take(1, 40, 8210, 4, 4)
    check(q, k, v, causal=True, what="Tq=40 Tk=8210", probs=False)


def test_causal_needs_tq_at_most_tk():
    q, k, v = (dev(a) for a in take(1, 9, 8, 4, 4))
    with pytest.raises(ValueError):
        laser_amd.attention(q, k, v, causal=True)
    st = (C.c_int64 * 3)(36, 0, 4)
    o = torch.zeros(36, device="cuda")
    rc = _lib.lib().laser_hip_attention_f32_dev(o.data_ptr(), st, q.data_ptr(), st, k.data_ptr(), st, v.data_ptr(), st, None, None, None,
                                                None, 1, 1, 9, 8, 4, 4, 1.0, 1, None)
    assert rc == _lib.E_INVALID and b"causal" in _lib.lib().laser_hip_last_error()


# ---- 3. layouts ------------------------------------------------------------------------------------------------------------------
def test_fused_projection_views_and_a_strided_output():
    b, h, t, d = 2, 3, 45, 16
    rng = np.random.default_rng(11)
    buf = rng.normal(0, 1, (b, t, 3, h, d)).astype(np.float32)
    dbuf = dev(buf)
    q, k, v = (dbuf[:, :, i].permute(0, 2, 1, 3) for i in range(3))          # (B, H, T, d) views, no copy
    assert not q.is_contiguous()
    obuf = torch.full((b, h, t, d + 3), float(SENTINEL), dtype=torch.float32, device="cuda")
    pbuf = torch.full((b, h, t, t + 5), float(SENTINEL), dtype=torch.float32, device="cuda")
    o, p, m, s = laser_amd.attention(q, k, v, causal=True, out=obuf[..., :d], probs=pbuf[..., :t], stats=True)
    assert last_kernel() == 0
    hq, hk, hv = (np.ascontiguousarray(buf[:, :, i].transpose(0, 2, 1, 3)).reshape(b * h, t, d) for i in range(3))
    want = model(hq, hk, hv, causal=True)
    same_bits(host(obuf)[..., :d].reshape(b * h, t, d), want[0], "O")
    same_bits(host(pbuf)[..., :t].reshape(b * h, t, t), want[1], "P")
    same_bits(host(m).reshape(b * h, t), want[2], "row_max")
    same_bits(host(s).reshape(b * h, t), want[3], "row_sum")
    assert (host(obuf)[..., d:] == SENTINEL).all() and (host(pbuf)[..., t:] == SENTINEL).all()


def test_bases_shifted_by_one_element_take_the_single_element_form():
    q, k, v = take(2, 37, 70, 16, 16)
    base = run(q, k, v)
    assert last_kernel() == 0 and plan(2, 37, 70, 16, 16, 0, 1)[1] == 0 and plan(2, 37, 70, 16, 16, 0, 0)[1] == 1

    def shifted(a):
        flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = dev(a).reshape(-1)
        return flat[1:].view(a.shape)
    o = torch.full((2 * 37 * 16 + 1,), float(SENTINEL), dtype=torch.float32, device="cuda")
    r = laser_amd.attention(shifted(q), shifted(k), shifted(v), out=o[1:].view(2, 37, 16), probs=True, stats=True)
    assert last_kernel() == 1
    assert host(o)[0] == SENTINEL
    for name, a, b2 in zip(("O", "P", "m", "s"), base, (host(o)[1:].reshape(2, 37, 16), host(r[1]), host(r[2]), host(r[3]))):
        same_bits(b2, a, f"shifted {name}")


def test_more_units_than_workgroups():
    """the grid cap: the plan says that workgroups take a second unit"""
    bh = 1100
    p = plan(bh, 1, 3, 2, 2)
    assert p[4] == bh and p[2] < p[4], p
    rng = np.random.default_rng(3)
    q = rng.normal(0, 1, (bh, 1, 2)).astype(np.float32)
    k = rng.normal(0, 1, (bh, 3, 2)).astype(np.float32)
    v = rng.normal(0, 1, (bh, 3, 2)).astype(np.float32)
    check(q, k, v, what="1100 units")


@pytest.mark.parametrize("scale", [None, 0.0, -0.5, 3.0])
def test_scales(scale):
    q, k, v = take(1, 33, 65, 8, 8)
    check((q * np.float32(0.5)).astype(np.float32), k, v, scale=scale, what=f"scale={scale}")


# ---- 4. specials -----------------------------------------------------------------------------------------------------------------
def test_nan_and_inf_reach_exactly_the_rows_the_definition_says():
    q, k, v = (a.copy() for a in take(1, 40, 40, 8, 8))
    nan_rows = lambda o: set(np.nonzero(np.isnan(o[0]).any(axis=1))[0].tolist())
    qn = q.copy()
    qn[0, 7, 2] = np.nan
    for causal in (False, True):
        assert nan_rows(check(qn, k, v, causal=causal, what="NaN in Q")[0]) == {7}
    kn = k.copy()
    kn[0, 20, 1] = np.nan
    assert nan_rows(check(q, kn, v, what="NaN in K")[0]) == set(range(40))
    assert nan_rows(check(q, kn, v, causal=True, what="NaN in K, causal")[0]) == set(range(20, 40))        # n_i = i + 1 > 20
    vn = v.copy()
    vn[0, 20, 1] = np.nan
    for causal in (False, True):
        o = check(q, k, vn, causal=causal, what="NaN in V")[0]
        assert np.isnan(o[0, :, 1]).all() and not np.isnan(np.delete(o[0], 1, axis=1)).any()
    qi = q.copy()
    qi[0, 9, :] = 0
    qi[0, 9, 0] = np.inf
    ki = k.copy()
    ki[0, :, 0] = np.abs(ki[0, :, 0]) + 1                                    # every score of row 9 is +Inf
    assert nan_rows(check(qi, ki, v, what="+Inf scores")[0]) == {9}


# ---- 5. optional outputs ---------------------------------------------------------------------------------------------------------
def test_what_is_asked_for_has_the_same_bits_whatever_else_is():
    q, k, v = take(2, 37, 600, 16, 16)
    dq, dk, dv_ = dev(q), dev(k), dev(v)
    for causal in (False, True):
        o, p, m, s = (host(t) for t in laser_amd.attention(dq, dk, dv_, causal=causal, probs=True, stats=True))
        same_bits(host(laser_amd.attention(dq, dk, dv_, causal=causal)), o, "O alone")
        r = laser_amd.attention(dq, dk, dv_, causal=causal, out=False, probs=True)
        assert r[0] is None and r[2] is None
        same_bits(host(r[1]), p, "P alone (no P V sweep)")
        r = laser_amd.attention(dq, dk, dv_, causal=causal, out=False, stats=True)
        same_bits(host(r[2]), m, "row_max alone")
        same_bits(host(r[3]), s, "row_sum alone")
    with pytest.raises(ValueError):
        laser_amd.attention(dq, dk, dv_, out=False)


# ---- 6. the device cross-check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tq,tk,d,dv", [(40, 1025, 65, 65), (33, 70, 16, 8), (64, 513, 64, 64)])
def test_fused_equals_the_composition_on_the_device(tq, tk, d, dv):
    """matmul (alpha = scale) + softmax + matmul in laser-order mode, +0 and -0 taken as equal"""
    assert laser_amd.get_float_mode() == _lib.F32_LASER_ORDER
    q, k, v = take(2, tq, tk, d, dv)
    o, p, _, _ = run(q, k, v)
    scale = float(M.default_scale(d))
    for i in range(2):
        s = laser_amd.matmul(dev(q[i]), dev(k[i]).T, alpha=scale)
        pc = laser_amd.softmax(s, out=torch.empty_like(s))
        oc = laser_amd.matmul(pc, dev(v[i]))
        same_bits(p[i], host(pc), f"P slice {i}", zeros_equal=True)
        same_bits(o[i], host(oc), f"O slice {i}", zeros_equal=True)


# ---- 7. the softmax gradient -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_draws():
    rng = np.random.default_rng(77)
    n = max(GRAD_NS)
    y = np.stack([M.exp_model.softmax_row(r) for r in rng.normal(0, 2, (max(GRAD_ROWS), n)).astype(np.float32)])
    dy = rng.normal(0, 1, y.shape).astype(np.float32)
    dy[1, ::5] = -0.0
    y.setflags(write=False)
    dy.setflags(write=False)
    return dy, y


@functools.lru_cache(maxsize=None)
def grad_model(n):
    dy, y = grad_draws()
    return M.softmax_grad(dy[:, :n], y[:, :n])


def grad_last():
    return _lib.lib().laser_hip_softmax_grad_last_kernel()


@pytest.mark.parametrize("n", GRAD_NS)
def test_softmax_backward_row_lengths(n):
    dy, y = (a[:, :n] for a in grad_draws())
    want = grad_model(n)
    code = 0 if n <= 1024 else 1 if n <= 8192 else 2
    for rows in (GRAD_ROWS if n in (5, 1025, 8193) else [max(GRAD_ROWS)]):
        out = torch.full((rows, n + 4), float(SENTINEL), dtype=torch.float32, device="cuda")       # row stride n + 4: 16-byte rows
        laser_amd.softmax_backward(dev(dy[:rows]), dev(y[:rows]), out=out[:, :n])
        if rows:
            assert grad_last() == code + (0 if n % 4 == 0 or rows == 1 else 4), (n, rows, grad_last())
        same_bits(host(out)[:, :n], want[:rows], f"n={n} rows={rows}")
        assert (host(out)[:, n:] == SENTINEL).all()
    # in place on dy and on y, and a base off its alignment: the same bits
    for which in (0, 1):
        ops = [dev(dy), dev(y)]
        r = laser_amd.softmax_backward(ops[0], ops[1], out=ops[which])
        assert r is ops[which]
        same_bits(host(r), want, f"n={n} in place on {'dy y'.split()[which]}")
    flat = torch.full((dy.size + 1,), float(SENTINEL), dtype=torch.float32, device="cuda")
    laser_amd.softmax_backward(dev(dy), dev(y), out=flat[1:].view(dy.shape))
    assert grad_last() == code + 4 and host(flat)[0] == SENTINEL
    same_bits(host(flat)[1:].reshape(dy.shape), want, f"n={n} misaligned")


@pytest.mark.parametrize("n,rows", [(3, 8200), (1028, 2100), (8196, 2051)])
def test_softmax_backward_rows_past_the_workgroup_cap(n, rows):
    out3 = (C.c_int64 * 3)()
    assert _lib.lib().laser_hip_softmax_grad_plan(rows, n, 1, out3) == 0
    assert out3[1] == 2048 and rows > 2048 * (4 if n <= 1024 else 1)
    dy, y = (a[:, :n] for a in grad_draws())
    reps = -(-rows // dy.shape[0])
    got = host(laser_amd.softmax_backward(dev(np.tile(dy, (reps, 1))[:rows]), dev(np.tile(y, (reps, 1))[:rows])))
    same_bits(got, np.tile(grad_model(n), (reps, 1))[:rows], f"n={n} rows={rows}")


# ---- 8. the composed backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bh,tq,tk,d,dv,causal", [(3, 33, 65, 5, 7, False), (2, 64, 513, 64, 64, False), (2, 65, 65, 32, 32, True)])
def test_attention_backward_against_the_model(bh, tq, tk, d, dv, causal):
    q, k, v = take(bh, tq, tk, d, dv)
    dout = np.random.default_rng(tq).normal(0, 1, (bh, tq, dv)).astype(np.float32)
    ops = [dev(a) for a in (dout, q, k, v)]
    got = [host(t) for t in laser_amd.attention_backward(*ops, causal=causal)]
    want = [np.stack(x) for x in zip(*(M.backward(dout[i], q[i], k[i], v[i], None, causal) for i in range(bh)))]
    for name, g, w in zip(("dq", "dk", "dv"), got, want):
        same_bits(g, w, name)
    for need in (("q",), ("k",), ("v",), ("q", "v"), "k"):
        r = laser_amd.attention_backward(*ops, causal=causal, need=need)
        for name, g, t in zip("qkv", got, r):
            if name in need:
                same_bits(host(t), g, f"need={need}: d{name}")
            else:
                assert t is None
    # 4-D operands with (batch, head) dims that do not collapse: one GEMM launch per batch, the same bits
    if bh == 2:
        def four(a):                                                               # (2, 2, T, d) inside (2, 3, T, d): slices a[0], a[1] twice
            big = np.zeros((2, 3) + a.shape[1:], np.float32)
            big[:, :2] = a[None]
            return dev(big)[:, :2]
        r = laser_amd.attention_backward(*(four(a) for a in (dout, q, k, v)), causal=causal)
        for name, g, t in zip("qkv", got, r):
            for b in range(2):
                same_bits(host(t)[b], g, f"4-D d{name}, batch {b}")


def test_two_training_steps_lower_the_loss_and_repeat_bit_for_bit():
    """one attention block y = attention(x Wq, x Wk, x Wv) fitted to a target with plain gradient steps"""
    rng = np.random.default_rng(99)
    t, d = 48, 16
    x = rng.normal(0, 1, (t, d)).astype(np.float32)
    target = rng.normal(0, 1, (1, t, d)).astype(np.float32)
    w0 = [rng.normal(0, 0.3, (d, d)).astype(np.float32) for _ in range(3)]

    def train():
        dx, dt = dev(x), dev(target)
        w = [dev(a) for a in w0]
        losses = []
        for _ in range(3):
            q, k, v = (laser_amd.matmul(dx, wi).reshape(1, t, d) for wi in w)
            o = laser_amd.attention(q, k, v, causal=True, out=torch.empty(1, t, d, device="cuda"))
            do = o - dt
            losses.append(float(0.5 * (do.double() ** 2).sum()))
            grads = laser_amd.attention_backward(do, q, k, v, causal=True)
            for wi, g in zip(w, grads):
                gw = laser_amd.matmul(dx.T, torch.from_numpy(host(g)[0]).cuda())
                wi -= 0.01 * gw
        return losses, [host(wi) for wi in w]

    l1, w1 = train()
    l2, w2 = train()
    assert l1[2] < l1[1] < l1[0], l1
    assert l1 == l2
    for a, b in zip(w1, w2):
        same_bits(a, b, "weights after two steps")


# ---- 9. the C++ mirror -----------------------------------------------------------------------------------------------------------
def test_cpp_mirror_program(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    exe = tmp_path / "attention_mirror"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I",
                    os.path.join(ROOT, "laser_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "attention_mirror.cpp"), "-o", str(exe),
                    "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
