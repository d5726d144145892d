"""The F+tree weighted sampler on an MI355X (laser_amd.newSampler / multinomial / laser_hip_sampler_*; include/laser_hip.h
"F+tree weighted sampler"), bit for bit against the numpy model of tests/fplus_tree_model.py: trees with same_bits, indices
with ==.  Build at every row length where the kernels change path (whole rows in LDS up to 512 leaves, segments of 1024
leaves, the hand-over to the second launch) over 1, 3 and 67 rows, padded and offset layouts with sentinels; draws with and
without replacement, update, rows independent of each other, softmax -> multinomial end to end, the Python argument checks
and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import exp_model as E
from tests import fplus_tree_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)
TOP = np.float32(1) - np.float32(2.0 ** -24)      # the largest float32 below 1
KINDS = 6                                          # uniform, 60 % zeros, x 1e30, x 1e-30, denormals, all zero

# the issue's list, plus the bound of the LDS kernel (512 leaves) +- 1 and the segment size / hand-over (1024, 2048 leaves) +- 1
N_GRID = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 50000,
          65537]
# (at most 67 rows here; more rows, segments and draws than the cap of 16384 workgroups holds are in test_gpu_grid_stride.py)


def L():
    return laser_amd.lib()


def plan(rows, n):
    out = (C.c_int64 * 4)()
    assert L().laser_hip_sampler_plan(rows, n, out) == 0
    return list(out)


def test_the_grid_covers_the_kernels_bounds():
    small = max(n for n in N_GRID if plan(1, n)[0] == 0)
    assert plan(1, small + 1)[0] == 1 and small in N_GRID and small - 1 in N_GRID and small + 1 in N_GRID
    seg = plan(1, small + 1)[1]
    for n in (seg - 1, seg, seg + 1, 2 * seg - 1, 2 * seg, 2 * seg + 1):
        assert n in N_GRID


def weights(rows, n, seed=0):
    rng = np.random.default_rng(1000 * n + rows + seed)
    w = rng.uniform(0, 1, (rows, n)).astype(np.float32)
    for r in range(rows):
        kind = r % KINDS if rows > 1 else n % (KINDS - 1)        # a lone row is never the all-zero one
        if kind == 1:
            w[r][rng.random(n) < 0.6] = 0
        elif kind == 2:
            w[r] *= np.float32(1e30)
        elif kind == 3:
            w[r] *= np.float32(1e-30)
        elif kind == 4:
            w[r] = (rng.integers(0, 1 << 20, n).astype(np.uint32)).view(np.float32)       # denormals (and some zeros)
        elif kind == 5:
            w[r] = 0
    return w


_cases = {}


def case(rows, n):
    """weights and the model's trees, computed once per (rows, n) and never written again"""
    if (rows, n) not in _cases:
        w = weights(rows, n)
        t = M.build(w)
        w.setflags(write=False)
        t.setflags(write=False)
        _cases[(rows, n)] = (w, t)
    return _cases[(rows, n)]


def dev(a):
    return laser_amd.toTensor(np.ascontiguousarray(a), a.dtype)


def ptr(t, off=0):
    return C.c_void_p(t.unsafe_raw_data() + off * t.dtype.itemsize)


def stream():
    from laser_amd.tensor import _stream
    return _stream()


def gpu_build(w, w_off=0, ws=None, t_off=0, t_pad=0):
    """the trees of `w` through the C entry point in the given layout: (rows, 2 P) images, and the whole tree buffer"""
    rows, n = w.shape
    P = M.leaves(n)
    ws = n if ws is None else ws
    ts = 2 * P + t_pad
    wbuf = np.full(w_off + rows * ws + 4, SENTINEL, np.float32)
    for r in range(rows):
        wbuf[w_off + r * ws:w_off + r * ws + n] = w[r]
    tbuf = np.full(t_off + rows * ts + 8, SENTINEL, np.float32)
    dw, dt = dev(wbuf), dev(tbuf)
    rc = L().laser_hip_sampler_build_f32_dev(ptr(dt, t_off), ts, ptr(dw, w_off), ws, rows, n, stream())
    assert rc == 0, L().laser_hip_last_error()
    out = dt.to_numpy()
    body = out[t_off:t_off + rows * ts].reshape(rows, ts)
    assert np.all(out[:t_off] == SENTINEL) and np.all(out[t_off + rows * ts:] == SENTINEL), "wrote outside the rows"
    assert np.all(body[:, 2 * P:] == SENTINEL), "wrote into the gap between two rows"
    return body[:, :2 * P], dt


@pytest.mark.parametrize("n", N_GRID)
def test_build_matches_the_model(n):
    for rows in (1, 3, 67):
        w, want = case(rows, n)
        pad4 = (n + 3) // 4 * 4 + 4
        layouts = [(0, n, 0, 0), (1, n + 3, 1, 5)]
        if rows < 67 or n <= 4097:
            layouts += [(0, pad4, 0, 5), (1, n + 3, 0, 0), (0, pad4, 0, 4)]
        for w_off, ws, t_off, t_pad in layouts:
            got, _ = gpu_build(w, w_off, ws, t_off, t_pad)
            assert E.same_bits(got, want), (n, rows, w_off, ws, t_off, t_pad)
            assert not np.signbit(got[:, 0]).any()


def special_rows(n):
    """the KINDS kinds, a NaN row, an Inf row and a sparse row; which rows must give -1"""
    w = weights(KINDS + 3, n, seed=7).copy()
    w[KINDS, n // 2] = np.nan
    w[KINDS + 1, n - 1] = np.inf
    w[KINDS + 2][np.random.default_rng(n).random(n) < 0.9] = 0
    dead = ~(np.isfinite(M.build(w)[:, 1]) & (M.build(w)[:, 1] > 0))
    assert dead[5] and dead[KINDS] and dead[KINDS + 1]
    return w, dead


def uniforms(rows, m, seed):
    u = np.random.default_rng(seed).random((rows, m), dtype=np.float32)
    if m >= 2:
        u[:, 0], u[:, -1] = 0, TOP
    else:
        u[0::2, 0], u[1::2, 0] = 0, TOP
    return u


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 1000, 1025, 4097, 50000])
def test_sample_matches_the_model(n):
    w, dead = special_rows(n)
    rows = w.shape[0]
    want_tree = M.build(w)
    s = laser_amd.newSampler(dev(w))
    assert (s.rows, s.n, s.tree.shape) == (rows, n, (rows, 2 * M.leaves(n)))
    assert E.same_bits(s.tree.to_numpy(), want_tree)
    for m in (1, 7, 64, 1000):
        u = uniforms(rows, m, 31 * n + m)
        idx = s.sample(u, num=m).to_numpy()
        assert idx.dtype == np.int32 and idx.shape == (rows, m)
        assert np.array_equal(idx, M.draw(want_tree, u)), (n, m)
        assert np.all(idx[dead] == -1) and np.all(idx[~dead] >= 0) and np.all(idx[~dead] < n)
        live = np.flatnonzero(~dead)
        assert np.all(np.take_along_axis(w[live], idx[live].astype(np.int64), 1) > 0), (n, m)
    assert E.same_bits(s.tree.to_numpy(), want_tree), "sample wrote into the tree"


def test_sample_from_an_offset_padded_tree():
    """a base off its 8-byte boundary and an odd row stride: the single-element loads, the same indices"""
    for n in (5, 1025):
        w, dead = special_rows(n)
        rows, P = w.shape[0], M.leaves(n)
        got, dt = gpu_build(w, 1, n + 3, 1, 5)
        u = uniforms(rows, 64, n)
        du, di = dev(u), laser_amd.newTensor(np.int32, rows, 64)
        assert L().laser_hip_sampler_sample_f32_dev(ptr(di), ptr(dt, 1), 2 * P + 5, ptr(du), rows, n, 64, stream()) == 0
        assert np.array_equal(di.to_numpy(), M.draw(M.build(w), u))


def check_removal(w, k, seed):
    rows, n = w.shape
    u = uniforms(rows, k, seed)
    model = M.build(w)
    want = M.draw_remove(model, u)
    s = laser_amd.newSampler(dev(w))
    idx = s.sampleAndRemove(u, num=k).to_numpy()
    assert np.array_equal(idx, want), (n, k)
    after = s.tree.to_numpy()
    assert E.same_bits(after, model), (n, k)
    w2 = w.copy()
    for r in range(rows):
        drawn = idx[r][idx[r] >= 0]
        assert len(set(drawn.tolist())) == drawn.size, "an element was drawn twice"
        assert np.all(w[r, drawn] > 0)
        w2[r, drawn] = 0
    assert E.same_bits(after, M.build(w2)), "update does not give the bits of a rebuild"
    assert E.same_bits(after, laser_amd.newSampler(dev(w2)).tree.to_numpy())
    return idx


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65])
def test_sample_and_remove_matches_the_model(n):
    w = weights(7, n, seed=3)
    for k in (1, 10, n + 2):
        idx = check_removal(w, k, 17 * n + k)
        if k == n + 2:
            pos = (w > 0).sum(1)
            for r in range(7):          # every positive element once, then -1
                assert sorted(idx[r, :pos[r]].tolist()) == np.flatnonzero(w[r] > 0).tolist() and np.all(idx[r, pos[r]:] == -1)


def test_sample_and_remove_at_the_reference_shape():
    """bench_multinomial_samplers.nim: 128 rows of 50 000 probabilities, 10 words without replacement"""
    rng = np.random.default_rng(50)
    w = rng.uniform(0, 1, (128, 50000)).astype(np.float32)
    w /= w.sum(1, keepdims=True, dtype=np.float32)
    idx = check_removal(w, 10, 51)
    assert idx.min() >= 0 and idx.max() < 50000


@pytest.mark.parametrize("n", [1, 5, 1000, 50000])
def test_update_equals_a_rebuild(n):
    rows = 67
    w = weights(rows, n, seed=9)
    rng = np.random.default_rng(n)
    elem = rng.integers(0, n, rows).astype(np.int32)
    elem[3], elem[10], elem[11] = -1, n - 1, 0
    wt = rng.uniform(0, 2, rows).astype(np.float32)
    wt[20] = 0
    s = laser_amd.newSampler(dev(w))
    assert s.update(elem, wt) is s
    w2 = w.copy()
    live = elem >= 0
    w2[np.flatnonzero(live), elem[live]] = wt[live]
    assert E.same_bits(s.tree.to_numpy(), M.build(w2))
    assert E.same_bits(s.tree.to_numpy(), M.update(M.build(w), elem, wt, n=n))
    # indices outside the row, given on the device where the host cannot check them: skipped
    out = elem.copy()
    out[::2] = np.array([n, 2 * M.leaves(n) + 3, -2, 1 << 30])[np.arange(rows)[::2] % 4]
    s.update(dev(out), dev(wt))
    w3 = w2.copy()
    odd = np.flatnonzero((np.arange(rows) % 2 == 1) & live)
    w3[odd, elem[odd]] = wt[odd]
    assert E.same_bits(s.tree.to_numpy(), M.build(w3))


def test_rows_in_one_call_equal_one_row_calls():
    for n in (5, 300, 1500):
        w, want = case(67, n)
        u = uniforms(67, 8, n)
        s = laser_amd.newSampler(dev(w))
        tree, idx = s.tree.to_numpy(), s.sample(u, num=8).to_numpy()
        rem = s.sampleAndRemove(u, num=8).to_numpy()
        for r in range(67):
            one = laser_amd.newSampler(dev(w[r]))                      # 1-D: one row
            assert (one.rows, one.n) == (1, n)
            assert E.same_bits(one.tree.to_numpy()[0], tree[r]) and E.same_bits(tree[r], want[r])
            assert np.array_equal(one.sample(u[r:r + 1], num=8).to_numpy()[0], idx[r])
            assert np.array_equal(one.sampleAndRemove(u[r:r + 1], num=8).to_numpy()[0], rem[r])


def test_softmax_to_multinomial_end_to_end():
    import torch
    rng = np.random.default_rng(11)
    logits = rng.uniform(-8, 8, (5, 1000)).astype(np.float32)
    p = laser_amd.softmax(dev(logits))
    host_p = p.to_numpy()
    u = uniforms(5, 3, 12)
    got = laser_amd.multinomial(p, 3, u=u).to_numpy()
    assert np.array_equal(got, M.draw_remove(M.build(host_p), u))
    got = laser_amd.multinomial(p, num_samples=3, replacement=True, u=u).to_numpy()
    assert np.array_equal(got, M.draw(M.build(host_p), u))
    # a torch tensor in, the uniforms on the device or drawn there
    tp = torch.from_numpy(host_p).cuda()
    assert np.array_equal(laser_amd.multinomial(tp, 3, replacement=True, u=torch.from_numpy(u).cuda()).to_numpy(), got)
    drawn = laser_amd.multinomial(tp, 4).to_numpy()
    assert drawn.shape == (5, 4) and drawn.min() >= 0 and drawn.max() < 1000
    assert all(len(set(r.tolist())) == 4 for r in drawn)
    assert laser_amd.multinomial(tp, 0).to_numpy().shape == (5, 0)


def test_python_argument_checks_raise():
    import torch
    w = np.full((3, 5), 0.2, np.float32)
    s = laser_amd.newSampler(dev(w))
    ok = np.full((3, 2), 0.5, np.float32)
    for bad in (np.array([[0.5, 1.0]] * 3, np.float32), np.array([[-0.1, 0.5]] * 3, np.float32), np.array([[np.nan, 0.5]] * 3, np.float32)):
        with pytest.raises(ValueError):
            s.sample(bad, num=2)
        with pytest.raises(ValueError):
            s.sampleAndRemove(torch.from_numpy(bad).cuda(), num=2)
    with pytest.raises(ValueError):
        s.sample(ok, num=3)                                            # shape (rows, num)
    with pytest.raises(ValueError):
        s.sample(ok[:2], num=2)
    with pytest.raises(TypeError):
        s.sample(ok.astype(np.float64), num=2)
    with pytest.raises(ValueError):
        s.sample(ok, num=-1)
    with pytest.raises(ValueError):
        s.sample(torch.from_numpy(np.full((3, 4), 0.5, np.float32)).cuda()[:, ::2], num=2)      # not row-major
    with pytest.raises(TypeError):
        laser_amd.newSampler(dev(w.astype(np.float64)))
    with pytest.raises(ValueError):
        laser_amd.newSampler(dev(np.zeros((2, 3, 4), np.float32)))
    with pytest.raises(ValueError):
        laser_amd.newSampler(dev(np.zeros((8, 6), np.float32)).T)        # the elements of a row must be contiguous
    with pytest.raises(TypeError):
        laser_amd.newSampler(w)                                          # a host array
    for elem in ([0, 5, 1], [0, -2, 1], [0, 1], [0.5, 1, 2]):
        with pytest.raises(ValueError):
            s.update(elem, [1, 1, 1])
    with pytest.raises(ValueError):
        s.update([0, 1, 2], [1, 1])
    with pytest.raises(TypeError):
        s.update(dev(np.zeros(3, np.int64)), dev(np.zeros(3, np.float32)))
    assert E.same_bits(s.tree.to_numpy(), M.build(w))                    # nothing above touched the trees


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "sampler_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "sampler_mirror.cpp"), "-o", exe, "-L", lib, "-llaser_hip",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
