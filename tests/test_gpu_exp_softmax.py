"""lexp and the row softmax on an MI355X (laser_amd.exp / laser_amd.softmax / laser_exp in forEach bodies; include/laser_hip.h
"exp and row softmax"), bit for bit against the numpy model of tests/exp_model.py: exp on the edge set, on contiguous,
offset, transposed, reversed and broadcast views, in place and through forEach / forEachReduce; softmax at every row length
where the kernels change path, for 1, 3 and 67 rows, padded row strides, an offset base and in place, on rows with a wide
spread, a NaN, equal values and all -Inf; 67 rows against 67 one-row calls; and one accuracy check against float64."""
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import exp_model as E
from tests import reduce_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SOFTMAX_N = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 8191, 8192, 8193, 16389]
ROWS = 67                   # (far below the cap of 2048 workgroups: rows past it are in test_gpu_grid_stride.py)
SENTINEL = np.float32(-12345.0)


def opt(name):
    return laser_amd.primitives.get_option(name)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not E.same_bits(got, want):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


# ---- exp ------------------------------------------------------------------------------------------------------------------
def test_exp_edges():
    x = E.edges()
    got = laser_amd.exp(dev(x)).to_numpy()
    assert_bits(got, E.lexp(x), "edges")
    assert np.isnan(got[np.isnan(x)]).all()
    x = E.ties()
    assert_bits(laser_amd.exp(dev(x)).to_numpy(), E.lexp(x), "ties")


def test_exp_contiguous_sizes_and_an_offset_base():
    rng = np.random.default_rng(21)
    for n in (1, 3, 4, 5, 1023, 4097):
        x = rng.uniform(-90, 90, n + 1).astype(np.float32)
        d = dev(x)
        assert_bits(laser_amd.exp(d[:n]).to_numpy(), E.lexp(x[:n]), f"n={n}")
        assert_bits(laser_amd.exp(d[1:]).to_numpy(), E.lexp(x[1:]), f"n={n}, base off by one element")
        import torch
        out = torch.full((n + 2,), float(SENTINEL), device="cuda")
        laser_amd.exp(d[1:], out=out[1:n + 1])
        o = out.cpu().numpy()
        assert_bits(o[1:n + 1], E.lexp(x[1:]), f"n={n}, both bases off")
        assert o[0] == SENTINEL and o[n + 1] == SENTINEL


def test_exp_strided_views_broadcast_and_in_place():
    rng = np.random.default_rng(22)
    x = rng.uniform(-90, 90, (37, 53)).astype(np.float32)
    want = E.lexp(x)
    t = laser_amd.toTensor(x)
    assert_bits(laser_amd.exp(t.T).to_numpy(), want.T, "transposed source")
    assert_bits(laser_amd.exp(t[::-1, ::-1]).to_numpy(), want[::-1, ::-1], "negative strides")
    assert_bits(laser_amd.exp(t[::2, 1::3]).to_numpy(), want[::2, 1::3], "steps")
    out = laser_amd.newTensor(np.float32, 53, 37)
    laser_amd.exp(t, out=out.T)
    assert_bits(out.to_numpy(), want.T, "transposed destination")
    out = laser_amd.newTensor(np.float32, 37, 53)
    laser_amd.exp(t[::-1], out=out[:, ::-1])
    assert_bits(out.to_numpy(), want[::-1, ::-1], "negative stride on the destination")
    row = laser_amd.toTensor(x[3])
    out = laser_amd.newTensor(np.float32, 5, 53)
    laser_amd.exp(row, out=out)
    assert_bits(out.to_numpy(), np.broadcast_to(want[3], (5, 53)), "broadcast source")
    one = laser_amd.toTensor(x[:1, :1])
    out = laser_amd.newTensor(np.float32, 7, 9)
    laser_amd.exp(one, out=out)
    assert_bits(out.to_numpy(), np.full((7, 9), want[0, 0], np.float32), "one element broadcast")
    laser_amd.exp(t, out=t)
    assert_bits(t.to_numpy(), want, "dst == src")
    v = laser_amd.toTensor(x)
    laser_amd.exp(v.T, out=v.T)
    assert_bits(v.to_numpy(), want, "dst == src, strided")
    with pytest.raises(laser_amd.LaserHipError):
        laser_amd.exp(t, out=_zero_stride_out())      # stride 0 on the destination


def _zero_stride_out():
    import torch
    return laser_amd.fromTorch(torch.zeros(53, device="cuda").expand(37, 53))


def test_exp_host_form():
    x = np.concatenate([E.edges(), np.random.default_rng(23).uniform(-90, 90, 5000).astype(np.float32)])
    assert_bits(laser_amd.exp(x), E.lexp(x), "host pointers")


def test_laser_exp_in_foreach_bodies():
    rng = np.random.default_rng(24)
    x = np.concatenate([E.edges(), rng.uniform(-90, 90, 20001).astype(np.float32)])
    tx, ty = laser_amd.toTensor(x), laser_amd.newTensor(np.float32, x.size)
    laser_amd.forEach("y = laser_exp(x)", y=ty, x=tx)
    assert_bits(ty.to_numpy(), laser_amd.exp(tx).to_numpy(), "forEach body = the entry point")
    assert_bits(ty.to_numpy(), E.lexp(x), "forEach body = the model")
    x = rng.uniform(-20, 20, 20001).astype(np.float32)
    m = np.float32(x.max())
    tx, ty = laser_amd.toTensor(x), laser_amd.newTensor(np.float32, x.size)
    s = laser_amd.forEachReduce("y = laser_exp(x - m); acc += y", merge="acc += other", init=np.float32(0),
                                params={"m": m}, writable=("y",), y=ty, x=tx)
    e = E.lexp((x - m).astype(np.float32))
    assert_bits(ty.to_numpy(), e, "forEachReduce body: y")
    assert np.float32(s).view(np.uint32) == np.float32(M.model_sum(e)).view(np.uint32), (s, M.model_sum(e))


# ---- softmax --------------------------------------------------------------------------------------------------------------
_cases = {}


def case(n):
    """67 rows of n values and the model's softmax of them, computed once: row 0 uniform on [-20, 20], row 1 with a spread of
    200 (the clamp and the subnormal region), row 2 with a NaN, row 3 all equal, row 4 all -Inf, the others uniform"""
    if n not in _cases:
        rng = np.random.default_rng(1000 + n)
        x = rng.uniform(-20, 20, (ROWS, n)).astype(np.float32)
        x[1] = rng.uniform(-100, 100, n).astype(np.float32)
        if n > 1:
            x[1, 0], x[1, n - 1] = 100, -100
        x[2, n // 2] = np.nan
        x[3] = np.float32(1.25)
        x[4] = -np.inf
        x.setflags(write=False)
        y = E.softmax_rows(x)
        y.setflags(write=False)
        _cases[n] = (x, y)
    return _cases[n]


def run_softmax(x, stride, offset, in_place=False):
    """softmax of the rows of x laid out with `stride` elements between rows, `offset` elements into the allocation;
    returns the result and checks that nothing outside the rows was written"""
    import torch
    rows, n = x.shape
    host = np.full(offset + rows * stride + 1, SENTINEL, np.float32)
    hv = host[offset:offset + rows * stride].reshape(rows, stride)
    hv[:, :n] = x
    src = torch.from_numpy(host).cuda()
    dst = src if in_place else torch.full_like(src, float(SENTINEL))
    view = lambda b: b[offset:offset + rows * stride].view(rows, stride)[:, :n]
    laser_amd.softmax(view(src), out=view(dst))
    out = dst.cpu().numpy()
    ov = out[offset:offset + rows * stride].reshape(rows, stride)
    assert (out[:offset] == SENTINEL).all() and out[-1] == SENTINEL and (ov[:, n:] == SENTINEL).all(), "wrote outside the rows"
    return ov[:, :n].copy()


@pytest.mark.parametrize("n", SOFTMAX_N)
def test_softmax_matches_the_model_bit_for_bit(n):
    x, want = case(n)
    kernel = 0 if n <= 1024 else 1 if n <= 8192 else 2
    for rows in (1, 3, ROWS):
        for stride in (n, n + 3):
            assert_bits(run_softmax(x[:rows], stride, 0), want[:rows], f"rows={rows} stride={stride}")
            assert opt("last_softmax_kernel") % 4 == kernel
    assert_bits(run_softmax(x, n, 1), want, "base off by one element")
    assert opt("last_softmax_kernel") == kernel + 4
    assert_bits(run_softmax(x, n + 3, 0, in_place=True), want, "in place, padded stride")
    assert_bits(run_softmax(x, n, 1, in_place=True), want, "in place, base off by one element")
    assert_bits(run_softmax(x, (n + 3) // 4 * 4, 0), want, "aligned rows")
    assert opt("last_softmax_kernel") == kernel                # rows on 16-byte boundaries: the vector instance
    assert np.isnan(want[2]).all() and np.isnan(want[4]).all() and not np.isnan(want[[0, 1, 3]]).any()


@pytest.mark.parametrize("n", [5, 1025, 8193])
def test_rows_together_and_one_by_one_give_the_same_bits(n):
    x, want = case(n)
    d = dev(x)
    import torch
    out = torch.empty_like(d)
    for r in range(ROWS):
        laser_amd.softmax(d[r:r + 1], out=out[r:r + 1])
    assert_bits(out.cpu().numpy(), want, "one-row calls")
    assert_bits(laser_amd.softmax(d).to_numpy(), want, "one call")


def test_softmax_python_argument_checks():
    x, _ = case(64)
    d = dev(x)
    with pytest.raises(ValueError):
        laser_amd.softmax(d.T)                      # last stride is not 1
    with pytest.raises(ValueError):
        laser_amd.softmax(d[0])                     # rank 1
    with pytest.raises(ValueError):
        laser_amd.softmax(d, out=dev(x[:3]))
    with pytest.raises(TypeError):
        laser_amd.softmax(dev(x.astype(np.float64)))
    with pytest.raises(laser_amd.LaserHipError):
        laser_amd.softmax(d[0:1].expand(3, 64))     # row stride 0 < n
    L = laser_amd.lib()
    assert L.laser_hip_softmax_rows_f32_dev(None, 64, None, 64, 0, 64, None) == 0      # rows = 0: nothing happens


def test_softmax_accuracy_against_float64():
    """the tolerance is the model's own: twice its largest deviation from float64 numpy on these inputs"""
    for n in (257, 4096, 16389):
        x, want = case(n)
        rows = [0] + list(range(5, ROWS))           # the rows on [-20, 20]
        x64 = x[rows].astype(np.float64)
        e = np.exp(x64 - x64.max(axis=1, keepdims=True))
        ref = e / e.sum(axis=1, keepdims=True)
        tol = 2 * np.max(np.abs(want[rows].astype(np.float64) - ref))
        got = laser_amd.softmax(dev(x)).to_numpy()[rows]
        err = np.max(np.abs(got.astype(np.float64) - ref))
        print(f"n={n}: max |softmax - float64| = {err:.3e}, tolerance {tol:.3e}")
        assert err <= tol


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "exp_softmax_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "exp_softmax_mirror.cpp"), "-o", exe, "-L", lib, "-llaser_hip",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
