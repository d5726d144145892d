"""The softmax along an axis on an MI355X (laser_amd.softmax(t, axis=) / laser_hip_softmax_axis_f32_dev; include/laser_hip.h
"exp and row softmax"), bit for bit against the model of tests/softmax_axis_model.py (softmax_row per column; any NaN equals
any NaN): every axis length where a kernel changes path against every strip shape (narrower than a strip, one strip, ragged
last strips, several strips), one and three outer indices, contiguous, padded, offset, aligned and in-place layouts with a
sentinel around and between the strip rows, a lone strided column, 2^20 rows (128 chunk partials), the row kernels on the
transposed matrix, every axis of a rank-4 tensor, the Python argument checks and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import exp_model as E
from tests import softmax_axis_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)
SPECIAL = 5          # column 0 uniform on [-20, 20], 1 a spread of 200, 2 one NaN, 3 all equal, 4 all -Inf
UNIFORM = 7          # distinct uniform columns behind them, repeated with a period no strip width divides


def opt(name):
    return laser_amd.primitives.get_option(name)


def plan(outer, n, inner, vec=1):
    out = (C.c_int64 * 4)()
    assert laser_amd.lib().laser_hip_softmax_axis_plan(outer, n, inner, vec, 256, out) == 0
    return list(out)


CW = None
BOUND = None


def setup_module(_):
    global CW, BOUND
    CW = plan(1, 1, 2)[1]
    n = 1
    while plan(1, 2 * n, 2)[0] == 8:
        n *= 2
    BOUND = n
    assert plan(1, BOUND, 2)[0] == 8 and plan(1, BOUND + 1, 2)[0] == 9 and BOUND >= 1024 and CW in (16, 32)


N_GRID = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 8191, 8192, 8193, 16389]
# (at most 3 x 5 strips here; more strips than the cap of 2048 workgroups are in test_gpu_grid_stride.py)

_pools = {}


def pool(n):
    """SPECIAL + UNIFORM columns of n values and the model's softmax of each, computed once per n and never written again"""
    if n not in _pools:
        rng = np.random.default_rng(5000 + n)
        x = rng.uniform(-20, 20, (SPECIAL + UNIFORM, n)).astype(np.float32)
        x[1] = rng.uniform(-100, 100, n).astype(np.float32)
        if n > 1:
            x[1, 0], x[1, n - 1] = 100, -100
        x[2, n // 2] = np.nan
        x[3] = np.float32(1.25)
        x[4] = -np.inf
        y = E.softmax_rows(x)
        assert np.isnan(y[2]).all() and np.isnan(y[4]).all() and not np.isnan(y[[0, 1, 3] + list(range(5, 12))]).any()
        x.setflags(write=False)
        y.setflags(write=False)
        _pools[n] = (x, y)
    return _pools[n]


def case(outer, n, inner):
    """x[o, :, i] and the model's softmax of it: the first SPECIAL columns of every outer index are the special ones (so a NaN
    column and an all -Inf column sit in a strip with clean ones), the others uniform"""
    px, py = pool(n)
    i = np.arange(inner)[None, :]
    o = np.arange(outer)[:, None]
    idx = np.where(i < SPECIAL, i, SPECIAL + (i + 3 * o) % UNIFORM)            # (outer, inner)
    return np.ascontiguousarray(px[idx].transpose(0, 2, 1)), np.ascontiguousarray(py[idx].transpose(0, 2, 1))


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not E.same_bits(got, want):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


def run(x, astride, ostride, offset, in_place=False):
    """softmax along the middle axis of x (outer, n, inner) laid out with the given element strides, `offset` elements into
    the allocation; returns the result and the kernel code, and checks that nothing outside the elements was written"""
    import torch
    outer, n, inner = x.shape
    size = offset + (outer - 1) * ostride + (n - 1) * astride + inner + 1
    host = np.full(size, SENTINEL, np.float32)
    hv = np.lib.stride_tricks.as_strided(host[offset:], x.shape, (4 * ostride, 4 * astride, 4))
    hv[...] = x
    src = torch.from_numpy(host).cuda()
    dst = src if in_place else torch.full_like(src, float(SENTINEL))
    view = lambda b: b.as_strided(x.shape, (ostride, astride, 1), offset)
    laser_amd.softmax(view(src), out=view(dst), axis=1)
    code = opt("last_softmax_kernel")
    out = dst.cpu().numpy()
    ov = np.lib.stride_tricks.as_strided(out[offset:], x.shape, (4 * ostride, 4 * astride, 4))
    got = ov.copy()
    ov[...] = SENTINEL
    assert (out == SENTINEL).all(), f"wrote outside the elements: {np.nonzero(out != SENTINEL)[0][:8]}"
    return got, code


def layouts(n, inner):
    """(name, axis stride, outer stride, offset in elements, in place)"""
    up4 = lambda v: (v + 3) // 4 * 4
    a_pad = inner + 3
    a_al = up4(inner) + 4
    return [("contiguous", inner, n * inner, 0, False),
            ("padded strides", a_pad, (n - 1) * a_pad + inner + 5, 0, False),
            ("base off by one element", inner, n * inner, 1, False),
            ("strip rows on 16-byte boundaries", a_al, up4((n - 1) * a_al + inner) + 8, 4, False),
            ("in place, padded strides", a_pad, (n - 1) * a_pad + inner + 5, 0, True),
            ("in place, base off by one element", inner, n * inner, 1, True)]


def check_shape(outer, n, inner):
    x, want = case(outer, n, inner)
    base = 8 if n <= BOUND else 9
    for name, astride, ostride, offset, in_place in layouts(n, inner):
        got, code = run(x, astride, ostride, offset, in_place)
        what = f"outer={outer} n={n} inner={inner}: {name}"
        assert_bits(got, want, what)
        vec = offset % 4 == 0 and (n == 1 or astride % 4 == 0) and (outer == 1 or ostride % 4 == 0)     # strides that are applied
        assert code == base + (0 if vec else 4), (what, code)
        if name.startswith("base off"):
            assert code == base + 4
        if name.startswith("strip rows"):
            assert code == base


@pytest.mark.parametrize("n", N_GRID + ["bound", "bound+1"])
def test_softmax_axis_matches_the_model_bit_for_bit(n):
    n = BOUND if n == "bound" else BOUND + 1 if n == "bound+1" else n
    inners = sorted({2, 15, 16, 17, 31, 32, 33, 67, CW - 1, CW + 1}) if n <= 1025 else sorted({17, CW + 1})
    for inner in inners:
        for outer in (1, 3):
            check_shape(outer, n, inner)


@pytest.mark.parametrize("n", N_GRID)
def test_a_lone_strided_column(n):
    """inner == 1 with axis stride 5: not the row kernels' layout, a strip one column wide"""
    for outer in (1, 3):
        x, want = case(outer, n, 1)
        got, code = run(x, 5, (n - 1) * 5 + 1 + 2, 0)
        assert_bits(got, want, f"outer={outer} n={n}")
        if n > 1:                                 # (one element has no axis stride: that is a row of length 1)
            assert code % 4 == (0 if n <= BOUND else 1) and code >= 8
        got, code = run(x, 5, (n - 1) * 5 + 1 + 2, 0, in_place=True)
        assert_bits(got, want, f"outer={outer} n={n}, in place")
    x, want = case(3, n, 4)                       # and inner == 1 with unit strides forwards to the row kernels
    import torch
    d = torch.from_numpy(np.ascontiguousarray(x[:, :, 0])).cuda()
    got = laser_amd.softmax(d.view(3, n, 1), axis=1).to_numpy()
    assert_bits(got[:, :, 0], want[:, :, 0], "forwarded")
    assert opt("last_softmax_kernel") % 4 == (0 if n <= 1024 else 1 if n <= 8192 else 2) and opt("last_softmax_kernel") < 8


def test_one_large_case_with_128_partials():
    n = 1 << 20
    x, want = case(1, n, 2)
    assert -(-n // 8192) == 128
    got, code = run(x, 2, n * 2, 0)
    assert_bits(got, want, "n = 2^20, inner = 2")
    assert code % 4 == 1 and code >= 8
    assert not np.isnan(got).any()


@pytest.mark.parametrize("n", [5 * 8192 + 1, 6 * 8192, 13 * 8192 + 7])
def test_a_partly_filled_second_level(n):
    """5, 6 and 14 chunk partials: the fold of the partials skips the empty slots of its tree (x + 0 = x), at every width of
    that skip -- one group of 4 left over, two groups, and groups on three levels"""
    x, want = case(1, n, 17)
    got, code = run(x, 17, n * 17, 0)
    assert_bits(got, want, f"n={n}")
    assert code == 13
    got, code = run(x, 20, n * 20, 0, in_place=True)
    assert_bits(got, want, f"n={n}, aligned rows, in place")
    assert code == 9


@pytest.mark.parametrize("n", [5, 1025, 8193])
def test_axis_0_agrees_with_the_row_kernels_on_the_transposed_matrix(n):
    import torch
    rng = np.random.default_rng(77 + n)
    x = rng.uniform(-20, 20, (n, 37)).astype(np.float32)
    x[n // 2, 2] = np.nan
    x[:, 4] = -np.inf
    X = torch.from_numpy(x).cuda()
    cols = laser_amd.softmax(X, axis=0).to_numpy()
    assert opt("last_softmax_kernel") >= 8
    rows = laser_amd.softmax(X.T.contiguous()).to_numpy()
    assert opt("last_softmax_kernel") < 8
    assert_bits(cols, np.ascontiguousarray(rows.T), f"n={n}")
    assert np.isnan(cols[:, 2]).all() and np.isnan(cols[:, 4]).all() and np.isnan(cols).sum() == 2 * n
    # the transposed view itself: its axis 0 is the unit-stride one and the other dim one stride -- the rows case, no copy
    Xt = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()          # (37, n) storage; Xt.T is (n, 37) with strides (1, n)
    out = torch.full_like(Xt, float(SENTINEL))
    laser_amd.softmax(Xt.T, out=out.T, axis=0)
    assert opt("last_softmax_kernel") < 8
    assert_bits(out.cpu().numpy(), rows, f"n={n}, transposed views")
    with pytest.raises(ValueError):
        laser_amd.softmax(Xt.T, axis=0)                              # a fresh result is row-major: not the rows case, make it contiguous


def test_every_axis_of_a_rank_4_tensor():
    import torch
    rng = np.random.default_rng(9)
    x = rng.uniform(-20, 20, (2, 7, 5, 6)).astype(np.float32)
    x[1, 3, 2, 4] = np.nan
    x[0, :, 1, 1] = -np.inf
    d = torch.from_numpy(x).cuda()
    for axis in (0, 1, 2, 3, -1, -2, -3, -4):
        want = A.softmax_axis(x, axis)
        assert_bits(laser_amd.softmax(d, axis=axis).to_numpy(), want, f"axis={axis}")
        assert_bits(laser_amd.softmax(laser_amd.toTensor(x), axis=axis).to_numpy(), want, f"axis={axis}, Tensor")
        out = torch.full_like(d, float(SENTINEL))
        assert laser_amd.softmax(d, out=out, axis=axis) is out
        assert_bits(out.cpu().numpy(), want, f"axis={axis}, out=")
    v = d[:, 1:6, :, :]                                   # a slice that keeps the collapse: outer stride 210, n = 5
    assert_bits(laser_amd.softmax(v, axis=1).to_numpy(), A.softmax_axis(x[:, 1:6], 1), "slice along the axis")
    assert_bits(laser_amd.softmax(d[1], axis=0).to_numpy(), A.softmax_axis(x[1], 0), "rank 3")
    assert_bits(laser_amd.softmax(d[1, 2, 3], axis=0).to_numpy(), A.softmax_axis(x[1, 2, 3], 0), "rank 1")


def test_python_argument_checks():
    import torch
    rng = np.random.default_rng(10)
    x = rng.uniform(-20, 20, (4, 6, 8)).astype(np.float32)
    d = torch.from_numpy(x).cuda()
    with pytest.raises(ValueError):
        laser_amd.softmax(d[:, :, ::2], axis=1)             # the dims after the axis are no unit-stride run
    with pytest.raises(ValueError):
        laser_amd.softmax(d[:, 0:4:2, :], axis=2)           # the dims before the axis, (4, 2) with strides (48, 16), do not collapse
    with pytest.raises(ValueError):
        laser_amd.softmax(d, out=torch.empty(4, 6, 7, device="cuda"), axis=1)
    with pytest.raises(ValueError):
        laser_amd.softmax(d, axis=3)
    with pytest.raises(TypeError):
        laser_amd.softmax(torch.from_numpy(x.astype(np.float64)).cuda(), axis=1)
    with pytest.raises(ValueError):
        laser_amd.softmax(d, axis=None)                     # without an axis: the 2-D row form and its errors, as before
    v = d[:, ::2, :]                                         # (4, 3) with strides (48, 16) is one stride of 16: 12 rows
    assert_bits(laser_amd.softmax(v, axis=2).to_numpy(), A.softmax_axis(x[:, ::2, :], 2), "rows at a uniform stride")
    m = d[0].contiguous()
    assert_bits(laser_amd.softmax(m).to_numpy(), E.softmax_rows(x[0]), "softmax(t) without axis")
    assert opt("last_softmax_kernel") < 8
    assert_bits(laser_amd.softmax(m, axis=1).to_numpy(), E.softmax_rows(x[0]), "the last axis of a matrix = the row form")
    assert opt("last_softmax_kernel") < 8
    L = laser_amd.lib()
    assert L.laser_hip_softmax_axis_f32_dev(None, 64, 8, None, 64, 8, 0, 8, 8, None) == 0      # outer = 0: nothing happens


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "softmax_axis_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "softmax_axis_mirror.cpp"), "-o", exe, "-L", lib, "-llaser_hip",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
