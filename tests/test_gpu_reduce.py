"""Reductions on an MI355X (laser_amd.reduce_sum / reduce_min / reduce_max / forEachReduce, include/laser_hip.h "Reductions"):
sums bit for bit against the numpy model of the canonical order at sizes that take 1, 2 and 3 levels, integer sums that wrap,
min / max under the NaN / signed-zero rule, the reference's own check, identical bits across calls, streams, base
alignments, strided views and the host-pointer form, forEachReduce against reduce_sum and the model (dot product, int8 into
int64 over more than 2^31 elements, a writable softmax-style body, an fmaxf merge), no recompiles for new values, and the
C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import reduce_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def torch_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def opt(name):
    return laser_amd.primitives.get_option(name)


def bits(v):
    v = np.asarray(v)
    return v.view({4: np.uint32, 8: np.uint64}[v.dtype.itemsize]) if v.dtype.kind == "f" else v


def assert_same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    if got.dtype.kind == "f" and np.isnan(want):
        assert np.isnan(got), (what, got)
    else:
        assert bits(got) == bits(want), f"{what}: {got!r} vs {want!r}"


def boundary_sizes(itemsize):
    """0, 1, 2 and each level boundary -1 / +0 / +1: one, two and three levels"""
    W, R = M.constants()
    s = R * W * M.vec(itemsize)
    return [0, 1, 2, s - 1, s, s + 1, s * s - 1, s * s, s * s + 1]


def data(kind, dt, n, rng):
    if kind == "normal":
        return rng.standard_normal(n).astype(dt)
    lim = 30 if dt == np.float32 else 200   # mixed magnitudes: cancellation and absorption everywhere
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-lim, lim, n)).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["normal", "mixed"])
def test_sum_matches_the_model_bit_for_bit(dt, kind):
    rng = np.random.default_rng(11)
    sizes = boundary_sizes(np.dtype(dt).itemsize)
    assert [M.levels(n, np.dtype(dt).itemsize) for n in sizes[3:]] == [1, 1, 2, 2, 2, 3]
    for n in sizes:
        x = data(kind, dt, n, rng)
        got = laser_amd.reduce_sum(torch_dev(x))
        assert_same(got, M.model_sum(x), f"n={n}")


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_integer_sums_wrap_like_numpy(dt):
    rng = np.random.default_rng(12)
    info = np.iinfo(dt)
    for n in (1, 100_003, boundary_sizes(np.dtype(dt).itemsize)[-1]):
        x = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        assert_same(laser_amd.reduce_sum(torch_dev(x)), np.sum(x, dtype=dt), f"n={n}")


@pytest.mark.parametrize("dt", [np.float32, np.float64, np.int32, np.int64])
def test_min_max_rule(dt):
    rng = np.random.default_rng(13)
    n = 1_000_003
    if np.dtype(dt).kind == "f":
        x = rng.standard_normal(n).astype(dt)
        cases = {"plain": x.copy()}
        zeros = np.zeros(n, dt)
        zeros[rng.random(n) < 0.5] = -0.0
        cases["signed zeros"] = zeros
        cases["all -0"] = np.full(n, -0.0, dt)
        y = np.abs(x)
        y[rng.integers(0, n, 50)] = -0.0
        y[rng.integers(0, n, 50)] = 0.0
        cases["zeros below positives"] = y
        z = x.copy()
        z[rng.integers(0, n, 3)] = np.inf
        z[rng.integers(0, n, 3)] = -np.inf
        cases["inf"] = z
        w = z.copy()
        w[n - 7] = np.nan
        cases["nan late"] = w
        w = z.copy()
        w[5] = np.nan
        cases["nan early"] = w
    else:
        info = np.iinfo(dt)
        cases = {"full range": rng.integers(info.min, info.max, n, dtype=dt, endpoint=True),
                 "narrow": rng.integers(-5, 5, n).astype(dt)}
    for name, v in cases.items():
        t = torch_dev(v)
        for op, f in (("min", laser_amd.reduce_min), ("max", laser_amd.reduce_max)):
            assert_same(f(t), M.model_minmax(v, op), f"{name} {op}")
    empty = torch_dev(np.zeros(0, dt))
    assert_same(laser_amd.reduce_min(empty), M.model_minmax(np.zeros(0, dt), "min"))
    assert_same(laser_amd.reduce_max(empty), M.model_minmax(np.zeros(0, dt), "max"))
    assert_same(laser_amd.reduce_sum(empty), dt(0))


def test_reference_check_size_100():
    """tests/test_x86_reductions.nim: 100 uniform [0, 1) float32, within 1e-5 of a naive loop"""
    a = np.random.default_rng(0xDEADBEEF).random(100).astype(np.float32)
    naive = {"sum": np.float32(0), "min": np.float32(np.inf), "max": np.float32(-np.inf)}
    for v in a:
        naive["sum"] = np.float32(naive["sum"] + v)
        naive["min"] = min(naive["min"], v)
        naive["max"] = max(naive["max"], v)
    for op in ("sum", "min", "max"):
        for t in (a, torch_dev(a)):
            got = float(getattr(laser_amd, f"reduce_{op}")(t))
            assert abs(got - float(naive[op])) < 1e-5 * abs(float(naive[op])) + 1e-30
            assert abs(got - float(naive[op])) < 1e-5


class NegativeView:
    """the 2-D device array d reversed along both axes, then every s0-th row and s1-th column (negative strides)"""

    def __init__(self, d, s0, s1):
        R, C = d.shape
        it = d.element_size()
        self.keep = d
        self.__cuda_array_interface__ = {
            "shape": (-(-R // s0), -(-C // s1)), "typestr": "<f4", "version": 3,
            "data": (d.data_ptr() + it * (R * C - 1), False), "strides": (-it * C * s0, -it * s1)}


def test_same_bits_across_calls_streams_alignment_views_and_host():
    import torch
    rng = np.random.default_rng(14)
    n = 3_000_017
    x = data("mixed", np.float32, n + 3, rng)
    base = torch_dev(x)
    want = M.model_sum(x[:n])
    t = base[:n]
    for _ in range(3):
        assert_same(laser_amd.reduce_sum(t), want, "repeat")
        assert opt("last_reduce_variant") == 0
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = torch.empty(1, dtype=torch.float32, device="cuda")
        assert laser_amd.reduce_sum(t, out=out) is None
        s.synchronize()
    assert_same(out.cpu().numpy()[0], want, "side stream, device out")
    for off in (1, 2, 3):   # a base 4..12 bytes off its 16-byte alignment: the scalar traversal
        assert_same(laser_amd.reduce_sum(base[off:off + n]), M.model_sum(x[off:off + n]), f"offset {off}")
        assert opt("last_reduce_variant") == 1
    assert_same(laser_amd.reduce_sum(x[:n]), want, "host pointer")
    # strided views against their contiguous copies (same values in the same logical order)
    m = x[: 1531 * 1789].reshape(1531, 1789)
    d = torch_dev(m)
    r6 = x[: 2 * 3 * 5 * 7 * 99 * 13].reshape(2, 3, 5, 7, 99, 13)
    views = {"transposed": (d.t(), m.T),
             "negative strides": (NegativeView(d, 2, 3), m[::-1, ::-1][::2, ::3]),
             "rank-6 permuted": (torch_dev(r6).permute(5, 3, 0, 4, 2, 1), r6.transpose(5, 3, 0, 4, 2, 1))}
    for name, (v, host_view) in views.items():
        got = laser_amd.reduce_sum(v)
        assert opt("last_reduce_variant") == 2, name
        c = np.ascontiguousarray(host_view)
        assert_same(got, laser_amd.reduce_sum(torch_dev(c)), name)
        assert opt("last_reduce_variant") == 0, name
        assert_same(got, M.model_sum(c), name)
        for op in ("min", "max"):
            assert_same(getattr(laser_amd, f"reduce_{op}")(v), M.model_minmax(c, op), f"{name} {op}")
    # a broadcast view (stride 0) sums its logical elements
    b = torch_dev(x[:1000]).expand(777, 1000)
    assert_same(laser_amd.reduce_sum(b), M.model_sum(np.broadcast_to(x[:1000], (777, 1000))), "broadcast")
    # a Tensor of the project
    assert_same(laser_amd.reduce_sum(laser_amd.toTensor(m)), M.model_sum(m), "laser_amd.Tensor")


def test_foreach_reduce_sum_equals_reduce_sum_and_dot_matches_the_model():
    rng = np.random.default_rng(15)
    for n in (0, 5, 65_537, 9_000_011):
        x, y = data("mixed", np.float32, n, rng), rng.standard_normal(n).astype(np.float32)
        tx, ty = torch_dev(x), torch_dev(y)
        got = laser_amd.forEachReduce("acc += x", merge="acc += other", init=np.float32(0), x=tx)
        assert_same(got, laser_amd.reduce_sum(tx), f"acc += x, n={n}")
        dot = laser_amd.forEachReduce("acc += x * y", merge="acc += other", init=np.float32(0), x=tx, y=ty)
        with np.errstate(all="ignore"):
            want = M.reduce(x * y, np.float32(0), M.add, M.add)
        assert_same(dot, want, f"dot n={n}")
    # strided operands take the strided kernel and keep the bits of the contiguous copy
    m = torch_dev(rng.standard_normal((999, 1001)).astype(np.float32))
    got = laser_amd.forEachReduce("acc += x", merge="acc += other", init=np.float32(0), x=m.t())
    assert opt("last_foreach_variant") == 2
    assert_same(got, laser_amd.reduce_sum(m.t().contiguous()))


def test_int8_into_int64_beyond_2_pow_31_elements():
    import torch
    n = 2 ** 31 + 4099
    g = torch.Generator(device="cuda").manual_seed(16)
    x = torch.randint(-128, 128, (n,), dtype=torch.int8, device="cuda", generator=g)
    got = laser_amd.forEachReduce("acc += x", merge="acc += other", init=np.int64(0), x=x)
    want = torch.sum(x, dtype=torch.int64).item()
    assert got == want and got.dtype == np.int64
    del x
    torch.cuda.empty_cache()


def test_writable_softmax_style_body():
    import torch
    rng = np.random.default_rng(17)
    n = 1_000_003
    x = (rng.standard_normal(n) * 10).astype(np.float32)
    m = np.float32(x.max())
    y = torch.zeros(n, dtype=torch.float32, device="cuda")
    s = laser_amd.forEachReduce("y = expf(x - m); acc += y", merge="acc += other", init=np.float32(0),
                                params={"m": m}, writable=("y",), x=torch_dev(x), y=y)
    yd = y.cpu().numpy()
    ref = np.exp((x - m).astype(np.float64)).astype(np.float32)
    ia, ib = yd.view(np.int32).astype(np.int64), ref.view(np.int32).astype(np.int64)
    assert np.abs(ia - ib).max() <= 2   # every value is positive: the integer views are ordered
    assert_same(s, M.model_sum(yd), "sum of the written y")


def test_fmaxf_merge_matches_reduce_max_on_finite_nonzero_data():
    rng = np.random.default_rng(18)
    x = rng.standard_normal(2_000_003).astype(np.float32)
    x[x == 0] = 1.0
    t = torch_dev(x)
    got = laser_amd.forEachReduce("acc = fmaxf(acc, x)", merge="acc = fmaxf(acc, other)", init=np.float32(-np.inf), x=t)
    assert_same(got, laser_amd.reduce_max(t))


def test_new_params_and_init_do_not_recompile():
    rng = np.random.default_rng(19)
    t = torch_dev(rng.standard_normal(10_000).astype(np.float32))
    body, merge = "acc += x * a", "acc += other"
    laser_amd.forEachReduce(body, merge=merge, init=np.float32(0), params={"a": np.float32(1)}, x=t)
    before = opt("foreach_compiles")
    r1 = laser_amd.forEachReduce(body, merge=merge, init=np.float32(0), params={"a": np.float32(2)}, x=t)
    r2 = laser_amd.forEachReduce(body, merge=merge, init=np.float32(5), params={"a": np.float32(2)}, x=t)
    assert opt("foreach_compiles") == before
    assert r1 != r2   # init 5 is not an identity of +: every private accumulator starts from it


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "reduce_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "reduce_mirror.cpp"), "-o", exe, "-L", lib, "-llaser_hip",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
