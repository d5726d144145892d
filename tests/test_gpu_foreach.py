"""forEach with an arbitrary body on an MI355X (laser_amd.forEach, laser_hip_foreach_* of include/laser_hip.h): every element
type bit for bit against numpy, Laser's own `x += y * z`, mixed element types, broadcasting, aliasing, rank-6 views with
negative strides, each kernel variant where it is expected, 64-bit indices, the device math library, parameters that do not
recompile, the stride-0 check and the C++ mirror."""
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from laser_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"]


def torch_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def opt(name):
    return laser_amd.primitives.get_option(name)


def float_operands(dt, n, rng):
    """values with subnormals, +-0, +-inf-bound magnitudes and ordinary numbers"""
    f = np.finfo(dt)
    special = np.array([0.0, -0.0, f.tiny, -f.tiny, f.tiny / 8, -f.smallest_subnormal, f.smallest_subnormal, f.max, -f.max,
                        1.0, -1.0, 3.0], dt)
    a = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e3], n)).astype(dt)
    a[: special.size] = special
    sub = rng.random(n) < 0.05
    a[sub] = (rng.standard_normal(int(sub.sum())) * f.tiny).astype(dt)
    return a


def assert_bits_equal(got, want):
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert np.array_equal(gn, wn), f"NaN masks differ at {np.flatnonzero(gn != wn)[:5]}"
        ib = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        g, w = got[~gn].view(ib), want[~wn].view(ib)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{bad.size} elements differ, first {got[~gn][bad[:3]]} vs {want[~wn][bad[:3]]}"
    else:
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{bad.size} elements differ, first at {bad[:3]}: {got[bad[:3]]} vs {want[bad[:3]]}"


@pytest.mark.parametrize("dt", DTYPES)
def test_every_dtype_matches_numpy_bit_for_bit(dt):
    rng = np.random.default_rng(DTYPES.index(dt))
    n = 100_003
    if dt.startswith("float"):
        y, z, w = (float_operands(dt, n, rng) for _ in range(3))
        body = "x = (y + z) * w - y / z"
        with np.errstate(all="ignore"):
            want = (y + z) * w - y / z
    else:
        info = np.iinfo(dt)
        y, z, w = (rng.integers(info.min, info.max, n, dtype=dt, endpoint=True) for _ in range(3))
        y[:4] = [info.max, info.min, info.max, info.min]
        z[:4] = [info.max, info.min, 1, -1 if info.min < 0 else 2]
        body = "x = y * z + w - y"  # overflows and wraps mod 2^n, as numpy does
        with np.errstate(all="ignore"):
            want = y * z + w - y
    x = torch_dev(np.zeros(n, dt))
    laser_amd.forEach(body, x=x, y=torch_dev(y), z=torch_dev(z), w=torch_dev(w))
    assert opt("last_foreach_variant") == 0
    assert_bits_equal(host(x), want.astype(dt))


def test_sqrtf_and_division_are_correctly_rounded():
    rng = np.random.default_rng(9)
    y = np.abs(float_operands(np.float32, 100_000, rng))
    z = float_operands(np.float32, 100_000, rng)
    x = torch_dev(np.zeros(100_000, np.float32))
    laser_amd.forEach("x = sqrtf(y) + y / z", x=x, y=torch_dev(y), z=torch_dev(z))
    with np.errstate(all="ignore"):
        assert_bits_equal(host(x), np.sqrt(y) + y / z)


def test_laser_example_in_place():
    rng = np.random.default_rng(1)
    a, b, c = (rng.standard_normal((64, 300)).astype(np.float32) for _ in range(3))
    ta = torch_dev(a)
    laser_amd.forEach("x += y * z", x=ta, y=torch_dev(b), z=torch_dev(c))
    assert_bits_equal(host(ta), a + b * c)


def test_mixed_element_types():
    rng = np.random.default_rng(2)
    y = rng.standard_normal(5000).astype(np.float32)
    k = rng.integers(-2**31, 2**31 - 1, 5000, dtype=np.int32)
    out = torch_dev(np.zeros(5000, np.float64))
    laser_amd.forEach("x = (double)y * k + alpha", x=out, y=torch_dev(y), k=torch_dev(k), params={"alpha": 0.25})
    assert_bits_equal(host(out), y.astype(np.float64) * k.astype(np.float64) + 0.25)


def test_broadcast_row_and_scalar():
    import torch
    rng = np.random.default_rng(3)
    row = rng.standard_normal(77).astype(np.float32)
    s = np.float32(1.5)
    out = torch_dev(np.zeros((33, 77), np.float32))
    laser_amd.forEach("x = r * s", x=out, r=torch_dev(row), s=torch.tensor(s, device="cuda"))
    assert_bits_equal(host(out), np.broadcast_to(row * s, (33, 77)))
    assert opt("last_foreach_variant") == 2


def test_aliasing_same_tensor():
    rng = np.random.default_rng(4)
    a = rng.standard_normal(10_000).astype(np.float32)
    t = torch_dev(a)
    laser_amd.forEach("x = y * y + x", x=t, y=t)
    assert_bits_equal(host(t), a * a + a)


def test_rank6_views_permuted_sliced_negative_strides():
    rng = np.random.default_rng(5)
    base = rng.standard_normal((3, 4, 5, 6, 7, 8))
    other = rng.integers(-1000, 1000, (6, 3, 4, 3, 6, 3)).astype(np.int32)
    perm_b, perm_o, perm_d = (5, 3, 0, 1, 4, 2), (4, 0, 1, 3, 2, 5), (3, 0, 1, 2, 4, 5)
    vb = laser_amd.toTensor(base)[::-1, 1:, ::2, :, ::-2, 2:].transpose(*perm_b)     # (6, 6, 3, 3, 4, 3)
    nb = base[::-1, 1:, ::2, :, ::-2, 2:].transpose(perm_b)
    vo = laser_amd.toTensor(other)[::-1, :, ::-1].transpose(*perm_o)
    no = other[::-1, :, ::-1].transpose(perm_o)
    dst = laser_amd.toTensor(np.zeros((6, 3, 3, 6, 4, 3)))
    vd = dst[:, :, ::-1, ::-1].transpose(*perm_d)                                  # writable, negative strides too
    nd = np.zeros((6, 3, 3, 6, 4, 3))
    assert tuple(vb.shape) == tuple(vo.shape) == tuple(vd.shape) == nb.shape == (6, 6, 3, 3, 4, 3)
    laser_amd.forEach("d = b * 2.0 - o", d=vd, b=vb, o=vo)
    assert opt("last_foreach_variant") == 2
    nd[:, :, ::-1, ::-1].transpose(perm_d)[...] = nb * 2.0 - no
    assert_bits_equal(dst.to_numpy(), nd)


def test_each_variant_runs_where_expected():
    rng = np.random.default_rng(6)
    a = rng.standard_normal(4099).astype(np.float32)
    t, u = torch_dev(a), torch_dev(np.zeros(4099, np.float32))
    laser_amd.forEach("x = y + 1.0f", x=u, y=t)                          # aligned, n % 4 != 0: vector kernel + tail
    assert opt("last_foreach_variant") == 0
    assert_bits_equal(host(u), a + np.float32(1))
    laser_amd.forEach("x = y + 1.0f", x=u[1:], y=t[1:])                  # base one element past the alignment
    assert opt("last_foreach_variant") == 1
    assert_bits_equal(host(u)[1:], a[1:] + np.float32(1))
    for n in (1, 3, 17, 1023):                                           # lengths that are not a multiple of E
        for dt in ("int8", "float64"):                                   # E = 16 and E = 2
            v = rng.integers(-100, 100, n).astype(dt)
            x = torch_dev(np.zeros(n, dt))
            laser_amd.forEach("x = y * 3", x=x, y=torch_dev(v))
            assert opt("last_foreach_variant") == 0
            assert_bits_equal(host(x), (v * 3).astype(dt))
    m = rng.standard_normal((123, 45)).astype(np.float32)
    out = torch_dev(np.zeros((45, 123), np.float32))
    laser_amd.forEach("x = y", x=out, y=torch_dev(m).t())
    assert opt("last_foreach_variant") == 2
    assert_bits_equal(host(out), m.T)


def test_64bit_indices_int8():
    import torch
    n = 2**31 + 4099
    x = torch.zeros(n, dtype=torch.int8, device="cuda")
    laser_amd.forEach("x += 3", x=x)
    assert opt("last_foreach_variant") == 0
    torch.cuda.synchronize()
    assert int(x.min()) == 3 and int(x.max()) == 3
    assert (x[-5000:] == 3).all().item() and x[n - 1].item() == 3
    del x
    torch.cuda.empty_cache()


def ulp_distance_f32(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
    ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return np.abs(ia - ib)


def test_expf_and_logf_within_2_ulp():
    rng = np.random.default_rng(7)
    e_in = rng.uniform(-87.0, 88.0, 200_000).astype(np.float32)
    l_in = np.exp(rng.uniform(-80.0, 80.0, 200_000)).astype(np.float32)
    out = torch_dev(np.zeros(200_000, np.float32))
    laser_amd.forEach("x = expf(y)", x=out, y=torch_dev(e_in))
    ref = np.exp(e_in.astype(np.float64)).astype(np.float32)
    assert ulp_distance_f32(host(out), ref).max() <= 2
    laser_amd.forEach("x = logf(y)", x=out, y=torch_dev(l_in))
    ref = np.log(l_in.astype(np.float64)).astype(np.float32)
    assert ulp_distance_f32(host(out), ref).max() <= 2


def test_parameters_do_not_recompile():
    rng = np.random.default_rng(8)
    y = rng.standard_normal(3000).astype(np.float32)
    x = torch_dev(np.zeros(3000, np.float32))
    ty = torch_dev(y)
    laser_amd.forEach("x = y * alpha", x=x, y=ty, params={"alpha": np.float32(2.5)})
    assert_bits_equal(host(x), y * np.float32(2.5))
    before = opt("foreach_compiles")
    laser_amd.forEach("x = y * alpha", x=x, y=ty, params={"alpha": np.float32(-0.75)})
    assert_bits_equal(host(x), y * np.float32(-0.75))
    assert opt("foreach_compiles") == before


def test_writable_stride_zero_is_rejected_before_launch():
    import torch
    base = torch.zeros(1, dtype=torch.float32, device="cuda")
    y = torch_dev(np.ones(100, np.float32))
    with pytest.raises(_lib.LaserHipError) as e:
        laser_amd.forEach("x = y", x=base.expand(100), y=y)
    assert e.value.code == _lib.E_INVALID
    assert host(base)[0] == 0.0


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "foreach_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "foreach_mirror.cpp"), "-o", exe, "-L", lib, "-llaser_hip",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
