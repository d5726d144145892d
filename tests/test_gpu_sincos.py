"""lsin, lcos and sincos on an MI355X (laser_amd.sin / cos / sincos, laser_sin and laser_cos in forEach bodies;
include/laser_hip.h "Sine and cosine"), bit for bit on uint32 views (NaN compared as masks) against the numpy model of
tests/sincos_model.py: the edge list and 2^16 random bit patterns, a rank-3 view with a negative stride and a gap, in place,
the lengths that cross the 16-byte path and its tail, the host-pointer forms, the reference's forEach bodies and the C++
mirror.  The inputs and the model's results are computed once and shared."""
import functools
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import reduce_model as M
from tests import sincos_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 255, 257, 4099]
SENTINEL = np.float32(-12345.0)


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    ng, nw = np.isnan(got), np.isnan(want)
    bad = np.nonzero((ng != nw) | (~ng & (g != w)))
    if bad[0].size:
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {g[first]:#x} vs {w[first]:#x}")


@functools.lru_cache(maxsize=None)
def values():
    """the edge list, 2^16 random bit patterns, and dense draws where arguments usually are; read-only"""
    rng = np.random.default_rng(51)
    bits = rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    dense = np.concatenate([rng.uniform(-10, 10, 1 << 12), rng.uniform(-2.0 ** 21, 2.0 ** 21, 1 << 12)])
    x = np.concatenate([S.edges(), bits, dense.astype(np.float32)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def model():
    s, c = S.lsincos(values())
    s.setflags(write=False)
    c.setflags(write=False)
    return s, c


def dev(a):
    return laser_amd.toTensor(np.array(a))


def test_edges_and_random_bit_patterns_through_sin_cos_and_sincos():
    x = values()
    ws, wc = model()
    t = dev(x)
    gs, gc = laser_amd.sin(t).to_numpy(), laser_amd.cos(t).to_numpy()
    assert_bits(gs, ws, "sin")
    assert_bits(gc, wc, "cos")
    bs, bc = laser_amd.sincos(t)
    assert_bits(bs.to_numpy(), ws, "sincos: sine")
    assert_bits(bc.to_numpy(), wc, "sincos: cosine")
    special = ~np.isfinite(x)
    assert special.sum() >= 8 and (gs[special].view(np.uint32) == S.NAN).all() and (gc[special].view(np.uint32) == S.NAN).all()
    fin = ~special
    assert (np.abs(gs[fin]) <= 1).all() and (np.abs(gc[fin]) <= 1).all()
    tiny = fin & (np.abs(x) < np.finfo(np.float32).tiny)                    # zeros and subnormals: x and 1, nothing flushed
    assert tiny.sum() >= 8 and np.array_equal(gs[tiny].view(np.uint32), x[tiny].view(np.uint32)) and (gc[tiny] == 1).all()
    assert_bits(laser_amd.sin(dev(-x)).to_numpy(), -ws, "lsin is odd bit for bit")
    assert_bits(laser_amd.cos(dev(-x)).to_numpy(), wc, "lcos is even bit for bit")


def test_rank3_view_with_a_negative_stride_and_a_gap_and_in_place():
    shape, keep = (5, 7, 40), 33
    n = shape[0] * shape[1] * shape[2]
    x = values()[100: 100 + n].reshape(shape)
    ws, wc = (m[100: 100 + n].reshape(shape) for m in model())
    view = lambda t: t[:, ::-1, :keep]                                      # (5, 7, 33): the middle axis reversed, the last one padded
    src = dev(x)
    for fn, want, name in ((laser_amd.sin, ws, "sin"), (laser_amd.cos, wc, "cos")):
        out = dev(np.full(shape, SENTINEL))
        fn(view(src), out=view(out))
        got = out.to_numpy()
        assert_bits(view(got), view(want), f"{name} on the view")
        assert (got[:, :, keep:] == SENTINEL).all(), "the gap elements were written"
        assert_bits(fn(view(src)).to_numpy(), view(want), f"{name} of the view into a fresh tensor")
        t = dev(x)
        fn(view(t), out=view(t))                                            # dst == src
        got = t.to_numpy()
        assert_bits(view(got), view(want), f"{name} in place on the view")
        assert_bits(got[:, :, keep:], x[:, :, keep:], "in place: the gap elements are left alone")
    assert_bits(src.to_numpy(), x, "the source is left alone")
    so, co = dev(np.full(shape, SENTINEL)), dev(np.full(shape, SENTINEL))
    laser_amd.sincos(view(src), out=(view(so), view(co)))
    for got, want in ((so.to_numpy(), ws), (co.to_numpy(), wc)):
        assert_bits(view(got), view(want), "sincos on the view = sin and cos run separately")
        assert (got[:, :, keep:] == SENTINEL).all()
    t, co = dev(x), dev(np.full(shape, SENTINEL))
    laser_amd.sincos(view(t), out=(view(t), view(co)))                      # the sine over the source
    assert_bits(view(t.to_numpy()), view(ws), "sincos, sine in place")
    assert_bits(view(co.to_numpy()), view(wc), "sincos, sine in place: the cosine")
    assert_bits(laser_amd.cos(src.T).to_numpy(), wc.T, "cos of a transposed view")


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_across_the_16_byte_path_and_its_tail(n):
    """contiguous and aligned (16-byte vectors plus the tail), then a base one element in (single elements); guards on both sides"""
    x = values()[300: 300 + n + 2]
    ws, wc = (m[300: 300 + n + 2] for m in model())
    for off in (0, 1):
        sl = slice(off, off + n)
        for fn, want, name in ((laser_amd.sin, ws, "sin"), (laser_amd.cos, wc, "cos")):
            out = dev(np.full(n + 2, SENTINEL))
            fn(dev(x)[sl], out=out[sl])
            got = out.to_numpy()
            assert_bits(got[sl], want[sl], f"{name} n={n} offset={off}")
            assert (np.delete(got, np.s_[sl]) == SENTINEL).all(), f"{name} n={n} offset={off} wrote outside"
        so, co = dev(np.full(n + 2, SENTINEL)), dev(np.full(n + 2, SENTINEL))
        laser_amd.sincos(dev(x)[sl], out=(so[sl], co[sl]))
        for got, want in ((so.to_numpy(), ws), (co.to_numpy(), wc)):
            assert_bits(got[sl], want[sl], f"sincos n={n} offset={off}")
            assert (np.delete(got, np.s_[sl]) == SENTINEL).all()


def test_host_pointer_forms():
    x = values()[:4099]
    ws, wc = (m[:4099] for m in model())
    assert_bits(laser_amd.sin(np.array(x)), ws, "sin, host pointers")
    assert_bits(laser_amd.cos(np.array(x)), wc, "cos, host pointers")
    assert laser_amd.sin(np.zeros(0, np.float32)).size == 0


def test_the_reference_bodies_in_foreach_and_foreachreduce():
    """iter_bench.nim's `o = x + y - sin z` on 1000 elements, and a sum of cosines, each operation rounded in float32"""
    rng = np.random.default_rng(52)
    f = np.float32
    x, y = rng.uniform(-4, 4, 1000).astype(f), rng.uniform(-4, 4, 1000).astype(f)
    z = np.concatenate([rng.uniform(-100, 100, 900), rng.uniform(-2.0 ** 24, 2.0 ** 24, 100)]).astype(f)
    o = laser_amd.newTensor(f, 1000)
    laser_amd.forEach("o = x + y - laser_sin(z)", o=o, x=dev(x), y=dev(y), z=dev(z))
    want = ((x + y).astype(f) - S.lsin(z)).astype(f)
    assert_bits(o.to_numpy(), want, "o = x + y - laser_sin(z)")
    laser_amd.forEach("o = laser_sin(z) + laser_cos(z)", o=o, z=dev(z))
    assert_bits(o.to_numpy(), (S.lsin(z) + S.lcos(z)).astype(f), "o = laser_sin(z) + laser_cos(z)")
    v = values()[np.isfinite(values())][:70001]
    got = laser_amd.forEachReduce("acc += laser_cos(x)", merge="acc += other", init=f(0), x=dev(v))
    want = M.reduce(S.lcos(v), f(0), M.add, M.add)
    assert np.asarray(got, f).view(np.uint32) == np.asarray(want, f).view(np.uint32), (got, want)
    t = dev(v)
    a, b = laser_amd.newTensor(f, v.size), laser_amd.newTensor(f, v.size)
    laser_amd.forEach("a = laser_sin(x); b = laser_cos(x)", writable=("a", "b"), a=a, b=b, x=t)
    assert_bits(a.to_numpy(), laser_amd.sin(t).to_numpy(), "laser_sin in a body = the kernel")
    assert_bits(b.to_numpy(), laser_amd.cos(t).to_numpy(), "laser_cos in a body = the kernel")


def test_arguments():
    d = dev(values()[:64])
    with pytest.raises(TypeError):
        laser_amd.sin(dev(np.ones(4, np.float64)))
    with pytest.raises(laser_amd.LaserHipError):
        laser_amd.sincos(d, out=(d, d))                                     # one buffer for both destinations
    with pytest.raises(ValueError):
        laser_amd.sincos(d, out=(dev(np.zeros(64, np.float32)), dev(np.zeros(32, np.float32))))


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "sincos_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "laser_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sincos_mirror.cpp"),
                    "-o", exe, "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
