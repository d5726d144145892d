"""The random numbers on the device (include/laser_hip.h "Random numbers") against the numpy model (tests/philox_model.py),
everything compared with == on the bits: the five fills at every length where the kernel changes path (partial head and tail
blocks, more than one workgroup, more than one block per lane), at offsets that carry into the second counter word and wrap
mod 2^64, on shifted destinations between sentinels; fills cut into chunks and run on two streams; the ranges; the sampler's
self-drawing entry points against uniform-fill followed by the existing ones; the Rng's bookkeeping; the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import fplus_tree_model as M
from tests import philox_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

N_GRID = [0, 1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1024, 1025, 65539]
OFFSETS = [0, 1, 2, 3, 2 ** 32 * 4 - 6, 2 ** 64 - 3]          # the carry into counter word 1, and the wrap
STREAMS = [(0xDEADBEEF00000001, 0), (0xDEADBEEF00000001, 2 ** 40 + 7), (0x0123456789ABCDEF, 0), (0x0123456789ABCDEF, 2 ** 40 + 7)]
RANGES = {"bits_u32": (0, 0), "uniform_f32": (-1.5, 2.25), "uniform_f64": (-1.5, 2.25), "uniform_i32": (-3, 5), "uniform_i64": (-3, 2 ** 40)}
KINDS = list(P.KINDS)
SENT32, SENT64 = 0x5A5A1234, 0x5A5A12345A5A4321


def L():
    return laser_amd.lib()


def stream():
    from laser_amd.tensor import _stream
    return _stream()


def plan(n, wpe, offset, mis):
    out = (C.c_int64 * 4)()
    assert L().laser_hip_random_plan(n, wpe, offset, mis, 256, out) == 0
    return list(out)


LAST_DST = [0]                                     # the device address the last gpu_fill wrote to


def gpu_fill(kind, n, lo, hi, seed, subseq, offset, shift=0):
    """the fill through the C entry point on the current stream, the destination `shift` elements into a buffer of sentinels,
    which stay"""
    dt = np.dtype(P.KINDS[kind])
    box = np.int64 if dt.itemsize == 8 else np.int32           # the Tensor element type that carries the bits
    sent = SENT64 if dt.itemsize == 8 else SENT32
    buf = np.full(shift + n + 5, sent, box)
    d = laser_amd.toTensor(buf, box)
    LAST_DST[0] = d.unsafe_raw_data() + shift * dt.itemsize
    dst, s = C.c_void_p(LAST_DST[0]), stream()
    if kind == "bits_u32":
        rc = L().laser_hip_random_bits_u32_dev(dst, n, seed, subseq, offset, s)
    else:
        rc = getattr(L(), f"laser_hip_random_{kind}_dev")(dst, n, lo, hi, seed, subseq, offset, s)
    assert rc == 0, L().laser_hip_last_error()
    out = d.to_numpy()
    assert np.all(out[:shift] == sent) and np.all(out[shift + n:] == sent), "wrote outside the destination"
    return out[shift:shift + n].view(dt)


def misaligned(wpe, offset):
    """the plan query's dst_misaligned for the last gpu_fill: its 16-byte runs start (offset & 3) - unit word words before it"""
    back = 4 * ((offset & 3) - (offset & 1 if wpe == 2 else 0))
    return int((LAST_DST[0] - back) % 16 != 0)


def model(kind, n, seed, subseq, offset, rng=None):
    lo, hi = RANGES[kind] if rng is None else rng
    return P.fill(kind, n, lo, hi, seed, subseq, offset)


@pytest.mark.parametrize("kind", KINDS)
def test_fills_match_the_model(kind):
    lo, hi = RANGES[kind]
    wpe = np.dtype(P.KINDS[kind]).itemsize // 4
    for seed, subseq in STREAMS:
        for off in OFFSETS:
            want = model(kind, max(N_GRID), seed, subseq, off)          # a fill of n elements is the first n of a longer one
            for n in N_GRID:
                if n > 1025 and (seed, subseq) != STREAMS[1]:
                    continue
                got = gpu_fill(kind, n, lo, hi, seed, subseq, off)
                assert P.same_bits(got, want[:n]), (kind, n, seed, subseq, off)
    # a length at which a lane walks more than one block, on both variants
    cap = plan(1 << 40, wpe, 0, 0)[1]
    n = cap * 256 * (4 // wpe) + 5
    assert plan(n, wpe, 3, 0)[2] >= 2
    seed, subseq = STREAMS[1]
    want = model(kind, n, seed, subseq, 3)
    variants = set()
    for shift in (1, 2, 3):                      # offset 3: 16-byte runs at shift 3 (32-bit types), at shifts 1 and 3 (64-bit types)
        got = gpu_fill(kind, n, lo, hi, seed, subseq, 3, shift=shift)
        assert P.same_bits(got, want), (kind, n, shift)
        variants.add(plan(n, wpe, 3, misaligned(wpe, 3))[0])
    assert variants == {0, 1}


@pytest.mark.parametrize("kind", KINDS)
def test_any_destination_alignment_gives_the_same_bits_and_touches_nothing_else(kind):
    lo, hi = RANGES[kind]
    seed, subseq = STREAMS[3]
    isz = np.dtype(P.KINDS[kind]).itemsize
    variants = set()
    for off in (0, 1, 2, 3, 2 ** 64 - 3):
        for n in (1, 3, 6, 257, 1031):
            want = model(kind, n, seed, subseq, off)
            for shift in range(4):
                got = gpu_fill(kind, n, lo, hi, seed, subseq, off, shift=shift)       # sentinels are checked inside
                assert P.same_bits(got, want), (kind, n, off, shift)
                variants.add(plan(n, isz // 4, off, misaligned(isz // 4, off))[0])
    assert variants == {0, 1}                                             # both kernels ran


def test_chunked_fills_and_two_streams():
    import torch
    seed, subseq = STREAMS[2]
    side = torch.cuda.Stream()
    for kind in KINDS:
        lo, hi = RANGES[kind]
        wpe = np.dtype(P.KINDS[kind]).itemsize // 4
        whole = gpu_fill(kind, 3000, lo, hi, seed, subseq, 0)
        assert P.same_bits(whole, model(kind, 3000, seed, subseq, 0))
        for a, b in ((0, 5), (1, 2), (3, 9), (1022, 1027), (1023, 2050), (2047, 3000), (6, 6)):
            part = gpu_fill(kind, b - a, lo, hi, seed, subseq, a * wpe)
            assert P.same_bits(part, whole[a:b]), (kind, a, b)
        with torch.cuda.stream(side):
            other = gpu_fill(kind, 3000, lo, hi, seed, subseq, 0)
        side.synchronize()
        assert P.same_bits(other, whole), kind


def test_ranges():
    seed, subseq = STREAMS[0]
    n, off = 4099, 2
    f = np.float32
    u01 = P.u01_f32(P.words(seed, subseq, off, n))
    for lo, hi in ((-1, 1), (-10, 10), (0, 1), (1, 2), (0.1, 0.3), (2.5, 2.5), (-3e38, 0)):
        got = gpu_fill("uniform_f32", n, lo, hi, seed, subseq, off)
        assert P.same_bits(got, model("uniform_f32", n, seed, subseq, off, (lo, hi))), (lo, hi)
        assert got.min() >= f(lo) and got.max() <= f(hi), (lo, hi)
        if (lo, hi) == (0, 1):
            assert P.same_bits(got, u01) and got.max() < 1
        if lo == hi:
            assert np.all(got == f(lo))
    for lo, hi in ((-1, 1), (0, 1), (1, 2), (-1e308, 0.5e308), (7.25, 7.25)):
        got = gpu_fill("uniform_f64", n, lo, hi, seed, subseq, off)
        assert P.same_bits(got, model("uniform_f64", n, seed, subseq, off, (lo, hi))), (lo, hi)
        assert got.min() >= lo and got.max() <= hi, (lo, hi)
    for lo, hi in ((-3, 5), (-2 ** 31, 2 ** 31 - 1), (9, 9), (2 ** 31 - 2, 2 ** 31 - 1)):
        got = gpu_fill("uniform_i32", n, lo, hi, seed, subseq, off)
        assert P.same_bits(got, model("uniform_i32", n, seed, subseq, off, (lo, hi))), (lo, hi)
        assert got.min() >= lo and got.max() <= hi, (lo, hi)
    assert sorted(set(gpu_fill("uniform_i32", n, -3, 5, seed, subseq, off).tolist())) == list(range(-3, 6))
    for lo, hi in ((-2 ** 63, 2 ** 63 - 1), (-3, 5), (-5, 2 ** 33 + 11), (2 ** 63 - 10, 2 ** 63 - 1), (-4, -4), (-2 ** 63, 2 ** 63 - 2)):
        got = gpu_fill("uniform_i64", n, lo, hi, seed, subseq, off)
        assert P.same_bits(got, model("uniform_i64", n, seed, subseq, off, (lo, hi))), (lo, hi)
        assert int(got.min()) >= lo and int(got.max()) <= hi, (lo, hi)
    assert int(gpu_fill("uniform_i64", n, -5, 2 ** 33 + 11, seed, subseq, off).max()) > 2 ** 32     # the span is used past 32 bits


# ---- the sampler's self-drawing entry points ------------------------------------------------------------------------------------

SAMPLER_KINDS = 6                                  # uniform, 60 % zeros, x 1e30, x 1e-30, denormals, all zero


def weights(rows, n, seed=0):
    """the recipe of tests/test_gpu_sampler.py"""
    rng = np.random.default_rng(1000 * n + rows + seed)
    w = rng.uniform(0, 1, (rows, n)).astype(np.float32)
    for r in range(rows):
        kind = r % SAMPLER_KINDS if rows > 1 else n % (SAMPLER_KINDS - 1)        # a lone row is never the all-zero one
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


@pytest.mark.parametrize("rows,n,m", [(1, 1, 1), (3, 5, 4), (67, 513, 7), (4, 4097, 3)])
def test_sampler_rng_draws_equal_uniform_fill_then_the_existing_entry_points(rows, n, m):
    w = weights(rows, n)
    tree = M.build(w)
    dw = laser_amd.toTensor(w, np.float32)
    seed, subseq = STREAMS[1]
    for off in (7, 2 ** 34 - 3, 2 ** 64 - 2):                              # offset & 3 != 0
        u_model = P.fill("uniform_f32", rows * m, 0, 1, seed, subseq, off).reshape(rows, m)
        # with replacement
        s = laser_amd.newSampler(dw)
        u = laser_amd.randomTensor((rows, m), (0, 1), np.float32, seed=seed, subseq=subseq, offset=off)
        assert P.same_bits(u.to_numpy(), u_model)
        two_step = s.sample(u, m).to_numpy()
        rng = laser_amd.Rng(seed, subseq, off)
        one_step = s.sample(num=m, rng=rng).to_numpy()
        assert rng.offset == (off + rows * m) % 2 ** 64
        assert one_step.dtype == np.int32 and np.array_equal(one_step, two_step), (rows, n, m, off)
        assert np.array_equal(one_step, M.draw(tree, u_model))
        assert P.same_bits(s.tree.to_numpy(), tree)                         # only read
        # without replacement: the indices and the trees afterwards
        a, b = laser_amd.newSampler(dw), laser_amd.newSampler(dw)
        two_step = a.sampleAndRemove(u, m).to_numpy()
        rng = laser_amd.Rng(seed, subseq, off)
        one_step = b.sampleAndRemove(num=m, rng=rng).to_numpy()
        assert rng.offset == (off + rows * m) % 2 ** 64
        assert np.array_equal(one_step, two_step), (rows, n, m, off)
        assert P.same_bits(b.tree.to_numpy(), a.tree.to_numpy())
        t = tree.copy()
        assert np.array_equal(one_step, M.draw_remove(t, u_model)) and P.same_bits(b.tree.to_numpy(), t)


def test_rng_bookkeeping():
    seed, subseq = STREAMS[3]
    for dt, kind, words in ((np.float32, "uniform_f32", 1), (np.float64, "uniform_f64", 2), (np.int32, "uniform_i32", 1), (np.int64, "uniform_i64", 2)):
        r = laser_amd.Rng(seed, subseq)
        a = r.randomTensor((3, 5), (-3, 5), dt)
        assert a.shape == (3, 5) and a.dtype == np.dtype(dt) and r.offset == 15 * words
        b = r.randomTensor(7, (-3, 5), dt)
        assert r.offset == 22 * words
        joint = laser_amd.Rng(seed, subseq).randomTensor(22, (-3, 5), dt).to_numpy()
        assert P.same_bits(np.concatenate([a.to_numpy().reshape(-1), b.to_numpy()]), joint)
        assert P.same_bits(joint, P.fill(kind, 22, -3, 5, seed, subseq, 0))
        assert P.same_bits(laser_amd.randomTensor(7, (-3, 5), dt, seed=seed, subseq=subseq, offset=15 * words).to_numpy(), b.to_numpy())
        mx = laser_amd.Rng(seed, subseq).randomTensor((2, 2), 5, dt).to_numpy()                # the `max` form: (0, max)
        assert P.same_bits(mx.reshape(-1), P.fill(kind, 4, 0, 5, seed, subseq, 0))
    r = laser_amd.Rng(seed, subseq, 2 ** 64 - 2)
    bits = r.bits(6).to_numpy()
    assert r.offset == 4 and P.same_bits(bits.view(np.uint32), P.words(seed, subseq, 2 ** 64 - 2, 6))
    assert r.randomTensor((0, 3), 1.0).shape == (0, 3) and r.offset == 4
    # multinomial advances by rows * num, with and without replacement
    w = weights(5, 33)
    dw = laser_amd.toTensor(w, np.float32)
    for repl in (True, False):
        r = laser_amd.Rng(seed, subseq, 9)
        idx = laser_amd.multinomial(dw, 4, replacement=repl, rng=r).to_numpy()
        assert r.offset == 9 + 5 * 4
        u = P.fill("uniform_f32", 20, 0, 1, seed, subseq, 9).reshape(5, 4)
        t = M.build(w)
        assert np.array_equal(idx, M.draw(t, u) if repl else M.draw_remove(t, u))
    with pytest.raises(ValueError):
        laser_amd.multinomial(dw, 4, u=np.zeros((5, 4), np.float32), rng=r)


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "random_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "random_mirror.cpp"), "-o", exe, "-L", lib, "-llaser_hip",
                    f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
    got = {ln.split()[0]: [int(t, 16) for t in ln.split()[1:]] for ln in r.stdout.splitlines() if ln and ln.split()[0] != "SUCCESS"}
    seed, subseq = 0x0123456789ABCDEF, 2 ** 40 + 7                          # the constants of random_mirror.cpp
    off = 0
    for name, kind, n, rng in (("f32", "uniform_f32", 10, (-1, 1)), ("f64", "uniform_f64", 5, (-1, 1)), ("i32", "uniform_i32", 6, (-3, 5)),
                               ("i64", "uniform_i64", 3, (0, 2 ** 40)), ("bits", "bits_u32", 7, (0, 0))):
        want = P.fill(kind, n, *rng, seed, subseq, off)
        assert got[name] == [int(v) for v in want.view(np.uint64 if want.itemsize == 8 else np.uint32)], name
        off += n * (want.itemsize // 4)
    w = np.array([[0.3, 1.5, 0.4, 0.3, 0.3], [0.0, 2.0, 0.0, 1.0, 0.0]], np.float32)
    t = M.build(w)
    u = P.fill("uniform_f32", 8, 0, 1, seed, subseq, off).reshape(2, 4)
    assert got["sample"] == [int(v) & 0xFFFFFFFF for v in M.draw(t, u).reshape(-1)]
    u = P.fill("uniform_f32", 8, 0, 1, seed, subseq, off + 8).reshape(2, 4)
    assert got["remove"] == [int(v) & 0xFFFFFFFF for v in M.draw_remove(t, u).reshape(-1)]
    assert got["offset"] == [off + 16]
