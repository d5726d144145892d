"""The normal random fill on an MI355X (laser_hip_random_normal_f32_dev, laser_amd.Rng.randomNormalTensor; include/laser_hip.h
"Random numbers"), bit for bit on uint32 views against the numpy model of tests/normal_model.py: the lengths and offsets that
cut a pair and a Philox block, the destination 0 to 3 elements off a 16-byte boundary (both plan variants, guards on both
sides), chunked fills, two subsequences, a mean and a standard deviation, the Rng bookkeeping and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import laser_amd
from tests import normal_model as N
from tests import philox_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 1023, 4099]
OFFSETS = [0, 1, 2, 3, 2 ** 32 - 1]
SEED, SUBSEQ = 0x0123456789abcdef, 2 ** 40 + 7
SENT = 0x5A5A1234
LAST_DST = [0]


def L():
    return laser_amd.lib()


def stream():
    from laser_amd.tensor import _stream
    return _stream()


def gpu_fill(n, mean, std, seed, subseq, offset, shift=0):
    """the fill through the C entry point, the destination 4 + `shift` elements into a buffer of sentinels, which stay on both
    sides"""
    buf = np.full(4 + shift + n + 5, SENT, np.int32)
    d = laser_amd.toTensor(buf, np.int32)
    base = d.unsafe_raw_data()
    lead = 4 + shift                                   # four guard elements, then the shift
    LAST_DST[0] = base + lead * 4
    rc = L().laser_hip_random_normal_f32_dev(C.c_void_p(LAST_DST[0]), n, mean, std, seed, subseq, offset, stream())
    assert rc == 0, L().laser_hip_last_error()
    out = d.to_numpy()
    assert np.all(out[:lead] == SENT) and np.all(out[lead + n:] == SENT), "wrote outside the destination"
    return out[lead:lead + n].view(np.float32)


def variant(n, offset):
    """the plan's variant for the last gpu_fill: its 16-byte runs start offset & 3 words before the destination"""
    mis = int((LAST_DST[0] - 4 * (offset & 3)) % 16 != 0)
    out = (C.c_int64 * 4)()
    assert L().laser_hip_random_plan(n, 1, offset, mis, 256, out) == 0
    return out[0]


@pytest.mark.parametrize("offset", OFFSETS)
def test_lengths_offsets_and_destination_alignments(offset):
    want = N.fill(max(LENGTHS), 0.0, 1.0, SEED, SUBSEQ, offset)             # a fill of n elements is the first n of a longer one
    variants = set()
    for n in LENGTHS:
        for shift in range(4):
            got = gpu_fill(n, 0.0, 1.0, SEED, SUBSEQ, offset, shift=shift)      # the guards are checked inside
            assert P.same_bits(got, want[:n]), (n, offset, shift)
            variants.add(variant(n, offset))
    assert variants == {0, 1}                                               # both kernels ran
    assert np.isfinite(want).all() and np.abs(want).max() <= N.Z_MAX


def test_chunked_fills_equal_one_fill_and_two_subsequences_differ():
    whole = gpu_fill(3000, 0.0, 1.0, SEED, SUBSEQ, 1)
    assert P.same_bits(whole, N.fill(3000, 0.0, 1.0, SEED, SUBSEQ, 1))
    for a, b in ((0, 5), (1, 2), (3, 9), (1022, 1027), (1023, 2050), (2047, 3000), (6, 6), (0, 1), (2, 3)):   # even and odd cuts
        part = gpu_fill(b - a, 0.0, 1.0, SEED, SUBSEQ, 1 + a)
        assert P.same_bits(part, whole[a:b]), (a, b)
    other = gpu_fill(3000, 0.0, 1.0, SEED, SUBSEQ + 1, 1)
    assert P.same_bits(other, N.fill(3000, 0.0, 1.0, SEED, SUBSEQ + 1, 1)) and not P.same_bits(other, whole)
    assert (other != whole).mean() > 0.99


def test_mean_and_std():
    z = N.z_fill(4099, SEED, SUBSEQ, 3)
    for mean, std in ((0.0, 1.0), (3.0, 0.5), (-1e-3, 7.25), (2.5, 0.0), (1e30, 1e29)):
        got = gpu_fill(4099, mean, std, SEED, SUBSEQ, 3)
        assert P.same_bits(got, N.scale(z, mean, std)), (mean, std)
    assert (gpu_fill(64, 2.5, 0.0, SEED, SUBSEQ, 3) == np.float32(2.5)).all()
    # a sample of 2^16 has the moments it should: a coarse check that the device draws are the model's distribution
    big = gpu_fill(1 << 16, 1.0, 2.0, SEED, SUBSEQ, 0).astype(np.float64)
    assert abs(big.mean() - 1.0) < 5 * 2.0 / 256 and abs(big.std() - 2.0) < 5 * 2.0 / np.sqrt(2.0 * 65536)


def test_rng_bookkeeping():
    rng = laser_amd.Rng(SEED, SUBSEQ)
    a = rng.randomNormalTensor((7, 11), 0.5, 2.0)
    assert rng.offset == 77 and a.shape == (7, 11)
    assert P.same_bits(a.to_numpy().reshape(-1), N.fill(77, 0.5, 2.0, SEED, SUBSEQ, 0))
    u = rng.randomTensor(100, (0.0, 1.0))                                   # a following uniform fill continues the stream
    assert rng.offset == 177
    assert P.same_bits(u.to_numpy(), P.fill("uniform_f32", 100, 0.0, 1.0, SEED, SUBSEQ, 77))
    b = rng.randomNormalTensor(5)                                           # starts at an odd position: a sine branch first
    assert rng.offset == 182 and P.same_bits(b.to_numpy(), N.fill(5, 0.0, 1.0, SEED, SUBSEQ, 177))
    pure = laser_amd.randomNormalTensor((7, 11), 0.5, 2.0, seed=SEED, subseq=SUBSEQ)
    assert P.same_bits(pure.to_numpy(), a.to_numpy())
    assert laser_amd.randomNormalTensor(0, 0.0, 1.0, seed=1).size == 0
    with pytest.raises(ValueError):
        rng.randomNormalTensor(4, 0.0, -1.0)
    assert rng.offset == 182
    assert L().laser_hip_random_normal_f32_dev(C.c_void_p(a.unsafe_raw_data()), 4, 0.0, float("nan"), 1, 0, 0, stream()) != 0


def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "normal_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "laser_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "normal_mirror.cpp"),
                    "-o", exe, "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
