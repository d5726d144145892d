"""CPU-side checks of the normal random fill (include/laser_hip.h "Random numbers"; laser_amd/csrc/normal_core.h): the header as
a host program (g++, ASan + UBSan, its own main) gives the bits of the numpy model at every offset and length that cuts a pair
or a block and on forced word values; chunked fills add up; mean and std act as stated; |z| <= 5.77; 2^20 model draws from a
fixed seed pass the moment, correlation and Kolmogorov-Smirnov bounds; the entry point validates, plans with one word per
element and fails loudly without a GPU."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import normal_model as N
from tests import philox_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "cpp", "normal_core_host.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
NAME = "laser_hip_random_normal_f32_dev"
SEED, SUBSEQ = 0x0123456789abcdef, 0xfedcba9876543210
OFFSETS = [0, 1, 2, 3, 2 ** 32 - 1, 2 ** 64 - 2]
LENGTHS = [1, 2, 3, 4, 5, 1023]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """normal_core.h as a stand-alone host program under ASan and UBSan: (fill, pairs)"""
    exe = tmp_path_factory.mktemp("normal_host") / "normal_core_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN, "-I", CSRC, HOST, "-o", str(exe)], check=True)

    def fill(n, mean, std, seed, subseq, offset):
        p = subprocess.run([str(exe), "fill", str(seed), str(subseq), str(offset), str(n), str(f32_bits(mean)), str(f32_bits(std))],
                           capture_output=True)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return np.frombuffer(p.stdout, np.float32)

    def pairs(w):
        p = subprocess.run([str(exe), "pairs"], input=np.ascontiguousarray(w, np.uint32).tobytes(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return np.frombuffer(p.stdout, np.float32).reshape(-1, 4)
    return fill, pairs


@pytest.mark.parametrize("offset", OFFSETS)
def test_host_build_matches_the_model_at_every_cut(host, offset):
    fill, _ = host
    for n in LENGTHS:
        for mean, std in ((0.0, 1.0), (-3.25, 0.1)):
            got, want = fill(n, mean, std, SEED, SUBSEQ, offset), N.fill(n, mean, std, SEED, SUBSEQ, offset)
            assert N.same_bits(got, want), (offset, n, mean, std)
            assert np.isfinite(got).all()


def test_forced_word_values_cover_both_ends_of_u_and_all_four_quadrants(host):
    _, pairs = host
    vals = [0, 0xffffffff, 0xff, 0xffffff00, 0x40000000, 0x80000000, 0xc0000000, 0x3fffffff, 0x20000000, 0x1fffffff, 0x60000000, 0xe0000000]
    w = np.array([[a, b] for a in vals for b in vals], np.uint32)
    got = pairs(w)
    zc, zs = N.z_pair(w[:, 0], w[:, 1])
    assert N.same_bits(got[:, 0].copy(), zc) and N.same_bits(got[:, 1].copy(), zs)
    assert N.same_bits(got[:, 2].copy(), zc) and N.same_bits(got[:, 3].copy(), zs)          # a half on its own = the pair's half
    at = lambda a, b: got[vals.index(a) * len(vals) + vals.index(b)]
    top = np.sqrt(np.float32(-2) * np.float32(np.log(np.float32(2.0 ** -24))))
    r = at(0, 0)                                        # u = 2^-24, k = 0: the largest radius on the cosine branch, sine +0
    assert abs(r[0] - top) <= np.spacing(top) and r[0] < N.Z_MAX and r[1] == 0 and not np.signbit(r[1])
    for b in vals:                                      # u = 1: radius +0 whatever the angle
        assert (at(0xffffffff, b) == 0).all()
    quadrant = {0: (1, 0), 0x40000000: (0, 1), 0x80000000: (-1, 0), 0xc0000000: (0, -1)}
    for b, (c, s) in quadrant.items():                  # the four axes, exactly
        z = at(0, b)
        assert z[0] == c * r[0] and z[1] == s * r[0], (hex(b), z)
    for b, (sc, ss) in ((0x20000000, (1, 1)), (0x60000000, (-1, 1)), (0xe0000000, (1, -1))):   # the diagonals: |cos| = |sin|
        z = at(0, b)
        assert np.sign(z[0]) == sc and np.sign(z[1]) == ss and abs(abs(z[0]) - abs(z[1])) <= np.spacing(abs(z[0]))
    assert (np.abs(got) <= N.Z_MAX).all()


def test_chunked_fills_add_up_at_even_and_odd_cuts():
    n, off = 1023, 2 ** 32 - 3
    whole = N.fill(n, 1.5, 2.0, SEED, SUBSEQ, off)
    for cuts in ([512], [511], [1, 2, 3], [4, 9, 500, 501], [1022]):
        edges = [0] + cuts + [n]
        parts = [N.fill(b - a, 1.5, 2.0, SEED, SUBSEQ, off + a) for a, b in zip(edges, edges[1:])]
        assert N.same_bits(np.concatenate(parts), whole), cuts
    assert not N.same_bits(N.fill(n, 1.5, 2.0, SEED, SUBSEQ + 1, off), whole)
    assert not N.same_bits(N.fill(n, 1.5, 2.0, SEED + 1, SUBSEQ, off), whole)


def test_chunked_fills_add_up_on_the_host_build(host):
    fill, _ = host
    whole = fill(200, 0.0, 1.0, SEED, SUBSEQ, 5)
    assert N.same_bits(np.concatenate([fill(7, 0.0, 1.0, SEED, SUBSEQ, 5), fill(100, 0.0, 1.0, SEED, SUBSEQ, 12), fill(93, 0.0, 1.0, SEED, SUBSEQ, 112)]), whole)


def test_mean_and_std(host):
    fill, _ = host
    z = N.z_fill(4096, SEED, SUBSEQ, 7)
    plain = N.fill(4096, 0.0, 1.0, SEED, SUBSEQ, 7)
    assert np.array_equal(plain, z)                     # the values of z (a -0 comes out as +0)
    assert N.same_bits(fill(4096, 0.0, 1.0, SEED, SUBSEQ, 7), plain)
    for mean in (0.0, -2.5, 1e30):
        assert N.same_bits(fill(64, mean, 0.0, SEED, SUBSEQ, 7), np.full(64, mean, np.float32))       # std = 0 returns mean
    got = N.fill(4096, 3.0, 0.5, SEED, SUBSEQ, 7)
    assert N.same_bits(got, (np.float32(3) + (np.float32(0.5) * z).astype(np.float32)).astype(np.float32))


def test_every_z_is_bounded_and_the_moments_and_the_distribution_are_normal():
    """2^20 model draws from a fixed seed: deterministic, so never flaky.  The bounds are five standard errors for the mean, the
    variance and the correlation of the two branches of a pair, and the 0.001 critical value 1.95 / sqrt(n) of the
    Kolmogorov-Smirnov distance against Phi."""
    n = 1 << 20
    z = N.z_fill(n, 2024, 0, 0).astype(np.float64)
    assert np.abs(z).max() <= N.Z_MAX
    mean, var = z.mean(), z.var()
    corr = np.corrcoef(z[0::2], z[1::2])[0, 1]
    zs = np.sort(z)
    erf = np.vectorize(math.erf, otypes=[np.float64])
    cdf = 0.5 * (1.0 + erf(zs / math.sqrt(2.0)))
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max((i / n - cdf).max(), (cdf - (i - 1) / n).max())
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} corr {corr:.3e} ks {ks:.3e}")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(var - 1) < 5 * math.sqrt(2 / n)
    assert abs(corr) < 5 / math.sqrt(n / 2)
    assert ks < 1.95 / math.sqrt(n)


def test_validity_plan_exports_and_mirrors(L):
    from laser_amd import _lib
    import laser_amd
    assert N.params_ok(0, 1) and N.params_ok(-1e30, 0) and not N.params_ok(0, -1) and not N.params_ok(np.nan, 1)
    assert not N.params_ok(np.inf, 1) and not N.params_ok(0, np.inf) and not N.params_ok(0, np.nan) and not N.params_ok(0, -0.5)
    fn = getattr(L, NAME)
    p = C.c_void_p(4096)                                # never dereferenced: arguments are checked first
    for mean, std in ((np.nan, 1), (np.inf, 1), (-np.inf, 1), (0, -1), (0, np.nan), (0, np.inf), (0, -1e-45)):
        assert fn(p, 4, mean, std, 1, 0, 0, None) == _lib.E_INVALID, (mean, std)
    assert fn(p, -1, 0, 1, 1, 0, 0, None) == _lib.E_INVALID
    assert fn(p, (1 << 60) + 1, 0, 1, 1, 0, 0, None) == _lib.E_INVALID
    if not have_gpu():
        assert fn(p, 4, 0, 1, 1, 0, 0, None) == _lib.E_NODEVICE
        assert fn(None, 0, 0, 1, 1, 0, 0, None) == _lib.E_NODEVICE                          # the device is looked for before n = 0
        with pytest.raises(laser_amd.LaserHipError) as e:
            laser_amd.randomNormalTensor((2, 3), 0.0, 1.0, seed=1)
        assert e.value.code == _lib.E_NODEVICE
    with pytest.raises(ValueError):
        laser_amd.Rng(1).randomNormalTensor(4, 0.0, -1.0)
    with pytest.raises(ValueError):
        laser_amd.Rng(1).randomNormalTensor(4, float("nan"), 1.0)
    # the plan: one word per element, as for the 32-bit uniform fills
    out = (C.c_int64 * 4)()
    for n, offset, mis in ((1023, 0, 0), (1023, 3, 0), (4099, 2 ** 32 - 1, 1), (1 << 26, 2, 0), (1, 3, 1)):
        assert L.laser_hip_random_plan(n, 1, offset, mis, 0, out) == 0
        blocks = ((offset & 3) + n - 1) // 4 + 1
        wgs = min(-(-blocks // 256), 256 * 8)
        assert list(out) == [mis, wgs, -(-blocks // (wgs * 256)), offset >> 2], (n, offset, mis, list(out))
    # declared, exported, mirrored
    hdr = re.sub(r"\s+", " ", subprocess.run(["gcc", "-E", "-P", HDR], check=True, capture_output=True, text=True).stdout)
    assert re.search(r"\bint " + NAME + r" ?\(", hdr)
    exported = subprocess.run(["nm", "-D", "--defined-only", SO], check=True, capture_output=True, text=True).stdout
    assert NAME in exported and NAME in _lib.declared_symbols() and fn.argtypes is not None
    nim = open(os.path.join(ROOT, "nim", "laser_hip.nim")).read()
    hpp = open(os.path.join(ROOT, "include", "laser.hpp")).read()
    assert f'importc: "{NAME}"' in nim and re.search(r"proc randomNormalTensor\*", nim)
    assert NAME in hpp and re.search(r"Tensor<float> randomNormalTensor\(", hpp) and hpp.count("randomNormalTensor(") >= 3
    assert callable(laser_amd.randomNormalTensor) and callable(laser_amd.Rng.randomNormalTensor)
    core = open(os.path.join(CSRC, "normal_core.h")).read()
    for inc in ("philox_core.h", "log_core.h", "sincos_core.h"):
        assert f'#include "{inc}"' in core
    for text in (open(HDR).read(), open(os.path.join(CSRC, "philox_core.h")).read()):
        assert "Not built: float64 normals, other distributions" in text


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "normal_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)
