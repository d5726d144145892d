"""CPU-side checks of the random numbers (include/laser_hip.h "Random numbers"): the numpy model (tests/philox_model.py)
reproduces the published Philox4x32-10 vectors and the values the header quotes; philox_core.h and random_plan.h, built as a
host program with g++ alone under ASan and UBSan, agree with the model bit for bit; the model's numbers pass two statistical
checks; the plan query follows its header without a device; the entry points are declared, exported and mirrored, refuse bad
arguments before a device is looked for, and the Python mirror refuses `u` together with `rng`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import philox_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
FILLS = ["laser_hip_random_bits_u32_dev", "laser_hip_random_uniform_f32_dev", "laser_hip_random_uniform_f64_dev",
         "laser_hip_random_uniform_i32_dev", "laser_hip_random_uniform_i64_dev"]
NEW = ["laser_hip_random_plan"] + FILLS + ["laser_hip_sampler_sample_rng_f32_dev", "laser_hip_sampler_sample_remove_rng_f32_dev"]
DEAD = 0xDEADBEEF
OFFSETS = [0, 1, 2, 3, 2 ** 32 - 1, 2 ** 34 - 2, 2 ** 64 - 3]
RANGES = {"bits_u32": (0, 0), "uniform_f32": (-1.5, 2.25), "uniform_f64": (-1.5, 2.25), "uniform_i32": (-3, 5),
          "uniform_i64": (-3, 2 ** 40)}


def hexwords(a):
    return " ".join("%08x" % v for v in np.asarray(a, np.uint32))


# ---- the model against the known answers ------------------------------------------------------------------------------------

def test_model_reproduces_the_random123_vectors():
    assert hexwords(P.philox4x32_10([0] * 4, [0] * 2)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert hexwords(P.philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert hexwords(P.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0])) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_model_stream_layout():
    assert hexwords(P.words(DEAD, 0, 0, 8)) == "cab08791 5fe5ff83 ec61bd87 82a4e06b 63adb1c7 ca65142a 4ea81475 50c963c4"
    assert hexwords(P.words(DEAD, 0, 2 ** 34 - 2, 4)) == "5f4c8de9 18e09d74 4dffa72f a4a4544f"   # carry into counter word 1
    assert hexwords(P.words(0x0123456789ABCDEF, 7, 5, 3)) == "1ee17293 3ec6e16d c5949040"
    # a word is a function of its index: any cut of a stream gives the same words, and the index wraps mod 2^64
    whole = P.words(DEAD, 3, 2 ** 64 - 5, 13)
    assert P.same_bits(whole[5:], P.words(DEAD, 3, 0, 8)) and P.same_bits(whole[:5], P.words(DEAD, 3, 2 ** 64 - 5, 5))
    assert not P.same_bits(P.words(DEAD, 0, 0, 8), P.words(DEAD, 1, 0, 8)) and not P.same_bits(P.words(DEAD, 0, 0, 8), P.words(DEAD + 1, 0, 0, 8))
    # the subsequence and the seed use their high words
    assert not P.same_bits(P.words(DEAD, 1 << 32, 0, 4), P.words(DEAD, 0, 0, 4)) and not P.same_bits(P.words(DEAD | 1 << 32, 0, 0, 4), P.words(DEAD, 0, 0, 4))


def test_model_distributions_quoted_in_the_header():
    u = P.fill("uniform_f32", 4, 0, 1, DEAD, 0, 0)
    assert u.dtype == np.float32 and u.tolist() == [np.float32(v) for v in (0.7917561, 0.3746032, 0.92336637, 0.5103283)]
    assert P.same_bits(u, P.u01_f32(P.words(DEAD, 0, 0, 4)))                 # lo = 0, hi = 1: u01's bits
    d = P.fill("uniform_f64", 1, 0, 1, DEAD, 0, 0)
    assert d.dtype == np.float64 and d[0] == 0.3746032425648895
    assert P.fill("uniform_i32", 8, -3, 5, DEAD, 0, 0).tolist() == [4, 0, 5, 1, 0, 4, -1, -1]
    top = np.array([0xffffffff], np.uint32)
    assert P.u01_f32(top)[0] == np.float32(1) - np.float32(2.0 ** -24) and P.u01_f32(np.zeros(1, np.uint32))[0] == 0
    assert P.u01_f64(np.array([2 ** 64 - 1], np.uint64))[0] == 1 - 2.0 ** -53
    f = np.float32
    for lo, hi in ((f(1), f(2)), (f(0.1), f(0.3)), (f(3), np.nextafter(f(3), f(4)))):
        v = P.uniform_f32(top, lo, hi)
        assert v.dtype == np.float32 and v[0] == hi, (lo, hi, v)
    assert f(0.1) + P.u01_f32(top)[0] * f(f(0.3) - f(0.1)) >= f(0.3)           # why the min is there
    # the integer rules at their ends
    assert P.uniform_i32(np.array([0, 0xffffffff], np.uint32), -2 ** 31, 2 ** 31 - 1).tolist() == [-2 ** 31, 2 ** 31 - 1]
    assert P.uniform_i32(np.array([0, 0xffffffff], np.uint32), 7, 7).tolist() == [7, 7]
    x = np.array([0, 1, 2 ** 63, 2 ** 64 - 1], np.uint64)
    assert P.uniform_i64(x, -2 ** 63, 2 ** 63 - 1).tolist() == [0, 1, -2 ** 63, -1]       # span 0: x as a signed value
    assert P.uniform_i64(x, -3, 5).tolist() == [-3, -3, 1, 5]
    assert P.uniform_i64(x, 2 ** 63 - 10, 2 ** 63 - 1).tolist() == [2 ** 63 - 10, 2 ** 63 - 10, 2 ** 63 - 5, 2 ** 63 - 1]
    assert [int(v) for v in P.mulhi64(x, 2 ** 64 - 1)] == [(int(v) * (2 ** 64 - 1)) >> 64 for v in x]


def test_model_statistics_of_the_first_65536_words():
    """seed 42: the mean of u01 within 5 standard errors, the top byte's chi-square within 5 standard deviations of its 255
    degrees of freedom (written down before the first run: the model gives 0.86 and 290.5)"""
    N = 1 << 16
    w = P.words(42, 0, 0, N)
    u = P.u01_f32(w).astype(np.float64)
    z = abs(u.mean() - 0.5) * np.sqrt(12 * N)
    counts = np.bincount(w >> np.uint32(24), minlength=256)
    chi2 = float(((counts - N / 256) ** 2 / (N / 256)).sum())
    print("z", z, "chi2", chi2)
    assert z < 5
    assert chi2 < 255 + 5 * np.sqrt(510)
    assert u.min() >= 0 and u.max() < 1


# ---- philox_core.h and random_plan.h as a host program --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("philox") / "philox_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-static-libasan", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "philox_host.cpp"),
                    "-o", str(exe)], check=True)

    def ask(lines):
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return ask


def bound(kind, v):
    return float(v).hex() if "_f" in kind else str(int(v))


def test_host_program_agrees_with_the_model_for_all_five_outputs(host):
    assert host(["kat 243f6a88 85a308d3 13198a2e 03707344 a4093822 299f31d0"]) == ["d16cfe09 94fdcceb 5001e420 24126ea1"]
    cases = [(kind, seed, subseq, off) for kind in P.KINDS for seed, subseq in ((DEAD, 0), (0x0123456789ABCDEF, 2 ** 40 + 7))
             for off in OFFSETS]
    n = 11
    lines = ["fill %s %x %x %x %d %s %s" % (k, s, q, o, n, bound(k, RANGES[k][0]), bound(k, RANGES[k][1])) for k, s, q, o in cases]
    for (kind, seed, subseq, off), got in zip(cases, host(lines)):
        want = P.fill(kind, n, *RANGES[kind], seed, subseq, off)
        bits = want.view(np.uint64 if want.itemsize == 8 else np.uint32)
        assert [int(t, 16) for t in got.split()] == [int(v) for v in bits], (kind, seed, subseq, off)
        if kind != "bits_u32":
            assert want.min() >= RANGES[kind][0] and want.max() <= RANGES[kind][1]
    # the float32 ranges that reach hi, the full i64 range and lo == hi
    f = np.float32
    top = 3                                                                 # any stream: compare at every word instead
    for lo, hi in ((f(1), f(2)), (f(0.1), f(0.3)), (f(3), np.nextafter(f(3), f(4))), (f(-10), f(10)), (f(2.5), f(2.5))):
        got = host(["fill uniform_f32 %x 0 0 64 %s %s" % (top, float(lo).hex(), float(hi).hex())])[0]
        want = P.fill("uniform_f32", 64, lo, hi, top, 0, 0)
        assert [int(t, 16) for t in got.split()] == want.view(np.uint32).tolist(), (lo, hi)
    got = host(["fill uniform_i64 %x 0 1 16 %d %d" % (DEAD, -2 ** 63, 2 ** 63 - 1)])[0]
    assert [int(t, 16) for t in got.split()] == [int(v) for v in P.fill("uniform_i64", 16, -2 ** 63, 2 ** 63 - 1, DEAD, 0, 1).view(np.uint64)]
    got = host(["fill uniform_i32 %x 0 1 16 %d %d" % (DEAD, -2 ** 31, 2 ** 31 - 1)])[0]
    assert [int(t, 16) for t in got.split()] == P.fill("uniform_i32", 16, -2 ** 31, 2 ** 31 - 1, DEAD, 0, 1).view(np.uint32).tolist()


def test_host_program_range_checks(host):
    good = [("0", "1"), ("-1", "1"), ("2.5", "2.5"), ("-3e38", "0"), ("0", "3e38")]
    bad = [("1", "0"), ("nan", "1"), ("0", "nan"), ("0", "inf"), ("-inf", "0"), ("-3e38", "3e38")]
    assert host(["range32 %s %s" % p for p in good] + ["range64 %s %s" % p for p in good]) == ["1"] * (2 * len(good))
    assert host(["range32 %s %s" % p for p in bad]) == ["0"] * len(bad)
    assert host(["range64 %s %s" % p for p in bad]) == ["0"] * 5 + ["1"]     # hi - lo = 6e38 is finite in float64
    assert host(["range64 -1.5e308 1.5e308"]) == ["0"]


# ---- the library without a device ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def plan(L, n, wpe, offset, mis, cus=256):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    return L.laser_hip_random_plan(n, wpe, offset, mis, cus, out), list(out)


def test_header_declares_library_exports_and_mirrors_carry_the_entry_points(L):
    from laser_amd import _lib
    import laser_amd
    hdr = re.sub(r"\s+", " ", subprocess.run(["gcc", "-E", "-P", HDR], check=True, capture_output=True, text=True).stdout)
    out = subprocess.run(["nm", "-D", "--defined-only", SO], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    nim = open(os.path.join(ROOT, "nim", "laser_hip.nim")).read()
    hpp = open(os.path.join(ROOT, "include", "laser.hpp")).read()
    for name in NEW:
        assert re.search(r"\bint " + name + r" ?\(", hdr), f"{name} not declared"
        assert name in exported, f"{name} not exported"
        assert name in _lib.declared_symbols()
        assert getattr(L, name).argtypes is not None, f"{name}: no prototype in _lib.py"
        assert f'importc: "{name}"' in nim
    for name in NEW[1:]:
        assert name in hpp
    assert re.search(r"struct Rng \{", hpp) and re.search(r"\brandomTensor\(", hpp)
    assert re.search(r"proc randomTensor\*\[T\]\(shape: openarray\[int\], valrange: Slice\[T\], rng: var HipRng\)", nim)
    assert re.search(r"proc randomTensor\*\[T\]\(shape: openarray\[int\], max: T, rng: var HipRng\)", nim)
    for name in ("Rng", "randomTensor"):
        assert hasattr(laser_amd, name)
    for meth in ("bits", "randomTensor"):
        assert callable(getattr(laser_amd.Rng, meth))
    text = open(HDR).read()
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3    # symbols were only added
    assert "an on-device RNG" not in text and "holds no random number generator" not in text


def test_plan_query(L, host):
    from laser_amd import _lib
    assert plan(L, 1000, 1, 0, 0) == (0, [0, 1, 1, 0]) and plan(L, 1000, 1, 0, 1) == (0, [1, 1, 1, 0])   # the variant flips
    assert plan(L, 1025, 1, 0, 0)[1][1] == 2 and plan(L, 1024, 1, 0, 0)[1][1] == 1 and plan(L, 1022, 1, 3, 0)[1][1] == 2   # 256 blocks a group
    assert plan(L, 512, 2, 0, 0)[1][1] == 1 and plan(L, 513, 2, 0, 0)[1][1] == 2 and plan(L, 512, 2, 3, 0)[1][1] == 2
    cap = 8 * 256
    assert plan(L, cap * 1024, 1, 0, 0)[1][1:3] == [cap, 1] and plan(L, cap * 1024 + 1, 1, 0, 0)[1][1:3] == [cap, 2]   # capped
    assert plan(L, 1 << 40, 1, 0, 0, cus=64)[1][1:3] == [512, (1 << 38) // (512 * 256)] and plan(L, 1 << 40, 1, 0, 0, cus=0)[1][1] == cap
    assert plan(L, 5, 1, 2 ** 34 - 2, 0)[1] == [0, 1, 1, 2 ** 32 - 1] and plan(L, 5, 2, 2 ** 64 - 3, 0)[1][3] == 2 ** 62 - 1
    assert plan(L, 0, 1, 7, 0) == (0, [0, 0, 0, 1]) and plan(L, 1 << 60, 2, 3, 1)[0] == 0
    for args in ((-1, 1, 0, 0), ((1 << 60) + 1, 1, 0, 0), (4, 0, 0, 0), (4, 3, 0, 0)):
        assert plan(L, *args)[0] == _lib.E_INVALID, args
    assert L.laser_hip_random_plan(4, 1, 0, 0, 256, None) == _lib.E_INVALID
    cases = [(1000, 1, 0, 0, 256), (1000, 2, 1, 1, 256), (cap * 1024 + 1, 1, 0, 0, 256), (77, 2, 2 ** 64 - 3, 0, 64), (0, 1, 5, 0, 0), (-1, 1, 0, 0, 1)]
    for c, got in zip(cases, host(["plan %d %d %x %d %d" % c for c in cases])):
        rc, p = plan(L, *c)
        got = [int(v) for v in got.split()]
        assert (got[0] == 0) == (rc == 0), c
        assert rc != 0 or got[1:] == p, (c, got, p)


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def calls(L):
    p, q = C.c_void_p(4096), C.c_void_p(1 << 20)                    # never dereferenced: arguments are checked first
    f = {"bits": lambda n, lo=None, hi=None, a=p: L.laser_hip_random_bits_u32_dev(a, n, 1, 2, 3, None)}
    for sfx in ("f32", "f64", "i32", "i64"):
        f[sfx] = lambda n, lo, hi, a=p, e=getattr(L, f"laser_hip_random_uniform_{sfx}_dev"): e(a, n, lo, hi, 1, 2, 3, None)
    f["sample"] = lambda ts, rows, n, m, a=p, b=q: L.laser_hip_sampler_sample_rng_f32_dev(a, b, ts, 1, 2, 3, rows, n, m, None)
    f["remove"] = lambda ts, rows, n, k, a=p, b=q: L.laser_hip_sampler_sample_remove_rng_f32_dev(a, b, ts, 1, 2, 3, rows, n, k, None)
    return f


def test_bad_arguments_are_invalid_before_a_device_is_looked_for(L):
    from laser_amd import _lib
    f = calls(L)
    inf, nan, big = float("inf"), float("nan"), 3e38
    bad = [f["bits"](-1), f["bits"]((1 << 60) + 1),
           f["f32"](4, 1.0, 0.0), f["f32"](4, nan, 1.0), f["f32"](4, 0.0, nan), f["f32"](4, 0.0, inf), f["f32"](4, -inf, 0.0),
           f["f32"](4, -big, big), f["f32"](-1, 0.0, 1.0),
           f["f64"](4, 1.0, 0.0), f["f64"](4, nan, 1.0), f["f64"](4, 0.0, inf), f["f64"](4, -1.5e308, 1.5e308), f["f64"](-1, 0.0, 1.0),
           f["i32"](4, 1, 0), f["i32"](-1, 0, 1), f["i64"](4, 1, 0), f["i64"](4, 2 ** 63 - 1, -2 ** 63), f["i64"](-1, 0, 1),
           f["sample"](16, 2, 0, 1), f["sample"](16, -1, 5, 1), f["sample"](16, 2, 5, -1), f["sample"](15, 2, 5, 1),
           f["sample"](16, 2, (1 << 24) + 1, 1),
           f["remove"](16, 2, (1 << 24) + 1, 1), f["remove"](16, -1, 5, 1), f["remove"](16, 2, 5, -1), f["remove"](15, 2, 5, 1)]
    assert bad == [_lib.E_INVALID] * len(bad), bad
    assert f["f32"](4, 1.0, 0.0, a=None) == _lib.E_INVALID                  # with a null pointer too
    assert f["f32"](4, 0.0, inf) == _lib.E_INVALID and b"finite" in L.laser_hip_last_error()


def test_good_arguments_need_a_gfx950_device(L):
    """argument errors first, then the device, then n = 0 and null buffers -- the order of the sampler entry points"""
    from laser_amd import _lib
    f = calls(L)
    if have_gpu():
        assert f["bits"](0, a=None) == 0 and f["f32"](0, 0.0, 1.0, a=None) == 0 and f["i64"](0, -3, 5, a=None) == 0   # nothing happens
        assert f["sample"](16, 0, 5, 3, a=None, b=None) == 0 and f["remove"](16, 2, 5, 0, a=None, b=None) == 0
        assert f["f64"](4, 0.0, 1.0, a=None) == _lib.E_INVALID and f["sample"](16, 2, 5, 3, a=None) == _lib.E_INVALID
        return
    got = [f["bits"](4), f["bits"](0), f["bits"](4, a=None), f["f32"](4, 0.0, 1.0), f["f32"](4, 2.5, 2.5), f["f32"](4, -3e38, 0.0),
           f["f64"](4, -3e38, 3e38), f["f64"](0, 0.0, 1.0), f["i32"](4, -2 ** 31, 2 ** 31 - 1), f["i32"](4, 7, 7),
           f["i64"](4, -2 ** 63, 2 ** 63 - 1), f["i64"](1 << 60, 0, 0),
           f["sample"](16, 2, 5, 3), f["sample"](16, 2, 5, 0), f["remove"](16, 2, 5, 3), f["remove"](16, 0, 5, 3)]
    assert got == [_lib.E_NODEVICE] * len(got), got
    assert f["f32"](4, 1.0, 0.0) == _lib.E_INVALID
    assert plan(L, 4, 1, 0, 0)[0] == 0                                       # the plan needs no device


def test_python_mirror_refuses_u_together_with_rng_and_checks_its_arguments(L):
    import laser_amd
    from laser_amd import random as R
    rng = laser_amd.Rng(5, subseq=2 ** 40 + 7)
    u = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="not both"):
        laser_amd.multinomial(np.ones((2, 5), np.float32), 3, u=u, rng=rng)
    s = laser_amd.Sampler(None, 2, 5)                                        # the check comes before anything touches the tree
    for draw in (s.sample, s.sampleAndRemove):
        with pytest.raises(ValueError, match="not both"):
            draw(u, 3, rng=rng)
        with pytest.raises(TypeError):
            draw(None, 3, rng=np.random.default_rng(0))
    assert (rng.seed, rng.subseq, rng.offset) == (5, 2 ** 40 + 7, 0)         # nothing was drawn
    assert rng.advance(2 ** 64 - 1) == 0 and rng.advance(3) == 2 ** 64 - 1 and rng.offset == 2     # wraps mod 2^64
    assert laser_amd.Rng(-1).seed == 2 ** 64 - 1
    for bad in (1.5, "7", True, 2 ** 64):
        with pytest.raises((TypeError, ValueError)):
            laser_amd.Rng(bad)
    f32, i32, i64 = np.dtype(np.float32), np.dtype(np.int32), np.dtype(np.int64)
    assert R._range(2.5, f32) == (0.0, 2.5) and R._range((-1, 1), f32) == (-1.0, 1.0) and R._range(slice(2, 9), i32) == (2, 9)
    assert R._range(2 ** 63 - 1, i64) == (0, 2 ** 63 - 1) and R._range((0.1, 0.3), f32) == (float(np.float32(0.1)), float(np.float32(0.3)))
    for arg, dt in (((1, 0), f32), ((0, float("inf")), f32), (float("nan"), f32), ((-3e38, 3e38), f32), ((0, 2 ** 31), i32),
                    ((0.5, 3), i32), ((5, 4), i64)):
        with pytest.raises(ValueError):
            R._range(arg, dt)
    with pytest.raises(TypeError):
        rng.randomTensor((2, 3), 1.0, np.int16)
