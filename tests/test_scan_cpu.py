"""CPU-side checks of the row cumsum, searchsorted and the inverse-CDF sampler (include/laser_hip.h "Row cumsum, searchsorted
and the inverse-CDF sampler"): the entry points are declared, exported, prototyped and mirrored, the ABI version and the option
table stay, invalid arguments are refused in the stated order before a device is looked for, the plan follows scan_plan.h, the
plan and order headers run as a host program under ASan and UBSan, and the numpy model (tests/scan_model.py) has the
properties the header claims."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
TYPES = ("f32", "f64", "i32", "i64")
NEW = ([f"laser_hip_cumsum_{t}_dev" for t in TYPES] + [f"laser_hip_searchsorted_{t}_dev" for t in TYPES] +
       ["laser_hip_cumsum_plan", "laser_hip_cdf_sample_f32_dev", "laser_hip_cdf_sample_remove_f32_dev",
        "laser_hip_cdf_sample_rng_f32_dev", "laser_hip_cdf_sample_remove_rng_f32_dev"])
MAX_N = 1 << 24
R = M.run()
TOP = np.float32(1) - np.float32(2.0 ** -24)      # the largest float32 below 1
TINY = np.float32(2.0 ** -149)                    # the smallest denormal


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def plan(L, rows, n, elem=4, cus=0):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    return L.laser_hip_cumsum_plan(rows, n, elem, cus, out), list(out)


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
        assert name == "laser_hip_cumsum_plan" or name in hpp or name.replace("f32", "##SFX##") in hpp, name
    for proc in ("cumsum", "searchsorted", "sample"):
        assert re.search(r"proc " + proc + r"\*\[", nim) or re.search(r"proc " + proc + r"\*\(", nim), proc
    assert re.search(r"proc searchsorted\*\[T\]\(input: \w+\[T\], values: \w+\[T\], leftSide", re.sub(r"\s+", " ", nim))
    for fn in ("cumsum", "searchsorted", "cdfSample", "cdfSampleAndRemove"):
        assert re.search(r"\b" + fn + r"\(", hpp), fn
        assert callable(getattr(laser_amd, fn)), fn
    text = open(HDR).read()
    assert re.search(r"#define LASER_HIP_SCAN_MAX_N \(1ll << 24\)", text)
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3
    assert "a parallel float prefix sum is not monotone, so a zero-probability element could be drawn" not in text
    assert re.search(r"#define LH_SCAN_RUN (8|16|32)\b", open(os.path.join(CSRC, "scan_core.h")).read()) and R in (8, 16, 32)


def test_the_option_table_is_unchanged(L):
    names = re.findall(r'^\s*\{"(\w+)"', open(os.path.join(CSRC, "capi.cpp")).read(), re.M)
    assert len(names) == 51 and not [n for n in names if "scan" in n or "cumsum" in n or "cdf" in n]


def test_multinomial_takes_a_method():
    import inspect
    import laser_amd
    sig = inspect.signature(laser_amd.multinomial)
    assert sig.parameters["method"].default == "ftree"
    assert list(sig.parameters)[:5] == ["probs", "num_samples", "replacement", "u", "rng"]


PLAN_GRID = [(rows, n, elem, cus) for rows in (0, 1, 3, 4, 5, 67, 2048, 2049, 8193, 1 << 40)
             for n in (1, 2, R - 1, R, R + 1, 2 * R + 1, 64 * R - 1, 64 * R, 64 * R + 1, 256 * R - 1, 256 * R, 256 * R + 1,
                       512 * R - 1, 512 * R + 1, 50000, 65537, MAX_N)
             for elem in (4, 8) for cus in (0, 1, 256, 304)]


def test_plan_follows_the_header(L):
    from laser_amd import _lib
    for rows, n, elem, cus in PLAN_GRID:
        rc, p = plan(L, rows, n, elem, cus)
        short = n <= 64 * R
        per = 4 if short else 1
        tile = 256 // per * R
        cap = 8 * (cus if cus > 0 else 256)
        assert rc == 0 and p == [0 if short else 1, per, min(-(-rows // per), cap), -(-n // tile)], (rows, n, elem, cus, p)
    for args in ((-1, 4, 4, 0), (1, 0, 4, 0), (1, MAX_N + 1, 4, 0), (1, 4, 2, 0), (1, 4, 16, 0)):
        assert plan(L, *args)[0] == _lib.E_INVALID, args
    assert L.laser_hip_cumsum_plan(1, 4, 4, 0, None) == _lib.E_INVALID


def test_plan_and_order_headers_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """scan_plan.h and scan_core.h have no HIP dependency: g++ alone builds them, with ASan and UBSan, and the plan's answers
    are the library's"""
    exe = tmp_path / "scan_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                    "-static-libasan", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "scan_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = PLAN_GRID + [(5, MAX_N + 1, 4, 0), (1, 0, 8, 0), (-1, 7, 4, 0), (3, 7, 3, 0)]
    r = subprocess.run([str(exe), "-"], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0), c
        if rc == 0:
            assert got[1:] == p, (c, got, p)


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def calls(L):
    """every entry point with its sizes and strides as keywords; the pointers are never dereferenced: arguments are checked first"""
    p, q, r, s = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(1 << 21), C.c_void_p(1 << 22)
    f = {}
    for t in TYPES:
        f["cumsum_" + t] = lambda rows=2, n=5, s0=5, s1=5, m=1, a=p, b=q, c=r, d=s, t=t: getattr(L, f"laser_hip_cumsum_{t}_dev")(
            a, s0, b, s1, rows, n, None)
        f["search_" + t] = lambda rows=2, n=5, s0=5, s1=5, m=1, a=p, b=q, c=r, d=s, t=t: getattr(L, f"laser_hip_searchsorted_{t}_dev")(
            a, b, s0, c, rows, n, m, 1, None)
    f["sample"] = lambda rows=2, n=5, s0=5, s1=5, m=1, a=p, b=q, c=r, d=s: L.laser_hip_cdf_sample_f32_dev(a, b, s0, c, rows, n, m, None)
    f["remove"] = lambda rows=2, n=5, s0=5, s1=5, m=1, a=p, b=q, c=r, d=s: L.laser_hip_cdf_sample_remove_f32_dev(
        a, b, s0, c, s1, d, rows, n, m, None)
    f["sample_rng"] = lambda rows=2, n=5, s0=5, s1=5, m=1, a=p, b=q, c=r, d=s: L.laser_hip_cdf_sample_rng_f32_dev(
        a, b, s0, 1, 2, 3, rows, n, m, None)
    f["remove_rng"] = lambda rows=2, n=5, s0=5, s1=5, m=1, a=p, b=q, c=r, d=s: L.laser_hip_cdf_sample_remove_rng_f32_dev(
        a, b, s0, c, s1, 1, 2, 3, rows, n, m, None)
    return f


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    for name, f in calls(L).items():
        two = name.startswith("cumsum") or name.startswith("remove")        # two row strides
        counted = not name.startswith("cumsum")                             # an m or a k
        bad = [f(n=0), f(n=-3), f(n=MAX_N + 1), f(rows=-1), f(s0=4)] + ([f(s1=4)] if two else []) + ([f(m=-1)] if counted else [])
        assert bad == [_lib.E_INVALID] * len(bad), (name, bad)
        assert f(s0=4, a=None, b=None, c=None, d=None) == _lib.E_INVALID, name      # with null pointers too
        assert f(n=MAX_N + 1) == _lib.E_INVALID and b"2^24" in L.laser_hip_last_error(), name   # the text says which bound
        assert f(rows=0, n=0) == _lib.E_INVALID, name                              # sizes before the empty call


def test_needs_a_gfx950_device_in_the_order_of_the_sampler_entry_points(L):
    """argument errors first, then the device, then empty calls and null buffers"""
    from laser_amd import _lib
    fs = calls(L)
    if have_gpu():
        for name, f in fs.items():
            assert f(rows=0, a=None, b=None, c=None, d=None) == 0, name                # nothing happens
            if not name.startswith("cumsum"):
                assert f(m=0, a=None, b=None, c=None, d=None) == 0, name
            assert f(a=None) == _lib.E_INVALID and f(b=None) == _lib.E_INVALID, name
        return
    for name, f in fs.items():
        got = [f(), f(rows=0), f(a=None, b=None, c=None, d=None), f(m=0)]
        assert got == [_lib.E_NODEVICE] * len(got), (name, got)
        assert f(s0=4) == _lib.E_INVALID, name
    assert plan(L, 2, 5)[0] == 0                                                        # this needs no device


# ---- the model ---------------------------------------------------------------------------------------------------------

def rows_of(rng, rows, n):
    """non-negative float32 rows: uniform, 60 % zeros, and both scaled by 1e30 and 1e-30, kinds cycling over the rows"""
    w = rng.uniform(0, 1, (rows, n)).astype(np.float32)
    for r in range(rows):
        if r % 2:
            w[r][rng.random(n) < 0.6] = 0
        w[r] *= np.float32([1, 1, 1e30, 1e30, 1e-30, 1e-30][r % 6])
    return w


def test_model_by_hand():
    """R + 2 elements: loc inside run 0, then one addition of the carry per element of run 1"""
    f = np.float32
    x = np.arange(1, R + 3).astype(np.float32) * f(0.1)
    want, acc = [], f(0)
    for i in range(R):
        acc = x[i] if i == 0 else f(acc + x[i])
        want.append(acc)
    carry = want[-1]
    want += [f(carry + x[R]), f(carry + f(x[R] + x[R + 1]))]
    got = M.cumsum(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.array(want, np.float32).view(np.uint32))
    assert np.array_equal(M.cumsum(x.reshape(1, -1))[0].view(np.uint32), got.view(np.uint32))
    neg0 = np.array([-0.0] * (R + 1), np.float32)                  # run 0 keeps -0; the carry addition keeps it too (-0 + -0)
    assert np.all(np.signbit(M.cumsum(neg0)))


def test_model_is_monotone_and_zero_weights_do_not_move_it():
    rng = np.random.default_rng(1)
    for n in (1, 2, R - 1, R, R + 1, 2 * R + 1, 1000, 3000, 4097):
        w = rows_of(rng, 12, n)
        w[:, n // 2] = np.float32(-0.0)                             # either sign of zero
        c = M.cumsum(w)
        assert np.all(np.isfinite(c))
        assert np.all(c[:, 1:] >= c[:, :-1]), n                                                     # (a)
        assert np.all((c[:, 1:] == c[:, :-1]) | (w[:, 1:] != 0)), n                                 # (b)
        for other in (8, 16, 32):                                   # the same properties at every run the sweep builds
            c2 = M.cumsum(w, other)
            assert np.all(c2[:, 1:] >= c2[:, :-1]) and np.all((c2[:, 1:] == c2[:, :-1]) | (w[:, 1:] != 0)), (n, other)


def test_model_vectorised_equals_element_by_element():
    rng = np.random.default_rng(2)
    x = rows_of(rng, 6, 5 * R + 3)
    want = np.empty_like(x)
    for r in range(x.shape[0]):
        carry = loc = np.float32(0)
        for i in range(x.shape[1]):
            loc = x[r, i] if i % R == 0 else np.float32(loc + x[r, i])
            want[r, i] = loc if i < R else np.float32(carry + loc)
            if i % R == R - 1:
                carry = want[r, i]
    assert np.array_equal(M.cumsum(x).view(np.uint32), want.view(np.uint32))


def test_model_integer_scans_wrap_like_numpy():
    rng = np.random.default_rng(3)
    for dt in (np.int32, np.int64):
        info = np.iinfo(dt)
        for n in (1, R, R + 1, 1000, 65537):
            x = rng.integers(info.min, info.max, (3, n), dtype=dt, endpoint=True)
            assert np.array_equal(M.cumsum(x), np.cumsum(x, axis=1, dtype=dt)), (dt, n)


def test_model_long_rows_take_milliseconds():
    import time
    x = np.random.default_rng(4).uniform(0, 1, (3, 65537)).astype(np.float32)
    t0 = time.perf_counter()
    M.cumsum(x)
    assert time.perf_counter() - t0 < 0.5


def test_numpy_accumulate_is_the_references_serial_order():
    """cumsum of bench_multinomial_samplers.nim:49-53: result[i] = x[i] + result[i - 1]"""
    x = np.random.default_rng(5).uniform(0, 1, 1000).astype(np.float32)
    acc = np.add.accumulate(x, dtype=np.float32)
    assert np.array_equal(acc.view(np.uint32), M.serial(x).view(np.uint32))


def test_model_stays_within_the_summation_bound_of_the_serial_order():
    """each side is a float32 summation of the same i + 1 non-negative terms with at most i additions on any path, so each is
    within gamma_i * exact of the exact sum: |model - serial| <= 2 gamma_i exact, gamma_i = i u / (1 - i u), u = 2^-24"""
    rng = np.random.default_rng(6)
    for n in (R + 1, 1000, 50000):
        w = rows_of(rng, 6, n)
        exact = np.cumsum(w.astype(np.float64), axis=1)
        i = np.arange(n, dtype=np.float64)
        gamma = i * 2.0 ** -24 / (1 - i * 2.0 ** -24)
        diff = np.abs(M.cumsum(w).astype(np.float64) - np.add.accumulate(w, axis=1, dtype=np.float32).astype(np.float64))
        assert np.all(diff <= 2 * gamma * exact), n


def test_model_passes_the_references_searchsorted_checks():
    """sanityChecks, bench_multinomial_samplers.nim:63-82"""
    for dt in (np.int32, np.int64, np.float32, np.float64):
        p = np.array([1, 2, 3, 4, 5], dt)
        assert M.searchsorted(p, np.array([3], dt)).tolist() == [2]
        assert M.searchsorted(p, np.array([3], dt), right=True).tolist() == [3]
        assert M.searchsorted(p, np.array([-10, 10, 2, 3], dt)).tolist() == [0, 5, 1, 2]
        a = np.array([[0, 3, 9, 9, 10], [1, 2, 3, 4, 5]], dt)
        v = np.array([[2, 4, 9], [0, 2, 6]], dt)
        assert M.searchsorted(a, v).tolist() == [[1, 2, 2], [0, 1, 5]]
        assert M.searchsorted(a, v, right=True).tolist() == [[1, 2, 4], [0, 2, 5]]
    rng = np.random.default_rng(7)
    for n in (1, 2, 7, 64, 1000):                                       # on sorted rows the descent is numpy's searchsorted
        a = np.sort(rng.integers(0, 50, n)).astype(np.float32)
        v = rng.integers(-2, 53, 40).astype(np.float32)
        assert np.array_equal(M.searchsorted(a, v), np.searchsorted(a, v, "left"))
        assert np.array_equal(M.searchsorted(a, v, right=True), np.searchsorted(a, v, "right"))
    nan = np.array([np.nan], np.float32)
    assert M.searchsorted(np.array([1, 2, 3], np.float32), nan).tolist() == [0]              # NaN goes left
    assert M.searchsorted(np.array([1, 2, 3], np.float32), nan, right=True).tolist() == [0]


def test_model_draw_reaches_the_last_branch_at_a_denormal_total():
    w = np.array([[0, TINY, 0, 0, 0]], np.float32)
    cdf = M.cumsum(w)
    assert cdf[0, -1] == TINY and np.float32(TOP * TINY) == TINY           # u01 * total rounds up to total
    idx, past = M.draw(cdf, np.array([[TOP, 0, 0.5]], np.float32), branch=True)
    assert past.tolist() == [[True, False, False]] and idx.tolist() == [[1, 1, 1]]     # the last positive element, never n
    assert np.float32(np.float32(0.5) * TINY) == 0                                       # (half of it rounds to even: 0)
    w = np.array([[TINY, 0, TINY, 0]], np.float32)
    idx, past = M.draw(M.cumsum(w), np.array([[TOP, 0]], np.float32), branch=True)
    assert past.tolist() == [[True, False]] and idx.tolist() == [[2, 0]]


def test_model_draw_never_returns_a_zero_weight():
    rng = np.random.default_rng(8)
    draws = 0
    for n in (1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 1000, 1025, 4097):
        w = rng.uniform(0, 1, (18, n)).astype(np.float32)
        w[rng.random((18, n)) < 0.6] = 0
        w[np.arange(18), rng.integers(0, n, 18)] = np.float32(0.5)        # no row is empty
        w *= np.float32([1, 1e30, 1e-30])[np.arange(18) % 3][:, None]
        u = rng.random((18, 64), dtype=np.float32)
        u[:, 0], u[:, 1] = 0, TOP
        idx = M.draw(M.cumsum(w), u)
        assert idx.min() >= 0 and idx.max() < n, n
        assert np.all(np.take_along_axis(w, idx.astype(np.int64), 1) > 0), n
        draws += idx.size
    assert draws >= 10000
    dead = np.array([[0, 0, 0], [1, np.inf, 1], [1, np.nan, 1], [1, 2, 3]], np.float32)
    with np.errstate(invalid="ignore"):
        assert M.draw(M.cumsum(dead), np.full((4, 2), 0.5, np.float32))[:, 0].tolist() == [-1, -1, -1, 2]


def test_model_draw_follows_the_probabilities():
    p = np.array([[0.1, 0.4, 0.3, 0.2]], np.float32)
    N = 100000
    u = np.random.default_rng(9).random((1, N), dtype=np.float32)
    counts = np.bincount(M.draw(M.cumsum(p), u)[0], minlength=4)
    q = p[0].astype(np.float64) / p[0].astype(np.float64).sum()
    assert counts.sum() == N and np.all(np.abs(counts - N * q) <= 4 * np.sqrt(N * q * (1 - q))), counts


def test_model_draw_and_remove_returns_each_positive_index_once_then_minus_one():
    rng = np.random.default_rng(10)
    w = np.zeros((1, 9), np.float32)
    w[0, [1, 4, 5, 8]] = [0.5, 2, 0.25, 1]
    keep = w.copy()
    idx = M.draw_remove(w, rng.random((1, 10), dtype=np.float32))[0]
    assert sorted(idx[:4].tolist()) == [1, 4, 5, 8] and idx[4:].tolist() == [-1] * 5 + [-1]
    assert np.all(w == 0) and not np.signbit(w).any() and keep.sum() > 0
    w = np.full((2, 3), 0.25, np.float32)
    idx = M.draw_remove(w, rng.random((2, 5), dtype=np.float32))          # columns s >= n are -1
    assert np.all(idx[:, 3:] == -1) and all(sorted(r[:3].tolist()) == [0, 1, 2] for r in idx)
