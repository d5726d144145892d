"""CPU-side checks of the F+tree weighted sampler (include/laser_hip.h "F+tree weighted sampler"): the entry points are
declared, exported and mirrored, the ABI version and the option table stay, tree_elems and the build plan follow the header
without a device, the plan header runs as a host program under ASan and UBSan, invalid arguments are refused before a device
is looked for, and the numpy model (tests/fplus_tree_model.py) has the properties the header claims."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fplus_tree_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_sampler_tree_elems", "laser_hip_sampler_plan", "laser_hip_sampler_build_f32_dev",
       "laser_hip_sampler_sample_f32_dev", "laser_hip_sampler_sample_remove_f32_dev", "laser_hip_sampler_update_f32_dev"]
MAX_N = 1 << 24
TOP = np.float32(1) - np.float32(2.0 ** -24)      # the largest float32 below 1


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def elems(L, n):
    out = C.c_int64(-1)
    return L.laser_hip_sampler_tree_elems(n, C.byref(out)), out.value


def plan(L, rows, n):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    return L.laser_hip_sampler_plan(rows, n, out), list(out)


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
    for name in NEW[2:]:
        assert name in hpp
    assert re.search(r"struct Sampler \{", hpp)
    for proc in ("newSampler", "sample", "sampleAndRemove", "update"):
        assert re.search(r"proc " + proc + r"\*\(", nim), proc
        assert proc == "newSampler" or re.search(r"\b" + proc + r"\(", hpp), proc
    for name in ("Sampler", "newSampler", "multinomial"):
        assert hasattr(laser_amd, name)
    for meth in ("sample", "sampleAndRemove", "update"):
        assert callable(getattr(laser_amd.Sampler, meth))
    text = open(HDR).read()
    assert re.search(r"#define LASER_HIP_SAMPLER_MAX_N \(1ll << 24\)", text)
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3


def test_the_option_table_is_unchanged(L):
    names = re.findall(r'^\s*\{"(\w+)"', open(os.path.join(CSRC, "capi.cpp")).read(), re.M)
    assert len(names) == 51 and not [n for n in names if "sampler" in n]


def test_tree_elems_is_twice_the_next_power_of_two(L):
    from laser_amd import _lib
    want = {1: 2, 2: 4, 3: 8, 4: 8, 5: 16, 50000: 131072, 65536: 131072, 65537: 262144, MAX_N: 2 * MAX_N}
    for n, e in want.items():
        assert elems(L, n) == (0, e), n
        assert M.tree_elems(n) == e
    for n in (0, -1, MAX_N + 1, 1 << 40):
        assert elems(L, n)[0] == _lib.E_INVALID, n
    assert L.laser_hip_sampler_tree_elems(4, None) == _lib.E_INVALID


def test_plan_picks_the_build_kernel_by_the_leaves(L):
    from laser_amd import _lib
    for n in (1, 2, 3, 64, 511, 512):
        rc, p = plan(L, 67, n)
        per = 1024 // M.leaves(n)
        assert rc == 0 and p[0] == 0 and p[2] == -(-67 // per) and p[3] == 0, (n, p)
    for n in (513, 1024, 1025, 50000, MAX_N):
        rc, p = plan(L, 67, n)
        segs = M.leaves(n) // 1024
        assert rc == 0 and p[0] == 1 and p[1] == 1024 and p[2] == min(67 * segs, 16384) and p[3] == 67, (n, p)
    assert plan(L, 0, 50000)[1][2:] == [0, 0]
    assert plan(L, 1 << 62, MAX_N)[1][2:] == [16384, 16384] and plan(L, 1 << 62, 1)[1][2:] == [16384, 0]
    for args in ((-1, 4), (1, 0), (1, MAX_N + 1)):
        assert plan(L, *args)[0] == _lib.E_INVALID, args
    assert L.laser_hip_sampler_plan(1, 4, None) == _lib.E_INVALID


def test_plan_header_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """sampler_plan.h has no HIP dependency: g++ alone builds it, with ASan and UBSan, and its answers are the library's"""
    exe = tmp_path / "sampler_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "sampler_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = [(1, 1), (67, 5), (128, 50000), (4096, 50000), (3, 512), (3, 513), (1 << 40, 65537), (5, MAX_N), (5, MAX_N + 1), (0, 7)]
    r = subprocess.run([str(exe), "-"], input="".join("%d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0), c
        if rc == 0:
            assert got[1] == elems(L, c[1])[1] and got[2:] == p, (c, got, p)


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def calls(L):
    p, q, r = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(1 << 21)    # never dereferenced: arguments are checked first
    return {
        "build": lambda ts, ws, rows, n, a=p, b=q: L.laser_hip_sampler_build_f32_dev(a, ts, b, ws, rows, n, None),
        "sample": lambda ts, rows, n, m, a=p, b=q, c=r: L.laser_hip_sampler_sample_f32_dev(a, b, ts, c, rows, n, m, None),
        "remove": lambda ts, rows, n, k, a=p, b=q, c=r: L.laser_hip_sampler_sample_remove_f32_dev(a, b, ts, c, rows, n, k, None),
        "update": lambda ts, rows, n, a=p, b=q, c=r: L.laser_hip_sampler_update_f32_dev(a, ts, b, c, rows, n, None),
    }


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    f = calls(L)
    bad = [f["build"](16, 5, 2, 0), f["build"](16, 5, 2, MAX_N + 1), f["build"](16, 5, -1, 5), f["build"](15, 5, 2, 5),
           f["build"](16, 4, 2, 5), f["build"](2 * MAX_N - 1, MAX_N, 1, MAX_N),
           f["sample"](16, 2, 0, 1), f["sample"](16, -1, 5, 1), f["sample"](16, 2, 5, -1), f["sample"](15, 2, 5, 1),
           f["remove"](16, 2, MAX_N + 1, 1), f["remove"](16, -1, 5, 1), f["remove"](16, 2, 5, -1), f["remove"](15, 2, 5, 1),
           f["update"](16, 2, 0), f["update"](16, -1, 5), f["update"](15, 2, 5)]
    assert bad == [_lib.E_INVALID] * len(bad), bad
    assert f["build"](15, 5, 2, 5, a=None, b=None) == _lib.E_INVALID                   # with null pointers too
    assert f["build"](16, 5, 2, MAX_N + 1) == _lib.E_INVALID and b"2^24" in L.laser_hip_last_error()   # the text says which bound


def test_needs_a_gfx950_device_in_the_order_of_the_softmax_entry_points(L):
    """argument errors first, then the device, then rows = 0 and null buffers -- as laser_hip_softmax_rows_f32_dev"""
    from laser_amd import _lib
    f = calls(L)
    if have_gpu():
        assert f["build"](16, 5, 0, 5, a=None, b=None) == 0 and f["sample"](16, 0, 5, 3, a=None, b=None, c=None) == 0    # nothing happens
        assert f["sample"](16, 2, 5, 0, a=None, b=None, c=None) == 0 and f["remove"](16, 2, 5, 0, a=None, b=None, c=None) == 0
        assert f["update"](16, 0, 5, a=None, b=None, c=None) == 0
        assert f["build"](16, 5, 2, 5, a=None) == _lib.E_INVALID and f["update"](16, 2, 5, c=None) == _lib.E_INVALID
        return
    got = [f["build"](16, 5, 2, 5), f["build"](16, 5, 0, 5), f["build"](16, 5, 2, 5, a=None, b=None), f["sample"](16, 2, 5, 3),
           f["sample"](16, 2, 5, 0), f["remove"](16, 2, 5, 3), f["update"](16, 2, 5), f["update"](16, 0, 5)]
    assert got == [_lib.E_NODEVICE] * len(got), got
    assert f["build"](15, 5, 2, 5) == _lib.E_INVALID
    assert plan(L, 2, 5)[0] == 0 and elems(L, 5)[0] == 0                                # these need no device


# ---- the model ---------------------------------------------------------------------------------------------------------

def test_model_tree_of_the_demo_weights_by_hand():
    """fenwicktree.nim's demo row [0.3, 1.5, 0.4, 0.3, 0.3]: P = 8, 16 slots, shifted up by one against the reference's array"""
    f = np.float32
    w = [f(0.3), f(1.5), f(0.4), f(0.3), f(0.3)]
    a, b, c = f(w[0] + w[1]), f(w[2] + w[3]), f(w[4] + f(0))
    ab, c0 = f(a + b), f(c + f(0))
    want = np.array([0, f(ab + c0), ab, c0, a, b, c, 0, *w, 0, 0, 0], np.float32)
    t = M.build(np.array(w, np.float32))
    assert t.shape == (1, 16) and t.dtype == np.float32 and np.array_equal(t[0].view(np.uint32), want.view(np.uint32))
    assert not np.signbit(t[0, 0])
    one = M.build(np.array([[2.5], [0.0]], np.float32))                     # n = 1: the root is the leaf
    assert np.array_equal(one, np.array([[0, 2.5], [0, 0]], np.float32))


def test_model_levels_are_reduceat_of_adjacent_pairs():
    rng = np.random.default_rng(1)
    for n in (1, 2, 3, 5, 64, 65, 1000, 1025):
        w = (rng.uniform(0, 1, (3, n)) * 10.0 ** rng.integers(-30, 30, (3, 1))).astype(np.float32)
        t = M.build(w)
        P = M.leaves(n)
        assert t.shape == (3, 2 * P) and np.all(t[:, 0] == 0) and np.array_equal(t[:, P:P + n], w) and np.all(t[:, P + n:] == 0)
        size = P
        while size > 1:
            pairs = np.add.reduceat(t[:, size:2 * size], np.arange(0, size, 2), axis=1, dtype=np.float32)
            assert np.array_equal(t[:, size // 2:size].view(np.uint32), pairs.view(np.uint32)), (n, size)
            size //= 2


def test_model_draws_follow_the_probabilities():
    p = np.array([0.1, 0.4, 0.3, 0.2], np.float32)
    N = 100000
    u = np.random.default_rng(2).random((1, N), dtype=np.float32)
    idx = M.draw(M.build(p), u)[0]
    counts = np.bincount(idx, minlength=4)
    assert counts.sum() == N and idx.min() >= 0 and idx.max() < 4
    q = p.astype(np.float64) / p.astype(np.float64).sum()
    assert np.all(np.abs(counts - N * q) <= 4 * np.sqrt(N * q * (1 - q))), counts


def sparse_rows(rng, rows, n):
    w = rng.uniform(0, 1, (rows, n)).astype(np.float32)
    w[rng.random((rows, n)) < 0.6] = 0
    w[np.arange(rows), rng.integers(0, n, rows)] = np.float32(0.5)        # no row is empty
    return (w * np.float32(10.0) ** rng.integers(-30, 30, (rows, 1)).astype(np.float32)).astype(np.float32)


def test_model_guard_never_returns_an_impossible_element():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 5, 63, 64, 65, 1000, 1025, 4097):
        w = sparse_rows(rng, 24, n)
        u = rng.random((24, 64), dtype=np.float32)
        u[:, 0], u[:, 1] = 0, TOP
        t = M.build(w)
        idx = M.draw(t, u)
        assert idx.min() >= 0 and idx.max() < n, n
        assert np.all(np.take_along_axis(w, idx.astype(np.int64), 1) > 0), n
        ref = M.draw(t, u, guard=False)
        out = (ref >= n) | (np.take_along_axis(w, np.minimum(ref, n - 1).astype(np.int64), 1) <= 0)
        assert np.array_equal(idx[~out], ref[~out])        # the rules differ only where the reference's result is impossible


def test_model_draw_and_remove_returns_each_positive_index_once_then_minus_one():
    rng = np.random.default_rng(4)
    for n in (1, 2, 5, 64, 65, 300):
        w = sparse_rows(rng, 1, n)
        pos = np.flatnonzero(w[0] > 0)
        k = pos.size + 2
        u = rng.random((1, k), dtype=np.float32)
        u[0, 0], u[0, -3:] = TOP, (0, TOP, 0.5)
        t = M.build(w)
        idx = M.draw_remove(t, u)[0]
        assert sorted(idx[:-2].tolist()) == pos.tolist() and idx[-2:].tolist() == [-1, -1], n
        assert np.all(t[0, 1:] == 0) and not np.signbit(t[0]).any()


def test_model_update_gives_the_bits_of_a_rebuild():
    rng = np.random.default_rng(5)
    w = sparse_rows(rng, 6, 77)
    t = M.build(w)
    elem = np.array([0, 76, -1, 33, 5, 76])
    wt = rng.uniform(0, 3, 6).astype(np.float32)
    M.update(t, elem, wt, n=77)
    w2 = w.copy()
    for r, (e, x) in enumerate(zip(elem, wt)):
        if e >= 0:
            w2[r, e] = x
    assert np.array_equal(t.view(np.uint32), M.build(w2).view(np.uint32))
    before = t.copy()
    M.update(t, np.array([77, 100, -1, -2, 128, 77]), wt, n=77)             # outside the row: skipped
    assert np.array_equal(t.view(np.uint32), before.view(np.uint32))
