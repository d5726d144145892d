"""CPU-side checks of the softmax along an axis (include/laser_hip.h "exp and row softmax"): both entry points are declared,
exported and mirrored, the ABI version and the option table stay, laser_hip_softmax_axis_plan picks the kernels by the
bounds the header states without overflowing, the plan header runs as a host program under ASan and UBSan, every invalid
argument is refused before a device is looked for, and the model is softmax_row per column."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import exp_model as E
from tests import softmax_axis_model as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_softmax_axis_f32_dev", "laser_hip_softmax_axis_plan"]
MAX_N = 1 << 20


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def plan(L, outer, n, inner, vec=1, cus=256):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = L.laser_hip_softmax_axis_plan(outer, n, inner, vec, cus, out)
    return rc, list(out)


def test_header_declares_library_exports_and_mirrors_carry_the_entry_points(L):
    from laser_amd import _lib
    hdr = re.sub(r"\s+", " ", subprocess.run(["gcc", "-E", "-P", HDR], check=True, capture_output=True, text=True).stdout)
    out = subprocess.run(["nm", "-D", "--defined-only", SO], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    nim = open(os.path.join(ROOT, "nim", "laser_hip.nim")).read()
    hpp = open(os.path.join(ROOT, "include", "laser.hpp")).read()
    for name in NEW:
        assert re.search(r"\bint " + name + r" ?\(", hdr), f"{name} not declared"
        assert name in exported, f"{name} not exported"
        assert name in _lib.declared_symbols()
        assert f'importc: "{name}"' in nim
    assert "laser_hip_softmax_axis_f32_dev" in hpp and re.search(r"inline void softmax_axis\(", hpp)
    assert re.search(r"proc softmaxAxis\*", nim)
    text = open(HDR).read()
    assert re.search(r"#define LASER_HIP_SOFTMAX_AXIS_MAX_N \(1ll << 20\)", text)
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3


def test_the_option_table_is_unchanged_and_reports_the_kernel_read_only(L):
    from laser_amd import _lib
    names = re.findall(r'^\s*\{"(\w+)"', open(os.path.join(CSRC, "capi.cpp")).read(), re.M)
    assert len(names) == 51 and "last_softmax_kernel" in names
    assert L.laser_hip_set_option(b"last_softmax_kernel", 8) == _lib.E_INVALID


def test_plan_picks_the_kernels_by_the_bounds(L):
    rc, p = plan(L, 1, 1, 2)
    assert rc == 0 and p[0] == 8
    cw = p[1]
    assert cw in (16, 32)
    bound = 1024                                             # the resident bound: a power of two, at least 1024
    while plan(L, 1, 2 * bound, 2)[1][0] == 8:
        bound *= 2
    assert plan(L, 1, bound, 2)[1][0] == 8 and plan(L, 1, bound + 1, 2)[1][0] == 9 and bound <= 8192
    for n in (1, 2, 1023, 1024, bound):
        for vec in (0, 1):
            rc, p = plan(L, 3, n, 100, vec)
            assert rc == 0 and p[0] == 8 + (0 if vec else 4), (n, p)
            assert p[1] == cw and p[2] == 3 * -(-100 // cw) and 4096 < p[3] <= 160 * 1024
    for n in (bound + 1, 8192, 8193, MAX_N):
        for vec in (0, 1):
            rc, p = plan(L, 3, n, 100, vec)
            assert rc == 0 and p[0] == 9 + (0 if vec else 4), (n, p)
            assert p[3] >= 4096 + 128 * cw * 4               # the table and 128 partials per column
    # the grid: the strips, capped at 2048
    assert plan(L, 32, 256, 3136)[1][2] == 2048
    assert plan(L, 1, 256, 10 * cw + 1)[1][2] == 11
    for cus in (0, 64, 256, 304):                            # the grid does not depend on the compute-unit count
        assert plan(L, 1, 256, 1 << 20, cus=cus)[1][2] == 2048 and plan(L, 1, 256, 40, cus=cus)[1][2] == -(-40 // cw)
    assert plan(L, 0, 256, 64)[1][2] == 0
    for outer, inner in ((1 << 40, 3), (1 << 62, 1 << 62), (3, 1 << 62), ((1 << 63) - 1, (1 << 63) - 1)):
        rc, p = plan(L, outer, 1024, inner)
        assert rc == 0 and p[2] == 2048, (outer, inner, p)   # strips past 2^63 must not wrap into a small or negative grid
    # inner == 1: the row kernels' codes
    for n, code in ((1, 0), (1024, 0), (1025, 1), (8192, 1), (8193, 2), (1 << 26, 2)):
        rc, p = plan(L, 100, n, 1)
        assert rc == 0 and p[0] == code and p[1] == 0 and p[2] == (25 if code == 0 else 100), (n, p)
        assert plan(L, 100, n, 1, vec=0)[1][0] == code + 4
    from laser_amd import _lib
    for args in ((1, MAX_N + 1, 2), (1, 0, 2), (1, 4, 0), (-1, 4, 4), (1, (1 << 26) + 1, 1)):
        assert plan(L, *args)[0] == _lib.E_INVALID, args
    assert L.laser_hip_softmax_axis_plan(1, 4, 4, 1, 0, None) == _lib.E_INVALID


def test_plan_header_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """softmax_axis_plan.h has no HIP dependency: g++ alone builds it, with ASan and UBSan (signed overflow in the strip count
    would trap), and the program's answers are the library's"""
    exe = tmp_path / "softmax_axis_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "softmax_axis_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = [(1, 1024, 8192, 1, 256), (32, 256, 3136, 1, 256), (1 << 40, 5, 3, 0, 0), (1, 65536, 256, 1, 256), (7, 9000, 1, 0, 3),
             (1, MAX_N + 1, 2, 1, 0), (5, MAX_N, 2, 1, 1)]
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([str(exe), "-"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0), c
        if rc == 0:
            assert got[1:] == p, (c, got, p)


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    p = C.c_void_p(4096)    # never dereferenced: arguments are checked first
    q = C.c_void_p(1 << 20)
    sm = L.laser_hip_softmax_axis_f32_dev
    bad = [
        (p, 64, 8, q, 64, 8, 2, 0, 8),              # n = 0
        (p, 64, 8, q, 64, 8, 2, 8, 0),              # inner = 0
        (p, 64, 8, q, 64, 8, -1, 8, 8),             # outer < 0
        (p, 64, 7, q, 64, 8, 2, 8, 8),              # an axis stride below inner
        (p, 64, 8, q, 64, 7, 2, 8, 8),
        (p, 63, 8, q, 64, 8, 2, 8, 8),              # an outer stride below (n - 1) * axis_stride + inner
        (p, 64, 8, q, 63, 8, 2, 8, 8),
        (p, 64, 8, p, 64, 9, 1, 8, 8),              # in place with unequal strides
        (p, 80, 8, p, 64, 8, 2, 8, 8),
        (p, 1 << 40, 2, q, 1 << 40, 2, 1, MAX_N + 1, 2),     # n = 2^20 + 1 with inner = 2
        (p, 1 << 40, 5, q, 1 << 40, 5, 1, MAX_N + 1, 1),     # ... and a lone strided column
        (p, 1 << 40, 1, q, 1 << 40, 1, 1, (1 << 26) + 1, 1),  # the row kernels' bound
        (p, (1 << 63) - 1, 1 << 62, q, (1 << 63) - 1, 1 << 62, 2, 8, 8),   # (n - 1) * axis_stride past 2^63
    ]
    for args in bad:
        assert sm(*args, None) == _lib.E_INVALID, args
    assert sm(None, 64, 8, None, 64, 8, 2, 0, 8, None) == _lib.E_INVALID       # with null pointers too
    assert sm(p, 1 << 40, 2, q, 1 << 40, 2, 1, MAX_N + 1, 2, None) == _lib.E_INVALID
    assert b"2^20" in L.laser_hip_last_error()                                  # the text says which bound


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_needs_a_gfx950_device_in_the_order_of_the_rows_entry_point(L):
    """argument errors first, then the device, then outer = 0 and null buffers -- as laser_hip_softmax_rows_f32_dev"""
    if have_gpu():
        assert L.laser_hip_softmax_axis_f32_dev(None, 64, 8, None, 64, 8, 0, 8, 8, None) == 0     # outer = 0: nothing happens
        return
    from laser_amd import _lib
    p = C.c_void_p(4096)
    sm = L.laser_hip_softmax_axis_f32_dev
    assert sm(p, 64, 8, p, 64, 8, 2, 8, 8, None) == _lib.E_NODEVICE
    assert sm(p, 64, 8, p, 64, 8, 0, 8, 8, None) == _lib.E_NODEVICE
    assert sm(None, 64, 8, None, 64, 8, 2, 8, 8, None) == _lib.E_NODEVICE      # the null check needs the device first, as for rows
    assert L.laser_hip_softmax_rows_f32_dev(None, 8, None, 8, 2, 8, None) == _lib.E_NODEVICE
    assert sm(p, 64, 8, p, 64, 8, 2, 0, 8, None) == _lib.E_INVALID
    assert plan(L, 1, 8, 8)[0] == 0                                             # the plan needs no device


def test_model_is_softmax_row_per_column():
    rng = np.random.default_rng(7)
    x = rng.uniform(-20, 20, (2, 7, 5)).astype(np.float32)
    x[1, 3, 2] = np.nan
    x[0, :, 4] = -np.inf
    for axis in (0, 1, 2, -1, -3):
        y = A.softmax_axis(x, axis)
        assert y.shape == x.shape and y.dtype == np.float32
        for idx in np.ndindex(*np.delete(x.shape, axis % 3)):
            sl = list(idx)
            sl.insert(axis % 3, slice(None))
            assert E.same_bits(y[tuple(sl)], E.softmax_row(x[tuple(sl)]))
    y = A.softmax_axis(x, 1)
    assert np.isnan(y[1, :, 2]).all() and np.isnan(y[0, :, 4]).all() and np.isnan(y).sum() == 14   # that column and no other
    assert E.same_bits(A.softmax_axis(x.reshape(14, 5), 1), E.softmax_rows(x.reshape(14, 5)))


def test_python_softmax_takes_an_axis():
    import inspect
    import laser_amd
    sig = inspect.signature(laser_amd.softmax)
    assert list(sig.parameters) == ["t", "out", "axis"] and sig.parameters["axis"].default is None
    from laser_amd import simd_math as S

    class V:
        def __init__(self, shape, strides):
            self.shape, self.strides, self.rank = shape, strides, len(shape)
    # NCHW over C: outer N, inner H * W
    assert S._axis_view(V((32, 256, 56, 56), (256 * 3136, 3136, 56, 1)), 1)[0] == (32, 256 * 3136, 3136, 3136)
    assert S._axis_view(V((5, 7), (7, 1)), 0) == ((1, 0, 7, 7), None)
    strip, rows = S._axis_view(V((7, 5), (1, 7)), 0)              # a transposed view: the rows case
    assert strip is None and rows == (5, 7, 1, 1)
    assert S._axis_view(V((4, 6, 8), (96, 16, 2)), 1) == (None, None)     # the dims after the axis are no unit-stride run
    assert S._axis_view(V((4, 6, 8), (100, 10, 1)), 2)[0] is None          # the dims before the axis do not collapse
    assert S._axis_view(V((4, 6, 8), (100, 10, 1)), 1)[0] == (4, 100, 10, 8)
