"""CPU-side checks of the dense-layer backward pass (include/laser_hip.h "Dense-layer backward"): the entry points are
declared, exported and mirrored; laser_hip_bias_grad_plan follows the stated rules and is the plan header compiled alone,
which also runs as a host program under ASan and UBSan; every invalid argument is refused before a device is looked for; a
valid call needs a gfx950 device; the kernels move 16 bytes per lane and hold no fused multiply-add; the C++ mirror compiles;
the Python layer checks its operands."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import code_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_bias_grad_f32_dev", "laser_hip_bias_grad_plan", "laser_hip_bias_grad_last_kernel"]
MAX_ROWS = 1 << 26
NONE, RELU, TANH, SIGMOID = 0, 1, 2, 3
FMA = r"v_(pk_)?fma_f32|v_fmac_f32|v_mad_f32|v_mac_f32|v_(pk_)?fma_f64|v_fmac_f64"


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


def plan(L, rows, n, vec=1, cus=256):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = L.laser_hip_bias_grad_plan(rows, n, vec, cus, out)
    return rc, list(out)


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
        assert getattr(L, name).argtypes is not None, f"{name}: no argtypes in _lib.py"
        assert f'importc: "{name}"' in nim
    assert "laser_hip_bias_grad_f32_dev" in hpp
    for fn in ("bias_grad", "linear_backward"):
        assert callable(getattr(laser_amd, fn)) and re.search(r"inline [\w<>]+ %s\(" % fn, hpp), fn
    for proc in ("biasGrad", "linearBackward"):
        assert re.search(r"proc %s\*" % proc, nim), proc
    text = open(HDR).read()
    assert "Dense-layer backward" in text and re.search(r"#define LASER_HIP_BIAS_GRAD_MAX_ROWS \(1ll << 26\)", text)
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3
    assert L.laser_hip_bias_grad_last_kernel() in (-1, 0, 1)


def test_plan_follows_the_stated_rules(L):
    from laser_amd import _lib
    for rows in (0, 1, 5, 1024, 8191, 8192, 8193, 16384, 16385, 40961, 1 << 20, MAX_ROWS):
        for n in (1, 3, 15, 16, 17, 37, 1024, 32768, 32769, 1 << 31):
            for vec in (0, 1):
                rc, p = plan(L, rows, n, vec)
                chunks, strips = max(1, -(-rows // 8192)), -(-n // 16)
                assert rc == 0, (rows, n)
                assert p[0] == (0 if vec else 1)
                assert p[1] == min(2048, chunks * strips), (rows, n, p)        # workgroups = min(2048, units)
                assert p[2] == (1 if rows <= 8192 else 2), (rows, n, p)         # one launch up to a chunk of rows, else two
                assert p[3] == (0 if rows <= 8192 else chunks * n), (rows, n, p)
    for cus in (0, 64, 256, 304):                                               # the plan does not depend on the compute units
        assert plan(L, 40961, 1000, cus=cus)[1] == [0, 6 * 63, 2, 6 * 1000]
    assert plan(L, 5, 0)[1][1:] == [0, 0, 0] and plan(L, 1 << 20, 0)[1][1:] == [0, 0, 0]     # n = 0: nothing is launched
    assert plan(L, 8192, (1 << 63) - 1)[1][1:3] == [2048, 1]                    # strips past 2^59 do not wrap
    for args in ((MAX_ROWS + 1, 4), (-1, 4), (4, -1), (MAX_ROWS, 1 << 48)):
        rc, p = plan(L, *args)
        assert rc == _lib.E_INVALID and p == [-1, -1, -1, -1], args             # -1 past 2^26 rows: nothing is written
    assert L.laser_hip_bias_grad_plan(4, 4, 1, 0, None) == _lib.E_INVALID


def test_plan_header_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """bias_grad_plan.h has no HIP dependency: g++ alone builds it, with ASan and UBSan (signed overflow in the unit count or
    the scratch size would trap), and the program's answers are the library's"""
    exe = tmp_path / "bias_grad_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "bias_grad_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = [(0, 17, 1, 256), (1, 1, 0, 0), (8192, 37, 1, 256), (8193, 37, 0, 3), (40961, 17, 1, 256), (65536, 1024, 1, 256),
             (4096, 4096, 1, 256), (256, 8192, 1, 256), (MAX_ROWS, 1 << 20, 1, 1), (MAX_ROWS + 1, 4, 1, 0), (7, 0, 1, 0), (-3, 4, 0, 0),
             (8192, (1 << 63) - 1, 1, 0), (MAX_ROWS, 1 << 48, 1, 0)]
    text = "".join("%d %d %d %d\n" % c for c in cases)
    r = subprocess.run([str(exe), "-"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0), c
        assert got[1:] == p, (c, got, p)


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    bg = L.laser_hip_bias_grad_f32_dev
    db, dz, dy, y = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))     # never dereferenced: arguments are checked first
    bad = [
        (db, 1, dz, 8, dy, 8, y, 8, -1, 8, TANH),                   # negative sizes
        (db, 1, dz, 8, dy, 8, y, 8, 4, -8, TANH),
        (db, 1, dz, 7, dy, 8, y, 8, 4, 8, TANH),                    # a row stride below n: dz, dy, y
        (db, 1, dz, 8, dy, 7, y, 8, 4, 8, TANH),
        (db, 1, dz, 8, dy, 8, y, 7, 4, 8, TANH),
        (db, 1, dz, 8, dy, 0, None, 0, 4, 8, NONE),
        (db, 1, dz, 1 << 40, dy, 1 << 40, y, 1 << 40, MAX_ROWS + 1, 8, RELU),    # rows past 2^26
        (db, 1, dz, 8, dy, 8, y, 8, 4, 8, 4),                       # a bad act
        (db, 1, dz, 8, dy, 8, y, 8, 4, 8, -1),
        (db, 1, dz, 8, dy, 8, y, 8, 4, 8, 0x100 | 1),
        (None, 1, dz, 8, dy, 8, y, 8, 4, 8, TANH),                  # NULL db
        (db, 1, dz, 8, dy, 8, None, 8, 4, 8, TANH),                 # NULL y with an activation
        (db, 1, dz, 8, dy, 8, None, 8, 4, 8, RELU),
        (db, 1, dz, 8, dy, 8, None, 8, 4, 8, SIGMOID),
        (db, 1, dz, 8, None, 8, y, 8, 4, 8, TANH),                  # NULL dy
        (db, 1, dy, 9, dy, 8, y, 8, 4, 8, TANH),                    # dz in place over dy / y with unequal row strides
        (db, 1, y, 8, dy, 8, y, 9, 4, 8, TANH),
    ]
    for args in bad:
        assert bg(*args, None) == _lib.E_INVALID, args
    # NULL-safe ordering: the sizes, the strides and the code are judged before any pointer, with every pointer NULL too
    assert bg(None, 1, None, 8, None, 8, None, 8, -1, 8, TANH, None) == _lib.E_INVALID
    assert bg(None, 1, None, 8, None, 7, None, 8, 4, 8, TANH, None) == _lib.E_INVALID
    assert bg(None, 1, None, 8, None, 8, None, 8, 4, 8, 9, None) == _lib.E_INVALID
    assert bg(None, 1, None, 8, None, 8, None, 8, MAX_ROWS + 1, 8, NONE, None) == _lib.E_INVALID
    assert b"2^26" in L.laser_hip_last_error()                       # the text says which bound


def test_a_valid_call_needs_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one, the calls that touch nothing succeed"""
    from laser_amd import _lib
    bg = L.laser_hip_bias_grad_f32_dev
    if have_gpu():
        assert bg(None, 1, None, 0, None, 0, None, 0, 4, 0, NONE, None) == 0          # n = 0: nothing happens
        return
    db, dz, dy, y = (C.c_void_p(4096 * k) for k in (1, 2, 3, 4))
    assert bg(db, 1, dz, 8, dy, 8, y, 8, 4, 8, TANH, None) == _lib.E_NODEVICE
    assert bg(db, 1, None, 0, dy, 8, None, 0, 4, 8, NONE, None) == _lib.E_NODEVICE      # the plain column sum
    assert bg(db, 1, dy, 8, dy, 8, y, 8, 4, 8, SIGMOID, None) == _lib.E_NODEVICE        # in place
    assert bg(db, 1, None, 0, None, 8, None, 0, 0, 8, NONE, None) == _lib.E_NODEVICE    # rows = 0 still writes db = +0
    assert bg(None, 1, None, 0, None, 0, None, 0, 4, 0, NONE, None) == _lib.E_NODEVICE  # n = 0 is judged after the device
    assert plan(L, 4, 8)[0] == 0                                                        # the plan needs no device
    import laser_amd
    assert not hasattr(np.ones((4, 8), np.float32), "__cuda_array_interface__")
    with pytest.raises(TypeError):
        laser_amd.bias_grad(np.ones((4, 8), np.float32))              # a host array is not taken (and nothing falls back)


def test_kernels_vectorise_and_hold_no_fused_multiply_adds(tmp_path):
    """the gfx950 code object with the dense-gradient kernels, cut out of the library's offload bundles: eight instances (four
    activation codes, vector and single-element); the vector ones move 16 bytes per lane both ways, none holds a fused
    multiply-add or a float64 operation, tanh and sigmoid hold float32 multiplies and subtractions"""
    seen = {}
    for name, k in code_objects.kernels(b"dense_grad_kernel", r"\w*dense_grad_kernelILi[0-3]ELb[01]E\w*", tmp_path):
        act, vec = re.search(r"dense_grad_kernelILi([0-3])ELb([01])E", name).groups()
        seen[(int(act), int(vec))] = k
    assert sorted(seen) == [(a, v) for a in range(4) for v in (0, 1)]
    for (act, vec), k in seen.items():
        assert not re.search(FMA, k) and not re.search(r"_f64", k), (act, vec)
        assert re.search(r"v_(pk_)?add_f32", k), (act, vec)
        if act in (TANH, SIGMOID):
            assert re.search(r"v_(pk_)?mul_f32", k) and re.search(r"v_(pk_)?(add|sub)_f32", k), (act, vec)
        if vec:
            assert re.search(r"global_load_dwordx4", k) and re.search(r"global_store_dwordx4", k), (act, vec)


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "dense_grad_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)


def test_python_layer_checks_its_operands():
    import inspect
    import laser_amd
    from laser_amd import nn
    assert list(inspect.signature(laser_amd.bias_grad).parameters) == ["dy", "y", "activation", "dz", "out"]
    assert list(inspect.signature(laser_amd.linear_backward).parameters) == ["x", "w", "dy", "y", "activation", "need_dx"]

    class V:      # a device operand as the layer sees it, never dereferenced
        def __init__(self, shape, strides):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "version": 3, "data": (4096, False),
                                             "strides": tuple(4 * s for s in strides)}
    assert nn._rows("dy", V((5, 7), (10, 1)))[1] == 10
    assert nn._rows("dy", V((1, 7), (0, 1)))[1] == 7               # the stride of a lone row is never applied
    with pytest.raises(ValueError):
        nn._rows("dy", V((5, 7), (1, 5)))                          # a transposed view
    with pytest.raises(ValueError):
        nn._rows("dy", V((5, 7, 2), (14, 2, 1)))
    with pytest.raises(ValueError):
        laser_amd.bias_grad(V((5, 7), (7, 1)), activation="tanh")  # an activation without y
    with pytest.raises(ValueError):
        laser_amd.bias_grad(V((5, 7), (7, 1)), V((5, 7), (7, 1)), activation="gelu")
    with pytest.raises(ValueError):
        laser_amd.bias_grad(V((5, 7), (7, 1)), V((5, 8), (8, 1)), activation="relu")
