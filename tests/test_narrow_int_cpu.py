"""CPU-side checks of the int8 / int16 GEMM entry points (every SomeNumber integer type of the reference's gemm_strided,
gemm.nim:184-248): the library exports them and the header declares them, the Python mirror binds them and maps every
integer dtype onto them, the ABI number moved to 3 everywhere, the Nim shim and laser.hpp reach them for every integer
type, and the int16 digit split of gemm_narrow_mfma.hip is an exact identity (replayed in numpy over all 65 536 values)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
NIM = os.path.join(ROOT, "nim", "laser_hip.nim")

NEW = []
for s in ("i8", "i16"):
    NEW += [f"laser_hip_gemm_strided_{s}", f"laser_hip_gemm_strided_{s}_dev", f"laser_hip_gemm_strided_batched_{s}_dev",
            f"laser_hip_gemm_packed_{s}", f"laser_hip_gemm_packed_{s}_dev"]
    for ab in "AB":
        NEW += [f"laser_hip_gemm_prepack{ab}_mem_required_{s}", f"laser_hip_gemm_prepack{ab}_{s}",
                f"laser_hip_gemm_prepack{ab}_{s}_dev"]


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    import laser_amd
    return laser_amd


def header_text():
    return subprocess.run(["gcc", "-E", "-P", HDR], check=True, capture_output=True, text=True).stdout


def test_library_exports_and_header_declares_every_narrow_entry_point(built):
    out = subprocess.run(["nm", "-D", "--defined-only", SO], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    hdr = re.sub(r"\s+", " ", header_text())
    for name in NEW:
        assert name in exported, f"{name} not exported"
        m = re.search(r"\b" + name + r" ?\(([^)]*)\)", hdr)
        assert m, f"{name} not declared in include/laser_hip.h"
        if "mem_required" not in name and "prepack" not in name:
            # alpha and beta travel as int32_t, the operands as int8_t / int16_t pointers
            params = [p.strip() for p in m.group(1).split(",")]
            assert sum(p.startswith("int32_t ") for p in params) == 2, (name, params)
            elem = "int8_t" if name.split("_")[-1] == "i8" or "_i8_" in name else "int16_t"
            assert any(p.startswith(f"{elem} *") or p.startswith(f"const {elem} *") for p in params) or "packed" in name, (name, params)
    assert set(NEW) <= set(built._lib.declared_symbols())


def test_python_mirror_binds_the_narrow_entry_points(built):
    L = built.lib()
    for s in ("i8", "i16"):
        assert getattr(L, f"laser_hip_gemm_strided_{s}").argtypes[3] is C.c_int32
        assert getattr(L, f"laser_hip_gemm_strided_{s}_dev").argtypes[10] is C.c_int32
        assert getattr(L, f"laser_hip_gemm_strided_batched_{s}_dev").argtypes[4] is C.c_int32
        assert getattr(L, f"laser_hip_gemm_packed_{s}").argtypes[3] is C.c_int32
        assert getattr(L, f"laser_hip_gemm_packed_{s}_dev").argtypes[6] is C.c_int32
        assert getattr(L, f"laser_hip_gemm_prepackA_mem_required_{s}").restype is C.c_int64
    assert "i8" not in built._lib._CT and "i16" not in built._lib._CT      # no _sharded / map_strided bindings for them


def test_abi_version_is_3_in_header_mirror_shim_and_library(built):
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", open(HDR).read())
    assert built._lib.ABI_VERSION == 3
    assert re.search(r"const laserHipAbi\* = 3\b", open(NIM).read())
    assert built.lib().laser_hip_abi_version() == 3


def test_prepack_sizes_of_the_narrow_types(built):
    L = built.lib()
    M, N, K = 130, 77, 600
    assert L.laser_hip_gemm_prepackA_mem_required_i8(M, N, K) == 256 * 608 + 64
    assert L.laser_hip_gemm_prepackB_mem_required_i16(M, N, K) == 2 * 256 * 608 + 64
    assert built.gemm_prepackA_mem_required(np.uint8, M, N, K) == 256 * 608 + 64
    assert built.gemm_prepackB_mem_required(np.uint16, M, N, K) == 2 * 256 * 608 + 64


def test_int16_digit_split_and_three_product_identity_over_every_value():
    a = np.arange(1 << 16, dtype=np.uint32)
    # the split as gemm_narrow_mfma.hip's packing pass computes it, two elements per 32-bit word
    w = a[0::2] | (a[1::2] << 16)
    hb = (((w >> 8) & 0x00FF00FF) + ((w >> 7) & 0x00010001)) & 0x00FF00FF
    s0 = np.empty(1 << 16, dtype=np.int64)
    s1 = np.empty(1 << 16, dtype=np.int64)
    s0[0::2], s0[1::2] = (w & 0xFF), ((w >> 16) & 0xFF)
    s1[0::2], s1[1::2] = (hb & 0xFF), ((hb >> 16) & 0xFF)
    s0, s1 = s0.astype(np.uint8).view(np.int8).astype(np.int64), s1.astype(np.uint8).view(np.int8).astype(np.int64)
    # ... which is (a + 0x80) ^ 0x80 byte by byte: low byte a balanced digit, high byte any representative
    d = ((a + 0x80) ^ 0x80) & 0xFFFF
    assert np.array_equal(s0 & 0xFF, d & 0xFF) and np.array_equal(s1 & 0xFF, (d >> 8) & 0xFF)
    assert s0.min() >= -128 and s0.max() <= 127
    assert np.array_equal((s0 + 256 * s1) % 65536, a.astype(np.int64))
    # a*b == s0 t0 + 256 (s0 t1 + s1 t0) (mod 2^16): every a against a spread of b (every b for a sample of a)
    rng = np.random.default_rng(7)
    for bs in (rng.integers(0, 1 << 16, 64), np.array([0, 1, 0x7F, 0x80, 0xFF, 0x100, 0x7FFF, 0x8000, 0xFFFF])):
        for b in bs:
            t0, t1 = s0[b], s1[b]
            want = (a.astype(np.int64) * int(b)) % 65536
            assert np.array_equal((s0 * t0 + 256 * (s0 * t1 + s1 * t0)) % 65536, want)
    sample = rng.integers(0, 1 << 16, 64)
    for x in sample:
        want = (int(x) * a.astype(np.int64)) % 65536
        assert np.array_equal((s0[x] * s0 + 256 * (s0[x] * s1 + s1[x] * s0)) % 65536, want)


def test_int8_digit_is_the_byte():
    a = np.arange(256, dtype=np.uint32)
    s0 = a.astype(np.uint8).view(np.int8).astype(np.int64)
    for b in range(256):
        assert np.array_equal((s0 * s0[b]) % 256, (a.astype(np.int64) * b) % 256)


def _nim_proc_body(src, header):
    i = src.index(header)
    j = src.find("\nproc ", i + 1)
    k = src.find("\n# ----", i + 1)
    end = min(x for x in (j, k, len(src)) if x > 0)
    return src[i:end]


def test_nim_shim_dispatches_every_integer_type():
    src = open(NIM).read()
    bodies = [_nim_proc_body(src, "proc gemm_strided*[T: SomeNumber](\n      M, N, K: int,\n      alpha: T,\n      A: ptr T,"),
              _nim_proc_body(src, "proc gemm_strided*[T: SomeNumber](\n      M, N, K: int,\n      alpha: T,\n      A: DevicePtr[T],")]
    for body in bodies:      # (the {.error.} branch is reached by no SomeNumber type)
        for t in ("int8", "uint8", "int16", "uint16", "int32", "uint32", "int64", "uint64", "int", "uint"):
            assert re.search(rf"T is {t}\b", body), f"no branch for {t}:\n{body[:200]}"
    # the pre-packed procs end in an `else` onto the int64 entry point: the narrow types and uint32 need their own branches
    for name in ("proc gemm_prepackA*[T]", "proc gemm_prepackB*[T]", "proc gemm_prepackA_mem_required*",
                 "proc gemm_prepackB_mem_required*", "proc gemm_packed*[T: SomeNumber]"):
        body = _nim_proc_body(src, name)
        for t in ("int8", "uint8", "int16", "uint16", "uint32"):
            assert re.search(rf"T is {t}\b", body), f"{name}: no branch for {t}"
    for s in ("i8", "i16"):
        assert f'importc: "laser_hip_gemm_strided_{s}"' in src and f'importc: "laser_hip_gemm_strided_{s}_dev"' in src
        assert f'importc: "laser_hip_gemm_packed_{s}"' in src


def test_cpp_mirror_instantiates_every_integer_type(tmp_path):
    src = tmp_path / "narrow.cpp"
    lines = ['#include "laser.hpp"']
    for t in ("int8_t", "uint8_t", "int16_t", "uint16_t", "uint32_t", "uint64_t"):
        lines.append(f"template void laser::gemm_strided<{t}>(int64_t, int64_t, int64_t, {t}, const {t} *, int64_t, int64_t, "
                     f"const {t} *, int64_t, int64_t, {t}, {t} *, int64_t, int64_t);")
        lines.append(f"template void laser::gemm_strided_dev<{t}>(int64_t, int64_t, int64_t, {t}, const {t} *, int64_t, int64_t, "
                     f"const {t} *, int64_t, int64_t, {t}, {t} *, int64_t, int64_t, void *);")
        lines.append(f"template void laser::gemm_packed<{t}>(int64_t, int64_t, int64_t, {t}, const void *, const void *, {t}, "
                     f"{t} *, int64_t, int64_t);")
        lines.append(f"template void laser::gemm_prepackA<{t}>(void *, int64_t, int64_t, int64_t, const {t} *, int64_t, int64_t);")
        lines.append(f"template int64_t laser::gemm_prepackB_mem_required<{t}>(int64_t, int64_t, int64_t);")
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_python_dtype_mapping_accepts_every_integer_dtype(built):
    from laser_amd import primitives as P
    want = {np.int8: "i8", np.uint8: "i8", np.int16: "i16", np.uint16: "i16", np.uint32: "i32", np.uint64: "i64"}
    for dt, sfx in want.items():
        assert P._sfx(np.zeros(1, dtype=dt)) == sfx
    import torch
    for dt, sfx in ((torch.int8, "i8"), (torch.uint8, "i8"), (torch.int16, "i16")):
        assert P._sfx(torch.zeros(1, dtype=dt)) == sfx
    # alpha / beta: reduced mod 2^n to the signed representative
    assert P._scalar("i8", 255).value == -1 and P._scalar("i16", 40000).value == 40000 - 65536
    assert P._scalar("i32", 2 ** 32 - 1).value == -1 and P._scalar("i64", 2 ** 64 - 1).value == -1
    # the fused epilogue stays float-only
    A = np.zeros((4, 4), dtype=np.int8)
    with pytest.raises(TypeError):
        built.matmul(A, A, activation="relu")
