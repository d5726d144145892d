"""CPU-side checks of forEach with a body (laser_hip_foreach_* in include/laser_hip.h): the entry points are declared and
exported, the generated source binds every operand and parameter, the compile path produces a gfx950 code object with the
three kernels, 16-byte memory operations and no contracted multiply-adds, compile errors and bad specs are reported,
liblaser_hip.so does not link hiprtc, and the C++ mirror compiles."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
NEW = ["laser_hip_foreach_source", "laser_hip_foreach_code", "laser_hip_foreach_kernel", "laser_hip_foreach_dev"]
F32, F64, I8, I32 = 0, 1, 2, 4


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def spec(body, ops, params=()):
    """ops: (name, dtype code, writable) -> the spec arguments of every laser_hip_foreach_* entry point"""
    n, m = len(ops), len(params)
    return [body.encode(), n, (C.c_char_p * n)(*[o[0].encode() for o in ops]), (C.c_int * n)(*[o[1] for o in ops]),
            (C.c_int * n)(*[int(o[2]) for o in ops]), m, (C.c_char_p * max(m, 1))(*[p[0].encode() for p in params]),
            (C.c_int * max(m, 1))(*[p[1] for p in params])]


def source(L, *a):
    n = C.c_int64()
    assert L.laser_hip_foreach_source(*spec(*a), None, 0, C.byref(n)) == 0
    buf = C.create_string_buffer(n.value)
    assert L.laser_hip_foreach_source(*spec(*a), buf, n.value, C.byref(n)) == 0
    return buf.value.decode()


def code(L, *a, arch=b"gfx950"):
    n = C.c_int64()
    rc = L.laser_hip_foreach_code(*spec(*a), arch, None, 0, C.byref(n))
    if rc:
        return rc, L.laser_hip_last_error().decode()
    buf = C.create_string_buffer(n.value)
    assert L.laser_hip_foreach_code(*spec(*a), arch, buf, n.value, C.byref(n)) == 0
    return 0, buf.raw


def disasm(blob, tmp_path, kernel):
    p = tmp_path / "k.co"
    p.write_bytes(blob)
    out = subprocess.run([OBJDUMP, "-d", str(p)], check=True, capture_output=True, text=True).stdout
    m = re.search(r"<" + kernel + r">:\n(.*?)s_endpgm", out, re.S)
    assert m, f"{kernel} not in the code object"
    return m.group(1)


AXPY = ("x = y + alpha * z", [("x", F32, 1), ("y", F32, 0), ("z", F32, 0)], [("alpha", F32)])


def test_header_declares_and_library_exports_the_entry_points(L):
    from laser_amd import _lib
    hdr = re.sub(r"\s+", " ", subprocess.run(["gcc", "-E", "-P", HDR], check=True, capture_output=True, text=True).stdout)
    out = subprocess.run(["nm", "-D", "--defined-only", SO], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert re.search(r"\bint " + name + r" ?\(", hdr), f"{name} not declared"
        assert name in exported, f"{name} not exported"
        assert name in _lib.declared_symbols()
    text = open(HDR).read()
    for d in ("F32", "F64", "I8", "I16", "I32", "I64", "U8", "U16", "U32", "U64"):
        assert f"LASER_HIP_DT_{d} " in text
    assert re.search(r"#define LASER_HIP_E_COMPILE 5\b", text)
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text)


def test_source_names_every_operand_and_parameter_read_only_const(L):
    src = source(L, "w = expf(a) * k + s", [("w", F64, 1), ("a", F32, 0), ("k", I32, 0)], [("s", F64)])
    sig = re.search(r"void lh_body\(([^)]*)\)", src).group(1)
    assert [p.strip() for p in sig.split(",")] == ["double &w", "const float a", "const int32_t k", "const double s"]
    assert "w = expf(a) * k + s" in src
    for k in ("lh_foreach_vector", "lh_foreach_scalar", "lh_foreach_strided"):
        assert k in src
    assert "#define LH_E 2" in src   # 16 bytes of the widest operand (f64)


def test_code_object_is_gfx950_with_three_kernels(L, tmp_path):
    rc, blob = code(L, *AXPY)
    assert rc == 0, blob
    assert blob[:4] == b"\x7fELF"
    p = tmp_path / "k.co"
    p.write_bytes(blob)
    hdr = subprocess.run([READELF, "-h", "-n", str(p)], check=True, capture_output=True, text=True).stdout
    assert "amdgcn-amd-amdhsa--gfx950" in hdr and "xnack+" not in hdr
    syms = subprocess.run([READELF, "-s", str(p)], check=True, capture_output=True, text=True).stdout
    for k in ("lh_foreach_vector", "lh_foreach_scalar", "lh_foreach_strided"):
        assert re.search(r"\b" + k + r"\b", syms)


def test_contiguous_kernel_moves_16_bytes_per_lane(L, tmp_path):
    for ops in (AXPY[1], [("x", F64, 1), ("y", F64, 0), ("z", F64, 0)], [("x", I8, 1), ("y", I8, 0), ("z", I8, 0)]):
        rc, blob = code(L, "x = y + alpha * z", ops, [("alpha", ops[0][1])])
        assert rc == 0, blob
        k = disasm(blob, tmp_path, "lh_foreach_vector")
        assert re.search(r"(global|buffer)_load_dwordx4", k) and re.search(r"(global|buffer)_store_dwordx4", k), ops[0]


def test_no_contraction_to_fma(L, tmp_path):
    rc, blob = code(L, "x = y * z + w", [("x", F32, 1), ("y", F32, 0), ("z", F32, 0), ("w", F32, 0)])
    assert rc == 0, blob
    k = disasm(blob, tmp_path, "lh_foreach_scalar")
    assert re.search(r"v_(pk_)?mul_f32", k) and re.search(r"v_(pk_)?add_f32", k)
    assert not re.search(r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak", k)


def test_compile_errors_carry_the_log(L):
    from laser_amd import _lib
    rc, log = code(L, "x = y +* ;; (", [("x", F32, 1), ("y", F32, 0)])
    assert rc == _lib.E_COMPILE and "error" in log
    rc, log = code(L, "y = x", [("x", F32, 1), ("y", F32, 0)])
    assert rc == _lib.E_COMPILE and "const" in log and "'y'" in log


@pytest.mark.parametrize("ops,params", [
    ([("x", F32, 1), ("1x", F32, 0)], []),            # not an identifier
    ([("x", F32, 1), ("x", F32, 0)], []),             # duplicate
    ([("x", F32, 1)], [("x", F32)]),                  # duplicate across operands and parameters
    ([("x", F32, 1), ("lh_y", F32, 0)], []),          # the template's prefix
    ([("x", F32, 1), ("__y", F32, 0)], []),           # reserved
    ([("x", F32, 1), ("float", F32, 0)], []),         # keyword
    ([("x", F32, 1), ("y-z", F32, 0)], []),
    ([("x", F32, 1), ("", F32, 0)], []),
    ([(f"v{i}", F32, 1) for i in range(9)], []),      # 9 operands
    ([("x", F32, 1)], [(f"p{i}", F32) for i in range(9)]),   # 9 parameters
    ([("x", 10, 1)], []),                             # unknown dtype
    ([("x", -1, 1)], []),
    ([("x", F32, 1)], [("p", 12)]),
])
def test_bad_specs_are_invalid(L, ops, params):
    from laser_amd import _lib
    n = C.c_int64()
    assert L.laser_hip_foreach_source(*spec("x = 1", ops, params), None, 0, C.byref(n)) == _lib.E_INVALID
    assert code(L, "x = 1", ops, params)[0] == _lib.E_INVALID


def test_xnack_plus_is_refused(L):
    from laser_amd import _lib
    assert code(L, *AXPY, arch=b"gfx950:xnack+")[0] == _lib.E_INVALID
    assert code(L, *AXPY, arch=b"gfx950:sramecc+:xnack-")[0] == 0


def test_library_does_not_link_hiprtc():
    out = subprocess.run(["readelf", "-d", SO], check=True, capture_output=True, text=True).stdout
    assert "NEEDED" in out and "hiprtc" not in out


def test_kernel_needs_a_gfx950_device(L):
    """E_NODEVICE without a GPU; on an MI355X the same call returns a handle."""
    from laser_amd import _lib
    try:
        import torch
        have = torch.cuda.is_available()
    except ImportError:
        have = False
    h = C.c_int64()
    rc = L.laser_hip_foreach_kernel(*spec(*AXPY), C.byref(h))
    if have:
        assert rc == 0 and h.value > 0, L.laser_hip_last_error()
    else:
        assert rc == _lib.E_NODEVICE


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "foreach_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)
