"""CPU-side checks of the reductions (include/laser_hip.h "Reductions" and "forEachReduce"): the entry points are declared
and exported, the header states the order with reduce_core.h's constants, the numpy model of that order behaves (empty,
exact, close to math.fsum), forEachReduce's generated source carries the body, the merge and the shared core and compiles to
a gfx950 code object without contracted multiply-adds, compile errors and bad specs are reported, every entry point needs a
device, and the C++ mirror compiles."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import reduce_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
F32, F64, I8, I32, I64 = 0, 1, 2, 4, 5
NEW = ["laser_hip_foreach_reduce_source", "laser_hip_foreach_reduce_code", "laser_hip_foreach_reduce_kernel",
       "laser_hip_foreach_reduce_dev", "laser_hip_reduce_sum_f32", "laser_hip_reduce_min_f32", "laser_hip_reduce_max_f32"]
NEW += [f"laser_hip_reduce_{op}_{t}_dev" for op in ("sum", "min", "max") for t in ("f32", "f64", "i32", "i64")]
KERNELS = ("lh_reduce_vector", "lh_reduce_scalar", "lh_reduce_strided", "lh_reduce_partials")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def spec(body, ops, params=(), acc=("acc", F32), merge="acc += other"):
    n, m = len(ops), len(params)
    return [body.encode(), n, (C.c_char_p * n)(*[o[0].encode() for o in ops]), (C.c_int * n)(*[o[1] for o in ops]),
            (C.c_int * n)(*[int(o[2]) for o in ops]), m, (C.c_char_p * max(m, 1))(*[p[0].encode() for p in params]),
            (C.c_int * max(m, 1))(*[p[1] for p in params]), acc[0].encode(), acc[1], merge.encode()]


def source(L, *a, **k):
    n = C.c_int64()
    assert L.laser_hip_foreach_reduce_source(*spec(*a, **k), None, 0, C.byref(n)) == 0, L.laser_hip_last_error()
    buf = C.create_string_buffer(n.value)
    assert L.laser_hip_foreach_reduce_source(*spec(*a, **k), buf, n.value, C.byref(n)) == 0
    return buf.value.decode()


def code(L, *a, arch=b"gfx950", **k):
    n = C.c_int64()
    rc = L.laser_hip_foreach_reduce_code(*spec(*a, **k), arch, None, 0, C.byref(n))
    if rc:
        return rc, L.laser_hip_last_error().decode()
    buf = C.create_string_buffer(n.value)
    assert L.laser_hip_foreach_reduce_code(*spec(*a, **k), arch, buf, n.value, C.byref(n)) == 0
    return 0, buf.raw


DOT = ("acc += x * y", [("x", F32, 0), ("y", F32, 0)])


def test_header_declares_and_library_exports_the_entry_points(L):
    from laser_amd import _lib
    hdr = re.sub(r"\s+", " ", subprocess.run(["gcc", "-E", "-P", HDR], check=True, capture_output=True, text=True).stdout)
    out = subprocess.run(["nm", "-D", "--defined-only", SO], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert re.search(r"\bint " + name + r" ?\(", hdr), f"{name} not declared"
        assert name in exported, f"{name} not exported"
        assert name in _lib.declared_symbols()
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", open(HDR).read())


def test_header_states_the_order_with_the_cores_constants():
    text = open(HDR).read()
    W, R = M.constants()
    assert re.search(rf"#define LASER_HIP_REDUCE_LANES {W}\b", text)
    assert re.search(rf"#define LASER_HIP_REDUCE_STEPS {R}\b", text)
    assert R in (4, 8, 16) and W == 256
    assert "-0 ranks below +0" in text and "any NaN gives NaN" in text


def test_model_of_the_empty_reduction_is_init():
    for dt in (np.float32, np.float64, np.int32, np.int64):
        got = M.model_sum(np.zeros(0, dt))
        assert got == 0 and got.dtype == dt
    assert M.model_minmax(np.zeros(0, np.float32), "min") == np.inf
    assert M.model_minmax(np.zeros(0, np.float32), "max") == -np.inf
    assert M.model_minmax(np.zeros(0, np.int32), "min") == np.iinfo(np.int32).max
    assert M.model_minmax(np.zeros(0, np.int64), "max") == np.iinfo(np.int64).min
    assert M.model_minmax(np.zeros(0, np.int32), "max").dtype == np.int32


def test_model_sums_of_representable_values_are_exact():
    rng = np.random.default_rng(1)
    W, R = M.constants()
    for n in (1, 2, 7, R * W * 4 - 1, R * W * 4, R * W * 4 + 1, 100_003):
        x = rng.integers(-1000, 1000, n).astype(np.float32)   # every partial sum stays below 2^24
        assert M.model_sum(x) == np.float32(x.astype(np.int64).sum()), n
        y = (rng.integers(-2 ** 20, 2 ** 20, n) * 0.25).astype(np.float64)
        assert M.model_sum(y) == y.astype(np.float64).sum(), n


def test_model_agrees_with_fsum():
    x = np.random.default_rng(2).standard_normal(10 ** 6).astype(np.float32)
    want = math.fsum(x.astype(np.float64))
    assert abs(float(M.model_sum(x)) - want) <= 1e-5 * abs(want) + 1e-5 * math.sqrt(x.size)
    want = math.fsum(np.abs(x).astype(np.float64))
    assert abs(float(M.model_sum(np.abs(x))) - want) <= 1e-5 * want


def test_model_integer_sums_wrap_like_numpy():
    rng = np.random.default_rng(3)
    for dt in (np.int32, np.int64):
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, 50_000, dtype=dt, endpoint=True)
        assert M.model_sum(x) == np.sum(x, dtype=dt)


def test_model_min_max_rule():
    z = np.array([0.0, -0.0, 1.0], np.float32)
    assert np.signbit(M.model_minmax(z, "min")) and M.model_minmax(z[:2], "min") == 0
    assert not np.signbit(M.model_minmax(z[:2], "max"))
    assert np.signbit(M.model_minmax(np.array([-0.0, -0.0], np.float32), "max"))
    assert np.isnan(M.model_minmax(np.array([1.0, np.nan, -np.inf], np.float32), "min"))
    assert M.model_minmax(np.array([1.0, -np.inf], np.float32), "min") == -np.inf


def test_source_carries_body_merge_and_the_shared_core(L):
    src = source(L, "acc += x * w", [("x", F32, 0), ("w", F64, 1)], [("k", I32)], acc=("total", F64),
                 merge="total = total + other")
    sig = re.search(r"void lh_body\(([^)]*)\)", src).group(1)
    assert [p.strip() for p in sig.split(",")] == ["lh_acc_t &total", "const float x", "double &w", "const int32_t k"]
    assert "typedef double lh_acc_t;" in src
    assert "acc += x * w" in src and "total = total + other" in src
    assert re.search(r"void lh_merge\(lh_acc_t &total, const lh_acc_t other\)", src)
    core = open(os.path.join(ROOT, "laser_amd", "csrc", "reduce_core.h")).read()
    assert core in src, "the order is not reduce_core.h's text"
    for k in KERNELS:
        assert k in src
    assert "#define LH_E 2" in src and "#define LH_EA 2" in src
    assert "void __launch_bounds__(256) lh_foreach_vector" not in src     # the forEach kernels stay out of reduce modules


def test_code_object_is_gfx950_without_contraction(L, tmp_path):
    rc, blob = code(L, *DOT)
    assert rc == 0, blob
    p = tmp_path / "k.co"
    p.write_bytes(blob)
    hdr = subprocess.run([READELF, "-h", "-n", str(p)], check=True, capture_output=True, text=True).stdout
    assert "amdgcn-amd-amdhsa--gfx950" in hdr and "xnack+" not in hdr
    syms = subprocess.run([READELF, "-s", str(p)], check=True, capture_output=True, text=True).stdout
    for k in KERNELS:
        assert re.search(r"\b" + k + r"\b", syms)
    out = subprocess.run([OBJDUMP, "-d", str(p)], check=True, capture_output=True, text=True).stdout
    for k in ("lh_reduce_vector", "lh_reduce_scalar"):   # (the strided kernel's 64-bit index divisions use FMA themselves)
        body = re.search(r"<" + k + r">:\n(.*?)s_endpgm", out, re.S).group(1)
        assert re.search(r"v_(pk_)?mul_f32", body) and re.search(r"v_(pk_)?add_f32", body)
        assert not re.search(r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak", body), k
    body = re.search(r"<lh_reduce_vector>:\n(.*?)s_endpgm", out, re.S).group(1)
    assert re.search(r"(global|buffer)_load_dwordx4", body)


def test_int8_operands_into_an_int64_accumulator_compile(L):
    rc, blob = code(L, "acc += x", [("x", I8, 0)], acc=("acc", I64))
    assert rc == 0, blob
    src = source(L, "acc += x", [("x", I8, 0)], acc=("acc", I64))
    assert "#define LH_E 16" in src and "#define LH_EA 2" in src


def test_a_bad_merge_carries_the_log(L):
    from laser_amd import _lib
    rc, log = code(L, *DOT, merge="acc +*= ;; other(")
    assert rc == _lib.E_COMPILE and "error" in log and "merge" in log


@pytest.mark.parametrize("ops,params,acc,merge", [
    ([("x", F32, 0), ("other", F32, 0)], [], ("acc", F32), "acc += other"),   # operand called other
    ([("x", F32, 0)], [("other", F32)], ("acc", F32), "acc += other"),        # parameter called other
    ([("x", F32, 0)], [], ("other", F32), "other += other"),                  # accumulator called other
    ([("x", F32, 0)], [], ("x", F32), "x += other"),                          # accumulator = an operand
    ([("x", F32, 0)], [("k", F32)], ("k", F32), "k += other"),                # accumulator = a parameter
    ([("x", F32, 0)], [], ("float", F32), "float += other"),                  # keyword
    ([("x", F32, 0)], [], ("lh_acc", F32), "lh_acc += other"),                # the template's prefix
    ([("x", F32, 0)], [], ("", F32), "acc += other"),
    ([("x", F32, 0)], [], ("acc", 10), "acc += other"),                       # unknown accumulator type
    ([("x", F32, 0)], [], ("acc", -1), "acc += other"),
    ([("x", F32, 0)], [], ("acc", F32), ""),                                  # empty merge
    ([("x", F32, 0)], [], ("acc", F32), "  ; "),
    ([("x", 11, 0)], [], ("acc", F32), "acc += other"),                       # unknown operand type
])
def test_bad_specs_are_invalid(L, ops, params, acc, merge):
    from laser_amd import _lib
    n = C.c_int64()
    assert L.laser_hip_foreach_reduce_source(*spec("acc += x", ops, params, acc=acc, merge=merge), None, 0,
                                             C.byref(n)) == _lib.E_INVALID
    assert code(L, "acc += x", ops, params, acc=acc, merge=merge)[0] == _lib.E_INVALID


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_every_entry_point_needs_a_device(L):
    """E_NODEVICE without a GPU (on an MI355X the GPU tests exercise the same calls)."""
    if have_gpu():
        pytest.skip("GPU present: the no-device path is for GPU-less hosts")
    from laser_amd import _lib
    shape, st = (C.c_int64 * 1)(4), (C.c_int64 * 1)(1)
    for op in ("sum", "min", "max"):
        for t in ("f32", "f64", "i32", "i64"):
            rc = getattr(L, f"laser_hip_reduce_{op}_{t}_dev")(C.c_void_p(0x1000), st, shape, 1, C.c_void_p(0x2000), None)
            assert rc == _lib.E_NODEVICE, (op, t)
        x, out = np.ones(4, np.float32), C.c_float()
        assert getattr(L, f"laser_hip_reduce_{op}_f32")(x.ctypes.data_as(C.c_void_p), 4, C.byref(out)) == _lib.E_NODEVICE
    h = C.c_int64()
    assert L.laser_hip_foreach_reduce_kernel(*spec(*DOT), C.byref(h)) == _lib.E_NODEVICE
    init = C.c_uint64(0)
    ptrs = (C.c_void_p * 2)(0x1000, 0x2000)
    assert L.laser_hip_foreach_reduce_dev(1, ptrs, (C.c_int64 * 2)(1, 1), shape, 1, None, C.byref(init),
                                          C.c_void_p(0x3000), None) == _lib.E_HANDLE


def test_python_mirror_fails_loudly_without_a_device():
    if have_gpu():
        pytest.skip("GPU present")
    import laser_amd
    with pytest.raises(laser_amd.LaserHipError) as e:
        laser_amd.reduce_sum(np.ones(8, np.float32))
    assert e.value.code == 3


def test_last_reduce_variant_is_an_option(L):
    v = C.c_int64(7)
    assert L.laser_hip_get_option(b"last_reduce_variant", C.byref(v)) == 0
    assert v.value in (-1, 0, 1, 2)


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "reduce_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)
