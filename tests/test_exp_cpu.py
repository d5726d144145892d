"""CPU-side checks of lexp and the row softmax (include/laser_hip.h "exp and row softmax"): the table and the constants of
laser_amd/csrc/exp_core.h are the correctly rounded ones, the header as a host program (g++, UBSan + ASan, its own main)
gives the bits of the numpy model, the entry points are declared, exported and mirrored and fail loudly without a GPU,
and the generated forEach source carries the definition."""
import ctypes as C
import os
import re
import subprocess
import zlib
from fractions import Fraction

import numpy as np
import pytest

from tests import code_objects, exp_model
from tests.test_foreach_cpu import code, disasm, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_exp_f32_dev", "laser_hip_exp_f32", "laser_hip_softmax_rows_f32_dev"]
F32 = 0


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


def test_table_is_the_correctly_rounded_one():
    """2^(i/1024) = (2^i)^(1/1024): the rounding boundary b between two float32 neighbours decides by comparing 2^i with
    b^1024, exactly, in integers -- no floating point involved."""
    lut = exp_model.header_table()
    assert lut.shape == (1024,)
    assert np.array_equal(lut, exp_model.LUT), np.nonzero(lut != exp_model.LUT)[0][:8]
    assert zlib.crc32(lut.astype("<u4").tobytes()) == exp_model.TABLE_CRC == 0x0c4cd4ff
    assert list(lut[:4]) == [0, 5680, 11364, 17052] and lut[1023] == 8377255
    for i in range(1024):
        m = int(lut[i])
        # the true value lies between the boundaries (m - 1/2) and (m + 1/2) ulps above 1, in units of 2^-24
        lo, hi = (1 << 24) + 2 * m - 1, (1 << 24) + 2 * m + 1
        two_i = (1 << i) << (24 * 1024)
        assert lo ** 1024 <= two_i <= hi ** 1024, i
        if i:
            assert lo ** 1024 != two_i and hi ** 1024 != two_i   # never on a boundary: no tie to break


def test_header_names_the_entry_where_glibc_powf_differs():
    """the reference fills its table with the host's powf; the header records the one index where glibc's differs"""
    text = open(os.path.join(CSRC, "exp_core.h")).read()
    assert re.search(r"index 88\b", text)


def test_constants():
    text = open(os.path.join(CSRC, "exp_core.h")).read()
    assert re.search(r"#define LH_EXP_A_BITS 0x44b8aa3bu", text) and re.search(r"#define LH_EXP_B_BITS 0x3a317218u", text)
    ln2 = Fraction(np.log(2.0)) + 0   # float64 ln 2: 2^-53 relative, far inside half a float32 ulp of both quotients
    for bits, q in ((0x44b8aa3b, Fraction(1024) / ln2), (0x3a317218, ln2 / 1024)):
        f = np.array([bits], np.uint32).view(np.float32)[0]
        ulp = np.spacing(f)
        assert abs(Fraction(float(f)) - q) < Fraction(float(ulp)) * Fraction(499, 1000)
    # rounding ln 2 to float32 first gives the same two bit patterns
    l32 = np.float32(np.log(np.float32(2)))
    assert np.float32(np.float32(1024) / l32) == exp_model.EXP_A and np.float32(l32 / np.float32(1024)) == exp_model.EXP_B


@pytest.fixture(scope="module")
def host_exp(tmp_path_factory):
    """exp_core.h as a stand-alone host program under UBSan and ASan"""
    exe = tmp_path_factory.mktemp("exp_host") / "exp_core_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=all", "-static-libasan", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "exp_core_host.cpp"),
                    "-o", str(exe)], check=True)

    def run(x):
        x = np.ascontiguousarray(x, np.float32)
        p = subprocess.run([str(exe)], input=x.tobytes(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return np.frombuffer(p.stdout, np.float32).reshape(x.shape)
    return run


def test_host_build_matches_the_model_on_the_edges(host_exp):
    x = exp_model.edges()
    got, want = host_exp(x), exp_model.lexp(x)
    assert exp_model.same_bits(got, want), [(a, hex(b), hex(c)) for a, b, c in
                                            zip(x, got.view(np.uint32), want.view(np.uint32)) if b != c and a == a]
    assert np.isnan(got[np.isnan(x)]).all()
    assert got[0] == 1 and got[1] == 1                       # lexp(+-0) = 1
    assert host_exp(np.float32([np.inf]))[0] == host_exp(np.float32([88]))[0]      # Inf clamps
    assert host_exp(np.float32([-np.inf]))[0] == host_exp(np.float32([-88]))[0]
    # below the threshold the second factor is subnormal: not an exponential any more, but the model's bits all the same
    assert got[x == np.float32(-88)][0] != np.float32(np.exp(np.float64(-88)))


def test_host_build_rounds_ties_to_even(host_exp):
    x = exp_model.ties()
    p = (x * exp_model.EXP_A).astype(np.float32)
    assert (np.abs(p - np.trunc(p)) == 0.5).all()
    r = np.rint(p)
    assert (r % 2 == 0).all() and (r != np.trunc(p)).any()    # some ties go away from zero: truncation would differ
    assert exp_model.same_bits(host_exp(x), exp_model.lexp(x))


def test_host_build_matches_the_model_on_random_values(host_exp):
    x = np.random.default_rng(1).uniform(-90, 90, 1_000_000).astype(np.float32)
    got, want = host_exp(x), exp_model.lexp(x)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad.size, x[bad[:5]])
    ok = (x > -87) & (x < 88)
    ref = np.exp(x[ok].astype(np.float64))
    assert np.max(np.abs(want[ok] - ref) / ref) < 1e-5        # and it is an exponential: a few float32 ulps


def test_model_softmax_is_a_softmax():
    x = np.random.default_rng(2).uniform(-20, 20, (3, 1500)).astype(np.float32)
    y = exp_model.softmax_rows(x)
    e = np.exp(x.astype(np.float64) - x.max(axis=1, keepdims=True))
    assert np.allclose(y, e / e.sum(axis=1, keepdims=True), rtol=1e-4, atol=0)
    assert np.isnan(exp_model.softmax_row(np.float32([1, np.nan, 2]))).all()
    assert np.isnan(exp_model.softmax_row(np.float32([-np.inf, -np.inf]))).all()
    assert exp_model.same_bits(exp_model.softmax_row(np.float32([3, 3, 3, 3])), np.float32([0.25] * 4))


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
        assert f'importc: "{name}"' in nim
    for name in ("laser_hip_exp_f32_dev", "laser_hip_softmax_rows_f32_dev"):
        assert name in hpp
    assert re.search(r"proc exp\*", nim) and re.search(r"proc softmax\*", nim)
    assert callable(laser_amd.exp) and callable(laser_amd.softmax)


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    i64 = C.c_int64
    p = C.c_void_p(4096)    # never dereferenced: arguments are checked first
    sm = L.laser_hip_softmax_rows_f32_dev
    assert sm(p, 8, p, 8, 1, 0, None) == _lib.E_INVALID                  # n = 0
    assert sm(p, 1 << 27, p, 1 << 27, 1, (1 << 26) + 1, None) == _lib.E_INVALID
    assert sm(p, 8, p, 8, -1, 8, None) == _lib.E_INVALID                 # rows < 0
    assert sm(p, 7, p, 8, 2, 8, None) == _lib.E_INVALID                  # a row stride below n
    assert sm(p, 8, p, 7, 2, 8, None) == _lib.E_INVALID
    assert sm(p, 8, p, 12, 2, 8, None) == _lib.E_INVALID                 # in place with unequal strides
    ex = L.laser_hip_exp_f32_dev
    one = (i64 * 7)(*[1] * 7)
    assert ex(p, one, p, one, one, 7, None) == _lib.E_INVALID            # rank 7
    assert ex(p, (i64 * 1)(0), p, (i64 * 1)(1), (i64 * 1)(4), 1, None) == _lib.E_INVALID     # stride 0 on dst
    assert ex(p, (i64 * 1)(1), p, (i64 * 1)(1), (i64 * 1)(-4), 1, None) == _lib.E_INVALID
    assert L.laser_hip_exp_f32(None, None, -1) == _lib.E_INVALID
    assert L.laser_hip_exp_f32(None, None, 3) == _lib.E_INVALID


def test_entry_points_need_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one the host-pointer form gives the model's bits"""
    from laser_amd import _lib
    x = exp_model.edges()
    y = np.empty_like(x)
    rc = L.laser_hip_exp_f32(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), x.size)
    if have_gpu():
        assert rc == 0 and exp_model.same_bits(y, exp_model.lexp(x))
        return
    assert rc == _lib.E_NODEVICE
    p = C.c_void_p(4096)
    one = (C.c_int64 * 1)(1)
    assert L.laser_hip_exp_f32_dev(p, one, p, one, (C.c_int64 * 1)(4), 1, None) == _lib.E_NODEVICE
    assert L.laser_hip_softmax_rows_f32_dev(p, 8, p, 8, 2, 8, None) == _lib.E_NODEVICE
    assert L.laser_hip_softmax_rows_f32_dev(p, 8, p, 8, 0, 8, None) == _lib.E_NODEVICE      # like every other entry point
    import laser_amd
    with pytest.raises(laser_amd.LaserHipError) as e:
        laser_amd.exp(np.ones(4, np.float32))
    assert e.value.code == _lib.E_NODEVICE


def _source(L, fn, args):
    n = C.c_int64()
    assert fn(*args, None, 0, C.byref(n)) == 0
    buf = C.create_string_buffer(n.value)
    assert fn(*args, buf, n.value, C.byref(n)) == 0
    return buf.value.decode()


def test_generated_sources_carry_the_definition(L):
    from laser_amd import _lib
    core = open(os.path.join(CSRC, "exp_core.h")).read()
    src = _source(L, L.laser_hip_foreach_source, spec("y = laser_exp(x)", [("y", F32, 1), ("x", F32, 0)]))
    red = _source(L, L.laser_hip_foreach_reduce_source,
                  spec("y = laser_exp(x - m); acc += y", [("y", F32, 1), ("x", F32, 0)], [("m", F32)]) + [b"acc", F32, b"acc += other"])
    for s in (src, red):
        assert core in s                                   # the header as it stands, table and all
        assert s.index("float laser_exp(") < s.index("void lh_body(")
    assert "lh_reduce_chunk" in red
    # the name is reserved like the lh_ names
    n = C.c_int64()
    for ops, params in (([("laser_exp", F32, 1)], []), ([("y", F32, 1)], [("laser_exp", F32)])):
        assert L.laser_hip_foreach_source(*spec("y = 1", ops, params), None, 0, C.byref(n)) == _lib.E_INVALID
    assert L.laser_hip_foreach_reduce_source(*spec("laser_exp += x", [("x", F32, 0)]), b"laser_exp", F32, b"laser_exp += other",
                                             None, 0, C.byref(n)) == _lib.E_INVALID


def test_body_with_laser_exp_compiles_without_fused_multiply_adds(L, tmp_path):
    rc, blob = code(L, "y = laser_exp(x)", [("y", F32, 1), ("x", F32, 0)])
    assert rc == 0, blob
    k = disasm(blob, tmp_path, "lh_foreach_vector")
    assert re.search(r"v_rndne_f32", k) and re.search(r"v_(pk_)?mul_f32", k)
    assert not re.search(r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak|v_mad_f32|v_mac_f32", k)


def test_precompiled_exp_kernel_has_no_fused_multiply_adds(tmp_path):
    """pointwise_vec_kernel<ExpOp> is lexp and nothing else: multiplies, a subtract and an add per element, never an fma; it
    moves 16 bytes per lane.  (The gfx950 code objects are cut out of the library's offload bundles: tests/code_objects.py.)"""
    found = code_objects.kernels(b"ExpOp", r"\w*pointwise_vec_kernelINS\w*ExpOp\w*", tmp_path)
    assert len(found) == 1, "the vector instance of ExpOp not disassembled"
    k = found[0][1]
    assert re.search(r"global_load_dwordx4", k) and re.search(r"global_store_dwordx4", k)
    assert re.search(r"v_rndne_f32", k) and re.search(r"ds_read", k)      # rounds to nearest even, gathers from LDS
    assert not re.search(r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak|v_mad_f32|v_mac_f32", k)


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "exp_softmax_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)
