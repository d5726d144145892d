"""CPU-side checks of llog and the row kernels' plan (include/laser_hip.h "log, logsumexp, log-softmax and cross-entropy"):
log_core.h as a host program (g++, ASan + UBSan, its own main) gives the bits of the numpy model; the range sweep proves
faithfulness and monotonicity over [1/2, 2], the subnormals and every 251st float elsewhere; the plan header as a host program
against the boundaries; the entry points are declared, exported and mirrored and fail loudly without a GPU; the generated
forEach source carries the definition and compiles without fused multiply-adds."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import code_objects
from tests import log_model as G
from tests.test_foreach_cpu import code, disasm, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_log_f32_dev", "laser_hip_log_f32", "laser_hip_logsumexp_rows_f32_dev", "laser_hip_log_softmax_rows_f32_dev",
       "laser_hip_softmax_xent_rows_f32_dev", "laser_hip_softmax_rows_plan"]
F32 = 0
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]


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


# ---- the model and the table ------------------------------------------------------------------------------------------------
def test_table_and_constants_of_the_header_are_the_models():
    inv, logc = G.header_table()
    assert inv.shape == (16,) and np.array_equal(inv.view(np.uint64), G.INVC.view(np.uint64))
    assert np.array_equal(logc.view(np.uint64), G.LOGC.view(np.uint64))
    assert inv[9] == 1 and logc[9] == 0 and not np.signbit(logc[9])
    # LOGC is -ln INVC to the ulp numpy's log promises, and the intervals tile [OFF, 2 OFF) around 1
    ref = -np.log(G.INVC)
    assert (np.abs(G.LOGC - ref) <= np.spacing(np.abs(ref))).all()
    lo, hi = G.intervals()
    assert lo[0] == 0.69921875 and hi[15] == 1.3984375 and np.array_equal(lo[1:], hi[:-1]) and lo[9] < 1 < hi[9]
    text = open(os.path.join(CSRC, "log_core.h")).read()
    for name, v in (("LN2", G.LN2), ("C2", G.C2), ("C3", G.C3), ("C4", G.C4), ("C5", G.C5), ("C6", G.C6)):
        bits = int(np.array([v], np.float64).view(np.uint64)[0])
        assert re.search(r"#define LH_LOG_%s_BITS 0x%016xull" % (name, bits), text), name
    assert abs(G.LN2 - np.log(2.0)) <= np.spacing(np.log(2.0))
    assert re.search(r"#define LH_LOG_OFF 0x%08xu" % G.OFF, text)
    assert "#pragma clang fp contract(off)" in text and "#include" not in text


def test_model_is_a_logarithm_with_the_stated_edges():
    f = np.float32
    got = G.llog(f([1, 0.0, -0.0, np.inf, -np.inf, -1, np.nan, 1e-45]))
    assert got.view(np.uint32)[0] == 0                                   # +0 exactly
    assert got[1] == -np.inf and got[2] == -np.inf and got[3] == np.inf
    assert np.isnan(got[4:7]).all()
    assert got[7] == f(np.log(2.0 ** -149))                              # the smallest subnormal, as the number it is
    x = np.abs(np.random.default_rng(3).integers(1, 0x7f800000, 200000).astype(np.uint32).view(np.float32))
    ref = np.log(x.astype(np.float64))
    assert (np.abs(G.llog(x).astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
    assert G.same_bits(G.log_softmax_row(f([0, -200])), f([0, -200]))
    assert G.logsumexp_row(f([-np.inf, -np.inf])) == -np.inf and G.logsumexp_row(f([1, np.inf])) == np.inf
    assert np.isnan(G.logsumexp_row(f([1, np.nan])))
    loss, g = G.xent_row(f([1, 2, 3]), 2)
    assert abs(loss - 0.40760596) < 1e-6 and abs(g.sum()) < 1e-6
    assert G.xent_row(f([1, 2]), -1)[0].view(np.uint32) == 0 and np.isnan(G.xent_row(f([1, 2]), 2)[0])


# ---- log_core.h as a host program --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_log(tmp_path_factory):
    """log_core.h as a stand-alone host program under ASan and UBSan"""
    exe = tmp_path_factory.mktemp("log_host") / "log_core_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN, "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "log_core_host.cpp"), "-o", str(exe)], check=True)

    def run(x):
        x = np.ascontiguousarray(x, np.float32)
        p = subprocess.run([str(exe)], input=x.tobytes(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return np.frombuffer(p.stdout, np.float32).reshape(x.shape)
    return run


def test_host_build_matches_the_model_on_the_edges(host_log):
    x = G.edges()
    got, want = host_log(x), G.llog(x)
    assert G.same_bits(got, want), [(a, hex(b), hex(c)) for a, b, c in zip(x, got.view(np.uint32), want.view(np.uint32)) if b != c and a == a]
    assert np.isnan(got[np.isnan(x)]).all() and np.isnan(got[x < 0]).all()
    assert (got[x == 0] == -np.inf).all() and (got[x == np.inf] == np.inf).all()
    assert got[x == 1].view(np.uint32)[0] == 0
    fin = (x > 0) & np.isfinite(x)
    ref = np.log(x[fin].astype(np.float64))
    assert (np.abs(got[fin].astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()


def test_host_build_matches_the_model_on_random_bit_patterns(host_log):
    x = np.random.default_rng(1).integers(0, 2 ** 32, 1 << 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    got, want = host_log(x), G.llog(x)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))[0]
    assert bad.size == 0, (bad.size, x[bad[:5]])


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = tmp_path_factory.mktemp("log_sweep") / "log_core_sweep"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "log_core_host.cpp"),
                    "-o", str(exe)], check=True)

    def run(lo, hi, stride):
        p = subprocess.run([str(exe), "sweep", hex(lo), hex(hi), str(stride)], capture_output=True, text=True)
        r = json.loads(p.stdout)
        assert p.returncode == 0 and r["unfaithful"] == 0 and r["not_monotone"] == 0, r
        return r
    return run


def test_faithful_and_monotone_over_half_to_two_the_subnormals_and_a_stride_elsewhere(sweep):
    """the full sweep (1 0x7f7fffff 1) is run by hand: profiles/log_softmax/README.md records it"""
    r = sweep(0x3f000000, 0x40000000, 1)                      # [1/2, 2]: where the cancellation lives
    assert r["count"] == (1 << 24) + 1 and r["max_ulp"] < 1
    print(r)
    r = sweep(0x00000001, 0x007fffff, 1)                      # every subnormal
    assert r["count"] == (1 << 23) - 1 and r["max_ulp"] < 1
    print(r)
    for lo, hi in ((0x00800000, 0x3effffff), (0x40000001, 0x7f7fffff)):
        r = sweep(lo, hi, 251)
        assert r["count"] == (hi - lo) // 251 + 1 and r["max_ulp"] < 1
        print(r)


def test_sweep_fails_on_a_wrong_logarithm(tmp_path):
    """the sweep can fail: with LN2 off by 1.2e-7, inputs near 32 (k = 5) are ulps off"""
    text = open(os.path.join(CSRC, "log_core.h")).read()
    broken = text.replace("0x3fe62e42fefa39efull", "0x3fe62e4400000000ull")
    assert broken != text
    (tmp_path / "log_core.h").write_text(broken)
    exe = tmp_path / "sweep_broken"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(tmp_path), os.path.join(ROOT, "tests", "cpp", "log_core_host.cpp"),
                    "-o", str(exe)], check=True)
    p = subprocess.run([str(exe), "sweep", "0x42000000", "0x42100000", "1"], capture_output=True, text=True)
    assert p.returncode == 1 and json.loads(p.stdout)["unfaithful"] > 0


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def want_plan(rows, n, vec):
    if rows < 0 or n < 1 or n > 1 << 26:
        return (-1, -1, -1, -1)
    k = 0 if n <= 1024 else 1 if n <= 8192 else 2
    groups = min(2048, -(-rows // 4) if k == 0 else rows)
    return (0, k + (0 if vec else 4), groups, 4096 + (1040 if k else 0) + (32768 if k == 2 else 0))


def plan_cases():
    ns = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193, 16385, (1 << 26) - 1, 1 << 26, (1 << 26) + 1]
    rows = [-1, 0, 1, 3, 4, 5, 9, 2047, 2048, 2049, 2050, 4 * 2048 - 1, 4 * 2048, 4 * 2048 + 1, 4 * 2048 + 5, 1 << 40]
    return [(r, n, v) for n in ns for r in rows for v in (0, 1)]


def test_plan_header_as_a_host_program_over_the_boundaries(tmp_path):
    exe = tmp_path / "softmax_rows_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *SAN, "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "softmax_rows_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    cases = plan_cases()
    p = subprocess.run([str(exe)], input="".join("%d %d %d\n" % c for c in cases), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [tuple(int(w) for w in line.split()) for line in p.stdout.splitlines()]
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == want_plan(*c), (c, g)
    text = open(os.path.join(CSRC, "softmax_rows_plan.h")).read()
    assert "#include" not in text                                      # no HIP, no includes: g++ alone built it


def test_plan_entry_point_and_the_launchers_use_the_header(L):
    from laser_amd import _lib
    out = (C.c_int64 * 3)()
    for c in plan_cases():
        rc = L.laser_hip_softmax_rows_plan(*c, out)
        w = want_plan(*c)
        if w[0]:
            assert rc == _lib.E_INVALID, c
        else:
            assert rc == 0 and tuple(out) == w[1:], (c, tuple(out))
    assert L.laser_hip_softmax_rows_plan(1, 1, 1, None) == _lib.E_INVALID
    hip = open(os.path.join(CSRC, "log_softmax.hip")).read()
    assert hip.count("lh_softmax_rows_plan(") == 1 and '#include "softmax_rows_plan.h"' in hip
    assert "atomic" not in re.sub(r"//[^\n]*", "", hip)               # no workgroup waits on another
    # the row launchers are all in that one file: exp_softmax.hip holds the elementwise lexp alone
    assert "softmax_rows_plan" not in open(os.path.join(CSRC, "exp_softmax.hip")).read()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------
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
    for name in NEW[:1] + NEW[2:5]:
        assert name in hpp
    for proc in ("log", "logsumexp", "logSoftmax", "softmaxCrossEntropy"):
        assert re.search(r"proc %s\*" % proc, nim), proc
    for fn in ("log", "logsumexp", "log_softmax", "softmax_cross_entropy"):
        assert callable(getattr(laser_amd, fn)) and re.search(r"inline [\w<>]+ %s\(" % fn, hpp), fn


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    i64 = C.c_int64
    p, q = C.c_void_p(4096), C.c_void_p(8192)    # never dereferenced: arguments are checked first
    for fn in (L.laser_hip_logsumexp_rows_f32_dev, L.laser_hip_log_softmax_rows_f32_dev):
        assert fn(q, 8, p, 8, 1, 0, None) == _lib.E_INVALID                  # n = 0
        assert fn(q, 1 << 27, p, 1 << 27, 1, (1 << 26) + 1, None) == _lib.E_INVALID
        assert fn(q, 8, p, 8, -1, 8, None) == _lib.E_INVALID                 # rows < 0
        assert fn(q, 8, p, 7, 2, 8, None) == _lib.E_INVALID                  # a source row stride below n
    assert L.laser_hip_logsumexp_rows_f32_dev(q, 0, p, 8, 2, 8, None) == _lib.E_INVALID
    assert L.laser_hip_log_softmax_rows_f32_dev(q, 7, p, 8, 2, 8, None) == _lib.E_INVALID
    assert L.laser_hip_log_softmax_rows_f32_dev(p, 8, p, 12, 2, 8, None) == _lib.E_INVALID      # in place with unequal strides
    xe = L.laser_hip_softmax_xent_rows_f32_dev
    assert xe(None, 1, None, 8, p, 8, q, 2, 8, 1.0, None) == _lib.E_INVALID   # neither loss nor grad
    assert xe(q, 0, None, 8, p, 8, q, 2, 8, 1.0, None) == _lib.E_INVALID      # loss stride 0
    assert xe(None, 1, q, 7, p, 8, q, 2, 8, 1.0, None) == _lib.E_INVALID      # gradient row stride below n
    assert xe(None, 1, p, 8, p, 8, q, 2, 8, 1.0, None) == _lib.E_INVALID      # the gradient over the logits
    assert xe(q, 1, None, 8, p, 8, q, 2, 0, 1.0, None) == _lib.E_INVALID      # n = 0
    lg = L.laser_hip_log_f32_dev
    one = (i64 * 7)(*[1] * 7)
    assert lg(p, one, p, one, one, 7, None) == _lib.E_INVALID                # rank 7
    assert lg(p, (i64 * 1)(0), p, (i64 * 1)(1), (i64 * 1)(4), 1, None) == _lib.E_INVALID     # stride 0 on dst
    assert lg(p, (i64 * 1)(1), p, (i64 * 1)(1), (i64 * 1)(-4), 1, None) == _lib.E_INVALID
    assert L.laser_hip_log_f32(None, None, -1) == _lib.E_INVALID
    assert L.laser_hip_log_f32(None, None, 3) == _lib.E_INVALID


def test_entry_points_need_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one the host-pointer form gives the model's bits"""
    from laser_amd import _lib
    x = G.edges()
    y = np.empty_like(x)
    rc = L.laser_hip_log_f32(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), x.size)
    if have_gpu():
        assert rc == 0 and G.same_bits(y, G.llog(x))
        return
    assert rc == _lib.E_NODEVICE
    p, q = C.c_void_p(4096), C.c_void_p(8192)
    one = (C.c_int64 * 1)(1)
    assert L.laser_hip_log_f32_dev(p, one, p, one, (C.c_int64 * 1)(4), 1, None) == _lib.E_NODEVICE
    assert L.laser_hip_logsumexp_rows_f32_dev(q, 1, p, 8, 2, 8, None) == _lib.E_NODEVICE
    assert L.laser_hip_log_softmax_rows_f32_dev(q, 8, p, 8, 2, 8, None) == _lib.E_NODEVICE
    assert L.laser_hip_softmax_xent_rows_f32_dev(q, 1, None, 8, p, 8, q, 2, 8, 1.0, None) == _lib.E_NODEVICE
    import laser_amd
    with pytest.raises(laser_amd.LaserHipError) as e:
        laser_amd.log(np.ones(4, np.float32))
    assert e.value.code == _lib.E_NODEVICE


# ---- forEach bodies -----------------------------------------------------------------------------------------------------------
def _source(L, fn, args):
    n = C.c_int64()
    assert fn(*args, None, 0, C.byref(n)) == 0
    buf = C.create_string_buffer(n.value)
    assert fn(*args, buf, n.value, C.byref(n)) == 0
    return buf.value.decode()


def test_generated_sources_carry_the_definition(L):
    from laser_amd import _lib
    core = open(os.path.join(CSRC, "log_core.h")).read()
    exp_core = open(os.path.join(CSRC, "exp_core.h")).read()
    src = _source(L, L.laser_hip_foreach_source, spec("y = laser_log(x)", [("y", F32, 1), ("x", F32, 0)]))
    red = _source(L, L.laser_hip_foreach_reduce_source,
                  spec("acc += laser_log(x) - m", [("x", F32, 0)], [("m", F32)]) + [b"acc", F32, b"acc += other"])
    for s in (src, red):
        assert core in s and exp_core in s                 # both headers as they stand
        assert s.index(exp_core) < s.index(core) < s.index("void lh_body(")
        assert s.index("float laser_log(") < s.index("void lh_body(")
    # the name is reserved like laser_exp
    n = C.c_int64()
    for ops, params in (([("laser_log", F32, 1)], []), ([("y", F32, 1)], [("laser_log", F32)])):
        assert L.laser_hip_foreach_source(*spec("y = 1", ops, params), None, 0, C.byref(n)) == _lib.E_INVALID
    assert L.laser_hip_foreach_reduce_source(*spec("laser_log += x", [("x", F32, 0)]), b"laser_log", F32, b"laser_log += other",
                                             None, 0, C.byref(n)) == _lib.E_INVALID


def test_body_with_laser_log_compiles_without_fused_multiply_adds(L, tmp_path):
    rc, blob = code(L, "y = laser_log(x)", [("y", F32, 1), ("x", F32, 0)])
    assert rc == 0, blob
    k = disasm(blob, tmp_path, "lh_foreach_vector")
    assert re.search(r"v_mul_f64", k) and re.search(r"v_add_f64", k) and re.search(r"v_cvt_f32_f64", k)
    assert not re.search(r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak|v_mad_f32|v_mac_f32", k)
    assert not re.search(r"v_log_f32|v_rcp_f64|v_div_", k)              # no device logarithm, no division


def test_precompiled_log_kernels_have_no_fused_multiply_adds(tmp_path):
    """pointwise_vec_kernel<LogOp> is llog and nothing else, 16 bytes per lane; the logsumexp and log-softmax kernels have no
    division, so they hold no fma either (the cross-entropy's gradient divides as the softmax does: a correctly rounded
    division is built from fmas).  The gfx950 code objects are cut out of the library's offload bundles (tests/code_objects.py)."""
    fma = r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak|v_mad_f32|v_mac_f32"
    found = code_objects.kernels(b"LogOp", r"\w*pointwise_vec_kernelINS\w*LogOp\w*", tmp_path)
    assert len(found) == 1, "the vector instance of LogOp not disassembled"
    k = found[0][1]
    assert re.search(r"global_load_dwordx4", k) and re.search(r"global_store_dwordx4", k) and re.search(r"v_mul_f64", k)
    assert not re.search(fma, k) and not re.search(r"v_log_f32", k)
    seen = 0
    for name, k in code_objects.kernels(b"LogOp", r"\w*rows_(?:wave|block|long)_kernelILb[01]ELi[012]E\w*", tmp_path):
        seen += 1
        if re.search(r"_kernelILb[01]ELi([012])E", name).group(1) in "01":   # logsumexp, log-softmax
            assert not re.search(fma, k), name
        assert re.search(r"v_mul_f64", k) and not re.search(r"v_log_f32", k), name
    assert seen == 18


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "log_softmax_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)
