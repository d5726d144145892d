"""CPU-side checks of ltanh, lsigmoid and the activation entry points (include/laser_hip.h "Activations"): the constants of
act_core.h are the model's; act_core.h as a host program (g++, ASan + UBSan, its own main) gives the bits of the numpy model;
a reduced range sweep checks faithfulness, monotonicity, oddness and the saturation points where they can go wrong, and fails
on a deliberately wrong build; the entry points are declared, exported and mirrored, refuse bad arguments and fail loudly
without a GPU; the generated forEach source carries the definition and its float64 pieces compile without fused
multiply-adds."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import code_objects
from tests import act_model as A
from tests.test_foreach_cpu import code, disasm, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "cpp", "act_core_host.cpp")
NEW = ["laser_hip_act_f32_dev", "laser_hip_act_f32", "laser_hip_act_grad_f32_dev"]
F32, F64 = 0, 1
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
REC = np.dtype([("tanh", "<u4"), ("sigmoid", "<u4"), ("exp", "<u8"), ("small", "<u8")])


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


def bits64(v):
    return np.asarray(v, np.float64).view(np.uint64)


# ---- the model and the constants --------------------------------------------------------------------------------------------
def test_constants_and_table_of_the_header_are_the_models():
    names, tab = A.header_constants()
    assert tab.shape == (64,) and np.array_equal(bits64(tab), bits64(A.T))
    want = {"INV": A.INV, "HI": A.HI, "LO": A.LO, "C2": A.C2, "C3": A.C3, "C4": A.C4, "C5": A.C5, "D3": A.D3, "D5": A.D5, "D7": A.D7,
            "RND": np.float64(1.5 * 2.0 ** 52), "SIG_CLAMP": A.SIG_CLAMP, "TANH_CLAMP": A.TANH_CLAMP, "TANH_SMALL": A.TANH_SMALL}
    assert set(names) == set(want)
    for k, v in want.items():
        assert bits64([names[k]])[0] == bits64([v])[0], k
    # what the constants are: the table is 2^(j/64) to an ulp of numpy's, T[0] = 1, T[32] = sqrt(2); HI has 24 low zero bits
    ref = 2.0 ** (np.arange(64) / 64.0)
    assert (np.abs(A.T - ref) <= np.spacing(ref)).all() and A.T[0] == 1 and A.T[32] == np.sqrt(2.0)
    assert int(bits64([A.HI])[0]) & 0xffffff == 0 and abs((A.HI + A.LO) - np.log(2.0) / 64) <= np.spacing(np.log(2.0) / 64)
    assert abs(A.INV - 64 / np.log(2.0)) <= np.spacing(64 / np.log(2.0))
    text = open(os.path.join(CSRC, "act_core.h")).read()
    assert text.count("#pragma clang fp contract(off)") == 4 and "#include" not in text
    assert not re.search(r"\b(exp|tanh|rint|fma)[fl]?\s*\(", re.sub(r"//[^\n]*", "", text).replace("lh_act_exp(", "").replace("lh_act_tanh(", ""))


def test_model_is_tanh_and_sigmoid_with_the_stated_edges():
    f = np.float32
    u = lambda v: np.asarray(v, f).view(np.uint32)
    x = f([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1, -1])
    t, s = A.ltanh(x), A.lsigmoid(x)
    assert list(u(t[:4])) == [0, 0x80000000, 0x3f800000, 0xbf800000] and np.isnan(t[4]) and np.isnan(s[4])
    assert list(u(t[5:7])) == [1, 0x80000001]                             # ltanh(x) = x for subnormal x
    assert list(u(s[:4])) == [0x3f000000, 0x3f000000, 0x3f800000, 0]
    assert t[7] == f(np.tanh(1.0)) and t[8] == -t[7] and s[7] == f(1 / (1 + np.exp(-1.0)))
    # the saturation points are where numpy's float64 functions put them
    for fn, b, val in ((A.ltanh, A.TANH_ONE_BITS, 1.0), (A.lsigmoid, A.SIG_ONE_BITS, 1.0), (A.lsigmoid, A.SIG_ZERO_BITS, 0.0)):
        at = np.array([b - 1, b], np.uint32).view(f)
        got = fn(at)
        assert got[1] == val and got[0] != val, (hex(b), got)
    # a subnormal sigmoid, rounded once
    assert A.lsigmoid(f([-100]))[0] == f(np.exp(np.float64(-100))) and 0 < A.lsigmoid(f([-100]))[0] < np.finfo(f).tiny
    x = np.random.default_rng(3).integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(f)
    x = x[np.isfinite(x)]
    with np.errstate(all="ignore"):
        rt = np.tanh(x.astype(np.float64))
        rs = np.where(x >= 0, 1 / (1 + np.exp(-x.astype(np.float64))), np.exp(x.astype(np.float64)) / (1 + np.exp(x.astype(np.float64))))
    ulp = lambda r: np.maximum(np.spacing(np.abs(r).astype(f)).astype(np.float64), 2.0 ** -149)
    assert (np.abs(A.ltanh(x).astype(np.float64) - rt) <= ulp(rt)).all()
    assert (np.abs(A.lsigmoid(x).astype(np.float64) - rs) <= ulp(rs)).all()
    assert np.array_equal(u(A.ltanh(-x)), u(A.ltanh(x)) ^ np.uint32(0x80000000))


def test_gradient_formulas_of_the_model_are_the_stated_operation_order():
    """against scalar float32 arithmetic written out one operation at a time; values where a fused or reordered form differs"""
    f = np.float32
    rng = np.random.default_rng(5)
    y = np.concatenate([f([0, 1, -1, -0.0, np.nan, 0.5, 1e-30, 0.99999994]), rng.uniform(-1, 1, 4000).astype(f)])
    dy = np.concatenate([f([3, np.nan, 7, -2, 1, np.inf, 1e30, -5]), rng.normal(0, 10, 4000).astype(f)])
    differs = {"tanh": 0, "sigmoid": 0}
    with np.errstate(all="ignore"):
        for kind in ("relu", "tanh", "sigmoid"):
            got = A.activation_grad(dy, y, kind)
            for i in range(y.size):
                a, g = y[i], dy[i]
                if kind == "relu":
                    want = g if a > 0 else f(0)
                elif kind == "tanh":
                    t = f(a * a)
                    want = f(g * f(f(1) - t))
                    differs[kind] += want != f(np.float64(g) * (1.0 - np.float64(a) * np.float64(a)))
                else:
                    uu = f(f(1) - a)
                    want = f(g * f(a * uu))
                    differs[kind] += want != f(f(g * a) * uu)
                assert A.same_bits(got[i:i + 1], f([want])), (kind, i, a, g)
    assert differs["tanh"] > 0 and differs["sigmoid"] > 0                  # the order matters on these inputs
    assert A.activation_grad(f([5]), f([np.nan]), "relu").view(np.uint32)[0] == 0       # NaN > 0 is false: +0
    assert A.same_bits(A.relu(f([np.nan, -0.0, -3, 2])), f([0, 0, 0, 2]))


# ---- act_core.h as a host program --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_act(tmp_path_factory):
    """act_core.h as a stand-alone host program under ASan and UBSan"""
    exe = tmp_path_factory.mktemp("act_host") / "act_core_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN, "-I", CSRC, HOST, "-o", str(exe)], check=True)

    def run(x):
        x = np.ascontiguousarray(x, np.float32)
        p = subprocess.run([str(exe)], input=x.tobytes(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return np.frombuffer(p.stdout, REC)
    return run


def check_host(host_act, x):
    r = host_act(x)
    assert r.size == x.size
    with np.errstate(all="ignore"):
        for name, want in (("tanh", A.ltanh(x)), ("sigmoid", A.lsigmoid(x))):
            got = r[name].view(np.float32)
            bad = np.nonzero(~(np.isnan(got) & np.isnan(want)) & (r[name] != want.view(np.uint32)))[0]
            assert bad.size == 0, (name, bad.size, [(x[i], hex(r[name][i]), hex(want.view(np.uint32)[i])) for i in bad[:5]])
        a = np.where(np.isnan(x), np.float32(0), np.abs(x)).astype(np.float64)
        e = A.exp_piece(-np.minimum(a, 208.0))
        p = A.tanh_small(np.minimum(a, 2.0 ** -6))
    assert np.array_equal(r["exp"], bits64(e)) and np.array_equal(r["small"], bits64(p))
    return r


def test_host_build_matches_the_model_on_the_edges(host_act):
    x = A.edges()
    r = check_host(host_act, x)
    t, s = r["tanh"].view(np.float32), r["sigmoid"].view(np.float32)
    assert np.isnan(t[np.isnan(x)]).all() and np.isnan(s[np.isnan(x)]).all()
    zero = x == 0
    assert np.array_equal(r["tanh"][zero], x[zero].view(np.uint32)) and (s[zero] == 0.5).all()
    assert (t[x == np.inf] == 1).all() and (t[x == -np.inf] == -1).all() and (s[x == np.inf] == 1).all()
    assert (r["sigmoid"][x == -np.inf] == 0).all()
    fin = np.isfinite(x)
    assert (np.abs(t[fin]) <= 1).all() and (s[fin] >= 0).all() and (s[fin] <= 1).all()


def test_host_build_matches_the_model_on_random_bit_patterns(host_act):
    x = np.random.default_rng(1).integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    check_host(host_act, x)
    # and densely where the work is: most random bit patterns saturate
    rng = np.random.default_rng(2)
    check_host(host_act, np.concatenate([rng.uniform(-110, 110, 1 << 17), rng.uniform(-1, 1, 1 << 17),
                                         rng.uniform(-0.03, 0.03, 1 << 17)]).astype(np.float32))


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = tmp_path_factory.mktemp("act_sweep") / "act_core_sweep"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, HOST, "-o", str(exe)], check=True)

    def run(fn, lo, hi, stride):
        p = subprocess.run([str(exe), "sweep", fn, hex(lo), hex(hi), str(stride)], capture_output=True, text=True)
        r = json.loads(p.stdout)
        print(r)
        assert p.returncode == 0 and r["unfaithful"] == 0 and r["not_monotone"] == 0 and r["not_odd"] == 0 and r["out_of_bounds"] == 0, r
        assert r["count"] == 2 * ((hi - lo) // stride + 1) and r["max_ulp"] < 1
        return r
    return run


def test_reduced_sweep_faithful_monotone_odd_bounded_with_the_saturation_points(sweep):
    """the full sweep (0 0x7f7fffff 1, both functions) is run by hand: profiles/activation/README.md records it.  Here, both
    signs throughout: stride 1 over [2^-7, 2^-5] (the seam of ltanh at 2^-6), over the binade of each saturation point and over
    every input whose sigmoid is subnormal; a prime stride over the rest."""
    seam = (0x3c000000, 0x3d000000)
    for fn in ("tanh", "sigmoid"):
        sweep(fn, *seam, 1)
    r = sweep("tanh", 0x41000000, 0x417fffff, 1)                           # [8, 16): tanh reaches 1 at 9.010914
    assert int(r["one_from"], 16) == A.TANH_ONE_BITS
    r = sweep("sigmoid", 0x41800000, 0x41ffffff, 1)                        # [16, 32): sigmoid reaches 1 at 17.32868
    assert int(r["one_from"], 16) == A.SIG_ONE_BITS
    r = sweep("sigmoid", 0x42ae0000, 0x42ffffff, 1)                        # from 87 to 128: every subnormal result, then 0
    assert int(r["zero_from"], 16) == A.SIG_ZERO_BITS
    x = np.array([0x42ae0000], np.uint32).view(np.float32)
    assert A.lsigmoid(-x)[0] >= np.finfo(np.float32).tiny                  # the range starts above the subnormal results
    rest = {"tanh": [(0, seam[0] - 1), (seam[1] + 1, 0x40ffffff), (0x41800000, 0x7f7fffff)],
            "sigmoid": [(0, seam[0] - 1), (seam[1] + 1, 0x417fffff), (0x42000000, 0x42adffff), (0x43000000, 0x7f7fffff)]}
    for fn, ranges in rest.items():
        for lo, hi in ranges:
            sweep(fn, lo, hi, 1009)


def test_sweep_fails_on_a_wrong_build(tmp_path):
    """the sweep can fail: with LO zeroed the reduced argument is off by k * 2.8e-11; at x = -32 (k = -2955) that is 8e-8 relative
    in e^x, more than a float32 ulp of the sigmoid.  (ltanh would not show it: where k is large, e^-2a is far below an ulp of 1.)"""
    exe = tmp_path / "sweep_broken"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DLH_ACT_LO_BITS=0x0000000000000000ull", "-I", CSRC, HOST,
                    "-o", str(exe)], check=True)
    p = subprocess.run([str(exe), "sweep", "sigmoid", "0x42000000", "0x42100000", "1"], capture_output=True, text=True)   # [32, 36]
    r = json.loads(p.stdout)
    assert p.returncode == 1 and r["unfaithful"] > 1000 and r["max_ulp"] > 1, r


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
    for name in (NEW[0], NEW[2]):
        assert name in hpp
    for proc in ("tanh", "sigmoid", "activationGrad"):
        assert re.search(r"proc %s\*" % proc, nim), proc
    for fn in ("tanh", "sigmoid", "activation_grad"):
        assert callable(getattr(laser_amd, fn)) and re.search(r"inline [\w<>]+ %s\(" % fn, hpp), fn
    assert callable(laser_amd.activation)
    text = open(HDR).read()
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text)
    for k, v in (("RELU", A.RELU), ("TANH", A.TANH), ("SIGMOID", A.SIGMOID)):
        assert re.search(r"#define LASER_HIP_ACT_%s %d\b" % (k, v), text)


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    i64 = C.c_int64
    p, q = C.c_void_p(4096), C.c_void_p(8192)    # never dereferenced: arguments are checked first
    one, four, zero = (i64 * 1)(1), (i64 * 1)(4), (i64 * 1)(0)
    fw, gr = L.laser_hip_act_f32_dev, L.laser_hip_act_grad_f32_dev
    for act in (0, 4, -1, 0x100 | 1, 0x200 | 2, 0x300, 1 << 16):              # NONE, unknown codes, the PRE_ bits
        assert fw(act, q, one, p, one, four, 1, None) == _lib.E_INVALID, act
        assert gr(act, q, one, p, one, p, one, four, 1, None) == _lib.E_INVALID, act
        assert L.laser_hip_act_f32(act, q, p, 4) == _lib.E_INVALID, act
    ones = (i64 * 7)(*[1] * 7)
    for act in (A.RELU, A.TANH, A.SIGMOID):
        assert fw(act, q, ones, p, ones, ones, 7, None) == _lib.E_INVALID                       # rank 7
        assert gr(act, q, ones, p, ones, p, ones, ones, 7, None) == _lib.E_INVALID
        assert fw(act, q, zero, p, one, four, 1, None) == _lib.E_INVALID                        # stride 0 on an output
        assert gr(act, q, zero, p, one, p, one, four, 1, None) == _lib.E_INVALID
        assert fw(act, q, one, p, one, (i64 * 1)(-4), 1, None) == _lib.E_INVALID                # a negative extent
        assert fw(act, q, None, p, one, four, 1, None) == _lib.E_INVALID                        # null strides
        assert gr(act, q, one, p, one, p, None, four, 1, None) == _lib.E_INVALID
        assert L.laser_hip_act_f32(act, None, None, -1) == _lib.E_INVALID
        assert L.laser_hip_act_f32(act, None, None, 3) == _lib.E_INVALID
    import laser_amd
    with pytest.raises(ValueError):
        laser_amd.activation(np.ones(4, np.float32), "gelu")


def test_entry_points_need_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one the host-pointer form gives the model's bits"""
    from laser_amd import _lib
    import laser_amd
    x = A.edges()
    y = np.empty_like(x)
    for act, fn in ((A.RELU, A.relu), (A.TANH, A.ltanh), (A.SIGMOID, A.lsigmoid)):
        rc = L.laser_hip_act_f32(act, y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), x.size)
        if have_gpu():
            assert rc == 0 and A.same_bits(y, fn(x))
        else:
            assert rc == _lib.E_NODEVICE
    if have_gpu():
        return
    p, q = C.c_void_p(4096), C.c_void_p(8192)
    one, four = (C.c_int64 * 1)(1), (C.c_int64 * 1)(4)
    for act in (A.RELU, A.TANH, A.SIGMOID):
        assert L.laser_hip_act_f32_dev(act, q, one, p, one, four, 1, None) == _lib.E_NODEVICE
        assert L.laser_hip_act_grad_f32_dev(act, q, one, p, one, p, one, four, 1, None) == _lib.E_NODEVICE
    for call in (lambda: laser_amd.tanh(np.ones(4, np.float32)), lambda: laser_amd.sigmoid(np.ones(4, np.float32)),
                 lambda: laser_amd.activation(np.ones(4, np.float32), "relu")):
        with pytest.raises(laser_amd.LaserHipError) as e:
            call()
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
    core = open(os.path.join(CSRC, "act_core.h")).read()
    log_core = open(os.path.join(CSRC, "log_core.h")).read()
    exp_core = open(os.path.join(CSRC, "exp_core.h")).read()
    src = _source(L, L.laser_hip_foreach_source, spec("y = laser_tanh(x) * laser_sigmoid(x)", [("y", F32, 1), ("x", F32, 0)]))
    red = _source(L, L.laser_hip_foreach_reduce_source,
                  spec("acc += laser_sigmoid(x) - m", [("x", F32, 0)], [("m", F32)]) + [b"acc", F32, b"acc += other"])
    for s in (src, red):
        assert core in s and log_core in s and exp_core in s                # the headers as they stand
        assert s.index(exp_core) < s.index(log_core) < s.index(core) < s.index("void lh_body(")
        assert s.index("float laser_tanh(") < s.index("void lh_body(") and s.index("float laser_sigmoid(") < s.index("void lh_body(")
    n = C.c_int64()
    for name in ("laser_tanh", "laser_sigmoid"):                            # reserved like laser_log
        for ops, params in (([(name, F32, 1)], []), ([("y", F32, 1)], [(name, F32)])):
            assert L.laser_hip_foreach_source(*spec("y = 1", ops, params), None, 0, C.byref(n)) == _lib.E_INVALID
        assert L.laser_hip_foreach_reduce_source(*spec(name + " += x", [("x", F32, 0)]), name.encode(), F32, (name + " += other").encode(),
                                                 None, 0, C.byref(n)) == _lib.E_INVALID


FMA = r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak|v_mad_f32|v_mac_f32"


@pytest.mark.parametrize("body", ["y = lh_act_exp(x)", "y = lh_act_tanh_small(x)"])
def test_float64_pieces_compile_without_fused_multiply_adds(L, tmp_path, body):
    """the pieces around the division, through a float64 forEach body: the full functions cannot be checked this way, because
    a correctly rounded division is built from fmas"""
    rc, blob = code(L, body, [("y", F64, 1), ("x", F64, 0)])
    assert rc == 0, blob
    k = disasm(blob, tmp_path, "lh_foreach_vector")
    assert re.search(r"v_mul_f64", k) and re.search(r"v_add_f64", k)
    assert not re.search(FMA, k)
    assert not re.search(r"v_exp_f32|v_rcp_f64|v_div_|v_rndne", k)        # no device exponential, no division, no rounding instruction


def test_bodies_with_the_full_functions_compile(L, tmp_path):
    rc, blob = code(L, "y = laser_tanh(x); z = laser_sigmoid(x)", [("y", F32, 1), ("z", F32, 1), ("x", F32, 0)])
    assert rc == 0, blob
    k = disasm(blob, tmp_path, "lh_foreach_vector")
    assert re.search(r"v_div_fixup_f64", k) and re.search(r"v_cvt_f32_f64", k)           # the float64 division, one rounding
    assert not re.search(r"v_exp_f32|v_(pk_)?fma_f32|v_fmac_f32|v_mad_f32|v_mac_f32", k)   # nothing in float32, no device exp


def test_precompiled_kernels_vectorise_and_the_gradients_hold_no_fused_multiply_adds(tmp_path):
    """the gfx950 code object with the activation kernels, cut out of the library's offload bundles: the vector kernels move 16
    bytes per lane, the gradient kernels hold float32 multiplies and adds and nothing fused (the vector ones: the strided ones
    share the same inlined rule, but their 64-bit index divisions are lowered through float fmas), the forward kernels divide
    once per element in float64 and call no device exponential"""
    seen = 0
    for name, k in code_objects.kernels(b"ActGradOp", r"\w*pointwise_vec_kernelINS\w*ActGradOpILi[123]E\w*", tmp_path):
        seen += 1
        assert not re.search(FMA, k) and not re.search(r"_f64", k), name
        if re.search(r"ActGradOpILi([123])E", name).group(1) != "1":
            assert re.search(r"v_(pk_)?mul_f32", k) and re.search(r"v_(pk_)?(add|sub)_f32", k), name
        assert re.search(r"global_load_dwordx4", k) and re.search(r"global_store_dwordx4", k), name
    assert seen == 3
    seen = 0
    for name, k in code_objects.kernels(b"ActGradOp", r"\w*pointwise_vec_kernelINS\w*ActOpILi[123]E\w*", tmp_path):
        seen += 1
        assert re.search(r"global_load_dwordx4", k) and re.search(r"global_store_dwordx4", k), name
        assert not re.search(r"v_exp_f32|v_(pk_)?fma_f32|v_fmac_f32|v_mad_f32|v_mac_f32", k), name
        if re.search(r"ActOpILi([123])E", name).group(1) != "1":
            assert len(re.findall(r"v_div_fixup_f64", k)) == 5 and re.search(r"v_mul_f64", k), name   # 4 of a vector + the tail
    assert seen == 3


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "activation_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)
