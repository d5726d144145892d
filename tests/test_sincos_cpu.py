"""CPU-side checks of lsin, lcos and their entry points (include/laser_hip.h "Sine and cosine"): the constants and the 2/pi
table of sincos_core.h are what scripts/gen_sincos_constants.py recomputes from integer arithmetic; sincos_core.h as a host
program (g++, ASan + UBSan, its own main) gives the bits of the numpy model; a reduced sweep against 80-bit sinl / cosl checks
faithfulness, symmetry, the bound and monotonicity where they can go wrong, and fails on a deliberately wrong build; the entry
points are declared, exported and mirrored, refuse bad arguments and fail loudly without a GPU; the core compiles for gfx950
without fused multiply-adds and the two forEach bodies of the reference compile."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import code_objects
from tests import sincos_model as S
from tests.test_foreach_cpu import code, disasm, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
HOST = os.path.join(ROOT, "tests", "cpp", "sincos_core_host.cpp")
NEW = ["laser_hip_sin_f32_dev", "laser_hip_cos_f32_dev", "laser_hip_sincos_f32_dev", "laser_hip_sin_f32", "laser_hip_cos_f32"]
F32, F64 = 0, 1
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan"]
REC = np.dtype([("sin", "<u4"), ("cos", "<u4"), ("both_sin", "<u4"), ("both_cos", "<u4"), ("q", "<u4"), ("pad", "<u4"), ("r", "<u8")])
RETURNS_X = 0x39e89768          # the largest bits up to which lsin(x) = x without a gap (the full sweep reports it)
COS_ONE = 0x39800000            # and lcos(x) = 1: 2^-12
HALF_PI_BELOW = 0x3fc90fda      # the largest float32 <= pi/2
QUARTER_PI = 0x3f490fdb         # float32(pi/4)


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


def u32(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


# ---- (a) the constants ----------------------------------------------------------------------------------------------------------
def test_constants_and_table_of_the_header_are_what_the_script_recomputes():
    names, tab, big, nan = S.header_constants()
    want = {k: v for k, v in S.BITS.items() if k != "TWO_OVER_PI"}
    assert set(names) == set(want)
    for k, v in want.items():
        assert names[k] == v, (k, hex(names[k]), hex(v))
    assert tab == [0] + S.BITS["TWO_OVER_PI"] and len(tab) == 9
    assert big == S.BIG == int(u32([2.0 ** 20])[0]) and nan == S.NAN == 0x7fc00000
    # what the constants are, against numpy's float64 (an independent source)
    f = lambda name: S.K[name]
    assert f("INV") == np.float64(2 / np.pi) and f("PIO2") == np.float64(np.pi / 2) and f("RND") == 1.5 * 2.0 ** 52
    for name in ("P1", "P2"):                           # 24 significant bits: 29 low zero bits in the significand
        assert S.BITS[name] & ((1 << 29) - 1) == 0
    assert 0 < np.pi / 2 - (f("P1") + f("P2")) < 2.0 ** -47 and (f("P1") + f("P2")) + f("P3") == np.float64(np.pi / 2)   # cut, not rounded
    assert 0 < f("P3") < 2.0 ** -47 and f("P1") > f("P2") > f("P3")
    import math
    for j in range(1, 8):
        assert abs(f("S%d" % (2 * j + 1)) - (-1) ** j / math.factorial(2 * j + 1)) <= np.spacing(1 / math.factorial(2 * j + 1))
    for j in range(1, 9):
        assert abs(f("C%d" % (2 * j)) - (-1) ** j / math.factorial(2 * j)) <= np.spacing(1 / math.factorial(2 * j))
    # the table is 2/pi: its first 53 bits are float64(2/pi)'s significand, rounded up when the 54th bit is set
    top, bit54 = (tab[1] << 32 | tab[2]) >> 11, (tab[2] >> 10) & 1
    assert top + bit54 == (S.BITS["INV"] & ((1 << 52) - 1)) | (1 << 52)
    # the script prints the header's lines
    out = subprocess.run(["python3", os.path.join(ROOT, "scripts", "gen_sincos_constants.py")], check=True, capture_output=True, text=True).stdout
    text = open(S.CORE).read()
    squeeze = lambda s: re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", s))
    flat = squeeze(text.replace("#ifndef LH_SC_P3_BITS", "").replace("#endif", ""))
    for line in out.splitlines():
        if line.startswith("#define"):
            assert squeeze(line).strip() in flat, line
    assert squeeze(out[out.index("static const"):]).strip() in squeeze(text)
    assert text.count("#pragma clang fp contract(off)") == 4 and "#include" not in text
    body = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\b(sin|cos|sincos|fma|rint|floor)[fl]?\s*\(", body.replace("lh_sin(", "").replace("lh_cos(", "").replace("lh_sincos(", "").replace("laser_sin(", "").replace("laser_cos(", ""))
    assert "/" not in re.sub(r"#\w+[^\n]*", "", body)   # no division anywhere in the code


def test_model_is_sine_and_cosine_with_the_stated_edges():
    f = np.float32
    x = f([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1, -1])
    s, c = S.lsincos(x)
    assert list(u32(s[:2])) == [0, 0x80000000] and list(u32(c[:2])) == [0x3f800000] * 2
    assert list(u32(s[2:5])) == [S.NAN] * 3 and list(u32(c[2:5])) == [S.NAN] * 3
    assert list(u32(-x[4:5])) != [S.NAN] and list(u32(S.lsin(-x[4:5]))) == [S.NAN]          # whatever the sign and payload
    assert list(u32(s[5:7])) == [1, 0x80000001] and list(u32(c[5:7])) == [0x3f800000] * 2   # subnormals: x and 1
    assert s[7] == f(np.sin(1.0)) and s[8] == -s[7] and c[7] == f(np.cos(1.0)) and c[8] == c[7]
    assert S.returns_x_boundary() == RETURNS_X
    at = np.array([COS_ONE, COS_ONE + 1], np.uint32).view(f)
    assert list(S.lcos(at) == 1) == [True, False]
    # faithful against numpy's float64 functions where those are good to far below a float32 ulp (|x| < 2^20)
    x = np.random.default_rng(3).uniform(-2.0 ** 20, 2.0 ** 20, 200000).astype(f)
    x = np.concatenate([x, np.random.default_rng(4).uniform(-8, 8, 200000).astype(f)])
    ulp = lambda r: np.spacing(np.abs(r).astype(f)).astype(np.float64)
    for got, ref in ((S.lsin(x), np.sin(x.astype(np.float64))), (S.lcos(x), np.cos(x.astype(np.float64)))):
        assert (np.abs(got.astype(np.float64) - ref) <= ulp(ref)).all()
        assert (np.abs(got) <= 1).all()
    assert np.array_equal(u32(S.lsin(-x)), u32(S.lsin(x)) ^ np.uint32(0x80000000)) and np.array_equal(u32(S.lcos(-x)), u32(S.lcos(x)))
    # the largest float32: sin(2^128 - 2^104) = -0.5218765, cos = 0.8530210 (any correctly rounding library gives these)
    big = np.array([0x7f7fffff], np.uint32).view(f)
    assert S.lsin(big)[0] == f(-0.5218765) and S.lcos(big)[0] == f(0.8530210)


# ---- (b) sincos_core.h as a host program ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_sc(tmp_path_factory):
    """sincos_core.h as a stand-alone host program under ASan and UBSan"""
    exe = tmp_path_factory.mktemp("sc_host") / "sincos_core_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *SAN, "-I", CSRC, HOST, "-o", str(exe)], check=True)

    def run(x):
        x = np.ascontiguousarray(x, np.float32)
        p = subprocess.run([str(exe)], input=x.tobytes(), capture_output=True)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return np.frombuffer(p.stdout, REC)
    return run


def check_host(host_sc, x):
    r = host_sc(x)
    assert r.size == x.size
    s, c = S.lsincos(x)
    for name, want in (("sin", s), ("cos", c), ("both_sin", s), ("both_cos", c)):
        bad = np.nonzero(r[name] != u32(want))[0]       # the model's NaN is the header's one NaN: plain equality of bits
        assert bad.size == 0, (name, bad.size, [(x[i], hex(r[name][i]), hex(u32(want)[i])) for i in bad[:5]])
    fin = np.isfinite(x)
    q, red = S.reduce(u32(x)[fin] & np.uint32(0x7fffffff))
    assert np.array_equal(r["q"][fin], q.astype(np.uint32)) and np.array_equal(r["r"][fin], red.view(np.uint64))
    return r


def test_host_build_matches_the_model_on_the_edges(host_sc):
    x = S.edges()
    b = set(int(v) for v in u32(x))
    for need in (0, 0x80000000, 1, 0x007fffff, RETURNS_X, RETURNS_X + 1, S.BIG - 1, S.BIG, S.BIG + 1, 0x7f7fffff, 0x7f800000, 0xff800000,
                 0x7fc00000, 0x7f800001, HALF_PI_BELOW, HALF_PI_BELOW + 1, QUARTER_PI, *[e << 23 for e in range(1, 255)]):
        assert need in b, hex(need)
    for k in range(1, 17):
        near = int(u32([k * np.pi / 2])[0])
        assert {near - 1, near, near + 1} <= b
    r = check_host(host_sc, x)
    s, c = r["sin"].view(np.float32), r["cos"].view(np.float32)
    special = ~np.isfinite(x)
    assert (r["sin"][special] == S.NAN).all() and (r["cos"][special] == S.NAN).all()
    zero = x == 0
    assert np.array_equal(r["sin"][zero], u32(x)[zero]) and (c[zero] == 1).all()
    fin = ~special
    assert (np.abs(s[fin]) <= 1).all() and (np.abs(c[fin]) <= 1).all()
    sub = fin & (np.abs(x) < np.finfo(np.float32).tiny)
    assert sub.sum() >= 6 and np.array_equal(r["sin"][sub], u32(x)[sub]) and (c[sub] == 1).all()


def test_host_build_matches_the_model_on_random_bit_patterns(host_sc):
    x = np.random.default_rng(1).integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    check_host(host_sc, x)
    # and densely where arguments usually are: random bit patterns are mostly tiny or huge
    rng = np.random.default_rng(2)
    check_host(host_sc, np.concatenate([rng.uniform(-10, 10, 1 << 17), rng.uniform(-2.0 ** 20, 2.0 ** 20, 1 << 17),
                                        rng.uniform(-2.0 ** 22, 2.0 ** 22, 1 << 17)]).astype(np.float32))


# ---- (c), (d) the sweep ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sc_sweep") / "sincos_core_sweep"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, HOST, "-o", str(exe)], check=True)

    def run(fn, lo, hi, stride):
        p = subprocess.run([str(exe), "sweep", fn, hex(lo), hex(hi), str(stride)], capture_output=True, text=True)
        r = json.loads(p.stdout)
        print(r)
        assert p.returncode == 0 and r["unfaithful"] == 0 and r["not_monotone"] == 0 and r["not_symmetric"] == 0 and r["out_of_bounds"] == 0, r
        assert r["count"] == 2 * ((hi - lo) // stride + 1) and r["max_ulp"] < 1
        return r
    return run


# stride 1 over the binades around each seam (bits, inclusive): the polynomial-to-x boundary 2^-12 .. 2^-10 (lsin leaves x at
# 4.4e-4, lcos leaves 1 at 2^-12), pi/4 and pi/2 in [0.5, 2), the method threshold in [2^19, 2^21), the top binade
SEAMS = [(0x39800000, 0x3a7fffff), (0x3f000000, 0x3fffffff), (0x49000000, 0x49ffffff), (0x7f000000, 0x7f7fffff)]


@pytest.mark.parametrize("fn", ["sin", "cos"])
def test_reduced_sweep_faithful_symmetric_bounded_monotone(sweep, fn):
    """the full sweep (0 0x7f7fffff 1, both functions) is run by hand: profiles/sincos/README.md records it.  Here, both signs
    throughout: stride 1 over the binades around each seam, a prime stride over everything else."""
    for lo, hi in SEAMS:
        sweep(fn, lo, hi, 1)
    edge = 0
    for lo, hi in SEAMS + [(0x7f800000, 0)]:
        if lo > edge:
            r = sweep(fn, edge, lo - 1, 1009)
            if edge == 0:                               # every tiny input, subnormals included, returns x or 1
                assert r["trivial_to"] != "none 0x00000000" and r["max_ulp"] <= 0.5
        edge = hi + 1
    r = sweep(fn, 0x39000000, 0x39ffffff, 1)            # the boundary itself, from a start where the result still is x or 1
    assert int(r["trivial_to"], 16) == (RETURNS_X if fn == "sin" else COS_ONE)


def test_sweep_fails_on_a_wrong_build(tmp_path):
    """the sweep can fail: with P3 zeroed the reduced argument is off by k * 5.4e-15; in [2^19, 2^20) k is 3.3e5 to 6.7e5, the
    argument is off by 1.8e-9 to 3.6e-9, and wherever the result is below about 0.03 in magnitude that is more than its
    float32 ulp: some 2 % of the binade"""
    exe = tmp_path / "sweep_broken"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-DLH_SC_P3_BITS=0x0000000000000000ull", "-I", CSRC, HOST,
                    "-o", str(exe)], check=True)
    for fn in ("sin", "cos"):
        p = subprocess.run([str(exe), "sweep", fn, "0x48800000", "0x497fffff", "1"], capture_output=True, text=True)   # [2^18, 2^20)
        r = json.loads(p.stdout)
        assert p.returncode == 1 and r["unfaithful"] > 10000 and r["max_ulp"] > 1, r
    # and the model with the same wrong constant differs from the right one there
    x = np.arange(0x49000000, 0x49000000 + 100000, dtype=np.uint32).view(np.float32)
    assert (u32(S.lsin(x, p3=0.0)) != u32(S.lsin(x))).sum() > 1000


# ---- (e) the ABI -------------------------------------------------------------------------------------------------------------------
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
    for name in NEW[:3]:
        assert name in hpp
    for proc in ("sin", "cos", "sincos"):
        assert re.search(r"proc %s\*" % proc, nim), proc
        assert callable(getattr(laser_amd, proc)) and re.search(r"inline [\w<>:, ]+ %s\(" % proc, hpp), proc
    text = open(HDR).read()
    assert "Sine and cosine" in text and "0x7fc00000" in text and "laser_sin(x) and laser_cos(x)" in text
    assert "they need a bit-defined sincos" not in text + open(os.path.join(CSRC, "philox_core.h")).read()


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    i64 = C.c_int64
    p, q, t = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384)    # never dereferenced: arguments are checked first
    one, four, zero = (i64 * 1)(1), (i64 * 1)(4), (i64 * 1)(0)
    ones = (i64 * 7)(*[1] * 7)
    both = L.laser_hip_sincos_f32_dev
    for fn in (L.laser_hip_sin_f32_dev, L.laser_hip_cos_f32_dev):
        assert fn(q, ones, p, ones, ones, 7, None) == _lib.E_INVALID                        # rank 7
        assert fn(q, one, p, one, four, -1, None) == _lib.E_INVALID
        assert fn(q, zero, p, one, four, 1, None) == _lib.E_INVALID                         # stride 0 on the destination
        assert fn(q, one, p, one, (i64 * 1)(-4), 1, None) == _lib.E_INVALID                 # a negative extent
        assert fn(q, None, p, one, four, 1, None) == _lib.E_INVALID                         # null strides
        assert fn(q, one, p, None, four, 1, None) == _lib.E_INVALID
        assert fn(q, one, p, one, None, 1, None) == _lib.E_INVALID
    assert both(q, ones, t, ones, p, ones, ones, 7, None) == _lib.E_INVALID
    assert both(q, one, t, zero, p, one, four, 1, None) == _lib.E_INVALID                   # stride 0 on the second destination
    assert both(q, zero, t, one, p, one, four, 1, None) == _lib.E_INVALID
    assert both(q, one, t, None, p, one, four, 1, None) == _lib.E_INVALID
    assert both(q, one, t, one, p, one, (i64 * 1)(-1), 1, None) == _lib.E_INVALID
    for fn in (L.laser_hip_sin_f32, L.laser_hip_cos_f32):
        assert fn(None, None, -1) == _lib.E_INVALID
        assert fn(None, None, 3) == _lib.E_INVALID
        assert fn(q, None, 3) == _lib.E_INVALID


def test_entry_points_need_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one the host-pointer forms give the model's bits"""
    from laser_amd import _lib
    import laser_amd
    x = S.edges()
    y = np.empty_like(x)
    for name, fn in (("sin", S.lsin), ("cos", S.lcos)):
        rc = getattr(L, f"laser_hip_{name}_f32")(y.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), x.size)
        if have_gpu():
            assert rc == 0 and S.same_bits(y, fn(x))
        else:
            assert rc == _lib.E_NODEVICE
    if have_gpu():
        return
    p, q, t = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(16384)
    one, four = (C.c_int64 * 1)(1), (C.c_int64 * 1)(4)
    assert L.laser_hip_sin_f32_dev(q, one, p, one, four, 1, None) == _lib.E_NODEVICE
    assert L.laser_hip_cos_f32_dev(q, one, p, one, four, 1, None) == _lib.E_NODEVICE
    assert L.laser_hip_sincos_f32_dev(q, one, t, one, p, one, four, 1, None) == _lib.E_NODEVICE
    for call in (lambda: laser_amd.sin(np.ones(4, np.float32)), lambda: laser_amd.cos(np.ones(4, np.float32))):
        with pytest.raises(laser_amd.LaserHipError) as e:
            call()
        assert e.value.code == _lib.E_NODEVICE


# ---- (f) forEach bodies and the gfx950 code ---------------------------------------------------------------------------------------
def _source(L, fn, args):
    n = C.c_int64()
    assert fn(*args, None, 0, C.byref(n)) == 0
    buf = C.create_string_buffer(n.value)
    assert fn(*args, buf, n.value, C.byref(n)) == 0
    return buf.value.decode()


def test_generated_sources_carry_the_definition_only_when_a_body_names_it(L):
    from laser_amd import _lib
    core = open(os.path.join(CSRC, "sincos_core.h")).read()
    act_core = open(os.path.join(CSRC, "act_core.h")).read()
    src = _source(L, L.laser_hip_foreach_source, spec("o = x + y - laser_sin(z)", [("o", F32, 1), ("x", F32, 0), ("y", F32, 0), ("z", F32, 0)]))
    red = _source(L, L.laser_hip_foreach_reduce_source, spec("acc += laser_cos(x)", [("x", F32, 0)]) + [b"acc", F32, b"acc += other"])
    for s in (src, red):
        assert core in s and s.index(act_core) < s.index(core) < s.index("void lh_body(")
        assert s.index("float laser_sin(") < s.index("void lh_body(") and s.index("float laser_cos(") < s.index("void lh_body(")
    plain = _source(L, L.laser_hip_foreach_source, spec("y = x + 1", [("y", F32, 1), ("x", F32, 0)]))
    assert "laser_sin" not in plain and act_core in plain                   # other bodies do not pay for compiling it
    n = C.c_int64()
    for name in ("laser_sin", "laser_cos"):                                 # reserved like laser_log
        for ops, params in (([(name, F32, 1)], []), ([("y", F32, 1)], [(name, F32)])):
            assert L.laser_hip_foreach_source(*spec("y = 1", ops, params), None, 0, C.byref(n)) == _lib.E_INVALID
        assert L.laser_hip_foreach_reduce_source(*spec(name + " += x", [("x", F32, 0)]), name.encode(), F32, (name + " += other").encode(),
                                                 None, 0, C.byref(n)) == _lib.E_INVALID


FMA = r"v_(pk_)?fma|v_fmac|v_fmamk|v_fmaak|v_mad_f32|v_mac_f32|v_mad_f64"


I32 = 4


@pytest.mark.parametrize("body, src", [("y = lh_sc_sin_kernel(x)", F64), ("y = lh_sc_cos_kernel(x)", F64),
                                       ("double r; int q = lh_sc_reduce((unsigned int)x & 0x7fffffffu, &r); y = r + (double)q", I32)])
def test_float64_body_of_the_core_compiles_without_fused_multiply_adds(L, tmp_path, body, src):
    """the two kernels and the reduction (both methods, from the bits of a float32), through a forEach body on gfx950"""
    rc, blob = code(L, body, [("y", F64, 1), ("x", src, 0)])
    assert rc == 0, blob
    k = disasm(blob, tmp_path, "lh_foreach_vector")
    assert re.search(r"v_mul_f64", k) and re.search(r"v_add_f64", k)
    assert not re.search(FMA, k)
    assert not re.search(r"v_sin_f32|v_cos_f32|v_rcp_f64|v_div_|v_rndne|v_trig_preop|v_fract", k)   # no device trigonometry, no division


@pytest.mark.parametrize("body, ops", [("o = x + y - laser_sin(z)", [("o", F32, 1), ("x", F32, 0), ("y", F32, 0), ("z", F32, 0)]),
                                       ("o = laser_sin(s) + laser_cos(s)", [("o", F32, 1), ("s", F32, 0)])])
def test_the_reference_bodies_compile(L, tmp_path, body, ops):
    """iter_bench.nim's `o = x + y - sin z` and the examples' `sin(s) + cos(s)`, with the library's names"""
    rc, blob = code(L, body, ops)
    assert rc == 0, blob
    k = disasm(blob, tmp_path, "lh_foreach_vector")
    assert re.search(r"v_cvt_f32_f64", k) and re.search(r"v_mul_f64", k)
    assert not re.search(r"v_sin_f32|v_cos_f32|v_fma_f64|v_(pk_)?fma_f32|v_fmac_f32|v_mad_f32|v_mac_f32", k)   # one float32 add and sub, unfused


def test_precompiled_kernels_vectorise_and_hold_no_fused_multiply_adds(tmp_path):
    """the gfx950 code object with the sincos kernels, cut out of the library's offload bundles: the vector kernels move 16 bytes
    per lane and hold float64 multiplies and adds, nothing fused, no device trigonometry"""
    seen = 0
    for name, k in code_objects.kernels(b"SinCosOp", r"\w*pointwise_vec_kernelINS\w*SinCosOpILi[012]E\w*", tmp_path):
        seen += 1
        assert re.search(r"global_load_dwordx4", k) and re.search(r"global_store_dwordx4", k), name
        assert re.search(r"v_mul_f64", k) and re.search(r"v_add_f64", k) and re.search(r"v_cvt_f32_f64", k), name
        assert not re.search(FMA, k) and not re.search(r"v_sin_f32|v_cos_f32|v_div_|v_rcp_", k), name
        if re.search(r"SinCosOpILi([012])E", name).group(1) == "2":
            assert len(re.findall(r"global_store_dwordx4", k)) == 2, name
    assert seen == 3


# ---- (g) the C++ mirror --------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "sincos_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)
