"""CPU-side checks of attention and the softmax gradient (include/laser_hip.h "Attention", "Softmax gradient"): the entry
points are declared, exported and mirrored; laser_hip_attention_plan and laser_hip_softmax_grad_plan follow the stated rules
and are the plan headers compiled alone, which also run as a host program under ASan and UBSan; every invalid argument is
refused before a device is looked for; a valid call needs a gfx950 device; the C++ mirror compiles; the Python layer checks
its operands; and the numpy model (tests/attention_model.py) has the properties the definition promises and is as close to
float64 as a float32 attention can be expected to be."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import attention_model as M
from tests import exp_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_attention_f32_dev", "laser_hip_softmax_grad_rows_f32_dev", "laser_hip_attention_plan", "laser_hip_attention_last_kernel",
       "laser_hip_softmax_grad_plan", "laser_hip_softmax_grad_last_kernel"]
MAX_D, MAX_KEYS, BM = 128, 65536, 32
MAX_N = 1 << 26


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


def plan(L, bh, tq, tk, d, dv, causal=0, vec=1):
    out = (C.c_int64 * 5)(-1, -1, -1, -1, -1)
    rc = L.laser_hip_attention_plan(bh, tq, tk, d, dv, causal, vec, out)
    return rc, list(out)


def grad_plan(L, rows, n, vec=1):
    out = (C.c_int64 * 3)(-1, -1, -1)
    return L.laser_hip_softmax_grad_plan(rows, n, vec, out), list(out)


def lds_bytes(d):
    ld = (d + (d & 1)) | 1
    return 4096 + 4 * ((32 + 128) * ld + 32 * 129 + 4 * 32 + 32 * 32 + 32 * 8 + 2 * 32)


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
    assert "laser_hip_attention_f32_dev" in hpp and "laser_hip_softmax_grad_rows_f32_dev" in hpp
    for fn in ("attention", "attention_backward", "softmax_backward"):
        assert callable(getattr(laser_amd, fn)) and re.search(r"inline [\w<>]+ %s\(" % fn, hpp), fn
    for proc in ("attention", "attentionBackward", "softmaxBackward"):
        assert re.search(r"proc %s\*" % proc, nim), proc
    text = open(HDR).read()
    assert "Attention (f32)" in text and "Softmax gradient (f32)" in text
    assert re.search(r"#define LASER_HIP_ATTENTION_MAX_D %d\b" % MAX_D, text) and 128 <= MAX_D <= 512
    assert re.search(r"#define LASER_HIP_ATTENTION_MAX_KEYS %d\b" % MAX_KEYS, text) and MAX_KEYS >= 16384
    plan_h = open(os.path.join(CSRC, "attention_plan.h")).read()
    assert re.search(r"#define LH_ATTENTION_MAX_D %d\b" % MAX_D, plan_h) and re.search(r"#define LH_ATTENTION_MAX_KEYS %d\b" % MAX_KEYS, plan_h)
    assert "#include" not in plan_h                                   # no HIP dependency, no dependency at all
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3
    assert L.laser_hip_attention_last_kernel() in (-1, 0, 1)
    assert L.laser_hip_softmax_grad_last_kernel() in (-1, 0, 1, 2, 4, 5, 6)


def test_plan_follows_the_stated_rules(L):
    from laser_amd import _lib
    for bh, tq in ((1, 1), (6, 45), (64, 1024), (1, 32), (1, 33), (1100, 1), (3, 0), (0, 77), (1 << 20, 4096)):
        for tk, d, dv in ((1, 1, 1), (70, 5, 128), (65536, 128, 3), (8193, 64, 64)):
            for vec in (0, 1):
                units = bh * -(-tq // BM)
                assert plan(L, bh, tq, tk, d, dv, 0, vec) == (0, [BM, 0 if vec else 1, min(1024, units), lds_bytes(d), units]), (bh, tq, tk, d)
    assert lds_bytes(MAX_D) <= 160 * 1024                              # one workgroup fits a compute unit's LDS at the widest d
    # causal changes nothing in the plan but needs Tq <= Tk
    assert plan(L, 2, 70, 70, 16, 16, 1) == plan(L, 2, 70, 70, 16, 16, 0) and plan(L, 2, 1, 70, 16, 16, 1)[0] == 0
    # -1 past every limit, with nothing written
    bad = [(-1, 4, 4, 4, 4, 0), (1, -1, 4, 4, 4, 0), (1, 4, 0, 4, 4, 0), (1, 4, MAX_KEYS + 1, 4, 4, 0), (1, 4, 4, 0, 4, 0),
           (1, 4, 4, MAX_D + 1, 4, 0), (1, 4, 4, 4, 0, 0), (1, 4, 4, 4, MAX_D + 1, 0), (1, 5, 4, 4, 4, 1), (1 << 40, 33, 4, 4, 4, 0),
           ((1 << 63) - 1, (1 << 63) - 1, 4, 4, 4, 0)]
    for args in bad:
        rc, p = plan(L, *args)
        assert rc == _lib.E_INVALID and p == [-1] * 5, args
    assert plan(L, 1 << 40, 32, 4, 4, 4)[1][4] == 1 << 40
    assert L.laser_hip_attention_plan(1, 4, 4, 4, 4, 0, 1, None) == _lib.E_INVALID
    # the softmax gradient: the softmax rows' mapping, codes and grid; no table in LDS
    for n, code in ((1, 0), (1024, 0), (1025, 1), (8192, 1), (8193, 2), (MAX_N, 2)):
        for rows in (0, 1, 5, 8191, 8192, 8193, 100000):
            want = min(2048, -(-rows // 4) if code == 0 else rows)
            lds = (1040 if code >= 1 else 0) + (32768 if code == 2 else 0)
            assert grad_plan(L, rows, n, 1) == (0, [code, want, lds]) and grad_plan(L, rows, n, 0) == (0, [code + 4, want, lds]), (n, rows)
            rows_out = (C.c_int64 * 3)()
            assert L.laser_hip_softmax_rows_plan(rows, n, 1, rows_out) == 0 and list(rows_out) == [code, want, lds + 4096]
    for args in ((-1, 4), (4, 0), (4, MAX_N + 1)):
        rc, p = grad_plan(L, *args)
        assert rc == _lib.E_INVALID and p == [-1, -1, -1], args
    assert L.laser_hip_softmax_grad_plan(4, 4, 1, None) == _lib.E_INVALID


def test_plan_headers_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """attention_plan.h and softmax_rows_plan.h have no HIP dependency: g++ alone builds them, with ASan and UBSan (signed
    overflow in the unit count would trap), and the program's answers are the library's"""
    exe = tmp_path / "attention_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "attention_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = [(0, 17, 5, 4, 4, 0, 1), (1, 1, 1, 1, 1, 1, 0), (6, 45, 45, 16, 16, 1, 1), (64, 1024, 1024, 64, 64, 0, 1), (8, 8192, 8192, 64, 64, 1, 1),
             (1100, 1, 3, 2, 2, 0, 0), (1, 8225, 8225, 4, 4, 1, 1), (2, 3, 65536, 128, 128, 0, 1), (2, 3, 65537, 128, 128, 0, 1),
             (2, 3, 16, 129, 128, 0, 1), (2, 3, 16, 128, 129, 0, 1), (2, 17, 16, 8, 8, 1, 1), (1 << 40, 32, 4, 4, 4, 0, 1), (1 << 40, 33, 4, 4, 4, 0, 1),
             ((1 << 63) - 1, (1 << 63) - 1, 4, 4, 4, 0, 0), (-3, 4, 4, 4, 4, 0, 1), (3, -4, 4, 4, 4, 0, 1)]
    text = "".join("%d %d %d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([str(exe), "-"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0), c
        assert got[1:] == p, (c, got, p)


def attn_args(**kw):
    """a valid call on (B, H, Tq, Tk, d, dv) = (2, 3, 5, 7, 4, 6) (pointers never dereferenced: arguments are judged first)"""
    st = lambda *s: (C.c_int64 * 3)(*s)
    a = dict(o=C.c_void_p(4096), os=st(90, 30, 6), q=C.c_void_p(8192), qs=st(60, 20, 4), k=C.c_void_p(12288), ks=st(84, 28, 4),
             v=C.c_void_p(16384), vs=st(126, 42, 6), p=C.c_void_p(20480), ps=st(105, 35, 7), m=C.c_void_p(24576), s=C.c_void_p(28672),
             b=2, h=3, tq=5, tk=7, d=4, dv=6, scale=0.5, causal=0)
    a.update(kw)
    return tuple(a[k] for k in ("o", "os", "q", "qs", "k", "ks", "v", "vs", "p", "ps", "m", "s", "b", "h", "tq", "tk", "d", "dv", "scale",
                                "causal")) + (None,)


def grad_args(**kw):
    a = dict(dx=C.c_void_p(4096), dxs=8, dy=C.c_void_p(8192), dys=8, y=C.c_void_p(12288), ys=8, rows=4, n=8)
    a.update(kw)
    return tuple(a[k] for k in ("dx", "dxs", "dy", "dys", "y", "ys", "rows", "n")) + (None,)


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    st = lambda *s: (C.c_int64 * 3)(*s)
    fwd, grad = L.laser_hip_attention_f32_dev, L.laser_hip_softmax_grad_rows_f32_dev
    limits = [(dict(d=MAX_D + 1), b"MAX_D"), (dict(dv=MAX_D + 1), b"MAX_D"), (dict(d=0), b"MAX_D"), (dict(dv=0), b"MAX_D"),
              (dict(tk=MAX_KEYS + 1), b"MAX_KEYS"), (dict(tk=0), b"MAX_KEYS"), (dict(tq=-1), b"Tq"), (dict(b=-1), b"batch"), (dict(h=-1), b"heads"),
              (dict(tq=8, causal=1), b"causal"), (dict(b=1 << 40, h=2), b"2^40"), (dict(b=1 << 40, tq=33), b"2^40")]
    for kw, word in limits:
        assert fwd(*attn_args(**kw)) == _lib.E_INVALID, kw
        assert word in L.laser_hip_last_error(), (kw, L.laser_hip_last_error())                 # the text says which limit
    q = C.c_void_p(8192)
    bad = [dict(o=None, p=None, m=None, s=None), dict(q=None), dict(k=None), dict(v=None), dict(qs=None), dict(os=None), dict(ps=None),
           dict(qs=st(60, 20, 3)), dict(ks=st(84, 28, 3)), dict(vs=st(126, 42, 5)), dict(os=st(90, 30, 5)), dict(ps=st(105, 35, 6)),
           dict(qs=st(-60, 20, 4)), dict(os=st(90, -30, 6)), dict(o=q), dict(p=q), dict(m=C.c_void_p(16384)), dict(s=C.c_void_p(4096))]
    for kw in bad:
        assert fwd(*attn_args(**kw)) == _lib.E_INVALID, kw
    # the sizes are judged before any pointer, with every pointer NULL too
    none = dict(o=None, q=None, k=None, v=None, p=None, m=None, s=None)
    assert fwd(*attn_args(d=MAX_D + 1, **none)) == _lib.E_INVALID and b"MAX_D" in L.laser_hip_last_error()
    dy = C.c_void_p(8192)
    bad_grad = [dict(rows=-1), dict(n=0), dict(n=-8), dict(n=MAX_N + 1, dxs=MAX_N + 1, dys=MAX_N + 1, ys=MAX_N + 1), dict(dx=None), dict(dy=None),
                dict(y=None), dict(dxs=7), dict(dys=7), dict(ys=7), dict(dx=dy, dxs=9), dict(dx=C.c_void_p(12288), dxs=9)]
    for kw in bad_grad:
        assert grad(*grad_args(**kw)) == _lib.E_INVALID, kw
    assert grad(*grad_args(n=0, dx=None, dy=None, y=None)) == _lib.E_INVALID


def test_a_valid_call_needs_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one, the calls that touch nothing succeed"""
    from laser_amd import _lib
    fwd, grad = L.laser_hip_attention_f32_dev, L.laser_hip_softmax_grad_rows_f32_dev
    none = dict(o=None, q=None, k=None, v=None, p=None, m=None, s=None)
    if have_gpu():
        assert fwd(*attn_args(b=0, o=C.c_void_p(4096), **{k: v for k, v in none.items() if k != "o"})) == 0        # B * H = 0: nothing happens
        assert grad(*grad_args(rows=0, dx=None, dy=None, y=None)) == 0
        return
    assert fwd(*attn_args()) == _lib.E_NODEVICE
    assert fwd(*attn_args(causal=1)) == _lib.E_NODEVICE
    assert fwd(*attn_args(o=None, m=None, s=None)) == _lib.E_NODEVICE                  # probs alone
    assert fwd(*attn_args(o=None, p=None)) == _lib.E_NODEVICE                          # the statistics alone
    assert fwd(*attn_args(tq=0)) == _lib.E_NODEVICE and fwd(*attn_args(h=0)) == _lib.E_NODEVICE
    assert fwd(*attn_args(scale=float("nan"))) == _lib.E_NODEVICE                      # IEEE, not refused
    assert fwd(*attn_args(d=MAX_D, qs=(C.c_int64 * 3)(0, 0, MAX_D), ks=(C.c_int64 * 3)(0, 0, MAX_D))) == _lib.E_NODEVICE    # stride 0: shared
    assert grad(*grad_args()) == _lib.E_NODEVICE
    assert grad(*grad_args(dx=C.c_void_p(8192))) == _lib.E_NODEVICE                    # in place over dy
    assert grad(*grad_args(dx=C.c_void_p(12288))) == _lib.E_NODEVICE                   # in place over y
    assert grad(*grad_args(rows=0, dx=None, dy=None, y=None)) == _lib.E_NODEVICE
    assert plan(L, 2, 5, 7, 4, 6)[0] == 0 and grad_plan(L, 4, 8)[0] == 0               # the plans need no device
    import laser_amd
    with pytest.raises(TypeError):
        laser_amd.attention(*(np.ones((2, 5, 4), np.float32),) * 3)                    # a host array is not taken (and nothing falls back)


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "attention_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)


def test_python_layer_checks_its_operands():
    import inspect
    import laser_amd
    from laser_amd import nn
    assert list(inspect.signature(laser_amd.attention).parameters) == ["q", "k", "v", "scale", "causal", "out", "probs", "stats"]
    assert list(inspect.signature(laser_amd.attention_backward).parameters) == ["dout", "q", "k", "v", "scale", "causal", "need"]
    assert inspect.signature(laser_amd.attention_backward).parameters["need"].default == ("q", "k", "v")
    assert list(inspect.signature(laser_amd.softmax_backward).parameters) == ["dy", "y", "out"]
    assert nn._attn_scale("f", None, 64) == 0.125 and np.float32(nn._attn_scale("f", None, 3)) == np.float32(1 / np.sqrt(np.float64(3)))

    class V:      # a device operand as the layer sees it, never dereferenced
        def __init__(self, shape, strides, typestr="<f4"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "version": 3, "data": (4096, False),
                                             "strides": tuple(int(typestr[2]) * s for s in strides)}
    assert nn._attn_view("f", "q", V((6, 5, 4), (20, 4, 1)))[1:] == (6, 1, 5, 4, (20, 0, 4))
    assert nn._attn_view("f", "q", V((2, 3, 5, 4), (60, 20, 4, 1)))[1:] == (2, 3, 5, 4, (60, 20, 4))
    assert nn._attn_view("f", "q", V((2, 3, 5, 4), (180, 4, 36, 1)))[1:] == (2, 3, 5, 4, (180, 4, 36))      # a (B, T, 3, H, d) slice
    q, k, v = V((6, 5, 4), (20, 4, 1)), V((6, 7, 4), (28, 4, 1)), V((6, 7, 3), (21, 3, 1))
    for bad in (V((5, 4), (4, 1)), V((6, 5, 4), (20, 1, 5)), V((6, 5, 4), (20, 3, 1)), V((6, 5, 4), (-20, 4, 1))):
        with pytest.raises(ValueError):
            laser_amd.attention(bad, k, v)
    with pytest.raises(TypeError):
        laser_amd.attention(V((6, 5, 4), (20, 4, 1), "<f8"), k, v)
    for args, kw in (((q, V((6, 7, 5), (35, 5, 1)), v), {}),                                               # k's d unlike q's
                     ((q, V((5, 7, 4), (28, 4, 1)), v), {}),                                               # leading shapes
                     ((q, k, V((6, 8, 3), (24, 3, 1))), {}),                                               # v's positions unlike k's
                     ((q, k, V((1, 6, 7, 3), (126, 21, 3, 1))), {}),                                       # ranks
                     ((V((6, 9, 4), (36, 4, 1)), k, v), dict(causal=True)),                                # Tq > Tk
                     ((q, k, v), dict(out=False)),                                                         # nothing asked for
                     ((q, k, v), dict(out=V((6, 5, 4), (20, 4, 1)))),                                      # out's width is dv
                     ((q, k, v), dict(probs=V((6, 5, 8), (40, 8, 1)))),
                     ((V((6, 5, 129), (645, 129, 1)), V((6, 7, 129), (903, 129, 1)), v), {}),              # past MAX_D
                     ((q, V((6, 0, 4), (0, 4, 1)), V((6, 0, 3), (0, 3, 1))), {})):                         # no keys
        with pytest.raises(ValueError):
            laser_amd.attention(*args, **kw)
    do = V((6, 5, 3), (15, 3, 1))
    for args, kw in (((V((6, 5, 4), (20, 4, 1)), q, k, v), {}), ((do, q, k, v), dict(need=())), ((do, q, k, v), dict(need=("q", "x")))):
        with pytest.raises(ValueError):
            laser_amd.attention_backward(*args, **kw)
    y = V((5, 7), (7, 1))
    for a, b2, kw in ((V((7,), (1,)), V((7,), (1,)), {}), (y, V((5, 8), (8, 1)), {}), (V((5, 7), (1, 5)), y, {}),
                      (y, y, dict(out=V((5, 7), (1, 5)))), (V((5, 0), (0, 1)), V((5, 0), (0, 1)), {}),
                      (V((2, 3, 7), (42, 7, 1)), V((2, 3, 7), (42, 7, 1)), {})):                            # leading dims do not collapse
        with pytest.raises(ValueError):
            laser_amd.softmax_backward(a, b2, **kw)
    with pytest.raises(TypeError):
        laser_amd.softmax_backward(V((5, 7), (7, 1), "<f8"), y)


# ---- the model has the properties the definition promises ----------------------------------------------------------------------
def seeded(tq, tk, d, dv, seed=0):
    """scores within [-30, 30], where the header states lexp's error: |q . k| * scale stays far below"""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (tq, d)).astype(np.float32), rng.normal(0, 1, (tk, d)).astype(np.float32),
            rng.normal(0, 1, (tk, dv)).astype(np.float32))


@pytest.mark.parametrize("tq,tk,d,dv", [(9, 70, 5, 7), (5, 1025, 65, 33), (3, 8200, 16, 4)])
def test_model_is_the_composition_of_the_oracle_gemm_and_the_model_softmax(tq, tk, d, dv):
    """(a) non-causal P and O equal, bit for bit (+0 and -0 taken as equal), softmax_rows(scale * oracle.matmul(Q, K^T)) and
    oracle.matmul(P, V)"""
    from oracle import oracle
    q, k, v = seeded(tq, tk, d, dv)
    o, p, m, s = M.forward(q, k, v)
    sc = (M.default_scale(d) * oracle.matmul(q, np.ascontiguousarray(k.T))).astype(np.float32)
    assert np.abs(sc).max() < 30
    assert M.same_bits(p, exp_model.softmax_rows(sc), zeros_equal=True)
    assert M.same_bits(o, oracle.matmul(p, v), zeros_equal=True)
    assert (s >= 1).all() and np.array_equal(m, sc.max(axis=1))


def test_causal_rows_are_the_non_causal_model_on_the_visible_keys():
    """(b) row i of the causal P is the non-causal model on K[:n_i], then +0; a masked NaN key never reaches the row"""
    tq, tk = 9, 40
    q, k, v = seeded(tq, tk, 6, 5, 1)
    k[35, 2] = np.nan
    o, p, m, s = M.forward(q, k, v, causal=True)
    for i in range(tq):
        n = i + (tk - tq) + 1
        o1, p1, m1, s1 = M.forward(q[i:i + 1], k[:n], v[:n])
        assert M.same_bits(p[i, :n], p1[0]) and (p[i, n:].view(np.uint32) == 0).all()
        assert M.same_bits(m[i:i + 1], m1) and M.same_bits(s[i:i + 1], s1)
        assert np.isnan(p[i]).any() == (n > 35)
    assert M.visible(0, 1, 100, True) == 100 and M.visible(4, 5, 5, True) == 5 and M.visible(4, 5, 5, False) == 5


# (c) measured here for the seeded inputs (numpy 64-bit host): the model's maximum absolute error against float64 attention, and
# torch float32's (softmax(q k^T * scale) v on the CPU) beside it for comparison.  The bound asserted is the measured figure
# with a margin of 2x, which only absorbs libm differences between hosts (the float64 reference calls the host's exp).
MEASURED = {(64, 600, 64, 64, False): 1.70e-7, (40, 1025, 16, 8, True): 1.01e-7, (33, 8200, 128, 5, False): 2.99e-8}


@pytest.mark.parametrize("tq,tk,d,dv,causal", sorted(MEASURED))
def test_model_is_close_to_float64(tq, tk, d, dv, causal):
    """(c) model 2.99e-8 / 1.01e-7 / 1.70e-7 for the three shapes in the order run; torch float32 gives 2.93e-8 / 5.55e-8 /
    1.75e-7 on the same inputs"""
    import torch
    q, k, v = seeded(tq, tk, d, dv, 2)
    scale = M.default_scale(d)
    o = M.forward(q, k, v, scale, causal)[0]
    want = M.reference64(q, k, v, scale, causal)[0]
    err = np.abs(o - want).max()
    s = torch.from_numpy(q) @ torch.from_numpy(k).T * float(scale)
    if causal:
        s = s.masked_fill(~torch.from_numpy(np.arange(tk)[None, :] < np.arange(tq)[:, None] + (tk - tq) + 1), float("-inf"))
    t32 = np.abs((torch.softmax(s, -1) @ torch.from_numpy(v)).numpy() - want).max()
    print(f"({tq}, {tk}, {d}, {dv}, causal={causal}): model {err:.3e}, torch float32 {t32:.3e}")
    assert err <= 2 * MEASURED[tq, tk, d, dv, causal], (err, t32)


GRAD_MEASURED = {1025: 4.20e-9, 8200: 1.23e-9}


@pytest.mark.parametrize("n", sorted(GRAD_MEASURED))
def test_softmax_gradient_model_is_close_to_the_float64_jacobian_product(n):
    """(d) dx = y * (dy - sum(dy * y)) in float64 on the same float32 y and dy: model 4.20e-9 (n = 1025) and 1.23e-9
    (n = 8200) maximum absolute error, measured here; asserted with the same margin of 2x"""
    rng = np.random.default_rng(n)
    y = exp_model.softmax_rows(rng.normal(0, 2, (5, n)).astype(np.float32))
    dy = rng.normal(0, 1, (5, n)).astype(np.float32)
    y8, dy8 = y.astype(np.float64), dy.astype(np.float64)
    want = y8 * (dy8 - (dy8 * y8).sum(axis=1, keepdims=True))
    got = M.softmax_grad(dy, y)
    err = np.abs(got - want).max()
    print(f"n = {n}: model {err:.3e}")
    assert got.dtype == np.float32 and err <= 2 * GRAD_MEASURED[n], err
    # -0 products, a zero row and n = 1: D is a sum from +0
    assert M.same_bits(M.softmax_grad_row(np.float32([-0.0, 0.0]), np.float32([1.0, 1.0])), np.float32([-0.0, 0.0]))
    assert M.same_bits(M.softmax_grad_row(np.float32([3.0]), np.float32([1.0])), np.float32([0.0]))
