"""CPU-side checks of the optimizer steps (include/laser_hip.h "Optimizer steps"): the entry points are declared, exported
and mirrored; laser_hip_adam_bias_correction is the model's square-and-multiply bit for bit; laser_hip_optim_plan follows the
stated rules and is the plan header compiled alone, which also runs as a host program under ASan and UBSan; every invalid
argument is refused before a device is looked for; a valid call needs a gfx950 device; optim_core.h compiled for the host
reproduces the numpy model (tests/optim_model.py) bit for bit; the C++ mirror compiles; the Python layer checks its operands."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import optim_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_sgd_step_f32_dev", "laser_hip_adam_step_f32_dev", "laser_hip_grad_norm_f32_dev", "laser_hip_adam_bias_correction",
       "laser_hip_optim_plan"]
MAX_LEN, MAX_COUNT = 1 << 26, 65536
SGD, ADAM, NORM = 0, 1, 2
T, TN = 64, 192             # LH_OPTIM_TENSORS, LH_OPTIM_NORM_TENSORS
F = np.float32


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


def plan(L, what, lens):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    arr = (C.c_int64 * max(1, len(lens)))(*lens)
    rc = L.laser_hip_optim_plan(what, arr, len(lens), out)
    return rc, list(out)


def model_plan(what, lens):
    if what == NORM:
        chunks = [max(1, -(-n // 8192)) for n in lens]
        groups = [sum(chunks[k:k + TN]) for k in range(0, len(lens), TN)]
        total, count = sum(chunks), len(lens)
        scratch = (total * 4 + 15) // 16 * 16 + (count * 4 + 15) // 16 * 16 if count else 0
        return [2 * len(groups) + 1, groups[0] if groups else 1, total, scratch]
    chunks = [-(-n // 4096) for n in lens]
    groups = [g for g in (sum(chunks[k:k + T]) for k in range(0, len(lens), T)) if g]
    return [len(groups), min(2048, groups[0]) if groups else 0, sum(chunks), 0]


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
        if name != "laser_hip_optim_plan":
            assert name in hpp
    for fn in ("sgd_step", "adam_step", "grad_norm", "adam_bias_correction"):
        assert callable(getattr(laser_amd, fn)) and re.search(r"inline [\w<>]+ %s\(" % fn, hpp), fn
    assert isinstance(laser_amd.SGD, type) and isinstance(laser_amd.Adam, type)
    for proc in ("sgdStep", "adamStep", "gradNorm", "adamBiasCorrection"):
        assert re.search(r"proc %s\*" % proc, nim), proc
    text = open(HDR).read()
    assert "Optimizer steps" in text and "Not built: float64 and mixed precision" in text
    assert re.search(r"#define LASER_HIP_OPTIM_MAX_LEN \(1ll << 26\)", text)
    assert re.search(r"#define LASER_HIP_OPTIM_MAX_COUNT 65536\b", text)
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3
    plan_h = open(os.path.join(CSRC, "optim_plan.h")).read()
    assert re.search(r"#define LH_OPTIM_TENSORS %d\b" % T, plan_h) and re.search(r"#define LH_OPTIM_NORM_TENSORS %d\b" % TN, plan_h)
    core = open(os.path.join(CSRC, "optim_core.h")).read()
    assert "#pragma clang fp contract(off)" in core and "#include" not in core          # plain C++ with no includes


# ---- the bias correction ---------------------------------------------------------------------------------------------------------
BETAS = [0.9, 0.999, 0.5, 0.0, 1.0]
STEPS = [1, 2, 3, 7, 1000, 10 ** 6, 2 ** 40]


def test_bias_correction_is_the_model_bit_for_bit(L):
    import laser_amd
    for beta in BETAS:
        for step in STEPS:
            out = C.c_float(-7.0)
            assert L.laser_hip_adam_bias_correction(beta, step, C.byref(out)) == 0
            want = M.bias_correction(beta, step)
            assert F(out.value).view(np.uint32) == want.view(np.uint32), (beta, step, out.value, want)
            assert F(laser_amd.adam_bias_correction(beta, step)).view(np.uint32) == want.view(np.uint32)
    assert M.bias_correction(0.9, 1) == F(1.0 - float(F(0.9)))
    assert M.bias_correction(0.9, 2 ** 40) == 1 and M.bias_correction(0.999, 10 ** 6) == 1      # beta^step underflows: bc = 1
    assert M.bias_correction(0.0, 1) == 1 and M.bias_correction(1.0, 2 ** 40) == 0 and M.bias_correction(0.5, 3) == F(0.875)
    assert 0 < M.bias_correction(0.999, 1000) < 1


def test_bias_correction_refuses_step_zero_and_a_null_result(L):
    from laser_amd import _lib
    import laser_amd
    out = C.c_float(-7.0)
    for step in (0, -1, -2 ** 40):
        assert L.laser_hip_adam_bias_correction(0.9, step, C.byref(out)) == _lib.E_INVALID and out.value == -7.0
    assert L.laser_hip_adam_bias_correction(0.9, 1, None) == _lib.E_INVALID
    with pytest.raises(_lib.LaserHipError):
        laser_amd.adam_bias_correction(0.9, 0)


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_follows_the_stated_rules(L):
    from laser_amd import _lib
    for length in (0, 1, 4095, 4096, 4097, 8191, 8192, 8193, MAX_LEN):
        for count in (0, 1, 64, 65, 129, 192, 193):
            lens = [length] * count
            for what in (SGD, ADAM, NORM):
                assert plan(L, what, lens) == (0, model_plan(what, lens)), (what, length, count)
            # the derivable condition: ceil(count / 64) step launches, at most three for the norm of up to 192 tensors
            steps = plan(L, ADAM, lens)[1][0]
            assert steps == (-(-count // T) if length else 0)
            assert plan(L, NORM, lens)[1][0] == 2 * -(-count // TN) + 1 and (count > TN or plan(L, NORM, lens)[1][0] <= 3)
    mixed = [0, 4095, 4096, 4097, MAX_LEN, 0, 1]
    for what in (SGD, ADAM, NORM):
        assert plan(L, what, mixed) == (0, model_plan(what, mixed))
    assert plan(L, ADAM, mixed)[1] == [1, 2048, 1 + 1 + 2 + 16384 + 1, 0]
    # chunk totals of 2048 and 2049: the grid is capped, the chunk walk takes a second trip
    assert plan(L, SGD, [1024 * 4096, 1024 * 4096])[1] == [1, 2048, 2048, 0]
    assert plan(L, SGD, [1024 * 4096, 1024 * 4096 + 1])[1] == [1, 2048, 2049, 0]
    assert plan(L, SGD, [2047 * 4096])[1] == [1, 2047, 2047, 0]
    # 70 small tensors: two launches, the second of six
    assert plan(L, ADAM, [300] * 70)[1] == [2, 64, 70, 0]
    # a group of empty tensors launches nothing
    assert plan(L, SGD, [0] * 130)[1] == [0, 0, 0, 0] and plan(L, SGD, [0] * 129 + [5])[1] == [1, 1, 1, 0]
    assert plan(L, NORM, [0] * 130)[1] == [3, 130, 130, 528 + 528]
    assert plan(L, NORM, [])[1] == [1, 1, 0, 0] and plan(L, NORM, [2 ** 21 + 3])[1] == [3, 257, 257, 1040 + 16]
    assert plan(L, NORM, [5] * MAX_COUNT)[1][0] == 2 * 342 + 1
    # refused, with nothing written
    for what, lens in ((3, [5]), (-1, [5]), (SGD, [-1]), (ADAM, [5, MAX_LEN + 1]), (NORM, [MAX_LEN + 1]), (NORM, [5, -3]),
                       (SGD, [1] * (MAX_COUNT + 1))):
        assert plan(L, what, lens) == (_lib.E_INVALID, [-1, -1, -1, -1]), (what, lens[:3])
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    assert L.laser_hip_optim_plan(SGD, None, 3, out) == _lib.E_INVALID and L.laser_hip_optim_plan(SGD, None, -1, out) == _lib.E_INVALID
    assert L.laser_hip_optim_plan(SGD, None, 0, out) == 0 and list(out) == [0, 0, 0, 0]
    assert L.laser_hip_optim_plan(SGD, (C.c_int64 * 1)(5), 1, None) == _lib.E_INVALID


def test_plan_header_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """optim_plan.h has no HIP dependency: g++ alone builds it, with ASan and UBSan, and the program's answers are the library's"""
    exe = tmp_path / "optim_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "optim_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = [(SGD, []), (ADAM, [0]), (NORM, []), (NORM, [0]), (SGD, [4095, 4096, 4097]), (ADAM, [MAX_LEN] * 3), (NORM, [MAX_LEN] * 3),
             (ADAM, [300] * 129), (NORM, [9000] * 193), (SGD, [1024 * 4096, 1024 * 4096 + 1]), (ADAM, [-1]), (NORM, [MAX_LEN + 1]),
             (3, [5]), (SGD, [0] * 64 + [7])]
    text = "".join("%d %d %s\n" % (w, len(lens), " ".join(str(n) for n in lens)) for w, lens in cases)
    r = subprocess.run([str(exe), "-"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for (what, lens), got in zip(cases, lines):
        rc, p = plan(L, what, lens)
        assert (got[0] == 0) == (rc == 0), (what, lens[:3])
        assert got[1:] == p, (what, lens[:3], got, p)


# ---- arguments -------------------------------------------------------------------------------------------------------------------------
def ptrs(*addresses):
    return (C.c_void_p * max(1, len(addresses)))(*addresses)


def lens_of(*values):
    return (C.c_int64 * max(1, len(values)))(*values)


def sgd_args(**kw):
    """a valid SGD call on two tensors (pointers never dereferenced: arguments are judged first), with replacements"""
    a = dict(w=ptrs(4096, 8192), g=ptrs(12288, 16384), m=ptrs(20480, 24576), lens=lens_of(8, 5), count=2, lr=0.1, mu=0.9, wd=0.0,
             nesterov=0, gscale=1.0, clip=None)
    a.update(kw)
    return tuple(a[k] for k in ("w", "g", "m", "lens", "count", "lr", "mu", "wd", "nesterov", "gscale", "clip")) + (None,)


def adam_args(**kw):
    a = dict(w=ptrs(4096, 8192), g=ptrs(12288, 16384), m=ptrs(20480, 24576), v=ptrs(28672, 32768), lens=lens_of(8, 5), count=2, lr=1e-3,
             b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=0, bc1=0.1, bc2=0.001, gscale=1.0, clip=None)
    a.update(kw)
    return tuple(a[k] for k in ("w", "g", "m", "v", "lens", "count", "lr", "b1", "b2", "eps", "wd", "decoupled", "bc1", "bc2", "gscale",
                                "clip")) + (None,)


def norm_args(**kw):
    a = dict(norm=C.c_void_p(4096), clip=C.c_void_p(8192), g=ptrs(12288, 16384), lens=lens_of(8, 5), count=2, max_norm=1.0)
    a.update(kw)
    return tuple(a[k] for k in ("norm", "clip", "g", "lens", "count", "max_norm")) + (None,)


def test_bad_arguments_are_invalid_before_a_device_is_looked_for(L):
    from laser_amd import _lib
    sgd, adam, norm = L.laser_hip_sgd_step_f32_dev, L.laser_hip_adam_step_f32_dev, L.laser_hip_grad_norm_f32_dev
    bad_list = [dict(count=-1), dict(count=MAX_COUNT + 1), dict(lens=None), dict(lens=lens_of(8, -1)), dict(lens=lens_of(MAX_LEN + 1, 5)),
                dict(g=None), dict(g=ptrs(12288, None))]
    for kw in bad_list + [dict(w=None), dict(w=ptrs(None, 8192)), dict(m=ptrs(20480, None)),
                          dict(m=None), dict(m=None, mu=0.0, nesterov=1), dict(m=None, mu=float("nan"))]:
        assert sgd(*sgd_args(**kw)) == _lib.E_INVALID, kw
    assert b"momentum" in L.laser_hip_last_error()
    for kw in bad_list + [dict(w=None), dict(m=None), dict(v=None), dict(v=ptrs(None, 32768)), dict(m=ptrs(20480, None))]:
        assert adam(*adam_args(**kw)) == _lib.E_INVALID, kw
    for kw in bad_list + [dict(norm=None, clip=None), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(max_norm=-float("inf")),
                          dict(max_norm=-1.0, count=0)]:
        assert norm(*norm_args(**kw)) == _lib.E_INVALID, kw
    assert sgd(*sgd_args(lens=lens_of(8, MAX_LEN + 1))) == _lib.E_INVALID and b"2^26" in L.laser_hip_last_error()


def test_a_valid_call_needs_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one, the calls that touch nothing succeed"""
    from laser_amd import _lib
    sgd, adam, norm = L.laser_hip_sgd_step_f32_dev, L.laser_hip_adam_step_f32_dev, L.laser_hip_grad_norm_f32_dev
    if have_gpu():
        assert sgd(*sgd_args(count=0, w=None, g=None, m=None, lens=None, mu=0.0)) == 0          # an empty list: nothing happens
        assert adam(*adam_args(lens=lens_of(0, 0), w=ptrs(None, None), g=ptrs(None, None), m=ptrs(None, None), v=ptrs(None, None))) == 0
        return
    assert sgd(*sgd_args()) == _lib.E_NODEVICE
    assert sgd(*sgd_args(m=None, mu=0.0)) == _lib.E_NODEVICE                                   # plain SGD
    assert sgd(*sgd_args(lr=float("nan"), wd=float("inf"), gscale=0.0)) == _lib.E_NODEVICE     # hyper-parameters are not judged
    assert sgd(*sgd_args(lens=lens_of(8, 0), w=ptrs(4096, None), g=ptrs(12288, None), m=ptrs(20480, None))) == _lib.E_NODEVICE
    assert sgd(*sgd_args(count=0, w=None, g=None, m=None, lens=None, mu=0.0)) == _lib.E_NODEVICE
    assert adam(*adam_args()) == _lib.E_NODEVICE
    assert adam(*adam_args(eps=0.0, bc1=0.0, decoupled=1, wd=0.01, clip=C.c_void_p(64))) == _lib.E_NODEVICE
    assert norm(*norm_args()) == _lib.E_NODEVICE
    assert norm(*norm_args(norm=None)) == _lib.E_NODEVICE and norm(*norm_args(clip=None)) == _lib.E_NODEVICE
    assert norm(*norm_args(max_norm=float("inf"))) == _lib.E_NODEVICE and norm(*norm_args(max_norm=0.0)) == _lib.E_NODEVICE
    assert norm(*norm_args(count=0, g=None, lens=None)) == _lib.E_NODEVICE
    import laser_amd
    with pytest.raises(TypeError):
        laser_amd.sgd_step([np.ones(4, np.float32)], [np.ones(4, np.float32)], lr=0.1)   # host arrays are not taken


# ---- optim_core.h on the host against the model ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def core_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("optim_core") / "optim_core_host"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "optim_core_host.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def run_core(exe, tmp, kind, flags, p, arrays=(), step=0, words=0):
    n = arrays[0].size if arrays else 0
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4iq", kind, n, flags, 0, step))
        f.write(np.asarray(list(p) + [0.0] * (12 - len(p)), F).tobytes())
        for a in arrays:
            f.write(np.ascontiguousarray(a, F).tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=120)
    out = np.fromfile(dst, F)
    return out.reshape(3, n) if arrays else out[:words]


def draws(n=4096, seed=7):
    """w, g, m, v with the special values of the header spread through them; v >= 0 except a few (sqrt of a negative: NaN)"""
    rng = np.random.default_rng(seed)
    w, g, m = (rng.normal(0, s, n).astype(F) for s in (1.0, 0.1, 0.05))
    v = (rng.normal(0, 0.05, n).astype(F)) ** 2
    specials = F([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, np.inf, -np.inf, np.nan, 3e38, -3e38, 1.0])
    for k, a in enumerate((w, g, m, v)):
        for j, s in enumerate(specials):
            a[(17 * k + 29 * j) % n] = s
            a[(n // 2 + 31 * k + 13 * j) % n] = s
    v[5], g[5], m[5] = 0.0, 0.0, 0.0            # v = g = 0: with eps = 0, 0 / 0
    v[6], g[6], m[6] = 0.0, -0.0, -0.0
    v[7] = F(-1e-3)
    return w, g, m, v


def test_optim_core_on_the_host_is_the_model_bit_for_bit(core_exe, tmp_path):
    w, g, m, v = draws()
    tmp = str(tmp_path)
    sgd_cases = [dict(lr=0.1), dict(lr=0.1, mu=0.9, has_m=True), dict(lr=0.05, mu=0.9, has_m=True, nesterov=True),
                 dict(lr=0.1, wd=0.01), dict(lr=0.1, gscale=1 / 128), dict(lr=0.1, clip=0.37, mu=0.5, has_m=True, wd=1e-4),
                 dict(lr=0.1, mu=0.0, has_m=True)]
    for c in sgd_cases:
        has_m, clip = c.get("has_m", False), c.get("clip")
        flags = int(c.get("nesterov", False)) | has_m << 1 | (clip is not None) << 2
        got = run_core(core_exe, tmp, 0, flags, [c["lr"], c.get("mu", 0), c.get("wd", 0), c.get("gscale", 1), clip or 0], (w, g, m, v))
        want_w, want_m = M.sgd(w, g, m if has_m else None, lr=c["lr"], mu=c.get("mu", 0), wd=c.get("wd", 0), nesterov=c.get("nesterov", False),
                               gscale=c.get("gscale", 1), clip=clip)
        assert M.same_bits(got[0], want_w), c
        assert M.same_bits(got[1], want_m if has_m else m), c                  # without a momentum value m is not touched
    adam_cases = [dict(step=1), dict(step=7, wd=0.01), dict(step=7, wd=0.01, decoupled=True), dict(step=1000, clip=0.37, gscale=1 / 128),
                  dict(step=3, eps=0.0), dict(step=2, eps=0.0, wd=0.1, decoupled=True), dict(step=1, lr=float("nan")),
                  dict(step=1, b1=0.0, b2=0.0), dict(step=5, b1=1.0)]           # b1 = 1: bc1 = 0, m / 0
    for c in adam_cases:
        lr, b1, b2, eps, wd = c.get("lr", 1e-3), c.get("b1", 0.9), c.get("b2", 0.999), c.get("eps", 1e-8), c.get("wd", 0.0)
        clip, dec = c.get("clip"), c.get("decoupled", False)
        bc1, bc2 = M.bias_correction(b1, c["step"]), M.bias_correction(b2, c["step"])
        flags = int(dec) | (clip is not None) << 2
        got = run_core(core_exe, tmp, 1, flags, [lr, b1, b2, eps, wd, bc1, bc2, c.get("gscale", 1), clip or 0], (w, g, m, v))
        want = M.adam(w, g, m, v, c["step"], lr=lr, b1=b1, b2=b2, eps=eps, wd=wd, decoupled=dec, gscale=c.get("gscale", 1), clip=clip)
        for name, a, b in zip("wmv", got, want):
            assert M.same_bits(a, b), (c, name)
    # what the header says about the edges
    w1, m1, v1 = M.adam(w, g, m, v, 3, lr=1e-3, eps=0.0)
    assert np.isnan(w1[5]) and np.isnan(w1[6]) and np.isnan(w1[7])             # 0 / 0, and the square root of a negative
    w2, _ = M.sgd(F([np.inf, 1.0]), F([1.0, 1.0]), lr=0.5, wd=0.0)
    assert w2[0] == np.inf and w2[1] == 0.5                                    # wd == 0: no 0 * Inf


def test_norm_clip_and_bias_correction_of_the_core_are_the_models(core_exe, tmp_path):
    tmp = str(tmp_path)
    for total, max_norm in ((4.0, 1.0), (4.0, 2.0), (4.0, 3.0), (0.0, 0.0), (0.0, 1.0), (4.0, 0.0), (np.nan, 1.0), (np.inf, 1.0),
                            (np.inf, np.inf), (1e-45, 1e-30), (3.0, 1.7320508)):
        norm, clip = run_core(core_exe, tmp, 2, 0, [total, max_norm], words=2)
        with np.errstate(all="ignore"):
            want_n = np.sqrt(F(total))
            want_c = F(max_norm) / want_n if want_n > F(max_norm) else F(1)
        assert M.same_bits(norm, want_n) and M.same_bits(clip, want_c), (total, max_norm, norm, clip)
    assert M.grad_norm([F([3.0]), F([]), F([4.0])], 1.0) == (F(5.0), F(0.2))
    assert M.grad_norm([], 1.0) == (F(0.0), F(1.0)) and M.same_bits(M.grad_norm([F([np.nan])], 1.0)[1], F(1.0))
    for beta in BETAS:
        for step in STEPS:
            got = run_core(core_exe, tmp, 3, 0, [beta], step=step, words=1)[0]
            assert got.view(np.uint32) == M.bias_correction(beta, step).view(np.uint32), (beta, step)


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "optim_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)


def test_python_layer_checks_its_operands():
    import inspect
    import laser_amd
    from laser_amd import optim
    assert list(inspect.signature(laser_amd.sgd_step).parameters) == ["params", "grads", "momentum", "lr", "mu", "wd", "nesterov", "gscale",
                                                                    "clip"]
    assert list(inspect.signature(laser_amd.adam_step).parameters) == ["params", "grads", "m", "v", "step", "lr", "b1", "b2", "eps", "wd",
                                                                     "decoupled", "gscale", "clip"]
    sig = inspect.signature(laser_amd.adam_step).parameters
    assert (sig["b1"].default, sig["b2"].default, sig["eps"].default) == (0.9, 0.999, 1e-8)
    assert list(inspect.signature(laser_amd.grad_norm).parameters) == ["grads", "max_norm"]

    class V:      # a device operand as the layer sees it, never dereferenced
        def __init__(self, shape, strides, typestr="<f4"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "version": 3, "data": (4096, False),
                                             "strides": tuple(int(typestr[2]) * s for s in strides)}
    a, b = V((5, 7), (7, 1)), V((35,), (1,))
    assert optim._flat("f", "x", a) == (4096, 35) and optim._flat("f", "x", V((0, 7), (7, 1))) == (0, 0)
    count, lens, arrs = optim._lists("f", [("params", [a, b]), ("grads", [b, a])])          # equal element counts: shapes may differ
    assert count == 2 and list(lens) == [35, 35] and len(arrs) == 2
    with pytest.raises(ValueError):
        laser_amd.sgd_step([a], [a])                                            # no lr
    with pytest.raises(ValueError):
        laser_amd.sgd_step([a], [a], lr=0.1, mu=0.9)                            # momentum without its list
    with pytest.raises(ValueError):
        laser_amd.sgd_step([a], [a], lr=0.1, nesterov=True)
    with pytest.raises(ValueError):
        laser_amd.sgd_step([a, a], [a], lr=0.1)                                 # lists of unequal length
    with pytest.raises(ValueError):
        laser_amd.sgd_step([a], [V((5, 6), (6, 1))], lr=0.1)                    # unequal element counts
    with pytest.raises(ValueError):
        laser_amd.sgd_step([V((5, 7), (1, 5))], [a], lr=0.1)                    # a transposed view
    with pytest.raises(TypeError):
        laser_amd.sgd_step([V((5, 7), (7, 1), "<f8")], [a], lr=0.1)
    with pytest.raises(ValueError):
        laser_amd.sgd_step([a], [a], lr=0.1, clip=V((2,), (1,)))                # clip is one float
    with pytest.raises(ValueError):
        laser_amd.adam_step([a], [a], [a], [a], 0, lr=1e-3)                     # steps count from 1
    with pytest.raises(ValueError):
        laser_amd.adam_step([a], [a], [a], [a, a], 1, lr=1e-3)
    with pytest.raises(ValueError):
        laser_amd.adam_step([a], [a], [a], [a], 1)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            laser_amd.grad_norm([a], bad)
    with pytest.raises(ValueError):
        laser_amd.sgd_step([V((1 << 27,), (1,))], [V((1 << 27,), (1,))], lr=0.1)
