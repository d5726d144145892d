"""CPU-side checks of layer normalization (include/laser_hip.h "Layer normalization"): the entry points are declared,
exported and mirrored; laser_hip_layer_norm_plan follows the stated rules and is the plan header compiled alone, which also
runs as a host program under ASan and UBSan; every invalid argument is refused before a device is looked for; a valid call
needs a gfx950 device; the C++ mirror compiles; the Python layer checks its operands; and the numpy model
(tests/layer_norm_model.py) is as close to float64 as torch's own float32 result, so it can serve as the contract."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import layer_norm_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
ENTRY = ["laser_hip_layer_norm_f32_dev", "laser_hip_layer_norm_grad_f32_dev", "laser_hip_layer_norm_plan"]
NEW = ENTRY + ["laser_hip_layer_norm_last_kernel"]
MAX = 1 << 26
FWD, DX, PARAMS = 0, 1, 2
CW = 8                      # LH_LAYER_NORM_CW: the strip width of the column kernel


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


def plan(L, rows, n, vec=1, what=FWD):
    out = (C.c_int64 * 4)(-1, -1, -1, -1)
    rc = L.laser_hip_layer_norm_plan(rows, n, vec, what, out)
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
    assert "laser_hip_layer_norm_f32_dev" in hpp and "laser_hip_layer_norm_grad_f32_dev" in hpp
    for fn in ("layer_norm", "layer_norm_backward"):
        assert callable(getattr(laser_amd, fn)) and re.search(r"inline [\w<>]+ %s\(" % fn, hpp), fn
    for proc in ("layerNorm", "layerNormBackward"):
        assert re.search(r"proc %s\*" % proc, nim), proc
    text = open(HDR).read()
    assert "Layer normalization" in text
    assert re.search(r"#define LASER_HIP_LAYER_NORM_MAX_N \(1ll << 26\)", text)
    assert re.search(r"#define LASER_HIP_LAYER_NORM_MAX_ROWS \(1ll << 26\)", text)
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3
    assert re.search(r"#define LH_LAYER_NORM_CW %d\b" % CW, open(os.path.join(CSRC, "layer_norm_plan.h")).read())
    for what in (FWD, DX, PARAMS):
        assert L.laser_hip_layer_norm_last_kernel(what) in (-1, 0, 1, 2, 4, 5, 6)
    assert L.laser_hip_layer_norm_last_kernel(3) == -1 and L.laser_hip_layer_norm_last_kernel(-1) == -1


def test_plan_follows_the_stated_rules(L):
    from laser_amd import _lib
    # the lane mapping depends on n alone; + 4 without 16-byte vectors
    for what in (FWD, DX):
        for n, code in ((1, 0), (1024, 0), (1025, 1), (8192, 1), (8193, 2), (MAX, 2)):
            for rows in (1, 5, 100000):
                assert plan(L, rows, n, 1, what)[1][0] == code, (n, rows)
                assert plan(L, rows, n, 0, what)[1][0] == code + 4, (n, rows)
        # four rows per workgroup in the wave mapping, one otherwise; the cap of 2048; one launch, none for no rows; no scratch
        for rows in (0, 1, 3, 4, 5, 9, 8191, 8192, 8193, 100000, MAX + 1):
            assert plan(L, rows, 1024, 1, what) == (0, [0, min(2048, -(-rows // 4)), 1 if rows else 0, 0]), rows
            assert plan(L, rows, 1025, 1, what) == (0, [1, min(2048, rows), 1 if rows else 0, 0]), rows
            assert plan(L, rows, 8193, 0, what) == (0, [6, min(2048, rows), 1 if rows else 0, 0]), rows
        assert plan(L, 8192, 100, 1, what)[1][1] == 2048 and plan(L, 8191, 100, 1, what)[1][1] == 2048
        assert plan(L, 8188, 100, 1, what)[1][1] == 2047 and plan(L, 2047, 5000, 1, what)[1][1] == 2047
    # the column sums: units of (8192 rows, CW columns); one launch up to 8192 rows, then one fold per sum and two matrices
    for rows in (0, 1, 5, 1024, 8191, 8192, 8193, 16384, 16385, 40961, 1 << 20, MAX):
        for n in (1, 3, 7, 8, 9, 37, 1024, 8193, MAX):
            for vec in (0, 1):
                rc, p = plan(L, rows, n, vec, PARAMS)
                chunks, strips = max(1, -(-rows // 8192)), -(-n // CW)
                assert rc == 0, (rows, n)
                assert p[0] == (0 if vec else 1)
                assert p[1] == min(2048, chunks * strips), (rows, n, p)
                assert p[2] == (1 if rows <= 8192 else 3), (rows, n, p)
                assert p[3] == (0 if rows <= 8192 else 2 * chunks * n * 4), (rows, n, p)
    assert plan(L, 8192, 37, 1, PARAMS)[1][2:] == [1, 0] and plan(L, 8193, 37, 1, PARAMS)[1][2:] == [3, 2 * 2 * 37 * 4]
    # -1 past the limits, with nothing written
    for args in ((-1, 4, 1, FWD), (4, 0, 1, FWD), (4, -1, 1, DX), (4, MAX + 1, 1, FWD), (4, MAX + 1, 1, DX), (4, MAX + 1, 1, PARAMS),
                 (MAX + 1, 4, 1, PARAMS), (-1, 4, 1, PARAMS), (4, 4, 1, 3), (4, 4, 1, -1)):
        rc, p = plan(L, *args)
        assert rc == _lib.E_INVALID and p == [-1, -1, -1, -1], args
    assert plan(L, MAX + 1, 4, 1, DX)[0] == 0                       # only the column sums bound the rows
    assert L.laser_hip_layer_norm_plan(4, 4, 1, 0, None) == _lib.E_INVALID


def test_plan_header_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """layer_norm_plan.h has no HIP dependency: g++ alone builds it, with ASan and UBSan (signed overflow in the unit count or
    the scratch size would trap), and the program's answers are the library's"""
    exe = tmp_path / "layer_norm_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "layer_norm_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = [(0, 17, 1, 0), (1, 1, 0, 1), (5, 1024, 1, 0), (5, 1025, 1, 1), (9, 8192, 0, 0), (9, 8193, 1, 1), (65536, 1024, 1, 0),
             (8192, 4096, 1, 1), (64, 1 << 20, 1, 0), (0, 17, 1, 2), (8192, 37, 1, 2), (8193, 37, 0, 2), (65536, 1024, 1, 2),
             (MAX, MAX, 1, 2), (MAX + 1, 4, 1, 2), (MAX + 1, 4, 1, 0), ((1 << 63) - 1, MAX, 0, 1), (7, 0, 1, 0), (-3, 4, 0, 2),
             (4, MAX + 1, 1, 1), (4, 4, 1, 3)]
    text = "".join("%d %d %d %d\n" % c for c in cases)
    r = subprocess.run([str(exe), "-"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0), c
        assert got[1:] == p, (c, got, p)


def fwd_args(**kw):
    """a valid forward call on (4, 8) (pointers never dereferenced: arguments are judged first), with replacements"""
    a = dict(y=C.c_void_p(4096), ys=8, mean=C.c_void_p(8192), ms=1, rstd=C.c_void_p(12288), rs=1, x=C.c_void_p(16384), xs=8,
             gamma=C.c_void_p(20480), gs=1, beta=C.c_void_p(24576), bs=1, rows=4, n=8, eps=1e-5)
    a.update(kw)
    return tuple(a[k] for k in ("y", "ys", "mean", "ms", "rstd", "rs", "x", "xs", "gamma", "gs", "beta", "bs", "rows", "n", "eps")) + (None,)


def grad_args(**kw):
    a = dict(dx=C.c_void_p(4096), dxs=8, dgamma=C.c_void_p(8192), dgs=1, dbeta=C.c_void_p(12288), dbs=1, dy=C.c_void_p(16384), dys=8,
             x=C.c_void_p(20480), xs=8, mean=C.c_void_p(24576), ms=1, rstd=C.c_void_p(28672), rs=1, gamma=C.c_void_p(32768), gs=1,
             rows=4, n=8)
    a.update(kw)
    return tuple(a[k] for k in ("dx", "dxs", "dgamma", "dgs", "dbeta", "dbs", "dy", "dys", "x", "xs", "mean", "ms", "rstd", "rs",
                                "gamma", "gs", "rows", "n")) + (None,)


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    fwd, grad = L.laser_hip_layer_norm_f32_dev, L.laser_hip_layer_norm_grad_f32_dev
    x = C.c_void_p(16384)
    bad_fwd = [dict(rows=-1), dict(n=0), dict(n=-8), dict(n=MAX + 1, ys=MAX + 1, xs=MAX + 1), dict(eps=-1e-5), dict(eps=float("nan")),
               dict(eps=-float("inf")), dict(y=None), dict(x=None), dict(ys=7), dict(xs=7), dict(ms=0), dict(rs=-1),
               dict(y=x, ys=9)]                                          # in place with unequal row strides
    for kw in bad_fwd:
        assert fwd(*fwd_args(**kw)) == _lib.E_INVALID, kw
    dy = C.c_void_p(16384)
    bad_grad = [dict(rows=-1), dict(n=0), dict(n=MAX + 1, dxs=MAX + 1, dys=MAX + 1, xs=MAX + 1), dict(dx=None, dgamma=None, dbeta=None),
                dict(rows=MAX + 1), dict(rows=MAX + 1, dx=None, dbeta=None), dict(rows=MAX + 1, dx=None, dgamma=None),
                dict(dy=None), dict(x=None), dict(mean=None), dict(rstd=None), dict(dxs=7), dict(dys=7), dict(xs=7),
                dict(dgs=0), dict(dbs=0), dict(dx=dy, dxs=9), dict(dx=C.c_void_p(20480), dxs=9)]
    for kw in bad_grad:
        assert grad(*grad_args(**kw)) == _lib.E_INVALID, kw
    assert grad(*grad_args(rows=MAX + 1, dx=None, dbeta=None)) == _lib.E_INVALID and b"2^26" in L.laser_hip_last_error()
    # the sizes are judged before any pointer, with every pointer NULL too
    none = dict(y=None, mean=None, rstd=None, x=None, gamma=None, beta=None)
    assert fwd(*fwd_args(rows=-1, **none)) == _lib.E_INVALID
    assert fwd(*fwd_args(eps=-1.0, **none)) == _lib.E_INVALID


def test_a_valid_call_needs_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one, the calls that touch nothing succeed"""
    from laser_amd import _lib
    fwd, grad = L.laser_hip_layer_norm_f32_dev, L.laser_hip_layer_norm_grad_f32_dev
    none = dict(y=None, mean=None, rstd=None, x=None, gamma=None, beta=None)
    if have_gpu():
        assert fwd(*fwd_args(rows=0, **none)) == 0                                     # no rows: nothing happens
        return
    assert fwd(*fwd_args()) == _lib.E_NODEVICE
    assert fwd(*fwd_args(mean=None, rstd=None, gamma=None, beta=None, eps=0.0)) == _lib.E_NODEVICE      # inference, eps = 0
    assert fwd(*fwd_args(y=C.c_void_p(16384))) == _lib.E_NODEVICE                      # in place
    assert fwd(*fwd_args(eps=float("inf"))) == _lib.E_NODEVICE                         # rstd = 0: IEEE, not refused
    assert fwd(*fwd_args(rows=MAX + 1, ys=8, xs=8)) == _lib.E_NODEVICE                 # the row kernels have no row bound
    assert fwd(*fwd_args(rows=0, **none)) == _lib.E_NODEVICE
    assert grad(*grad_args()) == _lib.E_NODEVICE
    assert grad(*grad_args(dx=None, dgamma=None)) == _lib.E_NODEVICE                   # dbeta alone
    assert grad(*grad_args(dgamma=None, dbeta=None, gamma=None, rows=MAX + 1)) == _lib.E_NODEVICE      # dx alone: any rows
    assert grad(*grad_args(dx=C.c_void_p(16384))) == _lib.E_NODEVICE                   # dx in place over dy
    assert grad(*grad_args(rows=0, dx=None, dy=None, x=None, mean=None, rstd=None)) == _lib.E_NODEVICE  # rows = 0 still writes +0
    assert plan(L, 4, 8)[0] == 0                                                       # the plan needs no device
    import laser_amd
    with pytest.raises(TypeError):
        laser_amd.layer_norm(np.ones((4, 8), np.float32))            # a host array is not taken (and nothing falls back)


def test_cpp_mirror_compiles(tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "layer_norm_mirror.cpp"), "-o", str(tmp_path / "m"), "-L", lib,
                    "-llaser_hip"], check=True)


def test_python_layer_checks_its_operands():
    import inspect
    import laser_amd
    from laser_amd import nn
    assert list(inspect.signature(laser_amd.layer_norm).parameters) == ["x", "gamma", "beta", "eps", "out", "stats"]
    assert list(inspect.signature(laser_amd.layer_norm_backward).parameters) == ["dy", "x", "mean", "rstd", "gamma", "need_dx",
                                                                               "need_params"]
    assert inspect.signature(laser_amd.layer_norm).parameters["eps"].default == 1e-5

    class V:      # a device operand as the layer sees it, never dereferenced
        def __init__(self, shape, strides, typestr="<f4"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "version": 3, "data": (4096, False),
                                             "strides": tuple(int(typestr[2]) * s for s in strides)}
    assert nn._ln_rows("f", "x", V((5, 7), (10, 1)))[1:] == (5, 7, 10)
    assert nn._ln_rows("f", "x", V((1, 7), (0, 1)))[1:] == (1, 7, 7)             # the stride of a lone row is never applied
    assert nn._ln_rows("f", "x", V((2, 3, 7), (21, 7, 1)))[1:] == (6, 7, 7)      # contiguous, rank 3: (6, 7)
    assert nn._ln_vector("f", "g", V((7,), (3,)), (7,))[1] == 3
    assert nn._ln_vector("f", "m", V((2, 3), (3, 1)), (2, 3))[1] == 1
    x = V((5, 7), (7, 1))
    for bad in (V((7,), (1,)), V((), ())):                                       # wrong ranks
        with pytest.raises(ValueError):
            laser_amd.layer_norm(bad)
    with pytest.raises(ValueError):
        laser_amd.layer_norm(V((5, 7), (1, 5)))                                  # a transposed view
    with pytest.raises(ValueError):
        laser_amd.layer_norm(V((2, 3, 7), (42, 7, 1)))                           # rank 3, not contiguous
    with pytest.raises(ValueError):
        laser_amd.layer_norm(V((5, 0), (0, 1)))                                  # empty rows
    with pytest.raises(TypeError):
        laser_amd.layer_norm(V((5, 7), (7, 1), "<f8"))
    with pytest.raises(ValueError):
        laser_amd.layer_norm(x, gamma=V((8,), (1,)))                             # wrong shapes
    with pytest.raises(ValueError):
        laser_amd.layer_norm(x, beta=V((7, 1), (1, 1)))
    with pytest.raises(ValueError):
        laser_amd.layer_norm(x, out=V((5, 8), (8, 1)))
    for eps in (-1e-5, float("nan"), -float("inf")):
        with pytest.raises(ValueError):
            laser_amd.layer_norm(x, eps=eps)
    m = V((5,), (1,))
    with pytest.raises(ValueError):
        laser_amd.layer_norm_backward(x, V((5, 8), (8, 1)), m, m)                # x unlike dy
    with pytest.raises(ValueError):
        laser_amd.layer_norm_backward(x, x, V((4,), (1,)), m)                    # one mean per row
    with pytest.raises(ValueError):
        laser_amd.layer_norm_backward(x, x, m, V((5, 1), (2, 1)))
    with pytest.raises(ValueError):
        laser_amd.layer_norm_backward(x, x, m, m, gamma=V((7, 7), (7, 1)))
    with pytest.raises(ValueError):
        laser_amd.layer_norm_backward(x, x, m, m, need_dx=False, need_params=False)
    with pytest.raises(ValueError):
        laser_amd.layer_norm_backward(x, x, m, m, need_params="both")
    with pytest.raises(ValueError):
        laser_amd.layer_norm_backward(x, x, m, m, need_dx=V((5, 7), (1, 5)))


# ---- the model is accurate enough to be a contract ---------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n", [(37, 1025), (9, 8193), (300, 37)])
def test_model_is_as_close_to_float64_as_torch_float32(rows, n):
    """The maximum absolute error of the model's y, dx, dgamma and dbeta against float64 torch.nn.functional.layer_norm
    (forward and autograd) is at most twice that of torch's own float32 CPU result on the same inputs: torch on the CPU is
    the yardstick, and the factor 2 allows for the different summation order."""
    import torch
    rng = np.random.default_rng(1000 * rows + n)
    x = rng.normal(3, 2, (rows, n)).astype(np.float32)
    gamma = rng.normal(1, 0.5, n).astype(np.float32)
    beta = rng.normal(0, 1, n).astype(np.float32)
    dy = rng.normal(0, 1, (rows, n)).astype(np.float32)
    eps = 1e-5

    def torch_run(dtype):
        tx = torch.tensor(x, dtype=dtype, requires_grad=True)
        tg = torch.tensor(gamma, dtype=dtype, requires_grad=True)
        tb = torch.tensor(beta, dtype=dtype, requires_grad=True)
        ty = torch.nn.functional.layer_norm(tx, (n,), tg, tb, eps)
        ty.backward(torch.tensor(dy, dtype=dtype))
        return [t.detach().numpy().astype(np.float64) for t in (ty, tx.grad, tg.grad, tb.grad)]

    ref = torch_run(torch.float64)
    t32 = torch_run(torch.float32)
    y, mean, rstd = M.forward(x, gamma, beta, eps)
    dx, dgamma, dbeta = M.backward(dy, x, mean, rstd, gamma)
    for name, mine, theirs, want in zip(("y", "dx", "dgamma", "dbeta"), (y, dx, dgamma, dbeta), t32, ref):
        assert mine.dtype == np.float32 and mine.shape == want.shape, name
        e_model = np.abs(mine.astype(np.float64) - want).max()
        e_torch = np.abs(theirs - want).max()
        print(f"{rows} x {n} {name}: model {e_model:.3e}, torch float32 {e_torch:.3e}, ratio {e_model / e_torch:.2f}")
        assert e_model <= 2 * e_torch, (name, e_model, e_torch)


def test_model_edge_rows():
    """n = 1, a row of -0, a constant row with eps = 0: what the header says"""
    y, mean, rstd = M.forward(np.float32([[5.0], [-0.0]]), None, None, 1e-5)
    assert M.same_bits(mean, np.float32([5.0, 0.0])) and M.same_bits(y, np.float32([[0.0], [-0.0]]))
    assert M.same_bits(rstd, np.float32(1) / np.sqrt(np.float32([1e-5, 1e-5])))
    y, mean, rstd = M.forward(np.float32([[-0.0] * 5, [2.5] * 5]), None, None, 0.0)
    assert M.same_bits(mean, np.float32([0.0, 2.5])) and np.isinf(rstd).all() and np.isnan(y).all()
    y, mean, rstd = M.forward(np.float32([[-0.0] * 5]), np.float32([1, -1, 2, 0, 1]), None, 1e-5)
    assert M.same_bits(y, np.float32([[-0.0, 0.0, -0.0, -0.0, -0.0]]))
