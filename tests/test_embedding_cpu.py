"""CPU-side checks of the embedding layer (include/laser_hip.h "Embedding"): the entry points are declared, exported and
mirrored; laser_hip_embedding_plan follows the stated rules and is the plan header compiled alone, which also runs as a host
program under ASan and UBSan; every invalid argument is refused before a device is looked for; a valid call needs a gfx950
device; the numpy model is consistent with itself; the Python layer checks its operands."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip.h")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_embedding_f32_dev", "laser_hip_embedding_group_i32_dev", "laser_hip_embedding_grad_f32_dev",
       "laser_hip_embedding_plan", "laser_hip_embedding_last_kernel"]
MAX_TOKENS, MAX_VOCAB = 1 << 26, 1 << 30


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


def plan(L, tokens, vocab, dim, vec=1, cus=256):
    out = (C.c_int64 * 8)(*([-1] * 8))
    rc = L.laser_hip_embedding_plan(tokens, vocab, dim, vec, cus, out)
    return rc, list(out)


def expected_plan(tokens, vocab, dim, vec):
    """the rules of laser_amd/csrc/embedding_plan.h, written out again"""
    passes = max(1, -(-int(vocab).bit_length() // 8))
    tile = 512
    while -(-tokens // tile) > 1 << 14:
        tile *= 2
    tiles = -(-tokens // tile)
    group_scratch = 0 if tokens == 0 else 2 * 256 * tiles * 4 + (tokens * 4 if passes > 1 else 0)
    sums = vocab > 0 and dim > 0
    return [passes, tile, -(-tiles // 4), 0 if vec else 1, 1 if tokens == 0 else 3 * passes + 1, 2 if sums else 0, group_scratch,
            group_scratch + tokens * 4 + (vocab + 1) * 4 if sums else 0]


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
    for fn in ("embedding", "embedding_group", "embedding_backward"):
        assert callable(getattr(laser_amd, fn)) and re.search(r"inline [\w<>]+ %s\(" % fn, hpp), fn
    for proc in ("embedding", "embeddingGroup", "embeddingBackward"):
        assert re.search(r"proc %s\*" % proc, nim), proc
    text = open(HDR).read()
    assert "Embedding (f32)" in text
    assert re.search(r"#define LASER_HIP_EMBEDDING_MAX_TOKENS \(1ll << 26\)", text)
    assert re.search(r"#define LASER_HIP_EMBEDDING_MAX_VOCAB \(1ll << 30\)", text)
    for word in ("int64 ids", "float64", "accumulation into an existing dW", "sparse (rows, values)", "scale_grad_by_freq", "max_norm",
                 "padding id other than -1", "general-purpose sort", "fused optimizer step"):
        assert word in re.sub(r"\s*\n \*\s*", " ", text), word                 # the "Not built" list
    assert re.search(r"#define LASER_HIP_ABI_VERSION 3\b", text) and L.laser_hip_abi_version() == 3
    assert all(L.laser_hip_embedding_last_kernel(w) in (-1, 0, 1, 2, 3, 4) for w in (0, 1, 2))
    assert L.laser_hip_embedding_last_kernel(4) == -1 and L.laser_hip_embedding_last_kernel(-1) == -1


def test_plan_follows_the_stated_rules(L):
    from laser_amd import _lib
    for tokens in (0, 1, 511, 512, 513, 2047, 2048, 2049, 131072, 1 << 23, (1 << 23) + 1, 1 << 24, (1 << 24) + 1, 1 << 25,
                   (1 << 25) + 1, MAX_TOKENS):
        for vocab in (0, 1, 2, 200, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, MAX_VOCAB):
            for dim in (0, 1, 4, 17, 4096):
                for vec in (0, 1):
                    rc, p = plan(L, tokens, vocab, dim, vec)
                    assert rc == 0 and p == expected_plan(tokens, vocab, dim, vec), (tokens, vocab, dim, vec, p)
    # a vocabulary of 200 does not pay for 32 bits; the pass count moves at 256, 65536 and 2^24 and nowhere else
    assert [plan(L, 1000, v, 4)[1][0] for v in (200, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, MAX_VOCAB)] == [1, 1, 2, 2, 3, 3, 4, 4]
    # the tile doubles where 512-position tiles would pass 2^14 of them; 2^26 tokens: 4096
    assert [plan(L, t, 9, 4)[1][1] for t in (1 << 23, (1 << 23) + 1, 1 << 24, (1 << 24) + 1, MAX_TOKENS)] == [512, 1024, 1024, 2048, 4096]
    for cus in (0, 64, 256, 304):                                               # the plan does not depend on the compute units
        assert plan(L, 131072, 32768, 1024, cus=cus)[1] == expected_plan(131072, 32768, 1024, 1)
    for args in ((MAX_TOKENS + 1, 4, 4), (-1, 4, 4), (4, -1, 4), (4, MAX_VOCAB + 1, 4), (4, 4, -1)):
        rc, p = plan(L, *args)
        assert rc == _lib.E_INVALID and p == [-1] * 8, args                     # nothing is written
    assert L.laser_hip_embedding_plan(4, 4, 4, 1, 0, None) == _lib.E_INVALID


def test_plan_header_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """embedding_plan.h has no HIP dependency and no includes: g++ alone builds it, with ASan and UBSan (signed overflow in a
    scratch size would trap), and the program's answers are the library's.  A stand-alone program: nothing is loaded into
    Python under a sanitizer."""
    alone = tmp_path / "alone.cpp"
    alone.write_text('#include "embedding_plan.h"\nint main() { long long o[8]; return lh_embedding_plan(1, 1, 1, 1, 0, o); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(alone), "-o", str(tmp_path / "alone")], check=True)
    assert "#include" not in open(os.path.join(CSRC, "embedding_plan.h")).read()
    exe = tmp_path / "embedding_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "embedding_plan_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, (r.stdout + r.stderr)[-2000:]
    cases = [(0, 17, 4, 1, 256), (1, 1, 1, 0, 0), (5, 0, 3, 1, 0), (5, 3, 0, 1, 0), (1500, 255, 4, 1, 256), (1500, 256, 4, 0, 3),
             (131072, 32768, 1024, 1, 256), (16384, 131072, 4096, 1, 256), (MAX_TOKENS, MAX_VOCAB, 1 << 40, 1, 1),
             (MAX_TOKENS + 1, 4, 4, 1, 0), (7, MAX_VOCAB + 1, 4, 1, 0), (-3, 4, 4, 0, 0), (4, 4, -4, 0, 0)]
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    r = subprocess.run([str(exe), "-"], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0), c
        assert got[1:] == p, (c, got, p)


def test_bad_arguments_are_invalid(L):
    from laser_amd import _lib
    fwd, grp, grad = L.laser_hip_embedding_f32_dev, L.laser_hip_embedding_group_i32_dev, L.laser_hip_embedding_grad_f32_dev
    y, w, idx, order, starts, dw, dy = (C.c_void_p(4096 * k) for k in range(1, 8))   # never dereferenced: arguments are checked first
    bad_fwd = [
        (y, 8, w, 8, idx, -1, 5, 8), (y, 8, w, 8, idx, 4, -1, 8), (y, 8, w, 8, idx, 4, 5, -1),           # negative sizes
        (y, 8, w, 8, idx, MAX_TOKENS + 1, 5, 8), (y, 8, w, 8, idx, 4, MAX_VOCAB + 1, 8),                # past the limits
        (y, 7, w, 8, idx, 4, 5, 8), (y, 8, w, 7, idx, 4, 5, 8),                                          # a row stride below dim
        (None, 8, w, 8, idx, 4, 5, 8), (y, 8, None, 8, idx, 4, 5, 8), (y, 8, w, 8, None, 4, 5, 8),     # a NULL buffer that is touched
    ]
    for args in bad_fwd:
        assert fwd(*args, None) == _lib.E_INVALID, args
    bad_grp = [(order, starts, idx, -1, 5), (order, starts, idx, 4, -1), (order, starts, idx, MAX_TOKENS + 1, 5),
               (order, starts, idx, 4, MAX_VOCAB + 1), (None, starts, idx, 4, 5), (order, None, idx, 4, 5), (order, starts, None, 4, 5),
               (None, None, None, 0, 5)]                                                                 # starts is always written
    for args in bad_grp:
        assert grp(*args, None) == _lib.E_INVALID, args
    bad_grad = [
        (dw, 8, dy, 8, idx, None, None, -1, 5, 8), (dw, 8, dy, 8, idx, None, None, 4, -1, 8), (dw, 8, dy, 8, idx, None, None, 4, 5, -1),
        (dw, 8, dy, 8, idx, None, None, MAX_TOKENS + 1, 5, 8), (dw, 8, dy, 8, idx, None, None, 4, MAX_VOCAB + 1, 8),
        (dw, 7, dy, 8, idx, None, None, 4, 5, 8), (dw, 8, dy, 7, idx, None, None, 4, 5, 8),              # a row stride below dim
        (dw, 8, dy, 8, idx, order, None, 4, 5, 8), (dw, 8, dy, 8, idx, None, starts, 4, 5, 8),          # exactly one of order / starts
        (None, 8, dy, 8, idx, None, None, 4, 5, 8), (dw, 8, None, 8, idx, None, None, 4, 5, 8), (dw, 8, dy, 8, None, None, None, 4, 5, 8),
        (None, 8, None, 8, None, None, None, 0, 5, 8),                                                   # tokens = 0 still writes dW
    ]
    for args in bad_grad:
        assert grad(*args, None) == _lib.E_INVALID, args
    # NULL-safe ordering: the sizes and the strides are judged before any pointer, with every pointer NULL too
    assert fwd(None, 8, None, 8, None, MAX_TOKENS + 1, 5, 8, None) == _lib.E_INVALID
    assert b"2^26" in L.laser_hip_last_error()                       # the text says which bound
    assert grad(None, 8, None, 7, None, None, None, 4, 5, 8, None) == _lib.E_INVALID
    assert b"below dim" in L.laser_hip_last_error()


def test_a_valid_call_needs_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); with one, the calls that touch nothing succeed"""
    from laser_amd import _lib
    fwd, grp, grad = L.laser_hip_embedding_f32_dev, L.laser_hip_embedding_group_i32_dev, L.laser_hip_embedding_grad_f32_dev
    if have_gpu():
        assert fwd(None, 8, None, 8, None, 0, 5, 8, None) == 0                            # no tokens: nothing happens
        assert grad(None, 0, None, 0, None, None, None, 4, 5, 0, None) == 0               # no columns: dW has no element
        return
    y, w, idx, order, starts, dw, dy = (C.c_void_p(4096 * k) for k in range(1, 8))
    assert fwd(y, 8, w, 8, idx, 4, 5, 8, None) == _lib.E_NODEVICE
    assert fwd(None, 8, None, 8, None, 0, 5, 8, None) == _lib.E_NODEVICE                  # judged after the device
    assert fwd(y, 8, None, 8, idx, 4, 0, 8, None) == _lib.E_NODEVICE                      # no vocabulary: W is never touched
    assert grp(order, starts, idx, 4, 5, None) == _lib.E_NODEVICE
    assert grp(None, starts, None, 0, 5, None) == _lib.E_NODEVICE                         # tokens = 0 still writes starts
    assert grad(dw, 8, dy, 8, idx, None, None, 4, 5, 8, None) == _lib.E_NODEVICE
    assert grad(dw, 8, dy, 8, idx, order, starts, 4, 5, 8, None) == _lib.E_NODEVICE       # the pre-grouped form
    assert grad(dw, 8, None, 8, None, None, None, 0, 5, 8, None) == _lib.E_NODEVICE       # tokens = 0 still writes dW = +0
    assert grad(None, 0, None, 0, None, None, None, 4, 5, 0, None) == _lib.E_NODEVICE
    assert plan(L, 4, 5, 8)[0] == 0                                                        # the plan needs no device
    import laser_amd
    with pytest.raises(TypeError):
        laser_amd.embedding(np.ones((4, 8), np.float32), np.zeros(3, np.int32))           # host arrays are not taken


def test_the_model_is_consistent_with_itself():
    from tests import embedding_model as M
    from tests import reduce_model as R
    rng = np.random.default_rng(1)
    idx = rng.integers(-2, 9, 200).astype(np.int32)
    order, starts = M.group(idx, 7)
    ok = (idx >= 0) & (idx < 7)
    assert sorted(order.tolist()) == list(range(200)) and starts[0] == 0 and starts[7] == ok.sum()
    assert (np.diff(order[starts[7]:]) > 0).all() and not ok[order[starts[7]:]].any()     # the others follow in ascending position
    for v in range(7):
        seg = order[starts[v]:starts[v + 1]]
        assert (idx[seg] == v).all() and (np.diff(seg) > 0).all() and seg.size == (idx == v).sum()
    dy = rng.normal(0, 1, (200, 3)).astype(np.float32)
    dw = M.grad(dy, idx, 7)
    assert dw[2, 1].view(np.uint32) == np.float32(R.model_sum(dy[idx == 2, 1])).view(np.uint32)
    one = M.grad(dy, np.zeros(200, np.int32), 1)
    assert np.array_equal(one[0].view(np.uint32), np.array([R.model_sum(dy[:, j]) for j in range(3)], np.float32).view(np.uint32))
    w = rng.normal(0, 1, (7, 3)).astype(np.float32)
    y = M.gather(w, idx.reshape(20, 10))
    assert y.shape == (20, 10, 3) and np.array_equal(y.reshape(-1, 3)[ok], w[idx[ok]])
    assert not y.reshape(-1, 3)[idx == -1].view(np.uint32).any()
    assert (y.reshape(-1, 3)[~ok & (idx != -1)].view(np.uint32) == 0x7FC00000).all()


def test_python_layer_checks_its_operands():
    import inspect
    import laser_amd
    assert list(inspect.signature(laser_amd.embedding).parameters) == ["w", "idx", "out"]
    assert list(inspect.signature(laser_amd.embedding_group).parameters) == ["idx", "vocab"]
    assert list(inspect.signature(laser_amd.embedding_backward).parameters) == ["dy", "idx", "vocab", "out", "group"]

    class V:      # a device operand as the layer sees it, never dereferenced
        def __init__(self, shape, strides, typestr="<f4"):
            size = int(typestr[2:])
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "version": 3, "data": (4096, False),
                                             "strides": tuple(size * s for s in strides)}
    w, i32 = V((9, 4), (4, 1)), V((2, 3), (3, 1), "<i4")
    with pytest.raises(ValueError, match="int32"):
        laser_amd.embedding(w, V((2, 3), (3, 1), "<i8"))                       # int64 ids: convert to int32
    with pytest.raises(ValueError, match="int32"):
        laser_amd.embedding_backward(V((6, 4), (4, 1)), V((6,), (1,), "<i8"), 9)
    with pytest.raises(ValueError, match="int32"):
        laser_amd.embedding_group(V((6,), (1,), "<i8"), 9)
    with pytest.raises(TypeError):
        laser_amd.embedding(w, V((2, 3), (3, 1)))                              # float ids
    with pytest.raises(ValueError):
        laser_amd.embedding(w, V((2, 3), (6, 1), "<i4"))                       # ids that are not contiguous
    with pytest.raises(ValueError):
        laser_amd.embedding(V((9, 4), (1, 9)), i32)                            # a transposed table
    with pytest.raises(ValueError):
        laser_amd.embedding(V((9, 4, 2), (8, 2, 1)), i32)                      # a table that is not 2-D
    with pytest.raises(ValueError):
        laser_amd.embedding(w, i32, out=V((2, 3, 5), (15, 5, 1)))              # a destination of another width
    with pytest.raises(ValueError):
        laser_amd.embedding(w, i32, out=V((6, 4), (1, 6)))                     # a non-unit column stride
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((5, 4), (4, 1)), i32, 9)                # dy of another token count
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((6, 4), (1, 6)), i32, 9)                # a non-unit column stride
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((6, 4), (4, 1)), i32, 9, out=V((8, 4), (4, 1)))     # dw of another vocab
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((6, 4), (4, 1)), i32, -1)
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((6, 4), (4, 1)), i32, (1 << 30) + 1)
    dw = V((9, 4), (4, 1))
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((6, 4), (4, 1)), i32, 9, out=dw, group=(V((5,), (1,), "<i4"), V((10,), (1,), "<i4")))   # order
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((6, 4), (4, 1)), i32, 9, out=dw, group=(V((6,), (1,), "<i4"), V((9,), (1,), "<i4")))    # starts
    with pytest.raises(ValueError):
        laser_amd.embedding_backward(V((6, 4), (4, 1)), i32, 9, out=dw, group=V((6,), (1,), "<i4"))                            # not a pair
