"""CPU-side checks of row selection (include/laser_hip_select.h "Row top-k, argmax and top-k sampling"): the entry points are
declared in the header of their own, exported and mirrored; laser_hip_topk_plan agrees with a restatement on both sides of every
threshold and is the plan header compiled alone; every limit is refused before a device is looked for and a valid call needs a
gfx950 device; the numpy model (tests/select_model.py) has the properties the header states and its fixtures tell a wrong tie
rule from the right one; the vector kernels load 16 bytes per lane; the Nim imports match the header; the C++ additions
compile; and every `_dev` entry point of the header has a stream-order row (tests/test_gpu_select_stream_order.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import code_objects
from tests import select_model as M
from tests import stream_order as SO
from tests import test_gpu_select_stream_order as ROWS
from tests import test_nim_shim_cpu as shim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO_PATH = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
HDR = os.path.join(ROOT, "include", "laser_hip_select.h")
NIM = os.path.join(ROOT, "nim", "laser_hip_select.nim")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
NEW = ["laser_hip_topk_rows_f32_dev", "laser_hip_argmax_rows_f32_dev", "laser_hip_take_rows_i32_dev", "laser_hip_topk_plan",
       "laser_hip_topk_last_kernel"]
MAX_N, MAX_ROWS, MAX_K = 1 << 24, 1 << 26, 1024


def plan_constant(name):
    text = open(os.path.join(CSRC, "select_plan.h")).read()
    return int(re.search(r"#define " + name + r" (\d+)", text).group(1))


WAVE_N, RESIDENT_N, CAP = plan_constant("LH_SELECT_WAVE_N"), plan_constant("LH_SELECT_RESIDENT_N"), plan_constant("LH_SELECT_MAX_WORKGROUPS")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO_PATH):
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


def header_text():
    return re.sub(r"\s+", " ", subprocess.run(["gcc", "-E", "-P", HDR], check=True, capture_output=True, text=True).stdout)


def plan(L, rows, n, k, vec=1):
    out = (C.c_int64 * 3)(-1, -1, -1)
    return L.laser_hip_topk_plan(rows, n, k, vec, out), list(out)


def test_a_header_of_its_own_declares_what_the_library_exports_and_the_mirrors_carry(L):
    from laser_amd import _lib
    import laser_amd
    hdr = header_text()
    declared = set(re.findall(r"\b(laser_hip_\w+)\s*\(", hdr))
    assert declared == set(NEW) == set(_lib.select_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", SO_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert re.search(r"\bint " + name + r" ?\(", hdr), name
        assert name in exported and getattr(L, name).argtypes is not None, name
    main = open(os.path.join(ROOT, "include", "laser_hip.h")).read()
    assert "laser_hip_select" not in main and not (declared & set(re.findall(r"\b(laser_hip_\w+)\s*\(", main)))
    assert '#include "laser_hip_select.h"' in open(os.path.join(ROOT, "include", "laser.hpp")).read()
    text = open(HDR).read()
    first = text[:text.index("*/")] if text.index("*/") < text.index("#ifndef") else ""
    assert "Folding this header into laser_hip.h" in first and "left to a change that may edit the table" in re.sub(r"\s+\*?\s*", " ", first)
    for word in ("Not built", "float64 and integer keys", "k > 1024", "a full row sort", "top-p", "another axis"):
        assert word in text or word.replace("another axis", "an axis other") in text, word
    assert re.search(r"at most FIVE times", text)
    for macro, value in (("MAX_N", "1ll << 24"), ("MAX_ROWS", "1ll << 26"), ("MAX_K", "1024")):
        assert re.search(r"#define LASER_HIP_SELECT_%s \(?%s\)?" % (macro, re.escape(value)), text), macro
    for fn in ("topk", "argmax", "argmin", "take_rows", "sample_top_k"):
        assert callable(getattr(laser_amd, fn)), fn
        assert re.search(r"inline [\w<>]+ %s\(" % fn, open(os.path.join(ROOT, "include", "laser.hpp")).read()), fn
    assert L.laser_hip_topk_last_kernel() in (-1, 0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14)
    assert "laser_hip_select.h" in open(os.path.join(ROOT, "README.md")).read()


def restated(rows, n, k, vec):
    """the plan in Python, from the header's words"""
    if not (0 <= rows <= MAX_ROWS and 1 <= n <= MAX_N and 1 <= k <= min(n, MAX_K)):
        return None
    code = 0 if n <= WAVE_N else 1 if n <= RESIDENT_N else 2
    want = -(-rows // 4) if code == 0 else rows
    lds = 4 * 256 * 8 if code == 0 else 1024 * 8 + 256 * 4 + 2 * 8 * 4 * 4 + 16
    return [code + (0 if vec else 4), min(CAP, want), lds]


PLAN_CASES = [(rows, n, k, vec)
              for rows in (0, 1, 3, 4, 5, CAP - 1, CAP, CAP + 1, 4 * CAP - 1, 4 * CAP, 4 * CAP + 1, 4 * CAP + 3, MAX_ROWS, MAX_ROWS + 1, -1)
              for n in (0, 1, 2, WAVE_N - 1, WAVE_N, WAVE_N + 1, RESIDENT_N - 1, RESIDENT_N, RESIDENT_N + 1, 70001, MAX_N, MAX_N + 1)
              for k in (0, 1, 7, MAX_K, MAX_K + 1, n, n + 1)
              for vec in (0, 1)]


def test_plan_agrees_with_a_restatement_on_both_sides_of_every_threshold(L):
    from laser_amd import _lib
    assert (WAVE_N, RESIDENT_N, CAP) == (256, 8192, 2048)          # what the header's section states
    taken = 0
    for rows, n, k, vec in PLAN_CASES:
        rc, got = plan(L, rows, n, k, vec)
        want = restated(rows, n, k, vec)
        if want is None:
            assert rc == _lib.E_INVALID and got == [-1, -1, -1], (rows, n, k)
        else:
            assert rc == 0 and got == want, (rows, n, k, vec, got, want)
            taken += 1
    assert taken > 500
    assert plan(L, 0, 5, 1)[1][1] == 0 and plan(L, 4 * CAP, 5, 1)[1][1] == CAP and plan(L, 4 * CAP - 4, 5, 1)[1][1] == CAP - 1
    assert plan(L, CAP + 1, 300, 1)[1][1] == CAP and plan(L, CAP - 1, 9000, 1)[1][1] == CAP - 1
    assert L.laser_hip_topk_plan(4, 4, 1, 1, None) == _lib.E_INVALID
    import laser_amd
    assert laser_amd.topk_plan(5, 300, 7) == (1, 5, restated(5, 300, 7, 1)[2])


def test_plan_header_as_a_host_program_under_the_sanitizers(L, tmp_path):
    """select_plan.h has no HIP dependency: g++ alone builds it, with ASan and UBSan, and the program's answers are the
    library's"""
    exe = tmp_path / "select_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "select_plan_host.cpp"), "-o", str(exe)], check=True)
    cases = PLAN_CASES + [((1 << 63) - 1, 5, 1, 1), (5, (1 << 63) - 1, 1, 0), (5, 9, (1 << 63) - 1, 1), (-(1 << 63), 5, 1, 1)]
    r = subprocess.run([str(exe)], input="".join("%d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(lines) == len(cases)
    for c, got in zip(cases, lines):
        rc, p = plan(L, *c)
        assert (got[0] == 0) == (rc == 0) and got[1:] == p, (c, got, p)


# ---- the limits, without a device ---------------------------------------------------------------------------------------------
def topk_args(**kw):
    """a valid call on (4, 300), k = 8 (pointers never dereferenced: arguments are judged first), with replacements"""
    a = dict(vals=C.c_void_p(1 << 20), vs=8, idx=C.c_void_p(2 << 20), is_=8, src=C.c_void_p(3 << 20), ss=300, rows=4, n=300, k=8, largest=1)
    a.update(kw)
    return tuple(a[k] for k in ("vals", "vs", "idx", "is_", "src", "ss", "rows", "n", "k", "largest")) + (None,)


def argmax_args(**kw):
    a = dict(idx=C.c_void_p(1 << 20), is_=1, val=C.c_void_p(2 << 20), vs=1, src=C.c_void_p(3 << 20), ss=300, rows=4, n=300, largest=1)
    a.update(kw)
    return tuple(a[k] for k in ("idx", "is_", "val", "vs", "src", "ss", "rows", "n", "largest")) + (None,)


def take_args(**kw):
    a = dict(out=C.c_void_p(1 << 20), os_=5, src=C.c_void_p(2 << 20), ss=8, j=C.c_void_p(3 << 20), js=5, rows=4, m=8, num=5)
    a.update(kw)
    return tuple(a[k] for k in ("out", "os_", "src", "ss", "j", "js", "rows", "m", "num")) + (None,)


def test_every_limit_is_refused_before_a_device_is_looked_for(L):
    from laser_amd import _lib
    topk, arg, take = L.laser_hip_topk_rows_f32_dev, L.laser_hip_argmax_rows_f32_dev, L.laser_hip_take_rows_i32_dev
    src = 3 << 20
    bad = [(dict(k=0), b"min(n, 1024)"), (dict(k=-1), b"min(n, 1024)"), (dict(k=301), b"min(n, 1024)"),
           (dict(k=1025, n=2000, ss=2000, vs=1025, is_=1025), b"min(n, 1024)"),
           (dict(n=0), b"2^24"), (dict(n=-5), b"2^24"), (dict(n=MAX_N + 1, ss=MAX_N + 1), b"2^24"),
           (dict(rows=-1), b"2^26"), (dict(rows=MAX_ROWS + 1), b"2^26"),
           (dict(vals=None, idx=None), b"neither"), (dict(src=None), b"null"),
           (dict(ss=299), b"row strides"), (dict(vs=7), b"row strides"), (dict(is_=7), b"row strides"),
           (dict(largest=2), b"largest"), (dict(largest=-1), b"largest"),
           (dict(vals=C.c_void_p(src + 4 * 100)), b"overlap"), (dict(idx=C.c_void_p(src + 4 * (3 * 300 + 299))), b"overlap"),
           (dict(idx=C.c_void_p(src - 4 * (3 * 8 + 8) + 4)), b"overlap")]
    for kw, word in bad:
        assert topk(*topk_args(**kw)) == _lib.E_INVALID, kw
        assert word in L.laser_hip_last_error(), (kw, L.laser_hip_last_error())
    # the sizes are judged before any pointer, with every pointer NULL too
    assert topk(*topk_args(k=0, vals=None, idx=None, src=None)) == _lib.E_INVALID and b"min(n, 1024)" in L.laser_hip_last_error()
    # no rows: nothing happens, with or without a device; the sizes are still judged
    assert topk(*topk_args(rows=0, vals=None, idx=None, src=None)) == 0
    assert topk(*topk_args(rows=0, k=301)) == _lib.E_INVALID
    for kw in (dict(n=0), dict(n=MAX_N + 1, ss=MAX_N + 1), dict(rows=-1), dict(rows=MAX_ROWS + 1), dict(idx=None), dict(src=None), dict(ss=299),
               dict(is_=0), dict(vs=0), dict(largest=3), dict(idx=C.c_void_p(src + 40)), dict(val=C.c_void_p(src + 4 * (3 * 300 + 299)))):
        assert arg(*argmax_args(**kw)) == _lib.E_INVALID, kw
    assert arg(*argmax_args(rows=0, idx=None, src=None)) == 0
    for kw in (dict(m=0), dict(m=MAX_N + 1, ss=MAX_N + 1), dict(num=-1), dict(num=MAX_N + 1, os_=MAX_N + 1, js=MAX_N + 1), dict(rows=-1),
               dict(rows=MAX_ROWS + 1), dict(out=None), dict(src=None), dict(j=None), dict(ss=7), dict(os_=4), dict(js=4),
               dict(out=C.c_void_p((2 << 20) + 8)), dict(out=C.c_void_p((3 << 20) + 4 * 19))):
        assert take(*take_args(**kw)) == _lib.E_INVALID, kw
    assert take(*take_args(rows=0, out=None)) == 0 and take(*take_args(num=0, out=None)) == 0


def test_a_valid_call_needs_a_gfx950_device(L):
    """E_NODEVICE without a GPU (no fallback); the plan and the last-kernel record need none"""
    from laser_amd import _lib
    if have_gpu():
        assert L.laser_hip_topk_rows_f32_dev(*topk_args(rows=0)) == 0
        return
    topk, arg, take = L.laser_hip_topk_rows_f32_dev, L.laser_hip_argmax_rows_f32_dev, L.laser_hip_take_rows_i32_dev
    for kw in (dict(), dict(vals=None), dict(idx=None), dict(largest=0), dict(k=300, vs=300, is_=300),
               dict(rows=MAX_ROWS, vals=C.c_void_p(1 << 44), idx=C.c_void_p(2 << 44), src=C.c_void_p(3 << 44)),
               dict(n=MAX_N, ss=MAX_N, k=1024, vs=1024, is_=1024, rows=1), dict(rows=1, ss=0, vs=0, is_=0),
               dict(vals=C.c_void_p((3 << 20) + 4 * 4 * 300))):                                 # right behind the source
        assert topk(*topk_args(**kw)) == _lib.E_NODEVICE, kw
    assert arg(*argmax_args()) == _lib.E_NODEVICE and arg(*argmax_args(val=None, largest=0)) == _lib.E_NODEVICE
    assert take(*take_args()) == _lib.E_NODEVICE
    assert plan(L, 4, 300, 8)[0] == 0
    import laser_amd
    with pytest.raises(TypeError):
        laser_amd.topk(np.ones((4, 8), np.float32), 2)               # a host array is not taken (and nothing falls back)
    with pytest.raises(TypeError):
        laser_amd.argmax(np.ones((4, 8), np.float32))


def test_python_layer_checks_its_operands():
    import inspect
    import laser_amd
    from laser_amd import select
    assert list(inspect.signature(laser_amd.topk).parameters) == ["x", "k", "largest", "values", "indices"]
    assert list(inspect.signature(laser_amd.sample_top_k).parameters) == ["logits", "k", "num_samples", "u", "rng"]
    assert list(inspect.signature(laser_amd.argmax).parameters) == list(inspect.signature(laser_amd.argmin).parameters) == ["x"]
    assert list(inspect.signature(laser_amd.take_rows).parameters) == ["src", "j"]

    class V:      # a device operand as the layer sees it, never dereferenced
        def __init__(self, shape, strides, typestr="<f4"):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "version": 3, "data": (4096, False),
                                             "strides": tuple(int(typestr[2]) * s for s in strides)}
    assert select._rows("f", "x", V((5, 7), (10, 1)))[1:] == (5, 7, 10)
    assert select._rows("f", "x", V((1, 7), (0, 1)))[1:] == (1, 7, 7)            # the stride of a lone row is never applied
    assert select._rows("f", "x", V((2, 3, 7), (21, 7, 1)))[1:] == (6, 7, 7)     # contiguous, rank 3: (6, 7)
    x = V((5, 7), (7, 1))
    for bad in (V((7,), (1,)), V((5, 7), (1, 5)), V((2, 3, 7), (42, 7, 1)), V((5, 0), (0, 1))):
        with pytest.raises(ValueError):
            laser_amd.topk(bad, 1)
        with pytest.raises(ValueError):
            laser_amd.argmax(bad)
    with pytest.raises(TypeError):
        laser_amd.topk(V((5, 7), (7, 1), "<f8"), 1)
    for k in (0, 8, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            laser_amd.topk(x, k)
    with pytest.raises(ValueError):
        laser_amd.topk(V((2, 2000), (2000, 1)), 1025)
    with pytest.raises(ValueError):
        laser_amd.topk(x, 2, values=False, indices=False)
    with pytest.raises(TypeError):
        laser_amd.take_rows(x, V((5, 2), (2, 1), "<i4"))
    with pytest.raises(ValueError):
        laser_amd.take_rows(V((5, 7), (7, 1), "<i4"), V((4, 2), (2, 1), "<i4"))
    with pytest.raises(ValueError):
        laser_amd.sample_top_k(V((7,), (1,)), 2)
    with pytest.raises(ValueError):
        laser_amd.sample_top_k(x, 2, u=np.zeros((5, 1), np.float32), rng=laser_amd.Rng(1))


# ---- the model ----------------------------------------------------------------------------------------------------------------
def test_the_model_orders_special_values_as_the_header_says():
    keys = M.key(M.SPECIALS)
    assert (np.diff(keys.astype(np.int64)) > 0).all()                # the fixture is in ascending key order, no two alike
    b = M.bits(M.SPECIALS)
    neg_nan, pos_nan = (b >> 31 != 0) & np.isnan(M.SPECIALS), (b >> 31 == 0) & np.isnan(M.SPECIALS)
    assert neg_nan[:3].all() and not neg_nan[3:].any() and pos_nan[-3:].all() and not pos_nan[:-3].any()
    assert b[3] == 0xFF800000 and b[-4] == 0x7F800000                # -Inf right above the negative NaNs, +Inf right below the positive
    assert b[9] == 0x80000000 and b[10] == 0                         # -0 right below +0
    finite = M.SPECIALS[3:-3].astype(np.float64)
    assert (np.diff(finite) >= 0).all()                              # between the NaNs the key order is the numeric order
    rng = np.random.default_rng(0)
    x = rng.permutation(np.tile(M.SPECIALS, 3))[None, :]
    vals, idx = M.topk(x, x.shape[1], True)
    assert M.bits(vals)[0, :3].tolist() == [0x7FFFFFFF] * 3 and (np.diff(idx[0, :3]) > 0).all()      # a positive NaN first, ties by column
    assert (np.diff(M.key(vals)[0].astype(np.int64)) <= 0).all()
    small, sidx = M.topk(x, x.shape[1], False)
    assert M.bits(small)[0, :3].tolist() == [0xFFFFFFFF] * 3 and (np.diff(sidx[0, :3]) > 0).all()
    assert M.same_bits(M.bits(small)[0][::-1].reshape(-1, 3)[:, 0], M.bits(vals)[0].reshape(-1, 3)[:, 0])
    zeros = np.float32([[0.0, -0.0, 0.0, -0.0]])
    assert M.topk(zeros, 4, True)[1].tolist() == [[0, 2, 1, 3]] and M.topk(zeros, 4, False)[1].tolist() == [[1, 3, 0, 2]]
    assert M.bits(M.topk(zeros, 4, True)[0]).tolist() == [[0, 0, 0x80000000, 0x80000000]]           # bit copies
    assert M.argmax(np.float32([[1.0, M.POS_NAN, 5.0]])).tolist() == [1] and M.argmax(np.float32([[3.0, 7.0, 7.0, 1.0, 1.0]])).tolist() == [1]
    assert M.argmax(np.float32([[3.0, 7.0, 7.0, 1.0, 1.0]]), False).tolist() == [3]
    assert M.take_rows([[5, 6, 7]], [[2, 0, 3, -1]]).tolist() == [[7, 5, -1, -1]]
    # a prefix of a longer selection is the shorter selection: what the GPU suite relies on
    y = M.data("three", 3, 500)
    assert np.array_equal(M.topk(y, 100)[1][:, :7], M.topk(y, 7)[1])


def test_a_wrong_tie_rule_differs_on_the_tie_fixtures():
    for kind in ("three", "one", "special"):
        x = M.data(kind, 3, 300, seed=1)
        for largest in (True, False):
            right, wrong = M.topk(x, 7, largest), M.topk(x, 7, largest, ties_by_highest_index=True)
            assert M.same_bits(right[0], wrong[0]) and not np.array_equal(right[1], wrong[1]), (kind, largest)
    for n, k, at in ((1100, 7, 1024), (8300, 64, 8192), (8300, 1024, 4096)):
        x = M.straddle(n, k, at)
        right, wrong = M.topk(x, k), M.topk(x, k, ties_by_highest_index=True)
        assert not np.array_equal(right[1], wrong[1])
        assert right[1][0, -5:].tolist() == [at - 5, at - 2, at - 1, at, at + 1]                     # on both sides of the boundary
    x = M.data("normal", 3, 300, seed=1)                             # no ties: the rule cannot show
    assert np.array_equal(M.topk(x, 7)[1], M.topk(x, 7, ties_by_highest_index=True)[1])
    for kind in ("low_byte", "high_byte"):                           # one radix digit decides
        k = M.key(M.data(kind, 2, 400))
        assert len(np.unique(k & (0xFFFFFF00 if kind == "low_byte" else 0x00FFFFFF))) == 1 and len(np.unique(k)) > 100


# ---- the code objects ---------------------------------------------------------------------------------------------------------
def test_the_vector_kernels_load_16_bytes_per_lane(L, tmp_path):
    found = code_objects.kernels(b"topk_resident_kernel", r"\w*(?:topk_(?:wave|resident|streaming)|argmax_(?:wave|block))_kernelILb[01]E\w*", tmp_path)
    assert len(found) == 10, [n for n, _ in found]
    for name, text in found:
        vec = "_kernelILb1E" in name
        assert bool(re.search(r"global_load_dwordx4", text)) == vec, name
        assert re.search(r"global_load_dword\b", text), name        # the tail of a row, element by element
        assert not re.search(r"v_(add|mul|fma|max|min)_f(32|64)|global_atomic", text), name          # integers only; LDS counters only
    for name, text in found:
        if "topk_resident" in name or "topk_streaming" in name:
            assert re.search(r"ds_add_(rtn_)?u32", text), name       # the histogram: integer LDS counters


# ---- the Nim imports ----------------------------------------------------------------------------------------------------------
def test_every_importc_of_the_new_shim_matches_the_new_header(L, monkeypatch):
    monkeypatch.setattr(shim, "NIM", NIM)
    src, imports = shim.parse_nim_imports()
    code = "\n".join(line.split("#", 1)[0] for line in src.splitlines())
    assert code.count("importc") == len(imports) == len(NEW)
    protos = {}
    for m in re.finditer(r"([\w ]+?[\w\*]) \*?(laser_hip_\w+) ?\(([^)]*)\) ?;", header_text()):
        ret, name, plist = m.groups()
        protos[name] = {"ret": shim.c_class(ret.strip()),
                        "params": [] if plist.strip() in ("", "void") else [shim.c_class(p) for p in plist.split(",")]}
    assert set(protos) == set(NEW)
    out = subprocess.run(["nm", "-D", "--defined-only", SO_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {imp["sym"] for imp in imports} == set(NEW)
    for imp in imports:
        sym = imp["sym"]
        assert imp["nim"] == sym and sym in exported
        assert imp["params"] == protos[sym]["params"], (sym, imp["params"], protos[sym]["params"])
        assert imp["ret"] == protos[sym]["ret"] == "i32", sym
    assert "`" not in code and not re.findall(r"(?<![\w\"])_\w+", code)
    main = open(os.path.join(ROOT, "nim", "laser_hip.nim")).read()
    assert not any(name in main for name in NEW)
    for proc in ("topk", "argmax", "argmin", "takeRows"):
        assert re.search(r"proc %s\*" % proc, src), proc


# ---- the C++ additions --------------------------------------------------------------------------------------------------------
def test_cpp_mirror_compiles(L, tmp_path):
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "select_mirror.cpp"),
                    "-o", str(tmp_path / "m"), "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    text = open(os.path.join(ROOT, "tests", "cpp", "select_mirror.cpp")).read()
    for fn in ("laser::topk(", "laser::argmax(", "laser::argmin(", "laser::take_rows(", "laser::sample_top_k("):
        assert fn in text, fn


# ---- the stream-order rows ----------------------------------------------------------------------------------------------------
def test_every_dev_entry_point_of_the_header_has_a_stream_order_row():
    declared = set(re.findall(r"\b(laser_hip_\w+)\s*\(", header_text()))
    dev = {s for s in declared if s.endswith("_dev")}
    assert len(dev) == 3, sorted(dev)                                # a new entry point changes this count, and needs a row
    named = {s for c in ROWS.CASES for s in c.symbols}
    assert named == dev, (sorted(dev - named), sorted(named - dev))
    names = [c.name for c in ROWS.CASES]
    assert len(names) == len(set(names)) and not (set(names) & {c.name for c in SO.CASES})
    assert all(isinstance(c, SO.Case) and not c.sync and not c.scratch for c in ROWS.CASES)         # no entry point here takes scratch
    assert not (named & {s for c in SO.CASES for s in c.symbols})    # the main table is as it was


@pytest.mark.parametrize("case", ROWS.CASES, ids=repr)
def test_the_decoy_is_a_valid_input_of_the_same_shapes(L, case):
    from tests.test_stream_order_cpu import test_the_decoy_is_a_valid_input_of_the_same_shapes as check
    import laser_amd
    check(laser_amd, case)
