"""Row top-k, argmax / argmin, take_rows and top-k sampling on an MI355X (include/laser_hip_select.h) against the numpy model
of tests/select_model.py, by exact equality: values as uint32 bits, indices as int32.  Every n on both sides of every
threshold of laser_amd/csrc/select_plan.h, every data class, source rows with gaps of positive NaN (the largest key: a kernel
that reads a gap selects it), output rows with gaps of a sentinel that must survive, a base one element off the alignment so
that the single-element kernels run, and laser_hip_topk_last_kernel() held against the plan in every case."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import exp_model
from tests import scan_model
from tests import select_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_constant(name):
    text = open(os.path.join(ROOT, "laser_amd", "csrc", "select_plan.h")).read()
    return int(re.search(r"#define " + name + r" (\d+)", text).group(1))


WAVE_N, RESIDENT_N, CAP, CHUNK = (plan_constant("LH_SELECT_" + k) for k in ("WAVE_N", "RESIDENT_N", "MAX_WORKGROUPS", "COLLECT_CHUNK"))
N_GRID = sorted({1, 2, 63, 64, 65, 70001} | {t + d for t in (WAVE_N, RESIDENT_N) for d in (-1, 0, 1)})
NAN_WORD = 0x7FC00000          # the gaps and tails of a source: positive NaN
SENT_VALS, SENT_IDX = 0x5EA1ED00, -77


@pytest.fixture(scope="module")
def la():
    import torch
    import laser_amd
    assert torch.cuda.is_available()
    return laser_amd


def ks_of(n):
    return sorted({k for k in (1, 2, 7, 64, 65, min(n, M.MAX_K)) if k <= n})


def stream():
    from laser_amd.tensor import _stream
    return _stream()


def ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + 4 * offset)


class Source:
    """rows of x on the device with a row stride above n; the gaps, the head and the tail hold positive NaN.  offset = 1 puts
    the base one element off the 16-byte alignment."""

    def __init__(self, x, offset=0, stride=None):
        import torch
        self.x = np.ascontiguousarray(x, np.float32)
        self.rows, self.n = self.x.shape
        self.offset = offset
        self.stride = stride if stride is not None else (self.n + 4) // 4 * 4          # > n, a multiple of 4
        host = np.full(8 + self.rows * self.stride + 8, NAN_WORD, np.uint32)
        for r in range(self.rows):
            at = 8 + offset + r * self.stride
            host[at:at + self.n] = M.bits(self.x[r])
        self.buf = torch.from_numpy(host.view(np.int32)).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.vec = offset % 4 == 0 and (self.rows <= 1 or self.stride % 4 == 0)

    def ptr(self):
        return ptr(self.buf, 8 + self.offset)


def device_topk(la, src, k, largest=True, want="both", pad=3):
    """(values as uint32, indices) of laser_hip_topk_rows_f32_dev on padded outputs, with every check that needs no model:
    the return code, the kernel against the plan, the sentinels"""
    import torch
    L = la.lib()
    rows, os_ = src.rows, k + pad
    vals = torch.full((rows * os_ + 8,), SENT_VALS, dtype=torch.int32, device="cuda") if want in ("both", "values") else None
    idx = torch.full((rows * os_ + 8,), SENT_IDX, dtype=torch.int32, device="cuda") if want in ("both", "indices") else None
    rc = L.laser_hip_topk_rows_f32_dev(ptr(vals) if vals is not None else None, os_, ptr(idx) if idx is not None else None, os_, src.ptr(),
                                       src.stride, rows, src.n, k, 1 if largest else 0, stream())
    assert rc == 0, L.laser_hip_last_error()
    assert L.laser_hip_topk_last_kernel() == la.topk_plan(rows, src.n, k, src.vec)[0], (rows, src.n, k, src.vec)
    out = []
    for t, sent in ((vals, SENT_VALS), (idx, SENT_IDX)):
        if t is None:
            out.append(None)
            continue
        h = t.cpu().numpy()
        body = h[:rows * os_].reshape(rows, os_)
        assert (body[:, k:] == sent).all() and (h[rows * os_:] == sent).all(), "a sentinel beside the results was overwritten"
        out.append(body[:, :k].copy())
    return (out[0].view(np.uint32) if out[0] is not None else None), out[1]


def check_topk(la, src, ref, k, largest, want="both"):
    vals, idx = device_topk(la, src, k, largest, want)
    wv, wi = ref
    what = (src.rows, src.n, k, largest, src.offset, want)
    if idx is not None:
        assert np.array_equal(idx, wi[:, :k]), what
    if vals is not None:
        assert np.array_equal(vals, M.bits(wv[:, :k])), what
    return vals, idx


def test_the_grid_brackets_every_threshold_of_the_plan(la):
    codes = {n: la.topk_plan(1, n, 1)[0] for n in range(1, 2 * RESIDENT_N)}
    switches = [n for n in range(1, 2 * RESIDENT_N - 1) if codes[n] != codes[n + 1]]
    assert switches == [WAVE_N, RESIDENT_N]
    assert la.topk_plan(1, 1 << 24, 1)[0] == codes[RESIDENT_N + 1] == 2
    for t in switches:
        assert {t - 1, t, t + 1} <= set(N_GRID)
    assert {la.topk_plan(1, n, 1)[0] for n in N_GRID} == {0, 1, 2}
    assert 70001 % 4 != 0 and 70001 > 2 * CHUNK


@pytest.mark.parametrize("n", N_GRID)
def test_topk_equals_the_model_for_every_data_class(la, n):
    for rows in (1, 3, 5):
        for kind in M.KINDS:
            x = M.data(kind, rows, n, seed=1)
            src = Source(x)
            for largest in (True, False):
                ref = M.topk(x, min(n, M.MAX_K), largest)          # the first k of it for every smaller k
                for k in ks_of(n):
                    check_topk(la, src, ref, k, largest)


@pytest.mark.parametrize("n", N_GRID)
def test_topk_off_the_alignment_runs_the_single_element_kernels(la, n):
    for kind in ("normal", "three", "special"):
        x = M.data(kind, 3, n, seed=2)
        for src in (Source(x, offset=1), Source(x, stride=n + 1 + (n % 4 == 3))):       # the base, then the row stride
            assert not src.vec and src.stride > n
            for largest in (True, False):
                ref = M.topk(x, min(n, M.MAX_K), largest)
                for k in ks_of(n):
                    check_topk(la, src, ref, k, largest)
                    assert la.lib().laser_hip_topk_last_kernel() >= 4


@pytest.mark.parametrize("n", N_GRID)
def test_a_result_does_not_depend_on_what_else_is_asked_for(la, n):
    for kind in ("normal", "three"):
        x = M.data(kind, 3, n, seed=3)
        src = Source(x)
        for largest in (True, False):
            ref = M.topk(x, min(n, M.MAX_K), largest)
            for k in ks_of(n):
                check_topk(la, src, ref, k, largest, "values")
                check_topk(la, src, ref, k, largest, "indices")


def test_more_rows_than_one_trip_of_the_capped_grid(la):
    rows, n = 4 * CAP + 3, 5
    assert la.topk_plan(rows, n, 1)[:2] == (0, CAP) and la.topk_plan(rows - 3, n, 1)[1] == CAP
    for kind in ("normal", "three"):
        x = M.data(kind, rows, n, seed=4)
        src = Source(x)
        for largest in (True, False):
            ref = M.topk(x, n, largest)
            for k in (1, 2, 5):
                check_topk(la, src, ref, k, largest)


def test_more_rows_than_one_trip_of_the_workgroup_kernels(la):
    """one row per workgroup: CAP + 2 rows of the shortest resident and the shortest streaming row run a second trip too"""
    for n in (WAVE_N + 1, RESIDENT_N + 1):
        rows = CAP + 2
        x = M.data("three", rows, n, seed=5)
        x[:, ::7] = M.data("normal", rows, n, seed=5)[:, ::7]
        src = Source(x)
        assert la.topk_plan(rows, n, 7)[1] == CAP
        check_topk(la, src, M.topk(x, 7, True), 7, True)


@pytest.mark.parametrize("n,at", [(1100, 1024), (RESIDENT_N, 1024), (RESIDENT_N, 4096), (RESIDENT_N + 108, 1024), (RESIDENT_N + 108, CHUNK),
                                  (RESIDENT_N + 108, 8192), (3 * CHUNK + 50, 2 * CHUNK + 1024), (3 * CHUNK + 50, 3 * CHUNK)])
def test_a_tie_group_across_the_kth_rank_and_a_chunk_boundary(la, n, at):
    for k in (7, 64, 65, 1024):
        x = M.straddle(n, k, at, seed=k)
        ref, wrong = M.topk(x, k, True), M.topk(x, k, True, ties_by_highest_index=True)
        assert not np.array_equal(ref[1], wrong[1]), "the fixture does not discriminate"
        taken = ref[1][0, -5:]
        assert taken.min() < at <= taken.max(), "the tie pick does not reach across the boundary"
        for src in (Source(x), Source(x, offset=1)):
            check_topk(la, src, ref, k, True)
        neg = -x                                                     # the same group for the smallest
        check_topk(la, Source(neg), M.topk(neg, k, False), k, False)


def test_special_values_rank_as_the_header_says(la):
    x = np.tile(M.SPECIALS, 2)[None, :].copy()                       # every special value twice: ties at every key
    n = x.shape[1]
    ref = M.topk(x, n, True)
    vals, idx = check_topk(la, Source(x), ref, n, True)
    assert vals[0, 0] == 0x7FFFFFFF and idx[0, 0] == len(M.SPECIALS) - 1 and idx[0, 1] == 2 * len(M.SPECIALS) - 1
    assert vals[0, -1] == 0xFFFFFFFF and idx[0, -1] == len(M.SPECIALS)
    zeros = np.float32([[0.0, -0.0, 0.0, -0.0]])
    vals, idx = check_topk(la, Source(zeros), M.topk(zeros, 4, True), 4, True)
    assert idx.tolist() == [[0, 2, 1, 3]] and vals.tolist() == [[0, 0, 0x80000000, 0x80000000]]
    vals, idx = check_topk(la, Source(zeros), M.topk(zeros, 4, False), 4, False)
    assert idx.tolist() == [[1, 3, 0, 2]]


@pytest.mark.parametrize("n", N_GRID)
def test_argmax_and_argmin_equal_topk_with_k_1(la, n):
    import torch
    L = la.lib()
    for rows in (1, 3, 5):
        for kind in M.KINDS:
            x = M.data(kind, rows, n, seed=6)
            for src in (Source(x), Source(x, offset=1)):
                for largest in (True, False):
                    idx = torch.full((rows * 3 + 4,), SENT_IDX, dtype=torch.int32, device="cuda")
                    val = torch.full((rows * 2 + 4,), SENT_VALS, dtype=torch.int32, device="cuda")
                    assert L.laser_hip_argmax_rows_f32_dev(ptr(idx), 3, ptr(val), 2, src.ptr(), src.stride, rows, n, 1 if largest else 0,
                                                           stream()) == 0, L.laser_hip_last_error()
                    assert L.laser_hip_topk_last_kernel() == la.topk_plan(rows, n, 1, src.vec)[0] + 8
                    hi, hv = idx.cpu().numpy(), val.cpu().numpy()
                    want = M.argmax(x, largest)
                    what = (rows, n, kind, largest, src.offset)
                    assert np.array_equal(hi[:rows * 3:3], want), what
                    assert np.array_equal(hv[:rows * 2:2].view(np.uint32), M.bits(x[np.arange(rows), want])), what
                    keep = np.ones(hi.shape, bool)
                    keep[:rows * 3:3] = False
                    assert (hi[keep] == SENT_IDX).all()
                    keep = np.ones(hv.shape, bool)
                    keep[:rows * 2:2] = False
                    assert (hv[keep] == SENT_VALS).all()


def test_the_python_mirror_takes_views_and_higher_ranks(la):
    import torch
    x = M.data("normal", 6, 300, seed=7)
    t = torch.from_numpy(x).cuda()
    vals, idx = la.topk(t.view(2, 3, 300), 9)
    assert vals.shape == (2, 3, 9) and idx.shape == (2, 3, 9)
    wv, wi = M.topk(x, 9)
    assert M.same_bits(vals.to_numpy().reshape(6, 9), wv) and np.array_equal(idx.to_numpy().reshape(6, 9), wi)
    assert np.array_equal(la.argmax(t.view(2, 3, 300)).to_numpy(), M.argmax(x).reshape(2, 3))
    assert np.array_equal(la.argmin(t).to_numpy(), M.argmax(x, False))
    view = t[:, 10:110]                                               # a view: row stride 300, base off the alignment
    wv, wi = M.topk(x[:, 10:110], 5, False)
    vals, idx = la.topk(view, 5, largest=False)
    assert M.same_bits(vals.to_numpy(), wv) and np.array_equal(idx.to_numpy(), wi)
    only = la.topk(view, 5, largest=False, values=False)
    assert only[0] is None and np.array_equal(only[1].to_numpy(), wi)
    with pytest.raises(ValueError):
        la.topk(t.T, 2)
    with pytest.raises(ValueError):
        la.topk(t, 301)


def test_take_rows_gathers_and_marks_what_is_outside(la):
    import torch
    L = la.lib()
    rng = np.random.default_rng(8)
    for rows, m, num in ((1, 1, 1), (3, 50, 7), (5, 1024, 300), (CAP + 3, 9, 130)):
        src = rng.integers(-2**31, 2**31 - 1, (rows, m)).astype(np.int32)
        j = rng.integers(-3, m + 3, (rows, num)).astype(np.int32)
        j[0, 0] = -2**31
        want = M.take_rows(src, j)
        assert (want == -1).any() or m == 1
        ss, js, os_ = m + 2, num + 1, num + 3
        hs, hj = np.full((rows, ss), 12345, np.int32), np.full((rows, js), 0, np.int32)
        hs[:, :m], hj[:, :num] = src, j
        ds, dj = torch.from_numpy(hs).cuda(), torch.from_numpy(hj).cuda()
        out = torch.full((rows * os_ + 4,), SENT_IDX, dtype=torch.int32, device="cuda")
        assert L.laser_hip_take_rows_i32_dev(ptr(out), os_, ptr(ds), ss, ptr(dj), js, rows, m, num, stream()) == 0, L.laser_hip_last_error()
        h = out.cpu().numpy()
        body = h[:rows * os_].reshape(rows, os_)
        assert np.array_equal(body[:, :num], want), (rows, m, num)
        assert (body[:, num:] == SENT_IDX).all() and (h[rows * os_:] == SENT_IDX).all()
        assert np.array_equal(la.take_rows(torch.from_numpy(src).cuda(), torch.from_numpy(j).cuda()).to_numpy(), want)


def test_sample_top_k_is_the_composition_of_the_models(la):
    import torch
    rng = np.random.default_rng(9)
    rows, n, k, num = 5, 9000, 50, 16
    logits = rng.normal(0, 3, (rows, n)).astype(np.float32)
    logits[1, :200] = logits[1, 0]                                   # a tie group among the candidates
    t = torch.from_numpy(logits).cuda()
    wv, wi = M.topk(logits, k)
    cdf = scan_model.cumsum(exp_model.softmax_rows(wv))

    def model(u):
        return M.take_rows(wi, scan_model.draw(cdf, u))

    u = rng.random((rows, num), dtype=np.float32)
    got = la.sample_top_k(t, k, num, u=u).to_numpy()
    assert got.shape == (rows, num) and got.dtype == np.int32 and np.array_equal(got, model(u))
    assert len(np.unique(got)) > rows and all(set(got[r]) <= set(wi[r]) for r in range(rows))
    # the generator: the uniform numbers of a fill from the same (seed, subseq, offset), and the stream advances
    g = la.Rng(5, 1, 7)
    ubuf = la.newTensor(np.float32, rows, num)
    assert la.lib().laser_hip_random_uniform_f32_dev(C.c_void_p(ubuf.unsafe_raw_data()), rows * num, 0.0, 1.0, 5, 1, 7, stream()) == 0
    got = la.sample_top_k(t, k, num, rng=g).to_numpy()
    assert g.offset == 7 + rows * num and np.array_equal(got, model(ubuf.to_numpy()))
    # k = 1 is argmax, whatever the uniform numbers
    assert np.array_equal(la.sample_top_k(t, 1, 3, u=u[:, :3]).to_numpy(), np.repeat(M.argmax(logits)[:, None], 3, axis=1))
    assert np.array_equal(la.sample_top_k(t, 1).to_numpy()[:, 0], la.argmax(t).to_numpy())
    with pytest.raises(ValueError):
        la.sample_top_k(t, k, num, u=u, rng=la.Rng(1))


def test_accuracy_from_the_device_argmax_equals_numpy(la):
    import torch
    rng = np.random.default_rng(10)
    rows, classes = 4099, 1000
    logits = rng.normal(0, 1, (rows, classes)).astype(np.float32)
    labels = rng.integers(0, classes, rows)
    logits[np.arange(rows)[::2], labels[::2]] += 6.0                 # about half of the rows are right
    pred = la.argmax(torch.from_numpy(logits).cuda()).to_numpy()
    accuracy = float((pred == labels).mean())
    assert accuracy == float((np.argmax(logits, axis=1) == labels).mean()) and 0.4 < accuracy < 0.6


def test_the_cpp_mirror_from_a_compiled_caller(la, tmp_path):
    """laser::topk / argmax / argmin / take_rows / sample_top_k of include/laser.hpp (tests/cpp/select_mirror.cpp)"""
    import subprocess
    lib = os.path.join(ROOT, "laser_amd", "lib")
    exe = str(tmp_path / "select_mirror")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "select_mirror.cpp"),
                    "-o", exe, "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
