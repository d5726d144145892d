"""The embedding layer on an MI355X (laser_amd.embedding / embedding_group / embedding_backward; include/laser_hip.h
"Embedding"), bit for bit against tests/embedding_model.py: the gather is a bit copy, the grouping is the stable argsort of the
keys, and dw[v, j] is reduce_model.model_sum of the occurrences of id v in token order.  Bits are compared as uint32 and NaN
positions separately (any NaN equals any NaN).  The draws are made once and sliced; a model result is computed once per case."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import laser_amd
from laser_amd import _lib
from tests import embedding_model as M
from tests import reduce_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(-12345.0)
MAXT, MAXD = 8200, 37                    # (rows wider than 1024, sort tiles above 512, 4 passes, capped grids: test_gpu_grid_stride.py)
INVALID = (-1, -2, 2 ** 31 - 1)          # and `vocab` itself, which depends on the case


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    ok = (got.view(np.uint32) == want.view(np.uint32)) | gn
    if not ok.all():
        bad = np.nonzero(~ok)
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


@functools.lru_cache(maxsize=None)
def draws():
    """dy of the largest shape, read-only: normal draws with exponents spread over about 2^+-8, so that the order of a sum
    shows in its bits"""
    rng = np.random.default_rng(411)
    dy = (rng.normal(0, 1, (MAXT, MAXD)) * 2.0 ** rng.uniform(-8, 8, (MAXT, MAXD))).astype(np.float32)
    dy.setflags(write=False)
    return dy


def table(vocab, dim):
    rng = np.random.default_rng(vocab * 131 + dim)
    return rng.normal(0, 1, (vocab, dim)).astype(np.float32)


def ids_for(tokens, vocab, kind="mixed"):
    rng = np.random.default_rng(tokens * 7 + vocab)
    if kind == "zero":
        return np.zeros(tokens, np.int32)
    idx = rng.integers(0, max(vocab, 1), tokens).astype(np.int32)
    if kind == "mixed" and tokens >= 5:            # some "no draw" entries and some wrong ids, scattered
        idx[rng.integers(0, tokens, max(1, tokens // 20))] = -1
        for k, bad in enumerate((vocab,) + INVALID[1:]):
            idx[(3 + 11 * k) % tokens::max(97, tokens // 7)] = np.int32(bad)
    if kind == "mostly0":                          # one long segment (more than a chunk) and a short one
        idx[:] = 0
        idx[5::3000] = 1
    return idx


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.to_numpy() if hasattr(t, "to_numpy") else t.cpu().numpy()


def plan(tokens, vocab, dim, vec=1):
    out = (C.c_int64 * 8)()
    assert _lib.lib().laser_hip_embedding_plan(tokens, vocab, dim, vec, 256, out) == 0
    return list(out)


def last(what):
    return _lib.lib().laser_hip_embedding_last_kernel(what)


@functools.lru_cache(maxsize=None)
def case(tokens, vocab, dim, kind):
    idx = ids_for(tokens, vocab, kind)
    dy = np.ascontiguousarray(draws()[:tokens, :dim])
    order, starts = M.group(idx, vocab)
    dw = M.grad(dy, idx, vocab, order, starts)
    for a in (idx, dy, order, starts, dw):
        a.setflags(write=False)
    return idx, dy, order, starts, dw


# ---- 1. the shape sweep ------------------------------------------------------------------------------------------------------
SWEEP = ([(0, 5, 7, "mixed"), (1, 1, 1, "mixed"), (5, 3, 1, "mixed"), (64, 7, 3, "mixed")] +
         [(300, 13, d, "mixed") for d in (1, 3, 4, 15, 16, 17, 37)] +                          # strip and vector edges
         [(1500, v, 4, "mixed") for v in (255, 256, 257, 65535, 65536, 65537)] +               # both sides of a pass boundary
         [(4099, 11, 17, "mixed"), (8192 + 5, 2, 20, "mostly0"), (1025, 1, 5, "zero"), (8193, 1, 16, "zero")])


@pytest.mark.parametrize("tokens,vocab,dim,kind", SWEEP)
def test_shape_sweep(tokens, vocab, dim, kind):
    idx, dy, order, starts, want = case(tokens, vocab, dim, kind)
    w = table(vocab, dim)
    didx, ddy, dw_ = dev(idx), dev(dy), dev(w)
    y = laser_amd.embedding(dw_, didx)
    assert tuple(y.shape) == (tokens, dim)
    same_bits(host(y), M.gather(w, idx), "y")
    o, s = laser_amd.embedding_group(didx, vocab)
    assert np.array_equal(host(o), order), "order"
    assert np.array_equal(host(s), starts), "starts"
    p = plan(tokens, vocab, dim)
    if tokens:
        assert last(1) == p[0] == max(1, -(-int(vocab).bit_length() // 8)) and last(3) == p[2]
    got = host(laser_amd.embedding_backward(ddy, didx, vocab))
    same_bits(got, want, f"dw {tokens} {vocab} {dim}")
    vec = int(dim % 4 == 0 or (tokens <= 1 and vocab <= 1))                    # contiguous rows: 16-byte rows or a lone row
    assert last(2) == plan(tokens, vocab, dim, vec)[3] == 1 - vec
    assert np.array_equal(host(ddy).view(np.uint32), dy.view(np.uint32)) and np.array_equal(host(didx), idx)     # inputs untouched
    never = np.diff(starts) == 0
    assert not got[never].view(np.uint32).any()                                # an id that never occurs gets +0
    if kind in ("zero", "mostly0") and vocab == 1:
        db, _ = laser_amd.bias_grad(ddy, dz=False)
        same_bits(got[0], host(db), "vocab = 1, every id 0: the bias gradient's bits")


def test_the_long_segment_takes_the_two_level_fold():
    idx, dy, order, starts, want = case(8192 + 5, 2, 20, "mostly0")
    assert starts[1] - starts[0] > 8192 and 0 < starts[2] - starts[1] <= 32


# ---- 2. id patterns ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["equal", "distinct", "descending", "repeats", "invalid"])
def test_id_patterns(pattern):
    tokens, vocab, dim = 777, 900, 6
    rng = np.random.default_rng(9)
    idx = {"equal": np.full(tokens, 5), "distinct": rng.permutation(vocab)[:tokens], "descending": np.arange(tokens)[::-1] // 3,
           "repeats": rng.integers(0, 40, tokens), "invalid": rng.integers(0, 40, tokens)}[pattern].astype(np.int32)
    if pattern == "invalid":
        idx[::5] = -1
        idx[1::7] = vocab
        idx[2::11] = -2
        idx[3::13] = 2 ** 31 - 1
    dy = np.array(draws()[:tokens, :dim])
    dy[idx == 7] = -0.0
    w = table(vocab, dim)
    didx = dev(idx)
    y = host(laser_amd.embedding(dev(w), didx))
    same_bits(y, M.gather(w, idx), "y")
    ok = (idx >= 0) & (idx < vocab)
    assert not y[idx == -1].view(np.uint32).any()                              # rows of +0
    assert (y[~ok & (idx != -1)].view(np.uint32) == 0x7FC00000).all()          # rows of quiet NaN
    order, starts = M.group(idx, vocab)
    o, s = laser_amd.embedding_group(didx, vocab)
    assert np.array_equal(host(o), order) and np.array_equal(host(s), starts)
    got = host(laser_amd.embedding_backward(dev(dy), didx, vocab))
    same_bits(got, M.grad(dy, idx, vocab), "dw")
    only_valid = host(laser_amd.embedding_backward(dev(dy[ok]), dev(idx[ok]), vocab))
    same_bits(got, only_valid, "tokens with an id outside [0, vocab) contribute nothing")
    assert not got[np.diff(starts) == 0].view(np.uint32).any()
    if (idx == 7).any():
        assert not got[7].view(np.uint32).any()                                # -0 occurrences give +0, a single one included


def test_a_single_negative_zero_occurrence_gives_positive_zero():
    idx = np.array([2, 0, 2], np.int32)
    dy = np.array([[1.5, -0.0], [-0.0, -0.0], [-1.5, 3.0]], np.float32)
    got = host(laser_amd.embedding_backward(dev(dy), dev(idx), 3))
    assert np.array_equal(got.view(np.uint32), np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 3.0]], np.float32).view(np.uint32))


# ---- 3. the data tells a stable grouping from an unstable one ------------------------------------------------------------------
def test_the_gradient_follows_token_order():
    tokens, vocab, dim = 4099, 11, 17
    idx, dy, order, starts, want = case(tokens, vocab, dim, "mixed")
    # precondition, on the CPU: reversing the occurrences of one id changes the model's bits
    v = int(np.argmax(np.diff(starts) >= 3))
    seg = order[starts[v]:starts[v + 1]]
    assert seg.size >= 3
    rev = np.array(order)
    rev[starts[v]:starts[v + 1]] = seg[::-1]
    other = M.grad(dy, idx, vocab, rev, starts)
    assert not np.array_equal(other[v].view(np.uint32), want[v].view(np.uint32)), "the draws cannot tell the order of a sum"
    # the same with a short segment, the one-lane instance's: 3 .. 32 occurrences
    idx2 = np.array(idx[:260]) % 37
    o2, s2 = M.group(idx2, 37)
    w2 = M.grad(dy[:260], idx2, 37, o2, s2)
    changed = 0
    for u in np.nonzero((np.diff(s2) >= 3) & (np.diff(s2) <= 32))[0]:
        r2 = np.array(o2)
        r2[s2[u]:s2[u + 1]] = o2[s2[u]:s2[u + 1]][::-1]
        changed += not np.array_equal(M.grad(dy[:260], idx2, 37, r2, s2)[u].view(np.uint32), w2[u].view(np.uint32))
    assert changed >= 5, "the draws cannot tell the order of a short sum"
    same_bits(host(laser_amd.embedding_backward(dev(dy), dev(idx), vocab)), want, "dw")
    same_bits(host(laser_amd.embedding_backward(dev(dy[:260]), dev(idx2), 37)), w2, "dw, short segments")


# ---- 4. independence -----------------------------------------------------------------------------------------------------------
def padded(a, off, stride):
    rows, n = a.shape
    buf = torch.full((off + rows * stride + 8,), float(SENTINEL), dtype=torch.float32, device="cuda")
    view = torch.as_strided(buf, (rows, n), (stride, 1), off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return buf, view


def padding_untouched(buf, off, rows, n, stride):
    h = buf.cpu().numpy()
    body = h[off:off + rows * stride].reshape(rows, stride)
    return (h[:off] == SENTINEL).all() and (body[:, n:] == SENTINEL).all() and (h[off + rows * stride:] == SENTINEL).all()


def test_a_row_depends_on_its_own_tokens_alone():
    tokens, vocab, dim = 4099, 11, 17
    idx, dy, order, starts, want = case(tokens, vocab, dim, "mixed")
    v = 4
    mine = idx == v
    rng = np.random.default_rng(3)
    # the tokens of the other ids permuted among themselves, some removed, some added; the tokens of id v keep their order
    others = np.nonzero(~mine)[0]
    perm = np.arange(tokens)
    perm[others] = rng.permutation(others)
    keep = np.sort(np.concatenate([np.nonzero(mine)[0], others[::3]]))
    for what, sel in (("permuted", perm), ("removed", keep), ("added", np.concatenate([others[:500], np.arange(tokens)]))):
        got = host(laser_amd.embedding_backward(dev(dy[sel]), dev(idx[sel]), vocab))
        same_bits(got[v], want[v], what)
    # another vocab (one more sort pass) and another dim (the row is a prefix of the columns)
    got = host(laser_amd.embedding_backward(dev(dy), dev(np.where(idx == vocab, 70000, idx).astype(np.int32)), 70000))
    same_bits(got[v], want[v], "vocab 70000")
    got = host(laser_amd.embedding_backward(dev(dy[:, :5]), dev(idx), vocab))
    same_bits(got[v], want[v, :5], "dim 5")
    # another stream
    ddy, didx = dev(dy), dev(idx)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = laser_amd.embedding_backward(ddy, didx, vocab)
    st.synchronize()
    same_bits(host(got), want, "another stream")


@pytest.mark.parametrize("off", [0, 1])
def test_padded_strides_offset_bases_and_both_instances(off):
    """row strides of dim + 3 = 20 (a multiple of 4: the vector instances when the bases are aligned, with the last strip
    partial) and the same one element off the 16-byte alignment (the single-element instances): same bits, padding untouched"""
    tokens, vocab, dim = 4099, 11, 17
    idx, dy, order, starts, want = case(tokens, vocab, dim, "mixed")
    stride = dim + 3
    w = table(vocab, dim)
    didx = dev(idx)
    bdy, vdy = padded(dy, off, stride)
    bdw, vdw = padded(np.zeros((vocab, dim), np.float32), off, stride)
    assert vdy.data_ptr() % 16 == 4 * off
    out = laser_amd.embedding_backward(vdy, didx, vocab, out=vdw)
    assert out is vdw and last(2) == plan(tokens, vocab, dim, 1 - off)[3] == off
    same_bits(host(vdw), want, "dw")
    assert padding_untouched(bdw, off, vocab, dim, stride) and padding_untouched(bdy, off, tokens, dim, stride)
    bw, vw = padded(w, off, stride)
    by, vy = padded(np.zeros((tokens, dim), np.float32), off, stride)
    laser_amd.embedding(vw, didx, out=vy)
    assert last(0) == off
    same_bits(host(vy), M.gather(w, idx), "y")
    assert padding_untouched(by, off, tokens, dim, stride) and padding_untouched(bw, off, vocab, dim, stride)


def test_both_instances_on_whole_strips():
    """dim = 16: whole strips and 16-byte rows -> the vector instances; the same values one element further -> single elements"""
    tokens, vocab, dim = 8192 + 5, 2, 16
    idx, dy, order, starts, want = case(tokens, vocab, dim, "mostly0")
    for off in (0, 1):
        _, vdy = padded(dy, off, dim)
        got = laser_amd.embedding_backward(vdy, dev(idx), vocab)
        assert last(2) == off
        same_bits(host(got), want, f"off {off}")


# ---- 5. special values ---------------------------------------------------------------------------------------------------------
def test_a_nan_and_an_inf_reach_one_element_each():
    tokens, vocab, dim = 4099, 11, 17
    idx, dy, order, starts, want = case(tokens, vocab, dim, "mixed")
    dy = np.array(dy)
    tn = int(np.nonzero(idx == 3)[0][40])
    ti = int(np.nonzero(idx == 9)[0][0])
    dy[tn, 5] = np.nan
    dy[ti, 16] = np.inf
    got = host(laser_amd.embedding_backward(dev(dy), dev(idx), vocab))
    assert np.isnan(got[3, 5]) and got[9, 16] == np.inf
    mask = np.ones_like(got, bool)
    mask[3, 5] = mask[9, 16] = False
    assert np.isfinite(got[mask]).all()
    same_bits(got[mask], want[mask], "every other element is that of the clean input")
    # the short-segment instance: a NaN in one column of one id
    idx2 = (np.arange(300) % 60).astype(np.int32)
    dy2 = np.array(draws()[:300, :8])
    dy2[61, 2] = np.nan
    got2 = host(laser_amd.embedding_backward(dev(dy2), dev(idx2), 60))
    assert np.isnan(got2[1, 2]) and np.isnan(got2).sum() == 1
    same_bits(got2, M.grad(dy2, idx2, 60), "short segments")


def test_the_forward_pass_copies_nan_payloads_and_negative_zero():
    vocab, dim = 6, 9
    bits = np.arange(vocab * dim, dtype=np.uint32).reshape(vocab, dim) * np.uint32(2654435761)
    bits[1, :] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF800000, 0x80000000, 0x00000001, 0x80000001, 0x7FFFFFFF, 0]
    w = bits.view(np.float32)
    idx = np.array([[1, 5, 1], [0, 1, 3]], np.int32)
    y = laser_amd.embedding(dev(w), dev(idx))
    assert tuple(y.shape) == (2, 3, dim)
    assert np.array_equal(host(y).view(np.uint32), bits[idx])


# ---- 6. the pre-grouped form and the plan ----------------------------------------------------------------------------------------
def test_a_group_given_has_the_bits_of_the_self_grouping_call():
    tokens, vocab, dim = 4099, 11, 17
    idx, dy, order, starts, want = case(tokens, vocab, dim, "mixed")
    didx, ddy = dev(idx), dev(dy)
    g = laser_amd.embedding_group(didx, vocab)
    same_bits(host(laser_amd.embedding_backward(ddy, didx, vocab, group=g)), want, "pre-grouped")
    same_bits(host(laser_amd.embedding_backward(ddy[:, :4], didx, vocab, group=g)), want[:, :4], "the same group, another table")


def test_the_plan_agrees_with_what_was_launched():
    for tokens, vocab, dim in ((1500, 255, 4), (1500, 256, 4), (1500, 65536, 4), (3000, 1 << 24, 1)):
        idx = ids_for(tokens, vocab)
        o, s = laser_amd.embedding_group(dev(idx), vocab)
        p = plan(tokens, vocab, dim)
        assert (last(1), last(3)) == (p[0], p[2]), (tokens, vocab)
        order, starts = M.group(idx, vocab)
        assert np.array_equal(host(o), order) and np.array_equal(host(s), starts)
    assert plan(1500, 255, 4)[0] == 1 and plan(1500, 256, 4)[0] == 2 and plan(1500, 65536, 4)[0] == 3 and plan(3000, 1 << 24, 1)[0] == 4


# ---- 7. a training loop ----------------------------------------------------------------------------------------------------------
def train(steps=30, lr=0.5):
    """A bag-of-tokens classifier: 48 samples of 6 token ids out of 40, an embedding of 8 columns summed over the positions
    (a product with the 0 / 1 pooling matrix), a dense layer to 3 classes; labels from a fixed rule on the token counts."""
    S, T, V, D, Cn = 48, 6, 40, 8, 3
    rng = np.random.default_rng(77)
    ids = rng.integers(0, V, (S, T)).astype(np.int32)
    counts = np.zeros((S, V))
    for s_ in range(S):
        np.add.at(counts[s_], ids[s_], 1)
    labels = np.argmax(counts @ rng.normal(0, 1, (V, Cn)), axis=1).astype(np.int32)
    pool = np.kron(np.eye(S, dtype=np.float32), np.ones((1, T), np.float32))            # (S, S * T)
    I, lab, P = laser_amd.toTensor(ids.reshape(-1)), laser_amd.toTensor(labels), laser_amd.toTensor(pool)
    W = {"e": laser_amd.toTensor(rng.normal(0, 0.5, (V, D)).astype(np.float32)),
         "w": laser_amd.toTensor(rng.normal(0, 0.5, (D, Cn)).astype(np.float32)), "b": laser_amd.toTensor(np.zeros(Cn, np.float32))}
    lr = np.float32(lr)
    group = laser_amd.embedding_group(I, V)
    losses = []
    for _ in range(steps):
        e = laser_amd.embedding(W["e"], I)                                                # (S * T, D)
        h = laser_amd.matmul(P, e)                                                        # the sum over the positions
        logits = laser_amd.matmul(h, W["w"], bias=W["b"])
        loss, g = laser_amd.softmax_cross_entropy(logits, lab, grad=True, scale=1.0 / S)
        dh, dw, db = laser_amd.linear_backward(h, W["w"], g)
        de = laser_amd.matmul(P.T, dh)
        dE = laser_amd.embedding_backward(de, I, V, group=group)
        for name, grad in (("e", dE), ("w", dw), ("b", db)):
            laser_amd.forEach("w -= lr * g", w=W[name], g=grad, params={"lr": lr})
        losses.append(loss.to_numpy())
    return np.stack(losses), {k: v.to_numpy() for k, v in W.items()}


def test_a_bag_of_tokens_classifier_trains_on_the_device_and_repeats_bit_for_bit():
    l1, p1 = train()
    l2, p2 = train()
    assert l1.shape == (30, 48) and np.isfinite(l1).all()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32))
    for k in p1:
        assert np.array_equal(p1[k].view(np.uint32), p2[k].view(np.uint32)), k
    mean = l1.astype(np.float64).mean(axis=1)
    print("mean loss, first and last step:", mean[0], mean[-1])
    assert mean[-1] < mean[0]                                     # a sanity condition, not a measurement


# ---- the C++ mirror ------------------------------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "embedding_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "laser_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "embedding_mirror.cpp"),
                    "-o", exe, "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr
