"""The optimizer steps on the device (include/laser_hip.h "Optimizer steps") against the numpy model (tests/optim_model.py),
bit for bit, any NaN equal to any NaN: the length sweep in every variant, several steps with the state on the device, base
alignments, the grouping of a list into calls and launches, lists past the cap of 2048 workgroups, equality with forEach,
isolation of NaN and Inf with sentinels round every tensor, the gradient norm's sums and edges, the C++ mirror and a small
network trained on two streams."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

import laser_amd
from laser_amd import _lib
from tests import optim_model as M
from tests import reduce_model as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LENS = [0, 1, 3, 4, 5, 255, 257, 4095, 4096, 4097, 8191, 8192, 8193, 16389]     # vector, chunk and reduction-chunk edges
SENTINEL = F(-12345.0)
GAP = 8                                                                          # sentinels between two tensors (floats)
CHUNK, CAP = 4096, 2048
PERIOD, NAN_AT = 13, 4


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not M.same_bits(got, want):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    return t.to_numpy() if hasattr(t, "to_numpy") else t.cpu().numpy()


class Arena:
    """The tensors of one list in one device buffer, sentinels before, between and after them; tensor k starts `off[k]` floats
    past a 16-byte boundary.  `flat` is the concatenation of the tensors' values (the model is elementwise, so it runs on it)."""

    def __init__(self, lens, flat, off=0):
        self.lens = list(lens)
        offs = [off] * len(self.lens) if np.isscalar(off) else list(off)
        self.starts, at = [], GAP
        for n, o in zip(self.lens, offs):
            at = -(-at // 4) * 4 + o
            self.starts.append(at)
            at += n + GAP
        self.size = -(-at // 4) * 4 + GAP
        image = np.full(self.size, SENTINEL, F)
        self.mask = np.ones(self.size, bool)                       # True where a sentinel must stay
        pos = 0
        for n, s in zip(self.lens, self.starts):
            image[s:s + n] = flat[pos:pos + n]
            self.mask[s:s + n] = False
            pos += n
        assert pos == flat.size
        self.buf = torch.from_numpy(image).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.views = [self.buf[s:s + n] for n, s in zip(self.lens, self.starts)]

    def read(self, what=""):
        """the concatenation of the tensors as they are now; the sentinels must be untouched"""
        image = self.buf.cpu().numpy()
        assert (image[self.mask].view(np.uint32) == SENTINEL.view(np.uint32)).all(), f"{what}: a sentinel was overwritten"
        return np.concatenate([image[s:s + n] for n, s in zip(self.lens, self.starts)]) if self.lens else np.zeros(0, F)


@functools.lru_cache(maxsize=None)
def draws(n, seed=11):
    """(w, g, m, v) of n elements, read-only: normal values with a few zeros of both signs, subnormals and large values"""
    rng = np.random.default_rng(seed)
    w, g, m = (rng.normal(0, s, n).astype(F) for s in (1.0, 0.1, 0.05))
    v = rng.normal(0, 0.05, n).astype(F) ** 2
    for k, a in enumerate((w, g, m, v)):
        for j, s in enumerate(F([0.0, -0.0, 1e-45, 1e-39, 3e38])):
            a[(7 * k + 11 * j) % n::997] = s
    for a in (w, g, m, v):
        a.setflags(write=False)
    return w, g, m, v


def clip_tensor(value):
    return None if value is None else dev(F([value]))


SGD_VARIANTS = {"plain": dict(), "momentum": dict(mu=0.9, has_m=True), "nesterov": dict(mu=0.9, has_m=True, nesterov=True),
                "wd": dict(wd=0.01), "gscale": dict(gscale=1 / 128), "clip": dict(clip=0.37, mu=0.5, has_m=True),
                "mu0-with-list": dict(mu=0.0, has_m=True)}
ADAM_VARIANTS = {"coupled": dict(wd=0.01), "decoupled": dict(wd=0.01, decoupled=True), "clip": dict(clip=0.37, gscale=1 / 128),
                 "eps0": dict(eps=0.0), "plain": dict()}


def run_sgd(lens, data, kw, off=0, lr=0.1, what=""):
    """one SGD step on the device over arenas built from `data`; returns (w, m) flat, sentinels checked"""
    kw = dict(kw)
    has_m, clip = kw.pop("has_m", False), kw.pop("clip", None)
    aw, ag, am = (Arena(lens, a, off) for a in data[:3])
    laser_amd.sgd_step(aw.views, ag.views, am.views if has_m else None, lr=lr, clip=clip_tensor(clip), **kw)
    same_bits(ag.read(what), data[1], what + " g is not written")
    return aw.read(what), am.read(what)


def model_sgd(data, kw, lr=0.1):
    kw = dict(kw)
    has_m = kw.pop("has_m", False)
    w, m = M.sgd(data[0], data[1], data[2] if has_m else None, lr=lr, **kw)
    return w, (m if has_m else data[2])


def run_adam(lens, data, kw, step=3, off=0, lr=1e-2, what=""):
    kw = dict(kw)
    clip = kw.pop("clip", None)
    aw, ag, am, av = (Arena(lens, a, off) for a in data)
    laser_amd.adam_step(aw.views, ag.views, am.views, av.views, step, lr=lr, clip=clip_tensor(clip), **kw)
    same_bits(ag.read(what), data[1], what + " g is not written")
    return aw.read(what), am.read(what), av.read(what)


# ---- 1. the length sweep, every variant ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(SGD_VARIANTS))
def test_sgd_length_sweep(variant):
    data = draws(sum(LENS))
    kw = SGD_VARIANTS[variant]
    got = run_sgd(LENS, data, kw, what=variant)
    want = model_sgd(data, kw)
    same_bits(got[0], want[0], f"sgd {variant} w")
    same_bits(got[1], want[1], f"sgd {variant} m")


@pytest.mark.parametrize("variant", list(ADAM_VARIANTS))
def test_adam_length_sweep(variant):
    data = draws(sum(LENS))
    kw = ADAM_VARIANTS[variant]
    got = run_adam(LENS, data, kw, what=variant)
    want = M.adam(*data, 3, lr=1e-2, **kw)
    for name, a, b in zip("wmv", got, want):
        same_bits(a, b, f"adam {variant} {name}")


# ---- 2. several steps, the state on the device -----------------------------------------------------------------------------------
def test_five_steps_carry_the_state_on_the_device():
    lens = [5, 4097, 0, 300]
    n = sum(lens)
    w0 = draws(n)[0]
    rng = np.random.default_rng(5)
    grads = [rng.normal(0, 0.1, n).astype(F) for _ in range(5)]
    zeros = np.zeros(n, F)
    # SGD with momentum and Nesterov through the state holder
    aw = Arena(lens, w0)
    opt = laser_amd.SGD(aw.views, lr=0.05, mu=0.9, wd=1e-3, nesterov=True)
    w, m = w0, zeros
    for g in grads:
        opt.step(Arena(lens, g).views)
        w, m = M.sgd(w, g, m, lr=0.05, mu=0.9, wd=1e-3, nesterov=True)
    same_bits(aw.read("sgd"), w, "five SGD steps, w")
    same_bits(np.concatenate([host(t).reshape(-1) for t in opt.momentum]), m, "five SGD steps, m")
    assert opt.steps == 5
    # Adam through the state holder: the bias corrections of steps 1 .. 5
    aw = Arena(lens, w0)
    opt = laser_amd.Adam(aw.views, lr=1e-2, wd=1e-2, decoupled=True)
    w, m, v = w0, zeros, zeros
    for t, g in enumerate(grads, 1):
        opt.step(Arena(lens, g).views)
        w, m, v = M.adam(w, g, m, v, t, lr=1e-2, wd=1e-2, decoupled=True)
    same_bits(aw.read("adam"), w, "five Adam steps, w")
    same_bits(np.concatenate([host(t).reshape(-1) for t in opt.m]), m, "five Adam steps, m")
    same_bits(np.concatenate([host(t).reshape(-1) for t in opt.v]), v, "five Adam steps, v")
    assert opt.steps == 5


# ---- 3. base alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 2, 3, "mixed"])
def test_offset_bases_give_the_same_bits(off):
    lens = [1, 5, 257, 4097, 8193, 0, 4096]
    data = draws(sum(lens))
    offs = [0, 1, 0, 3, 2, 1, 0] if off == "mixed" else off          # mixed: aligned and misaligned tensors in one call
    kw = SGD_VARIANTS["nesterov"]
    got = run_sgd(lens, data, kw, off=offs, what=f"off {off}")
    want = model_sgd(data, kw)
    same_bits(got[0], want[0], "w")
    same_bits(got[1], want[1], "m")
    got = run_adam(lens, data, ADAM_VARIANTS["coupled"], off=offs, what=f"off {off}")
    for name, a, b in zip("wmv", got, M.adam(*data, 3, lr=1e-2, **ADAM_VARIANTS["coupled"])):
        same_bits(a, b, f"adam {name}")
    if off == "mixed":                                                   # one operand of a tensor off its alignment is enough
        aw, ag, am, av = (Arena(lens, a, o) for a, o in zip(data, (0, 0, 0, [0, 0, 0, 2, 0, 0, 0])))
        laser_amd.adam_step(aw.views, ag.views, am.views, av.views, 3, lr=1e-2, **ADAM_VARIANTS["coupled"])
        for name, a, b in zip("wmv", (aw, am, av), M.adam(*data, 3, lr=1e-2, **ADAM_VARIANTS["coupled"])):
            same_bits(a.read(), b, f"adam, v alone misaligned, {name}")


# ---- 4. grouping: one per call, all in one call, reversed ------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 64, 65, 129])
def test_grouping_into_calls_and_launches_changes_no_bit(count):
    rng = np.random.default_rng(count)
    lens = [int(n) for n in rng.integers(5, 301, count)]
    data = draws(sum(lens))
    kw = dict(wd=0.01)
    want = M.adam(*data, 2, lr=1e-2, **kw)
    out = (C.c_int64 * 4)()
    assert _lib.lib().laser_hip_optim_plan(1, (C.c_int64 * count)(*lens), count, out) == 0 and out[0] == -(-count // 64)

    def run(order):
        arenas = [Arena(lens, a) for a in data]
        for group in order:
            laser_amd.adam_step(*([a.views[k] for k in group] for a in arenas), 2, lr=1e-2, **kw)
        return [a.read() for a in (arenas[0], arenas[2], arenas[3])]

    together = run([list(range(count))])
    for name, a, b in zip("wmv", together, want):
        same_bits(a, b, f"all in one call, {name}")
    for name, a, b in zip("wmv", run([list(range(count))[::-1]]), together):
        same_bits(a, b, f"reversed list, {name}")
    for name, a, b in zip("wmv", run([[k] for k in range(count)]), together):
        same_bits(a, b, f"one tensor per call, {name}")


# ---- 5. past the cap of 2048 workgroups --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiled_base():
    """13 base chunks of 4096 elements for w, g, m, v, chunk k scaled by 2^(k - 6), one g chunk with a NaN; and their model under
    Adam and SGD with momentum.  A tensor built by tiling them has chunk i = base chunk i mod 13, so a wrapped chunk changes bits."""
    rng = np.random.default_rng(13)
    scale = (2.0 ** (np.arange(PERIOD) - 6)).astype(F)[:, None]
    w, g, m = (rng.normal(0, s, (PERIOD, CHUNK)).astype(F) * scale for s in (1.0, 0.1, 0.05))
    v = (rng.normal(0, 0.05, (PERIOD, CHUNK)).astype(F) * scale) ** 2
    g[NAN_AT, CHUNK // 2] = np.nan
    adam = M.adam(w, g, m, v, 2, lr=1e-2, wd=0.01)
    sgd = M.sgd(w, g, m, lr=0.1, mu=0.9)
    keys = {a.tobytes() for a in adam[0]}
    assert len(keys) == PERIOD                                   # the 13 results differ pairwise
    return (w, g, m, v), adam, sgd


def tile(base, n):
    """the first n elements of the base chunks repeated"""
    reps = -(-n // (PERIOD * CHUNK))
    return np.tile(base.reshape(-1), reps)[:n]


def test_one_tensor_past_the_cap_takes_a_second_trip():
    n = CAP * CHUNK + 4099                                       # 2050 chunks: two wrap, the last holds three elements
    out = (C.c_int64 * 4)()
    assert _lib.lib().laser_hip_optim_plan(1, (C.c_int64 * 1)(n), 1, out) == 0 and list(out)[:3] == [1, CAP, CAP + 2]
    data, adam, _ = tiled_base()
    t = [dev(tile(a, n)) for a in data]
    laser_amd.adam_step([t[0]], [t[1]], [t[2]], [t[3]], 2, lr=1e-2, wd=0.01)
    for name, got, want in zip("wmv", (t[0], t[2], t[3]), adam):
        same_bits(host(got), tile(want, n), f"adam past the cap, {name}")


def test_a_list_of_70_tensors_whose_chunks_total_2052():
    lens = [32 * CHUNK - 5 * (k % 7) for k in range(62)] + [33 * CHUNK - 1, 32 * CHUNK + 1] + [0, 5, 0, 0, 300, 0]
    assert len(lens) == 70 and sum(-(-n // CHUNK) for n in lens) == 2052
    out = (C.c_int64 * 4)()
    assert _lib.lib().laser_hip_optim_plan(0, (C.c_int64 * 70)(*lens), 70, out) == 0 and list(out) == [2, CAP, 2052, 0]
    data, _, sgd = tiled_base()
    # every tensor starts at a chunk of the tiling of its own, so the model of tensor k is the tiled model from that chunk on
    first = [(3 * k) % PERIOD for k in range(70)]

    def tensor(base, k):
        return np.roll(base, -first[k], axis=0)

    ts = [[dev(tile(tensor(a, k), lens[k])) for k in range(70)] for a in data[:3]]
    laser_amd.sgd_step(ts[0], ts[1], ts[2], lr=0.1, mu=0.9)
    for k in range(70):
        same_bits(host(ts[0][k]), tile(tensor(sgd[0], k), lens[k]), f"w of tensor {k}")
        same_bits(host(ts[2][k]), tile(tensor(sgd[1], k), lens[k]), f"m of tensor {k}")


# ---- 6. equality with forEach ----------------------------------------------------------------------------------------------------
def test_plain_sgd_has_the_bits_of_foreach():
    lens = [5, 4097, 8193]
    w0, g0 = draws(sum(lens))[:2]
    lr = F(0.1)
    aw, ag = Arena(lens, w0), Arena(lens, g0)
    laser_amd.sgd_step(aw.views, ag.views, lr=float(lr))
    bw = Arena(lens, w0)
    for w, g in zip(bw.views, ag.views):
        laser_amd.forEach("w -= lr * g", w=w, g=g, params={"lr": lr})
    got = aw.read()
    same_bits(got, bw.read(), "sgd_step against forEach")
    same_bits(got, M.sgd(w0, g0, lr=lr)[0], "sgd_step against the model")


# ---- 7. isolation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_nan_or_inf_in_one_gradient_changes_no_other_tensor(poison):
    lens = [7, 4099, 300, 8193]
    data = [np.array(a) for a in draws(sum(lens))]
    clean = M.adam(*data, 2, lr=1e-2)
    starts = np.cumsum([0] + lens)
    g = data[1].copy()
    g[starts[1]:starts[2]] = F(poison)                             # the whole of tensor 1
    got = run_adam(lens, [data[0], g, data[2], data[3]], {}, step=2, what="poisoned")
    want = M.adam(data[0], g, data[2], data[3], 2, lr=1e-2)
    for name, a, b, c in zip("wmv", got, want, clean):
        same_bits(a, b, f"poisoned, {name}")
        keep = np.ones(sum(lens), bool)
        keep[starts[1]:starts[2]] = False
        same_bits(a[keep], c[keep], f"the other tensors are as without the poison, {name}")
    assert not np.isfinite(got[0][starts[1]:starts[2]]).any()      # (Inf: m and v are Inf, Inf / Inf)
    # one element alone: its neighbours in the same vector and chunk stay
    g = data[1].copy()
    g[starts[1] + 2049] = F(poison)
    got = run_sgd(lens, [data[0], g, data[2]], SGD_VARIANTS["momentum"], what="one element")
    cleanw, cleanm = model_sgd(data, SGD_VARIANTS["momentum"])
    keep = np.ones(sum(lens), bool)
    keep[starts[1] + 2049] = False
    same_bits(got[0][keep], cleanw[keep], "w beside one poisoned element")
    same_bits(got[1][keep], cleanm[keep], "m beside one poisoned element")
    assert not np.isfinite(got[0][starts[1] + 2049])


# ---- 8. the gradient norm: the per-tensor sums -------------------------------------------------------------------------------------
NORM_LENS = [0, 1, 8191, 8192, 8193, 3 * 8192 + 5, 2 ** 21 + 3]          # the last: 257 partials, past one leaf of the fold


@functools.lru_cache(maxsize=None)
def norm_draws():
    rng = np.random.default_rng(17)
    g = rng.normal(0, 1, max(NORM_LENS)).astype(F)
    g[5::1013] = 0.0
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("n", NORM_LENS)
@pytest.mark.parametrize("off", [0, 1])
def test_grad_norm_sum_of_one_tensor(n, off):
    g = norm_draws()[:n]
    a = Arena([n], g, off)
    norm, clip = laser_amd.grad_norm(a.views)
    s = M.sum_squares(g)
    if n:
        route = laser_amd.forEachReduce("acc += x * x", merge="acc += other", init=F(0), x=a.views[0])
        same_bits(F(route), s, f"the model's s_k is forEachReduce's, n {n}")
    same_bits(host(norm), np.sqrt(F(0) + s).reshape(1), f"norm, n {n}")
    same_bits(host(clip), F([1.0]), "no max_norm: clip 1")
    a.read("grad_norm reads only")


# ---- 9. the gradient norm: the list and the clip factor ----------------------------------------------------------------------------
def test_grad_norm_list_order_and_max_norm_edges():
    lens = [5, 8193, 0, 300, 4097]
    g = norm_draws()[:sum(lens)]
    a = Arena(lens, g, [0, 1, 0, 2, 0])
    parts = np.split(g, np.cumsum(lens)[:-1])
    norm, one = M.grad_norm(parts)
    got_n, got_c = laser_amd.grad_norm(a.views)
    same_bits(host(got_n), norm.reshape(1), "norm in list order")
    same_bits(host(got_c), one.reshape(1), "clip without a bound")
    # a permuted list is the permuted model (the list sum runs left to right)
    for perm in ([4, 3, 2, 1, 0], [1, 0, 4, 2, 3]):
        want = M.grad_norm([parts[k] for k in perm])[0]
        same_bits(host(laser_amd.grad_norm([a.views[k] for k in perm])[0]), want.reshape(1), f"permutation {perm}")
    # max_norm just below, at and just above the norm; 0; +Inf
    below, above = np.nextafter(norm, F(0)), np.nextafter(norm, F(np.inf))
    for bound in (below, norm, above, F(0), F(np.inf), F(1.0)):
        want_n, want_c = M.grad_norm(parts, bound)
        got_n, got_c = laser_amd.grad_norm(a.views, float(bound))
        same_bits(host(got_n), want_n.reshape(1), f"norm, bound {bound}")
        same_bits(host(got_c), want_c.reshape(1), f"clip, bound {bound}")
    assert M.grad_norm(parts, below)[1] < 1 and M.grad_norm(parts, norm)[1] == 1 and M.grad_norm(parts, above)[1] == 1
    # each result alone
    L = _lib.lib()
    n1, c1 = dev(F([-7.0])), dev(F([-7.0]))
    count, lens_c, arrs = laser_amd.optim._lists("t", [("grads", a.views)])
    assert L.laser_hip_grad_norm_f32_dev(C.c_void_p(n1.data_ptr()), None, arrs[0], lens_c, count, 1.0, laser_amd.tensor._stream()) == 0
    assert L.laser_hip_grad_norm_f32_dev(None, C.c_void_p(c1.data_ptr()), arrs[0], lens_c, count, 1.0, laser_amd.tensor._stream()) == 0
    want_n, want_c = M.grad_norm(parts, 1.0)
    same_bits(host(n1), want_n.reshape(1), "norm alone")
    same_bits(host(c1), want_c.reshape(1), "clip alone")
    # a NaN gradient: norm NaN, clip 1
    bad = np.array(g)
    bad[7] = np.nan
    got_n, got_c = laser_amd.grad_norm(Arena(lens, bad).views, 1.0)
    assert np.isnan(host(got_n)[0])
    same_bits(host(got_c), F([1.0]), "a NaN norm gives clip 1")
    # an empty list
    got_n, got_c = laser_amd.grad_norm([], 1.0)
    same_bits(host(got_n), F([0.0]), "count 0: norm +0")
    same_bits(host(got_c), F([1.0]), "count 0: clip 1")


@pytest.mark.parametrize("count", [64, 65, 192, 193])
def test_grad_norm_counts_round_the_launch_groups(count):
    rng = np.random.default_rng(count)
    lens = [int(n) for n in rng.integers(0, 301, count)]
    lens[count // 2] = 8193 + count                                # one tensor with two partials in the middle
    g = norm_draws()[:sum(lens)]
    a = Arena(lens, g)
    out = (C.c_int64 * 4)()
    assert _lib.lib().laser_hip_optim_plan(2, (C.c_int64 * count)(*lens), count, out) == 0 and out[0] == (3 if count <= 192 else 5)
    want_n, want_c = M.grad_norm(np.split(g, np.cumsum(lens)[:-1]), 2.0)
    got_n, got_c = laser_amd.grad_norm(a.views, 2.0)
    same_bits(host(got_n), want_n.reshape(1), f"norm of {count} tensors")
    same_bits(host(got_c), want_c.reshape(1), f"clip of {count} tensors")
    assert want_c < 1


def test_the_clip_factor_feeds_a_step_without_a_host_read():
    lens = [5, 4097, 0, 8193]
    data = draws(sum(lens))
    parts = np.split(data[1], np.cumsum(lens)[:-1])
    _, c = M.grad_norm(parts, 0.5)
    assert c < 1
    aw, ag, am, av = (Arena(lens, a) for a in data)
    _, clip = laser_amd.grad_norm(ag.views, 0.5)
    laser_amd.adam_step(aw.views, ag.views, am.views, av.views, 1, lr=1e-2, clip=clip)          # no host read in between
    laser_amd.sgd_step(aw.views, ag.views, am.views, lr=0.1, mu=0.9, clip=clip)
    w, m, v = M.adam(*data, 1, lr=1e-2, clip=c)
    w, m = M.sgd(w, data[1], m, lr=0.1, mu=0.9, clip=c)
    same_bits(aw.read(), w, "w after a clipped Adam and a clipped SGD step")
    same_bits(am.read(), m, "m")
    same_bits(av.read(), v, "v")
    same_bits(host(clip), c.reshape(1), "the factor itself")


# ---- 10. the C++ mirror and a small network ----------------------------------------------------------------------------------------
def test_cpp_mirror(tmp_path):
    exe = os.path.join(str(tmp_path), "optim_mirror")
    lib = os.path.join(ROOT, "laser_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "laser_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "optim_mirror.cpp"),
                    "-o", exe, "-L", lib, "-llaser_hip", f"-Wl,-rpath,{lib}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SUCCESS" in r.stdout, r.stdout + r.stderr


def train(optimizer, steps=3):
    """softmax(tanh(layer_norm(X W1 + b1)) W2 + b2) on 8 samples of 16 features, 12 hidden units, 4 classes: the existing
    layers, the gradient norm clipped to 0.5 and one optimizer call per step.  Returns the losses and the final parameters."""
    S, Fe, H, Cn = 8, 16, 12, 4
    rng = np.random.default_rng(2028)
    x = rng.normal(0, 1, (S, Fe)).astype(F)
    labels = np.argmax(x.astype(np.float64) @ rng.normal(0, 1, (Fe, Cn)), axis=1).astype(np.int32)
    T = laser_amd.toTensor
    X, lab = T(x), T(labels)
    P = {"w1": T(rng.normal(0, 0.5, (Fe, H)).astype(F)), "b1": T(np.zeros(H, F)), "gamma": T(np.ones(H, F)), "beta": T(np.zeros(H, F)),
         "w2": T(rng.normal(0, 0.5, (H, Cn)).astype(F)), "b2": T(np.zeros(Cn, F))}
    names = list(P)
    opt = (laser_amd.Adam([P[k] for k in names], lr=0.05) if optimizer == "adam"
           else laser_amd.SGD([P[k] for k in names], lr=0.5, mu=0.9, nesterov=True))
    losses = []
    for _ in range(steps):
        z = laser_amd.matmul(X, P["w1"], bias=P["b1"])
        a, mean, rstd = laser_amd.layer_norm(z, P["gamma"], P["beta"])
        h = laser_amd.tanh(a, out=a)
        logits = laser_amd.matmul(h, P["w2"], bias=P["b2"])
        loss, g = laser_amd.softmax_cross_entropy(logits, lab, grad=True, scale=1.0 / S)
        dh, dw2, db2 = laser_amd.linear_backward(h, P["w2"], g)
        da = laser_amd.activation_grad(dh, h, "tanh", out=dh)
        dz, dgamma, dbeta = laser_amd.layer_norm_backward(da, z, mean, rstd, P["gamma"], need_dx=da)
        _, dw1, db1 = laser_amd.linear_backward(X, P["w1"], dz, need_dx=False)
        grads = [dw1, db1, dgamma, dbeta, dw2, db2]
        _, clip = laser_amd.grad_norm(grads, 0.5)
        opt.step(grads, clip=clip)
        losses.append(loss)
    return losses, P


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_a_small_network_trains_on_two_streams_with_identical_bits(optimizer):
    results = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            losses, P = train(optimizer)
            s.synchronize()
            results.append((np.stack([t.to_numpy() for t in losses]), {k: v.to_numpy() for k, v in P.items()}))
    (l1, p1), (l2, p2) = results
    assert l1.shape == (3, 8) and np.isfinite(l1).all()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32))
    for k in p1:
        assert np.isfinite(p1[k]).all() and np.array_equal(p1[k].view(np.uint32), p2[k].view(np.uint32)), k
    assert not np.array_equal(p1["gamma"], np.ones(12, F)) and p1["beta"].any() and p1["b2"].any()      # they were trained
    print("mean loss per step:", l1.astype(np.float64).mean(axis=1))
