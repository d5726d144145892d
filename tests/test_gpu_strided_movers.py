"""The kernels that move data through strided views against numpy applying the same view to the same bytes:
copy_strided (deepCopy / copyFrom), map_strided (forEachMap), transpose_batched (transpose2D_copy / _batched, nchw2nhwc /
nhwc2nchw), and forEach / reduce_sum / forEachReduce on the same views.  The views come from tests/strided_views.py, whose
fixed-seed lists are steered to every branch of the launchers (tests/test_strided_views_cpu.py checks that they reach
them).  Sources hold random bit patterns (NaN payloads and -0.0 included) wherever nothing computes on them, and every
comparison covers the whole destination buffer as unsigned integers: a wrong element and a gap written by mistake both
fail.  One case per mover family puts element offsets past 2^31, compared on the device against torch."""
import numpy as np
import pytest

import laser_amd as la
from tests import reduce_model as M
from tests import strided_views as SV

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64, np.int32, np.int64)
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
TORCH_BITS = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}   # element types torch carries for the transposes
SENTINEL = 0xA5


def random_bits(rng, n, dtype):
    return np.frombuffer(rng.bytes(n * np.dtype(dtype).itemsize), dtype=dtype).copy()


def sentinel(n, dtype):
    return np.full(n * np.dtype(dtype).itemsize, SENTINEL, np.uint8).view(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def assert_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {g.shape} elements vs {w.shape}"
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (f"{what}: {bad.size} of {g.size} elements differ, first at flat indices {bad[:6].tolist()}: "
                           f"got {[hex(int(x)) for x in g[bad[:6]]]}, want {[hex(int(x)) for x in w[bad[:6]]]}")


def to_dev(host):
    import torch
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


class Buf:
    """a flat device buffer, the host array it was made from, and Tensor views over it"""

    def __init__(self, host):
        self.host = np.ascontiguousarray(host).copy()
        self.dev = to_dev(self.host)
        self.storage = la.fromTorch(self.dev).storage

    def view(self, v):
        t = v.tensor(la.Tensor, self.storage, self.host.dtype)
        assert (t.shape, t.strides, t.offset) == (v.shape, v.strides, v.elem_offset), v
        return t

    def read(self):
        return self.dev.cpu().numpy()            # ordered after the library's kernels: they run on torch's current stream


def dtname(dtype):
    return np.dtype(dtype).name


# ---- copy_strided: deepCopy, copyFrom, and forEach("x = y") over the same views --------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_strided_random_views_vs_numpy(dtype):
    rng = np.random.default_rng(101)
    for name, sv, dv in SV.copy_cases():
        src = Buf(random_bits(rng, sv.base_len, dtype))
        st = src.view(sv)
        want = sv.numpy(src.host)
        what = f"{name} dtype={dtname(dtype)} src={sv}"
        c = la.deepCopy(st)
        assert c.shape == want.shape and c.is_C_contiguous(), what
        assert_bits(c.to_numpy(), want, f"deepCopy {what}")
        exp = sentinel(dv.base_len, dtype)
        dv.numpy(exp)[...] = want
        dst = Buf(sentinel(dv.base_len, dtype))
        la.copyFrom(dst.view(dv), st)
        assert_bits(dst.read(), exp, f"copyFrom {what} dst={dv}")
        dst = Buf(sentinel(dv.base_len, dtype))
        la.forEach("x = y", x=dst.view(dv), y=st)
        assert_bits(dst.read(), exp, f"forEach('x = y') {what} dst={dv}")
        assert_bits(src.read(), src.host, f"source buffer changed: {what}")


# ---- map_strided: every forEachMap op ------------------------------------------------------------------------------
def _ops(dtype):
    """op -> (operands read, numpy reference(a, b, alpha, beta)) with alpha / beta for the element type"""
    return {
        "copy": (1, lambda a, b, al, be: a), "fill": (0, lambda a, b, al, be: np.full_like(a, al)),
        "neg": (1, lambda a, b, al, be: -a), "abs": (1, lambda a, b, al, be: np.abs(a)),
        "relu": (1, lambda a, b, al, be: np.maximum(a, 0)), "scale": (1, lambda a, b, al, be: al * a + be),
        "square": (1, lambda a, b, al, be: a * a), "add": (2, lambda a, b, al, be: a + b),
        "sub": (2, lambda a, b, al, be: a - b), "mul": (2, lambda a, b, al, be: a * b),
        "max": (2, lambda a, b, al, be: np.maximum(a, b)), "min": (2, lambda a, b, al, be: np.minimum(a, b)),
        "axpy": (2, lambda a, b, al, be: al * a + b), "axpby": (2, lambda a, b, al, be: al * a + be * b)}


def finite_values(rng, n, dtype):
    """small integers (floats: quarters) so that every op is exact in the element type: numpy's result is the kernel's"""
    if np.dtype(dtype).kind == "f":
        return (rng.integers(-64, 65, n) / 4).astype(dtype)
    return rng.integers(-1000, 1001, n).astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_map_strided_every_op_random_views_vs_numpy(dtype):
    assert set(_ops(dtype)) == set(la.MAP_OPS)
    rng = np.random.default_rng(102)
    fl = np.dtype(dtype).kind == "f"
    alpha, beta = (1.5, -0.25) if fl else (3, -2)
    al, be = np.dtype(dtype).type(alpha), np.dtype(dtype).type(beta)
    for name, dv, av, bv in SV.map_cases():
        in_place = av is dv
        A = Buf(finite_values(rng, av.base_len, dtype))
        B = Buf(finite_values(rng, bv.base_len, dtype))
        init = finite_values(rng, dv.base_len, dtype) if in_place else sentinel(dv.base_len, dtype)
        for op, (nin, ref) in _ops(dtype).items():
            what = f"{op} {name} dtype={dtname(dtype)} dst={dv} a={'dst' if in_place else av} b={bv}"
            D = Buf(init)
            dt = D.view(dv)
            at = dt if in_place else A.view(av)
            a_vals = dv.numpy(init).copy() if in_place else av.numpy(A.host)
            la.forEachMap(op, dt, at if nin >= 1 else None, B.view(bv) if nin == 2 else None,
                          alpha=alpha, beta=beta)
            exp = init.copy()
            dv.numpy(exp)[...] = ref(a_vals, bv.numpy(B.host), al, be)
            assert_bits(D.read(), exp, what)


# ---- transposes ---------------------------------------------------------------------------------------------------
def _call_transpose(fn, d, s, N, NR, NC):
    if fn == "batched":
        la.transpose2D_batched(d, s, N, NR, NC)
    elif fn == "copy":
        la.transpose2D_copy(d, s, NR, NC)
    elif fn == "nchw2nhwc":
        H, W = SV.split_hw(NC)
        la.nchw2nhwc(d, s, N, NR, H, W)
    else:
        H, W = SV.split_hw(NR)
        la.nhwc2nchw(d, s, N, NC, H, W)


@pytest.mark.parametrize("itemsize", [1, 2, 4, 8])
def test_transposes_vs_numpy(itemsize):
    rng = np.random.default_rng(103 + itemsize)
    dt = TORCH_BITS[itemsize]
    V = 16 // itemsize
    for fn, N, NR, NC, so, do in SV.transpose_cases(itemsize):
        total = N * NR * NC
        src_host = random_bits(rng, so + total + 3, dt)
        dst_host = sentinel(do + total + 2 * V + 1, dt)
        src, dst = to_dev(src_host), to_dev(dst_host)
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        kernel = SV.transpose_branch(N, NR, NC, itemsize, do * itemsize, so * itemsize)
        what = f"{fn} N={N} NR={NR} NC={NC} {itemsize}-byte src_off={so} dst_off={do} ({kernel} kernel)"
        _call_transpose(fn, dst[do:do + total], src[so:so + total], N, NR, NC)
        exp = dst_host.copy()
        exp[do:do + total] = src_host[so:so + total].reshape(N, NR, NC).transpose(0, 2, 1).reshape(-1)
        assert_bits(dst.cpu().numpy(), exp, what)
        assert_bits(src.cpu().numpy(), src_host, f"source changed: {what}")


def test_transpose_32x256_tile_above_2_pow_24_elements():
    import torch
    g = torch.Generator(device="cuda").manual_seed(104)
    for N, NR, NC in SV.BIG_TRANSPOSES:
        assert SV.transpose_branch(N, NR, NC, 4) == "vec32x256"
        total = N * NR * NC
        src = torch.randint(-2 ** 31, 2 ** 31 - 1, (total,), dtype=torch.int32, device="cuda", generator=g)
        sent = int(sentinel(1, np.int32)[0])
        dst = torch.full((total + 64,), sent, dtype=torch.int32, device="cuda")
        if N == 1:
            la.transpose2D_copy(dst[:total], src, NR, NC)
        else:
            la.transpose2D_batched(dst[:total], src, N, NR, NC)
        want = src.view(N, NR, NC).transpose(1, 2).reshape(-1)
        bad = (dst[:total] != want).nonzero()[:6].flatten().tolist()
        assert not bad, f"N={N} NR={NR} NC={NC} 4-byte (vec32x256 kernel): elements differ at flat indices {bad}"
        assert bool((dst[total:] == sent).all()), f"N={N} NR={NR} NC={NC}: written past the destination"
        del src, dst, want
    torch.cuda.empty_cache()


# ---- forEach and the reductions on the threshold views ------------------------------------------------------------
def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and bits(got) == bits(want), f"{what}: {got!r} vs {want!r}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_sum_and_foreach_reduce_on_threshold_views(dtype):
    rng = np.random.default_rng(105)
    fl = np.dtype(dtype).kind == "f"
    for name, sv, _ in SV.copy_cases():
        n = sv.base_len
        host = rng.standard_normal(n).astype(dtype) if fl else \
            rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max, n, dtype=dtype, endpoint=True)
        buf = Buf(host)
        t = buf.view(sv)
        c = np.ascontiguousarray(sv.numpy(buf.host))
        what = f"{name} dtype={dtname(dtype)} view={sv}"
        got = la.reduce_sum(t)
        assert_same(got, la.reduce_sum(to_dev(c)), f"reduce_sum(view) vs its contiguous copy: {what}")
        assert_same(got, M.model_sum(c), f"reduce_sum(view) vs the model: {what}")
        acc = la.forEachReduce("acc += x", merge="acc += other", init=np.dtype(dtype).type(0), x=t)
        assert_same(acc, got, f"forEachReduce('acc += x') vs reduce_sum: {what}")


# ---- element offsets past 2^31, one case per mover family ---------------------------------------------------------
BIG = 2 ** 31 + 2 ** 20                     # int32 elements (8 GiB)
# (shape, element strides, offset): the last element of each view lies beyond 2^31
BIG_VIEWS = (((1025, 512), (2 ** 21, 2), 3),            # short rows, a partial last workgroup
             ((3, 4096), (2 ** 30, 1), 5),              # long rows of 4 chunks
             ((2, 600, 3), (3 * 2 ** 29, 897_000, 5), 4))       # no dimension merges


def _big_buffer(seed, lo=-2 ** 31, hi=2 ** 31 - 1):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi, (BIG,), dtype=torch.int32, device="cuda", generator=g)


def _free():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    la.tensor.trimStorageCache()


def _check_big_view(shape, strides, off):
    """in bounds of the buffer, last element past 2^31, no element twice (the views are written)"""
    last = off + sum((n - 1) * s for n, s in zip(shape, strides))
    assert min(strides) > 0 and 2 ** 31 < last < BIG, (shape, strides, off, last)
    order = sorted(zip(strides, shape))
    assert all(order[i + 1][0] >= order[i][0] * order[i][1] for i in range(len(order) - 1)), (shape, strides)


def test_copy_strided_past_2_pow_31():
    import torch
    big = _big_buffer(106)
    base = la.fromTorch(big)
    try:
        for shape, strides, off in BIG_VIEWS:
            _check_big_view(shape, strides, off)
            what = f"shape={shape} strides={strides} offset={off} int32"
            v = la.Tensor(shape, strides, off, base.storage, np.int32)
            ref = big.as_strided(shape, strides, off)
            got = torch.as_tensor(la.deepCopy(v), device="cuda")
            assert torch.equal(got, ref), f"deepCopy {what}"
            # and back: copyFrom a dense source into the strided view; the buffer's sum changes by exactly what the view's
            # elements changed (a stray write elsewhere would have to cancel out)
            src = torch.arange(ref.numel(), dtype=torch.int32, device="cuda").view(shape) - 7
            old_sum, old_view = big.sum(dtype=torch.int64), ref.sum(dtype=torch.int64)
            la.copyFrom(v, la.fromTorch(src))
            assert torch.equal(big.as_strided(shape, strides, off), src), f"copyFrom into {what}"
            delta = big.sum(dtype=torch.int64) - old_sum
            assert delta == src.sum(dtype=torch.int64) - old_view, f"copyFrom wrote outside {what}"
    finally:
        del base, big
        _free()


def test_map_strided_past_2_pow_31():
    import torch
    big = _big_buffer(107, -2 ** 20, 2 ** 20)
    base = la.fromTorch(big)
    try:
        for shape, strides, off in BIG_VIEWS:
            _check_big_view(shape, strides, off)
            what = f"add: dst dense, a shape={shape} strides={strides} offset={off} int32, b a broadcast row"
            a = la.Tensor(shape, strides, off, base.storage, np.int32)
            row = torch.arange(shape[-1], dtype=torch.int32, device="cuda") * 3 - 11
            dst = torch.empty(shape, dtype=torch.int32, device="cuda")
            la.forEachMap("add", la.fromTorch(dst), a, la.fromTorch(row))
            assert torch.equal(dst, big.as_strided(shape, strides, off) + row), what
            # in place over the far view: dst is a
            before = big.as_strided(shape, strides, off).clone()
            la.forEachMap("neg", a, a)
            assert torch.equal(big.as_strided(shape, strides, off), -before), f"neg in place, {what}"
    finally:
        del base, big
        _free()


def test_transpose_batched_past_2_pow_31():
    import torch
    N, NR, NC = 2, 2 ** 15, 2 ** 15 + 16       # N * NR * NC = 2^31 + 2^20: the second matrix starts past 2^30, ends past 2^31
    assert N * NR * NC == BIG and SV.transpose_branch(N, NR, NC, 4) == "vec32x256"
    src = _big_buffer(108)
    dst = torch.empty(BIG, dtype=torch.int32, device="cuda")
    try:
        la.transpose2D_batched(dst, src, N, NR, NC)
        s3, d3 = src.view(N, NR, NC), dst.view(N, NC, NR)
        for n in range(N):
            for c0 in range(0, NC, 4096):
                ok = torch.equal(d3[n, c0:c0 + 4096], s3[n, :, c0:c0 + 4096].t())
                assert ok, f"transpose2D_batched N={N} NR={NR} NC={NC} int32: matrix {n}, destination rows {c0}.. differ"
    finally:
        del src, dst
        _free()
