"""relu, ltanh, lsigmoid and their gradients on an MI355X (laser_amd.tanh / sigmoid / activation / activation_grad, laser_tanh
and laser_sigmoid in forEach bodies; include/laser_hip.h "Activations"), bit for bit (any NaN equals any NaN) against the numpy
model of tests/act_model.py: the edge list and 2^20 random bit patterns, the float64 pieces through a float64 forEach body,
every size at which the kernels change path (the last vector, the tail, more than one workgroup, one size past the grid cap),
a base off its 16-byte alignment, a rank-3 view with a negative and a padded stride, a broadcast source, in place, and the
gradients with dx over dy and over y.  The inputs and the model's results are computed once and shared."""
import functools

import numpy as np
import pytest

import laser_amd
from tests import act_model as A

pytestmark = pytest.mark.gpu

KINDS = ["relu", "tanh", "sigmoid"]
CAP = 2048 * 256 * 4                     # elements one sweep of the vector kernel's capped grid covers
SIZES = [0, 1, 3, 4, 5, 255, 1027, 65537, CAP + 7]
SENTINEL = np.float32(-12345.0)


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not A.same_bits(got, want):
        bad = np.nonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))))
        first = tuple(int(b[0]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements differ, first at {first}: {got[first]!r} vs {want[first]!r}")


@functools.lru_cache(maxsize=None)
def values():
    """the edge list, 2^20 random bit patterns, and dense draws where the functions work; read-only"""
    rng = np.random.default_rng(41)
    bits = rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    dense = np.concatenate([rng.uniform(-110, 110, 1 << 16), rng.uniform(-1, 1, 1 << 16), rng.uniform(-0.03, 0.03, 1 << 16)])
    x = np.concatenate([A.edges(), bits, dense.astype(np.float32)])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def forward(kind):
    with np.errstate(all="ignore"):
        y = A.activation(values(), kind)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def upstream():
    """dy for values(): normal draws with NaN, Inf and zeros put in"""
    rng = np.random.default_rng(42)
    dy = rng.normal(0, 3, values().size).astype(np.float32)
    dy[::1001] = np.nan
    dy[1::1003] = np.inf
    dy[2::1007] = -0.0
    dy.setflags(write=False)
    return dy


@functools.lru_cache(maxsize=None)
def outputs(kind):
    """y for the gradient: the forward results with exactly 0, 1, -1, -0 and NaN put in"""
    y = np.array(forward(kind))
    y[5::997] = [0, 1, -1, -0.0, np.nan][KINDS.index(kind) % 5]
    for i, v in enumerate((0.0, 1.0, -1.0, -0.0, np.nan)):
        y[100 + i::5003] = v
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def gradient(kind):
    g = A.activation_grad(upstream(), outputs(kind), kind)
    g.setflags(write=False)
    return g


def dev(a):
    return laser_amd.toTensor(np.array(a))


@pytest.mark.parametrize("kind", KINDS)
def test_forward_on_the_edges_and_random_bit_patterns_and_the_host_form(kind):
    x, want = values(), forward(kind)
    got = laser_amd.activation(dev(x), kind).to_numpy()
    assert_bits(got, want, f"{kind} device")
    assert_bits(laser_amd.activation(x, kind), want, f"{kind} host pointers")
    fin = np.isfinite(x)
    if kind == "tanh":
        assert (np.abs(got[fin]) <= 1).all()
        assert_bits(laser_amd.tanh(dev(-x)).to_numpy(), -want, "ltanh is odd bit for bit")
        assert np.array_equal(got[x == 0].view(np.uint32), x[x == 0].view(np.uint32))
    if kind == "sigmoid":
        assert (got[fin] >= 0).all() and (got[fin] <= 1).all() and (got[x == 0] == 0.5).all()
        sub = (got > 0) & (got < np.finfo(np.float32).tiny)
        assert sub.sum() > 100                                                   # subnormal results are there and right
    if kind == "relu":
        assert (got[np.isnan(x)].view(np.uint32) == 0).all() and (got[x == 0].view(np.uint32) == 0).all()


def test_float64_pieces_through_a_float64_foreach_body():
    """the float32 outputs alone cannot tell a contracted polynomial from the stated one: the float64 bits can"""
    rng = np.random.default_rng(43)
    a = np.concatenate([-rng.uniform(0, 208, (1 << 16) - 4), [-0.0, -208.0, -1e-300, -104.0]])
    with np.errstate(all="ignore"):
        want = A.exp_piece(a)
    y = laser_amd.newTensor(np.float64, a.size)
    laser_amd.forEach("y = lh_act_exp(x)", y=y, x=dev(a))
    assert A.same_bits64(y.to_numpy(), want)
    s = np.concatenate([rng.uniform(0, 2.0 ** -6, (1 << 16) - 3), [0.0, 2.0 ** -6, 1e-300]])
    laser_amd.forEach("y = lh_act_tanh_small(x)", y=y, x=dev(s))
    assert A.same_bits64(y.to_numpy(), A.tanh_small(s))


@pytest.mark.parametrize("n", SIZES)
def test_sizes_offset_base_and_in_place(n):
    """contiguous and aligned (16-byte vectors), then a base one element in (single elements), then dst == src; every kind and
    its gradient, dx fresh, over dy and over y"""
    x, dy = values()[: n + 1], upstream()[: n + 1]
    if n > x.size - 1:                                                           # the size past the grid cap: tile the values
        reps = -(-(n + 1) // values().size)
        x, dy = np.tile(values(), reps)[: n + 1], np.tile(upstream(), reps)[: n + 1]
    dx_, ddy = dev(x), dev(dy)
    for kind in KINDS:
        with np.errstate(all="ignore"):
            want = A.activation(x, kind)
            y = want.copy()
            y[3::7] = [0, 1, -1][KINDS.index(kind)]
            g = A.activation_grad(dy, y, kind)
        for off in (0, 1):
            what = f"{kind} n={n} offset={off}"
            assert_bits(laser_amd.activation(dx_[off: off + n], kind).to_numpy(), want[off: off + n], what)
            dyv = dev(y)
            assert_bits(laser_amd.activation_grad(ddy[off: off + n], dyv[off: off + n], kind).to_numpy(), g[off: off + n], "grad " + what)
            t = dev(x)
            laser_amd.activation(t[off: off + n], kind, out=t[off: off + n])
            got = t.to_numpy()
            assert_bits(got[off: off + n], want[off: off + n], "in place " + what)
            assert_bits(np.delete(got, np.s_[off: off + n]), np.delete(x, np.s_[off: off + n]), "in place wrote outside " + what)
            over_dy, over_y = dev(dy), dev(y)
            laser_amd.activation_grad(over_dy[off: off + n], dyv[off: off + n], kind, out=over_dy[off: off + n])
            laser_amd.activation_grad(ddy[off: off + n], over_y[off: off + n], kind, out=over_y[off: off + n])
            assert_bits(over_dy.to_numpy()[off: off + n], g[off: off + n], "dx over dy " + what)
            assert_bits(over_y.to_numpy()[off: off + n], g[off: off + n], "dx over y " + what)
            assert_bits(np.delete(over_y.to_numpy(), np.s_[off: off + n]), np.delete(y, np.s_[off: off + n]), "dx over y wrote outside " + what)


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_on_the_shared_values_with_exact_outputs_and_nans(kind):
    dy, y, want = upstream(), outputs(kind), gradient(kind)
    assert np.isnan(dy).any() and np.isnan(y).any() and (y == 1).any() and (y == -1).any() and (y == 0).any()
    assert_bits(laser_amd.activation_grad(dev(dy), dev(y), kind).to_numpy(), want, f"{kind} gradient")
    got = laser_amd.activation_grad(dev(dy), dev(y), kind).to_numpy()
    if kind == "relu":
        assert (got[~(y > 0)].view(np.uint32) == 0).all()                       # NaN, 0 and negative outputs: +0, whatever dy is
    if kind == "tanh":
        ok = np.isfinite(dy) & (np.abs(y) == 1)
        assert (got[ok] == 0).all()                                              # 1 - 1 * 1 = 0


def rank3(keep):
    """a (.., .., keep) view of a rank-3 operand: the middle axis reversed (a negative stride), the last one padded"""
    return lambda t: t[:, ::-1, :keep]


@pytest.mark.parametrize("kind", KINDS)
def test_rank3_view_with_a_negative_and_a_padded_stride_and_a_broadcast_source(kind):
    shape, keep = (5, 6, 16), 11
    n = shape[0] * shape[1] * shape[2]
    x, dy = values()[40: 40 + n].reshape(shape), upstream()[40: 40 + n].reshape(shape)
    with np.errstate(all="ignore"):
        want = A.activation(x, kind)
        y = want.copy()
        y[1, 2, 3], y[2, 0, 0], y[4, 5, 10] = 1, 0, np.nan
        g = A.activation_grad(dy, y, kind)
    view = rank3(keep)
    src, out = dev(x), dev(np.full(shape, SENTINEL))
    laser_amd.activation(view(src), kind, out=view(out))
    got = out.to_numpy()
    assert_bits(view(got), view(want), f"{kind} rank-3 view")
    assert (got[:, :, keep:] == SENTINEL).all(), "the gaps of the padded stride were written"
    assert_bits(src.to_numpy(), x, "the source is left alone")
    assert_bits(laser_amd.activation(view(src), kind).to_numpy(), view(want), f"{kind} rank-3 view into a fresh tensor")
    assert_bits(laser_amd.activation(src.T, kind).to_numpy(), want.T, f"{kind} transposed (Python mirror on a view)")
    fn = {"tanh": laser_amd.tanh, "sigmoid": laser_amd.sigmoid}.get(kind)
    if fn is not None:
        assert_bits(fn(src[::2, 1::2]).to_numpy(), want[::2, 1::2], f"laser_amd.{kind} on a stepped view")
    # gradient: dx a padded reversed view, dy the same view of another buffer, y a plain view
    gout = dev(np.full(shape, SENTINEL))
    laser_amd.activation_grad(view(dev(dy)), dev(np.ascontiguousarray(view(y))), kind, out=view(gout))
    got = gout.to_numpy()
    assert_bits(view(got), view(g), f"{kind} gradient on rank-3 views")
    assert (got[:, :, keep:] == SENTINEL).all()
    both = dev(y)
    laser_amd.activation_grad(view(dev(dy)), view(both), kind, out=view(both))
    got = both.to_numpy()
    assert_bits(view(got), view(g), f"{kind} gradient, dx over y on the view")
    assert_bits(got[:, :, keep:], y[:, :, keep:], "the gaps of y are left alone")
    # stride 0: one row against a matrix, and one dy against a row of outputs
    row = dev(x[0, 0])
    wide = laser_amd.newTensor(np.float32, 7, shape[2])
    laser_amd.activation(row, kind, out=wide)
    assert_bits(wide.to_numpy(), np.broadcast_to(want[0, 0], (7, shape[2])), f"{kind} broadcast source")
    one = dev(dy[0, 0, :1])
    with np.errstate(all="ignore"):
        gw = A.activation_grad(np.broadcast_to(dy[0, 0, :1], (shape[2],)), y[0, 1], kind)
    assert_bits(laser_amd.activation_grad(one, dev(y[0, 1]), kind).to_numpy(), gw, f"{kind} gradient with a broadcast dy")


def test_names_in_foreach_and_foreachreduce_bodies_equal_the_kernels():
    x = values()[: 70001]
    t = dev(x)
    yt, ys = laser_amd.newTensor(np.float32, x.size), laser_amd.newTensor(np.float32, x.size)
    laser_amd.forEach("a = laser_tanh(x); b = laser_sigmoid(x)", writable=("a", "b"), a=yt, b=ys, x=t)
    assert_bits(yt.to_numpy(), laser_amd.tanh(t).to_numpy(), "laser_tanh in a body = the kernel")
    assert_bits(ys.to_numpy(), laser_amd.sigmoid(t).to_numpy(), "laser_sigmoid in a body = the kernel")
    assert_bits(yt.to_numpy(), forward("tanh")[: x.size], "and the model")
    m = x.reshape(-1)[: 257 * 101].reshape(257, 101)
    tm, ym = dev(m), laser_amd.newTensor(np.float32, 101, 257)
    laser_amd.forEach("y = laser_sigmoid(x)", y=ym, x=tm.T)
    assert_bits(ym.to_numpy(), forward("sigmoid")[: m.size].reshape(257, 101).T, "a body on strided views")
    with np.errstate(all="ignore"):
        top_t, top_s = np.nanmax(forward("tanh")[: x.size]), np.nanmax(np.where(x < 0, forward("sigmoid")[: x.size], 0))
    s = laser_amd.forEachReduce("acc = fmaxf(acc, laser_tanh(x))", merge="acc = fmaxf(acc, other)", init=np.float32(-np.inf), x=t)
    assert np.float32(s) == top_t
    s = laser_amd.forEachReduce("acc = fmaxf(acc, x < 0 ? laser_sigmoid(x) : 0.0f)", merge="acc = fmaxf(acc, other)", init=np.float32(0), x=t)
    assert np.float32(s) == top_s


def test_fused_gemm_relu_is_the_same_rule():
    rng = np.random.default_rng(44)
    a, b = rng.normal(0, 1, (16, 16)).astype(np.float32), rng.normal(0, 1, (16, 16)).astype(np.float32)
    ta, tb = dev(a), dev(b)
    fused = laser_amd.matmul(ta, tb, activation="relu").to_numpy()
    plain = laser_amd.matmul(ta, tb)
    assert (plain.to_numpy() < 0).any() and (fused > 0).any()
    assert_bits(fused, laser_amd.activation(plain, "relu").to_numpy(), "matmul(.., relu) = activation(matmul(..), relu)")


def test_arguments():
    d = dev(values()[:64])
    with pytest.raises(ValueError):
        laser_amd.activation(d, "gelu")
    with pytest.raises(ValueError):
        laser_amd.activation_grad(d, d, None)
    with pytest.raises(TypeError):
        laser_amd.tanh(dev(np.ones(4, np.float64)))
    import torch
    zero = laser_amd.fromTorch(torch.zeros(1, device="cuda").expand(64))          # stride 0 on a destination
    with pytest.raises(laser_amd.LaserHipError):
        laser_amd.activation(d, "tanh", out=zero)
    with pytest.raises(laser_amd.LaserHipError):
        laser_amd.activation_grad(d, d, "tanh", out=zero)
