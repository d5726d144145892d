"""What the shared elementwise template (laser_amd/csrc/pointwise.h) adds to the kernels it replaced, on an MI355X: its loops
over operand counts, at full rank and on the 16-byte path, for one function of each arity -- exp (1 in, 1 out),
activation_grad("tanh") (2 in, 1 out) and sincos (1 in, 2 out) -- bit for bit against the numpy models of tests/exp_model.py,
tests/act_model.py and tests/sincos_model.py.  The functions themselves are covered by their own files."""
import functools

import numpy as np
import pytest

import laser_amd
from tests import act_model as A
from tests import exp_model as E
from tests import sincos_model as S
from tests.test_gpu_sincos import assert_bits

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 2, 3, 2, 5)          # the logical shape of every view
BUFFER = (2, 4, 3, 3, 3, 12)        # padded on axes 1, 2, 4 and 5
BCAST_AXIS = 2                      # where the second input of the gradient has extent 1 (stride 0)
SENTINEL = np.float32(-12345.0)


def view(t):
    """rank 6: every second element of the padded last axis, axis 3 reversed, the other padded axes cut"""
    return t[:, :3, :2, ::-1, :2, :10:2]


def bview(t):
    return t[:, :3, :1, ::-1, :2, :10:2]


def dev(a):
    return laser_amd.toTensor(np.array(a))


@functools.lru_cache(maxsize=None)
def data():
    """buffers of the padded shape: x for exp and sincos, dy and y (inside (-1, 1), as a tanh gives) for the gradient; read-only"""
    rng = np.random.default_rng(77)
    x = rng.uniform(-20, 20, BUFFER).astype(np.float32)
    dy = rng.standard_normal(BUFFER).astype(np.float32)
    y = rng.uniform(-1, 1, BUFFER).astype(np.float32)
    for a in (x, dy, y):
        a.setflags(write=False)
    return x, dy, y


def test_no_two_dimensions_of_the_views_merge():
    """merge_dims folds dimension d into d - 1 when stride[d - 1] == stride[d] * extent[d] on EVERY operand: `view`, which every
    call below has among its operands, allows it nowhere"""
    a = view(np.empty(BUFFER, np.float32))
    st = [s // 4 for s in a.strides]
    assert a.shape == SHAPE and bview(a.base).shape == SHAPE[:BCAST_AXIS] + (1,) + SHAPE[BCAST_AXIS + 1:]
    assert all(st[d - 1] != st[d] * a.shape[d] for d in range(1, 6)), st


def check_outside(got, what):
    inside = np.zeros(BUFFER, bool)
    view(inside)[...] = True
    assert (got[~inside] == SENTINEL).all(), f"{what}: an element outside the view was written"


def test_rank6_views_one_in_one_out():
    x, _, _ = data()
    out = dev(np.full(BUFFER, SENTINEL))
    laser_amd.exp(view(dev(x)), out=view(out))
    got = out.to_numpy()
    assert_bits(view(got), E.lexp(view(x)), "exp on the rank-6 view")
    check_outside(got, "exp")


def test_rank6_views_two_in_one_out_the_second_broadcast():
    _, dy, y = data()
    out = dev(np.full(BUFFER, SENTINEL))
    laser_amd.activation_grad(view(dev(dy)), bview(dev(y)), "tanh", out=view(out))
    got = out.to_numpy()
    want = A.activation_grad(view(dy), np.broadcast_to(bview(y), SHAPE), "tanh")
    assert_bits(view(got), want, "tanh gradient on the rank-6 view, y broadcast along one axis")
    check_outside(got, "activation_grad")


def test_rank6_views_one_in_two_out():
    x, _, _ = data()
    so, co = dev(np.full(BUFFER, SENTINEL)), dev(np.full(BUFFER, SENTINEL))
    laser_amd.sincos(view(dev(x)), out=(view(so), view(co)))
    ws, wc = S.lsincos(np.ascontiguousarray(view(x)))
    for got, want, name in ((so.to_numpy(), ws, "sine"), (co.to_numpy(), wc, "cosine")):
        assert_bits(view(got), want, f"sincos on the rank-6 view: {name}")
        check_outside(got, f"sincos: {name}")


def test_five_contiguous_elements_one_vector_and_a_tail():
    """n = 5 in fresh (16-byte aligned, contiguous) tensors: one 16-byte vector and a one-element tail, with guards behind"""
    x, dy, y = (a.reshape(-1)[:5] for a in data())
    tail = lambda t: t.to_numpy()[5:]
    out = dev(np.full(8, SENTINEL))
    laser_amd.exp(dev(x), out=out[:5])
    assert_bits(out.to_numpy()[:5], E.lexp(x), "exp, n = 5")
    assert (tail(out) == SENTINEL).all()
    out = dev(np.full(8, SENTINEL))
    laser_amd.activation_grad(dev(dy), dev(y), "tanh", out=out[:5])
    assert_bits(out.to_numpy()[:5], A.activation_grad(dy, y, "tanh"), "tanh gradient, n = 5")
    assert (tail(out) == SENTINEL).all()
    so, co = dev(np.full(8, SENTINEL)), dev(np.full(8, SENTINEL))
    laser_amd.sincos(dev(x), out=(so[:5], co[:5]))
    ws, wc = S.lsincos(x)
    assert_bits(so.to_numpy()[:5], ws, "sincos, n = 5: sine")
    assert_bits(co.to_numpy()[:5], wc, "sincos, n = 5: cosine")
    assert (tail(so) == SENTINEL).all() and (tail(co) == SENTINEL).all()
