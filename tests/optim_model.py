"""The contract of include/laser_hip.h "Optimizer steps" in numpy float32: plain + - * / and np.sqrt on float32 arrays (each
one correctly rounded operation, never fused), in the order of laser_amd/csrc/optim_core.h; reduce_model.model_sum for the
sums of the gradient norm; the bias correction in Python floats (doubles).  Arrays are float32 of any shape; the steps return
new arrays and change nothing in place."""
import numpy as np

from tests import reduce_model as R

F = np.float32


def bias_correction(beta, step):
    """1 - beta^step: beta as float32, the power in double by square-and-multiply from the low bit, one rounding to float32"""
    assert step >= 1
    r, b = 1.0, float(F(beta))
    while step:
        if step & 1:
            r = r * b
        b = b * b
        step >>= 1
    return F(1.0 - r)


def grad(g, gscale=1.0, clip=None):
    """g2: the gradient scaled by gscale and, with a clip factor, by c"""
    with np.errstate(all="ignore"):
        x = np.asarray(g, F) * F(gscale)
        if clip is not None:
            x = x * F(clip)
    assert x.dtype == F
    return x


def sgd(w, g, m=None, lr=0.0, mu=0.0, wd=0.0, nesterov=False, gscale=1.0, clip=None):
    """(w', m'); m' is None without a momentum array"""
    w = np.asarray(w, F)
    lr, mu, wd = F(lr), F(mu), F(wd)
    with np.errstate(all="ignore"):
        g3 = grad(g, gscale, clip)
        if wd != 0:
            g3 = g3 + wd * w
        d = g3
        if m is not None:
            m = mu * np.asarray(m, F) + g3
            d = g3 + mu * m if nesterov else m
        else:
            assert mu == 0 and not nesterov
        w = w - lr * d
    assert w.dtype == F and (m is None or m.dtype == F)
    return w, m


def adam(w, g, m, v, step=None, lr=0.0, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False, gscale=1.0, clip=None, bc=None):
    """(w', m', v'); bc = (bc1, bc2) replaces the bias corrections of `step`"""
    w, m, v = np.asarray(w, F), np.asarray(m, F), np.asarray(v, F)
    lr, b1, b2, eps, wd = F(lr), F(b1), F(b2), F(eps), F(wd)
    bc1, bc2 = (F(bc[0]), F(bc[1])) if bc is not None else (bias_correction(b1, step), bias_correction(b2, step))
    omb1, omb2, lrwd = F(1) - b1, F(1) - b2, lr * wd
    with np.errstate(all="ignore"):
        g3 = grad(g, gscale, clip)
        if not decoupled and wd != 0:
            g3 = g3 + wd * w
        m = b1 * m + omb1 * g3
        v = b2 * v + (omb2 * g3) * g3
        mh = m / bc1
        vh = v / bc2
        den = np.sqrt(vh) + eps
        u = mh / den
        w1 = w - lrwd * w if decoupled and wd != 0 else w
        w = w1 - lr * u
    assert w.dtype == F and m.dtype == F and v.dtype == F
    return w, m, v


def sum_squares(g):
    """s_k: reduce_sum of g * g, the product rounded to float32"""
    g = np.asarray(g, F).reshape(-1)
    with np.errstate(all="ignore"):
        return F(R.model_sum(g * g))


def grad_norm(grads, max_norm=np.inf):
    """(norm, clip) of the list of gradient arrays, in list order"""
    total = F(0)
    with np.errstate(all="ignore"):
        for g in grads:
            total = F(total + sum_squares(g))
        norm = np.sqrt(total)
        clip = F(max_norm) / norm if norm > F(max_norm) else F(1)
    assert norm.dtype == F and clip.dtype == F
    return norm, clip


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
