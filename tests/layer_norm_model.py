"""The contract of include/laser_hip.h "Layer normalization" in numpy float32: plain + - * / and np.sqrt on float32 arrays
(each one correctly rounded operation, never fused) and reduce_model.model_sum -- the canonical reduction order applied to a
row or a column as a 1-D array -- for every sum.  x, dy: (rows, n) float32; gamma, beta: (n,) float32 or None."""
import numpy as np

from tests import reduce_model as R

F = np.float32


def rsum(a):
    """model_sum of every row of the 2-D float32 array a: (rows,)"""
    return np.array([R.model_sum(row) for row in a], F).reshape(a.shape[0])


def csum(a):
    """model_sum of every column of the 2-D float32 array a: (n,)"""
    return np.array([R.model_sum(a[:, j]) for j in range(a.shape[1])], F).reshape(a.shape[1])


def xhat_of(x, mean, rstd):
    with np.errstate(all="ignore"):
        return ((x - mean[:, None]) * rstd[:, None]).astype(F)


def forward(x, gamma=None, beta=None, eps=1e-5):
    """(y, mean, rstd)"""
    x = np.asarray(x, F)
    nf = F(x.shape[1])
    with np.errstate(all="ignore"):
        mean = rsum(x) / nf
        d = x - mean[:, None]
        var = rsum(d * d) / nf
        rstd = F(1) / np.sqrt(var + F(eps))
        y = d * rstd[:, None]
        if gamma is not None:
            y = y * np.asarray(gamma, F)[None, :]
        if beta is not None:
            y = y + np.asarray(beta, F)[None, :]
    assert y.dtype == F and mean.dtype == F and rstd.dtype == F
    return y, mean, rstd


def dx_of(dy, x, mean, rstd, gamma=None):
    dy, x = np.asarray(dy, F), np.asarray(x, F)
    nf = F(x.shape[1])
    with np.errstate(all="ignore"):
        xhat = xhat_of(x, mean, rstd)
        g = dy * np.asarray(gamma, F)[None, :] if gamma is not None else dy
        a = rsum(g) / nf
        b = rsum(g * xhat) / nf
        dx = ((g - a[:, None]) - xhat * b[:, None]) * rstd[:, None]
    assert dx.dtype == F
    return dx


def param_grads(dy, x, mean, rstd):
    """(dgamma, dbeta): the column sums of dy * xhat and of dy"""
    dy, x = np.asarray(dy, F), np.asarray(x, F)
    with np.errstate(all="ignore"):
        t = dy * xhat_of(x, mean, rstd)
    return csum(t), csum(dy)


def backward(dy, x, mean, rstd, gamma=None):
    """(dx, dgamma, dbeta)"""
    return (dx_of(dy, x, mean, rstd, gamma),) + param_grads(dy, x, mean, rstd)


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
