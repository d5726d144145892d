"""numpy model of the embedding layer of liblaser_hip.so (include/laser_hip.h "Embedding"): the gather, the stable grouping
of the token positions by id (np.argsort(kind="stable") on the keys) and the gradient, reduce_model.model_sum per (id, column)
over the occurrences of the id in token order."""
import numpy as np

from tests import reduce_model as R

QNAN = np.uint32(0x7FC00000)


def valid(idx, vocab):
    idx = np.asarray(idx, np.int32).reshape(-1)
    return (idx >= 0) & (idx < vocab)


def gather(w, idx):
    """y[t, :] = the bits of w[idx[t], :]; -1: +0; any other id outside [0, vocab): quiet NaN 0x7fc00000"""
    w = np.asarray(w, np.float32)
    idx = np.asarray(idx, np.int32)
    flat = idx.reshape(-1)
    ok = valid(flat, w.shape[0])
    y = np.zeros((flat.size, w.shape[1]), np.uint32)
    y[ok] = w.view(np.uint32)[flat[ok]]
    y[~ok & (flat != -1)] = QNAN
    return y.view(np.float32).reshape(idx.shape + (w.shape[1],))


def group(idx, vocab):
    """(order, starts): the positions sorted by (key, position), key = the id or `vocab` for every invalid id, and for every
    v in 0 .. vocab the number of tokens with a valid id below v"""
    flat = np.asarray(idx, np.int32).reshape(-1)
    keys = np.where(valid(flat, vocab), flat.astype(np.int64), vocab)
    order = np.argsort(keys, kind="stable").astype(np.int32)
    starts = np.searchsorted(keys[order], np.arange(vocab + 1), side="left").astype(np.int32)
    return order, starts


def grad(dy, idx, vocab, order=None, starts=None):
    """dw[v, j] = model_sum of dy[order[starts[v] : starts[v + 1]], j]; +0 for an id that never occurs"""
    dy = np.asarray(dy, np.float32)
    dy = dy.reshape(-1, dy.shape[-1])
    if order is None:
        order, starts = group(idx, vocab)
    dw = np.zeros((vocab, dy.shape[1]), np.float32)
    for v in np.nonzero(np.diff(starts))[0]:
        seg = dy[order[starts[v]:starts[v + 1]]]
        for j in range(dy.shape[1]):
            dw[v, j] = R.model_sum(np.ascontiguousarray(seg[:, j]))
    return dw
