"""Laser's table-driven exp and the row softmax on top of it (laser/primitives/simd_math/exp_log_*.nim; include/laser_hip.h
"exp and row softmax"), the way from logits to a loss (include/laser_hip.h "log, logsumexp, log-softmax and
cross-entropy"), the activations with their gradients (include/laser_hip.h "Activations") and the bit-defined sine and
cosine (include/laser_hip.h "Sine and cosine"), float32:

    laser_amd.exp(t)        lexp of every element: the exported SIMD `exp*` of the reference, bit for bit
    laser_amd.softmax(t)    softmax over the rows of a 2-D tensor, summed in the fixed order of the reductions
    laser_amd.softmax(t, axis=k)   the same along any axis of a tensor of rank 1 .. 6: bit for bit what the row form gives the
                            same values as rows (not built: float64)
    laser_amd.softmax_backward(dy, y)     the gradient from the softmax's OUTPUT: y * (dy - reduce_sum(dy * y)) per row
    laser_amd.log(t)        llog of every element: the bit-defined logarithm of laser_amd/csrc/log_core.h
    laser_amd.logsumexp(t)  one value per row of a 2-D tensor: max + llog(sum), max and sum exactly the softmax's
    laser_amd.log_softmax(t)       (x - max) - llog(sum) over the rows of a 2-D tensor
    laser_amd.softmax_cross_entropy(logits, labels, grad=False, scale=1.0)   the per-row loss for int32 labels (-1: ignore),
                            and with grad=True also (softmax - onehot) * scale
    laser_amd.tanh(t)       ltanh of every element: the bit-defined tanh of laser_amd/csrc/act_core.h
    laser_amd.sigmoid(t)    lsigmoid of every element: the bit-defined logistic function of the same header
    laser_amd.activation(t, kind, out=None)          kind "relu", "tanh" or "sigmoid": relu is x > 0 ? x : +0
    laser_amd.activation_grad(dy, y, kind, out=None)   the gradient from the forward OUTPUT y: relu y > 0 ? dy : +0,
                            tanh dy * (1 - y * y), sigmoid dy * (y * (1 - y)), every float32 operation rounded on its own
    laser_amd.sin(t), laser_amd.cos(t)    lsin / lcos of every element: the bit-defined sine and cosine of
                            laser_amd/csrc/sincos_core.h (faithful for every finite float32, lsin odd and lcos even bit for bit)
    laser_amd.sincos(t, out=None)         (lsin(t), lcos(t)) from one argument reduction, the same bits; out=(s, c)

An operand is a laser_amd.Tensor or a torch CUDA tensor (anything with __cuda_array_interface__); `exp` also takes a host
float32 numpy array, like the reference's benchmark loop.  With out=None a device call returns a fresh row-major Tensor;
with `out` it writes there (out may be the input) and returns it.  Device calls are asynchronous on the current torch
stream.  Inside forEach / forEachReduce bodies the same functions are `laser_exp(x)`, `laser_log(x)`, `laser_tanh(x)`,
`laser_sigmoid(x)`, `laser_sin(x)` and `laser_cos(x)`.
"""
import ctypes as C

import numpy as np

from . import _lib
from .foreach import _View
from .tensor import _bcast_strides, _stream, newTensor


def _f32(name, obj):
    v = _View(name, obj)
    if v.dtype != np.float32:
        raise TypeError(f"{name}: element type {v.dtype} (float32 only)")
    return v


def _elementwise(fn, outs, ins, lead=()):
    """laser_hip_{fn}_f32_dev over device operands: `outs` and `ins` are tuples of (name, operand).  The inputs broadcast
    against the outputs; an output given as None is a fresh Tensor of the inputs' broadcast shape.  `lead`: arguments of the
    entry point before its operands (the activation code).  Returns the outputs as a tuple."""
    src = [_f32(name, obj) for name, obj in ins]
    fresh = lambda: newTensor(np.float32, *np.broadcast_shapes(*(v.shape for v in src)))
    outs = [(name, fresh() if obj is None else obj) for name, obj in outs]
    dst = [_f32(name, obj) for name, obj in outs]
    if any(d.shape != dst[0].shape for d in dst):
        raise ValueError(f"{fn}: the two destinations have shapes {dst[0].shape} and {dst[1].shape}")
    shape, r = dst[0].shape, dst[0].rank
    arr = lambda v: (C.c_int64 * max(r, 1))(*v)
    ops = [a for d in dst for a in (C.c_void_p(d.ptr), arr(d.strides))]
    ops += [a for v in src for a in (C.c_void_p(v.ptr), arr(_bcast_strides(v, shape)))]
    _lib.check(getattr(_lib.lib(), f"laser_hip_{fn}_f32_dev")(*lead, *ops, arr(shape), r, _stream()))
    return tuple(obj for _, obj in outs)


def _unary(fn, t, out, lead=()):
    """one input, one output; a host array goes through the host-pointer form: contiguous float32, synchronous"""
    if isinstance(t, np.ndarray):
        if t.dtype != np.float32:
            raise TypeError(f"host arrays: float32 only (got {t.dtype})")
        if out is not None:
            raise TypeError("out= is for device inputs; a host array returns its result")
        a = np.ascontiguousarray(t)
        r = np.empty_like(a)
        _lib.check(getattr(_lib.lib(), f"laser_hip_{fn}_f32")(*lead, r.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), a.size))
        return r
    return _elementwise(fn, (("out", out),), (("t", t),), lead)[0]


def exp(t, out=None):
    """lexp(t), elementwise.  `t` broadcasts against `out` like numpy; out=None: a fresh Tensor of t's shape."""
    return _unary("exp", t, out)


def log(t, out=None):
    """llog(t), elementwise: the natural logarithm of laser_amd/csrc/log_core.h, faithful (error below one ulp) and monotone
    over every positive float32; +-0 gives -Inf, a negative value NaN, a subnormal is taken as the number it is.  Operands
    as `exp`: a device tensor (`t` broadcasts against `out`) or a host float32 array."""
    return _unary("log", t, out)


_ACT_CODES = {"relu": 1, "tanh": 2, "sigmoid": 3}      # LASER_HIP_ACT_RELU / _TANH / _SIGMOID


def _act_code(kind):
    if kind not in _ACT_CODES:
        raise ValueError(f"activation: kind {kind!r} (one of {sorted(_ACT_CODES)})")
    return _ACT_CODES[kind]


def activation(t, kind, out=None):
    """relu, ltanh or lsigmoid of every element (kind "relu", "tanh", "sigmoid").  relu is x > 0 ? x : +0, the rule of the
    fused GEMM / conv epilogue (NaN and -0 give +0); ltanh and lsigmoid are laser_amd/csrc/act_core.h's: faithful, monotone,
    ltanh odd bit for bit, lsigmoid(0) = 0.5.  Operands as `exp`: a device tensor or view (`t` broadcasts against `out`, `out`
    may be `t`) or a host float32 array."""
    return _unary("act", t, out, (_act_code(kind),))


def tanh(t, out=None):
    """ltanh(t), elementwise: activation(t, "tanh")"""
    return activation(t, "tanh", out)


def sigmoid(t, out=None):
    """lsigmoid(t), elementwise: activation(t, "sigmoid")"""
    return activation(t, "sigmoid", out)


def activation_grad(dy, y, kind, out=None):
    """The gradient of activation(x, kind) from the incoming gradient `dy` and the forward OUTPUT `y`: relu y > 0 ? dy : +0,
    tanh t = y * y, u = 1 - t, dy * u; sigmoid u = 1 - y, v = y * u, dy * v -- float32 operations rounded one by one.  `dy`
    and `y` are device tensors or views and broadcast against `out`; out=None: a fresh Tensor of their broadcast shape; `out`
    may be `dy` or `y`."""
    return _elementwise("act_grad", (("out", out),), (("dy", dy), ("y", y)), (_act_code(kind),))[0]


def sin(t, out=None):
    """lsin(t), elementwise: the bit-defined float32 sine of laser_amd/csrc/sincos_core.h -- faithful for every finite input,
    odd bit for bit, lsin(x) = x for tiny and subnormal x, NaN (bits 0x7fc00000) for NaN and +-Inf.  Operands as `exp`: a
    device tensor or view (`t` broadcasts against `out`, `out` may be `t`) or a host float32 array."""
    return _unary("sin", t, out)


def cos(t, out=None):
    """lcos(t), elementwise: the bit-defined float32 cosine of the same header -- faithful, even bit for bit, 1 for tiny x"""
    return _unary("cos", t, out)


def sincos(t, out=None):
    """(lsin(t), lcos(t)) of a device tensor or view from one argument reduction: the bits of sin(t) and cos(t).  out=None:
    two fresh row-major Tensors; out=(s, c): written there (either may be `t`; they must not overlap each other)"""
    s, c = (None, None) if out is None else out
    return _elementwise("sincos", (("out[0]", s), ("out[1]", c)), (("t", t),))


def _collapse(dims):
    """(count, stride) of the (extent, stride) pairs `dims` as one dimension, None when they do not collapse into one;
    extent-1 dimensions do not count, and nothing left is (1, None)"""
    dims = [(e, s) for e, s in dims if e != 1]
    count = 1
    for (e, s), (e1, s1) in zip(dims, dims[1:]):
        if s != s1 * e1:
            return None
    for e, _ in dims:
        count *= e
    return count, (dims[-1][1] if dims else None)


def _axis_view(v, axis):
    """(outer, outer_stride, axis_stride, inner) of `v` with the softmax along `axis`, as the strip kernels see it (the dims
    after the axis one unit-stride run) and as the row kernels see it (the axis unit-stride, every other dim one stride);
    None where the view does not fit"""
    dims = list(zip(v.shape, v.strides))
    n, sa = dims[axis]
    pre, post = _collapse(dims[:axis]), _collapse(dims[axis + 1:])
    strip = rows = None
    if pre is not None and post is not None and post[1] in (None, 1):
        inner = post[0]
        strip = (pre[0], pre[1] if pre[1] is not None else 0, sa if n > 1 else inner, inner)      # n == 1: no axis stride to speak of
    others = _collapse(dims[:axis] + dims[axis + 1:])
    if others is not None and (n == 1 or sa == 1):
        rows = (others[0], others[1] if others[1] is not None else 0, 1, 1)
    return strip, rows


def softmax(t, out=None, axis=None):
    """Softmax over the rows of the 2-D `t` (last stride 1): y = lexp(x - max) / sum, the sum in the order of reduce_sum, so
    a row's result depends on its values and length alone.  A NaN in a row, or a row of all -Inf, gives a NaN row.
    With `axis` (negative counts from the end) `t` has rank 1 .. 6 and the softmax runs along that axis, every 1-D slice along
    it exactly as a row above.  The dims before the axis must collapse into one stride and the dims after it into one
    unit-stride run (any C-contiguous tensor, and slices of one that keep that); or the axis itself has stride 1 and all
    other dims collapse into one stride (the rows of a transposed view; `out` must then be such a view too).  Anything else:
    ValueError -- make it contiguous."""
    if axis is not None:
        return _softmax_axis(t, out, axis)
    src = _f32("t", t)
    if out is None:
        out = newTensor(np.float32, *src.shape)
    dst = _f32("out", out)
    for name, v in (("t", src), ("out", dst)):
        if v.rank != 2:
            raise ValueError(f"softmax: {name} has rank {v.rank} (a 2-D tensor is needed)")
        if v.shape[1] != 1 and v.strides[1] != 1:
            raise ValueError(f"softmax: {name} has last stride {v.strides[1]} (the elements of a row must be contiguous)")
    if dst.shape != src.shape:
        raise ValueError(f"softmax: out has shape {dst.shape}, t has {src.shape}")
    rows, n = src.shape
    if n < 1:
        raise ValueError("softmax: empty rows")
    # a single row has no row stride to speak of
    ds, ss = (dst.strides[0], src.strides[0]) if rows > 1 else (n, n)
    _lib.check(_lib.lib().laser_hip_softmax_rows_f32_dev(C.c_void_p(dst.ptr), ds, C.c_void_p(src.ptr), ss, rows, n, _stream()))
    return out


def _grad_rows(name, v, shape=None):
    """(rows, row stride, n) of a softmax_backward operand: the last axis unit-stride, the leading dims one stride"""
    if v.rank < 2:
        raise ValueError(f"softmax_backward: {name} has rank {v.rank} (rows: rank 2 or more is needed)")
    if shape is not None and v.shape != shape:
        raise ValueError(f"softmax_backward: {name} has shape {v.shape}, dy has {shape}")
    n = v.shape[-1]
    if n < 1:
        raise ValueError("softmax_backward: empty rows")
    if n != 1 and v.strides[-1] != 1:
        raise ValueError(f"softmax_backward: {name} has last stride {v.strides[-1]} (the elements of a row must be contiguous)")
    lead = _collapse(list(zip(v.shape[:-1], v.strides[:-1])))
    if lead is None:
        raise ValueError(f"softmax_backward: the leading dims of {name} (shape {v.shape}, strides {v.strides}) do not collapse "
                         "into one row stride (make it contiguous)")
    rows, stride = lead
    return rows, (stride if rows > 1 and stride is not None else n), n


def softmax_backward(dy, y, out=None):
    """The gradient of softmax over the last axis from the incoming gradient `dy` and the softmax's OUTPUT `y`:
    D = reduce_sum(dy * y) per row (every product rounded, the sum in the order of the reductions), then
    dx = y * (dy - D), a rounded subtraction and a rounded multiplication -- a row's result depends on its values and length
    alone.  `dy`, `y` and `out` are device tensors or views of one shape, rank 2 or more, the last axis contiguous and the
    leading dims collapsing into one row stride; out=None: a fresh Tensor; `out` may be `dy` or `y`.  1 <= n <= 2^26."""
    vdy = _f32("dy", dy)
    rows, dys, n = _grad_rows("dy", vdy)
    vy = _f32("y", y)
    _, ys, _ = _grad_rows("y", vy, vdy.shape)
    if out is None:
        out = newTensor(np.float32, *vdy.shape)
    vdx = _f32("out", out)
    _, dxs, _ = _grad_rows("out", vdx, vdy.shape)
    if rows == 0:
        return out
    _lib.check(_lib.lib().laser_hip_softmax_grad_rows_f32_dev(C.c_void_p(vdx.ptr), dxs, C.c_void_p(vdy.ptr), dys, C.c_void_p(vy.ptr), ys,
                                                              rows, n, _stream()))
    return out


def _softmax_axis(t, out, axis):
    src = _f32("t", t)
    if not 1 <= src.rank <= 6:
        raise ValueError(f"softmax: t has rank {src.rank} (1 .. 6 with axis=)")
    if not isinstance(axis, (int, np.integer)) or not -src.rank <= axis < src.rank:
        raise ValueError(f"softmax: axis {axis!r} outside a tensor of rank {src.rank}")
    axis = int(axis) % src.rank
    if out is None:
        out = newTensor(np.float32, *src.shape)
    dst = _f32("out", out)
    if dst.shape != src.shape:
        raise ValueError(f"softmax: out has shape {dst.shape}, t has {src.shape}")
    n = src.shape[axis]
    if n < 1:
        raise ValueError("softmax: empty axis")
    if 0 in src.shape:
        return out
    for s, d in zip(_axis_view(src, axis), _axis_view(dst, axis)):
        if s is not None and d is not None:
            _lib.check(_lib.lib().laser_hip_softmax_axis_f32_dev(C.c_void_p(dst.ptr), d[1], d[2], C.c_void_p(src.ptr), s[1], s[2],
                                                                 s[0], n, s[3], _stream()))
            return out
    raise ValueError(f"softmax: axis {axis} of shapes {src.shape} with strides {src.strides} (t) and {dst.strides} (out): the dims "
                     "before the axis must collapse into one stride and the dims after it into one unit-stride run, in both "
                     "(make the tensor contiguous)")


def _rows_view(op, name, v, axis):
    """(rows, row stride, n) of `v` as rows of n contiguous elements: a 2-D operand with last stride 1, or with `axis` one
    whose axis has stride 1 while all other dims collapse into one stride"""
    if axis is None:
        if v.rank != 2:
            raise ValueError(f"{op}: {name} has rank {v.rank} (a 2-D tensor is needed)")
        if v.shape[1] != 1 and v.strides[1] != 1:
            raise ValueError(f"{op}: {name} has last stride {v.strides[1]} (the elements of a row must be contiguous)")
        rows, n = v.shape
        return rows, (v.strides[0] if rows > 1 else n), n
    n = v.shape[axis]
    if 0 in v.shape:
        return 0, max(n, 1), n
    fit = _axis_view(v, axis)[1]
    if fit is None or (fit[0] > 1 and fit[1] < n):
        raise ValueError(f"{op}: axis {axis} of {name} (shape {v.shape}, strides {v.strides}) is not the unit-stride one with all "
                         "other dims collapsing into one row stride; these kernels run along contiguous rows only -- move the axis "
                         "last first (transpose2D_batched)")
    return fit[0], (fit[1] if fit[0] > 1 else n), n


def _axis_arg(op, v, axis):
    if axis is None:
        return None
    if not 1 <= v.rank <= 6:
        raise ValueError(f"{op}: t has rank {v.rank} (1 .. 6 with axis=)")
    if not isinstance(axis, (int, np.integer)) or not -v.rank <= axis < v.rank:
        raise ValueError(f"{op}: axis {axis!r} outside a tensor of rank {v.rank}")
    return int(axis) % v.rank


def logsumexp(t, out=None, axis=None):
    """One value per row of the 2-D `t` (last stride 1): max + llog(sum of lexp(x - max)), max and sum exactly those of
    `softmax`, so it depends on the row's values and length alone.  A row whose maximum is +Inf gives +Inf, a row of all -Inf
    gives -Inf, a NaN in the row NaN.  Returns (or fills `out`, of) shape (rows,).  `axis` is accepted where that axis has
    stride 1 and all other dims collapse into one row stride (the result then has t's shape without the axis); any other
    layout: ValueError -- move the axis last with transpose2D_batched."""
    src = _f32("t", t)
    axis = _axis_arg("logsumexp", src, axis)
    rows, ss, n = _rows_view("logsumexp", "t", src, axis)
    shape = (rows,) if axis is None else src.shape[:axis] + src.shape[axis + 1:]
    if out is None:
        out = newTensor(np.float32, *shape)
    dst = _f32("out", out)
    if dst.shape != tuple(shape):
        raise ValueError(f"logsumexp: out has shape {dst.shape}, {tuple(shape)} is needed")
    if n < 1:
        raise ValueError("logsumexp: empty rows")
    if rows == 0:
        return out
    one = _collapse(list(zip(dst.shape, dst.strides)))
    if one is None:
        raise ValueError(f"logsumexp: out (shape {dst.shape}, strides {dst.strides}) does not collapse into one stride")
    ds = one[1] if one[1] is not None else 1
    if ds < 1:
        raise ValueError(f"logsumexp: out has stride {ds} (a positive stride is needed)")
    _lib.check(_lib.lib().laser_hip_logsumexp_rows_f32_dev(C.c_void_p(dst.ptr), ds, C.c_void_p(src.ptr), ss, rows, n, _stream()))
    return out


def log_softmax(t, out=None, axis=None):
    """log of the softmax over the rows of the 2-D `t` (last stride 1), without its underflow: y = (x - max) - llog(sum), two
    rounded subtractions, max and sum exactly those of `softmax`.  Every finite result is <= 0; a NaN in a row or a row of all
    -Inf gives a NaN row.  `out` may be `t`.  `axis` as in logsumexp (t and out must both fit)."""
    src = _f32("t", t)
    axis = _axis_arg("log_softmax", src, axis)
    if out is None:
        out = newTensor(np.float32, *src.shape)
    dst = _f32("out", out)
    if dst.shape != src.shape:
        raise ValueError(f"log_softmax: out has shape {dst.shape}, t has {src.shape}")
    rows, ss, n = _rows_view("log_softmax", "t", src, axis)
    _, ds, _ = _rows_view("log_softmax", "out", dst, axis)
    if n < 1:
        raise ValueError("log_softmax: empty rows")
    if rows == 0:
        return out
    _lib.check(_lib.lib().laser_hip_log_softmax_rows_f32_dev(C.c_void_p(dst.ptr), ds, C.c_void_p(src.ptr), ss, rows, n, _stream()))
    return out


def softmax_cross_entropy(logits, labels, grad=False, scale=1.0):
    """The softmax cross-entropy of the rows of the 2-D `logits` (last stride 1) against integer `labels` (int32, one per row,
    on the device: what the samplers return), in one launch: loss = llog(sum) - (x[label] - max), a fresh Tensor (rows,).
    grad=True returns (loss, grad) with grad = (softmax(logits) - onehot(labels)) * scale, a fresh Tensor like logits whose
    softmax has exactly the bits of `softmax`; scale is 1 for a summed loss and 1 / rows for a mean.  A label of -1 is
    ignored (loss +0, gradient row +0); any other label outside [0, n) gives a NaN loss and a NaN gradient row."""
    src = _f32("logits", logits)
    rows, ss, n = _rows_view("softmax_cross_entropy", "logits", src, None)
    lab = _View("labels", labels)
    if lab.dtype != np.int32:
        raise TypeError(f"softmax_cross_entropy: labels have element type {lab.dtype} (int32 only)")
    one = _collapse(list(zip(lab.shape, lab.strides)))
    count = 1
    for e in lab.shape:
        count *= e
    if count != rows or lab.rank < 1 or one is None or one[1] not in (None, 1):
        raise ValueError(f"softmax_cross_entropy: labels of shape {lab.shape}, strides {lab.strides} ({rows} contiguous labels, one per "
                         "row, are needed)")
    if n < 1:
        raise ValueError("softmax_cross_entropy: empty rows")
    loss = newTensor(np.float32, rows)
    g = newTensor(np.float32, rows, n) if grad else None
    if rows:
        _lib.check(_lib.lib().laser_hip_softmax_xent_rows_f32_dev(
            C.c_void_p(_View("loss", loss).ptr), 1, C.c_void_p(_View("grad", g).ptr) if grad else None, n, C.c_void_p(src.ptr), ss,
            C.c_void_p(lab.ptr), rows, n, float(scale), _stream()))
    return (loss, g) if grad else loss
