"""Optimizer steps over a whole list of parameter tensors, float32 (include/laser_hip.h "Optimizer steps"):

    laser_amd.sgd_step(params, grads, momentum=None, lr=..., mu=0, wd=0, nesterov=False, gscale=1, clip=None)
    laser_amd.adam_step(params, grads, m, v, step, lr=..., b1=.9, b2=.999, eps=1e-8, wd=0, decoupled=False, gscale=1, clip=None)
    laser_amd.grad_norm(grads, max_norm=inf) -> (norm, clip)        one-element device Tensors; clip feeds a step's clip=
    laser_amd.adam_bias_correction(beta, step) -> 1 - beta^step     the float32 the library computes, no device needed
    laser_amd.SGD(params, lr, ...), laser_amd.Adam(params, lr, ...)  hold the zero-initialised state and the step count

One call updates every tensor of the list in place, ceil(count / 64) launches; every float32 operation is rounded on its own
(laser_amd/csrc/optim_core.h is the definition), so an element's new value depends on its own w, g, m, v and the scalars
alone.  The clip factor of grad_norm stays on the device: nothing is read back between the backward pass and the update.
Operands are laser_amd.Tensors or torch CUDA tensors, float32 and contiguous, of any shape; calls are asynchronous on the
current torch stream.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .simd_math import _f32
from .tensor import _stream, newTensor

__all__ = ["sgd_step", "adam_step", "grad_norm", "adam_bias_correction", "SGD", "Adam", "OPTIM_MAX_LEN", "OPTIM_MAX_COUNT"]

OPTIM_MAX_LEN = 1 << 26
OPTIM_MAX_COUNT = 65536


def _flat(fn, name, obj):
    """(address, elements) of a contiguous float32 operand of any shape.  laser_amd.Tensors and torch tensors are read from
    their own fields (a list of a few hundred parameters is walked on every step); anything else through
    __cuda_array_interface__."""
    if getattr(obj, "_laser_hip_tensor", False):
        if obj.dtype != np.float32:
            raise TypeError(f"{name}: element type {obj.dtype} (float32 only)")
        if not obj.is_C_contiguous():
            raise ValueError(f"{fn}: {name} has shape {obj.shape}, strides {obj.strides} (contiguous is needed)")
        acc = obj.size
        ptr = obj.unsafe_raw_data() if acc else 0
    elif type(obj).__module__.startswith("torch") and hasattr(obj, "data_ptr"):
        if not obj.is_cuda:
            raise TypeError(f"operand {name}: a torch tensor on {obj.device} (a device array is needed)")
        if str(obj.dtype) != "torch.float32":
            raise TypeError(f"{name}: element type {obj.dtype} (float32 only)")
        if not obj.is_contiguous():
            raise ValueError(f"{fn}: {name} has shape {tuple(obj.shape)}, strides {tuple(obj.stride())} (contiguous is needed)")
        acc = obj.numel()
        ptr = obj.data_ptr() if acc else 0
    else:
        v = _f32(name, obj)
        acc = 1
        for e, st in zip(reversed(v.shape), reversed(v.strides)):
            if e > 1 and st != acc:
                raise ValueError(f"{fn}: {name} has shape {v.shape}, strides {v.strides} (contiguous is needed)")
            acc *= e
        ptr = v.ptr if acc else 0
    if acc > OPTIM_MAX_LEN:
        raise ValueError(f"{fn}: {name} has {acc} elements (at most 2^26 per tensor)")
    return ptr, acc


def _list(fn, name, ops, lens=None, first="params"):
    """(pointer array, lens array) of one list of operands; with `lens` (the first list's) the element counts must agree"""
    ops = list(ops)
    count = len(ops)
    if count > OPTIM_MAX_COUNT:
        raise ValueError(f"{fn}: {count} tensors (at most 65536 per call)")
    if lens is not None and count != len(lens):
        raise ValueError(f"{fn}: {name} has {count} tensors, {first} has {len(lens)}")
    flat = [_flat(fn, f"{name}[{k}]", obj) for k, obj in enumerate(ops)]
    if lens is None:
        lens = (C.c_int64 * count)(*[n for _, n in flat])
    else:
        for k, (_, n) in enumerate(flat):
            if n != lens[k]:
                raise ValueError(f"{fn}: {name}[{k}] has {n} elements, {first}[{k}] has {lens[k]}")
    return (C.c_void_p * count)(*[p or None for p, _ in flat]), lens


def _lists(fn, named):
    """(count, lens array, one pointer array per list) of equally long lists of operands with equal element counts"""
    arrays, lens = [], None
    for name, ops in named:
        arr, lens = _list(fn, name, ops, lens, named[0][0])
        arrays.append(arr)
    return len(lens), lens, arrays


def _clip_ptr(fn, clip):
    if clip is None:
        return None
    v = _f32("clip", clip)
    size = 1
    for e in v.shape:
        size *= e
    if size != 1:
        raise ValueError(f"{fn}: clip has shape {v.shape} (one device float is needed: grad_norm's second result)")
    return C.c_void_p(v.ptr)


def adam_bias_correction(beta, step):
    """1 - beta^step as the float32 every mirror of the library uses: beta^step in double by square-and-multiply from the low
    bit, one subtraction, one rounding.  step >= 1."""
    out = C.c_float()
    _lib.check(_lib.lib().laser_hip_adam_bias_correction(float(beta), int(step), C.byref(out)))
    return out.value


def _sgd_call(fn, count, lens, w, g, m, lr, mu, wd, nesterov, gscale, clip):
    if lr is None:
        raise ValueError(f"{fn}: lr is needed")
    if m is None and (float(mu) != 0.0 or nesterov):
        raise ValueError(f"{fn}: mu = {mu!r}, nesterov = {nesterov!r} need the momentum list")
    _lib.check(_lib.lib().laser_hip_sgd_step_f32_dev(w, g, m, lens, count, float(lr), float(mu), float(wd), int(bool(nesterov)),
                                                     float(gscale), _clip_ptr(fn, clip), _stream()))


def _adam_call(fn, count, lens, w, g, m, v, step, lr, b1, b2, eps, wd, decoupled, gscale, clip):
    if lr is None:
        raise ValueError(f"{fn}: lr is needed")
    step = int(step)
    if step < 1:
        raise ValueError(f"{fn}: step = {step} (steps count from 1)")
    bc1, bc2 = adam_bias_correction(b1, step), adam_bias_correction(b2, step)
    _lib.check(_lib.lib().laser_hip_adam_step_f32_dev(w, g, m, v, lens, count, float(lr), float(b1), float(b2), float(eps), float(wd),
                                                      int(bool(decoupled)), bc1, bc2, float(gscale), _clip_ptr(fn, clip), _stream()))


def sgd_step(params, grads, momentum=None, lr=None, mu=0.0, wd=0.0, nesterov=False, gscale=1.0, clip=None):
    """One SGD step on every tensor of `params`, in place: g' = g * gscale [* clip] [+ wd * w]; with `momentum` (a list of
    state tensors, zeros before the first step) m = mu * m + g' and d = g' + mu * m (nesterov) or m; without, d = g';
    w -= lr * d.  mu != 0 or nesterov needs the momentum list.  `clip`: grad_norm's second result."""
    named = [("params", params), ("grads", grads)] + ([("momentum", momentum)] if momentum is not None else [])
    count, lens, arrs = _lists("sgd_step", named)
    _sgd_call("sgd_step", count, lens, arrs[0], arrs[1], arrs[2] if momentum is not None else None, lr, mu, wd, nesterov, gscale, clip)


def adam_step(params, grads, m, v, step, lr=None, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False, gscale=1.0, clip=None):
    """One Adam step on every tensor of `params`, in place, `step` counting from 1: m = b1 * m + (1 - b1) * g',
    v = b2 * v + ((1 - b2) * g') * g', w -= lr * (m / bc1) / (sqrt(v / bc2) + eps) with bc = adam_bias_correction(b, step).
    wd: added to the gradient (wd * w), or with decoupled=True taken from the weight (w -= (lr * wd) * w, AdamW).  `m` and
    `v`: lists of state tensors, zeros before the first step."""
    count, lens, arrs = _lists("adam_step", [("params", params), ("grads", grads), ("m", m), ("v", v)])
    _adam_call("adam_step", count, lens, arrs[0], arrs[1], arrs[2], arrs[3], step, lr, b1, b2, eps, wd, decoupled, gscale, clip)


def grad_norm(grads, max_norm=math.inf):
    """(norm, clip) of a list of gradient tensors, one-element device Tensors: norm = sqrt of the sum over the list, in list
    order, of reduce_sum(g * g) of each tensor; clip = max_norm / norm when norm > max_norm, else 1.  Nothing comes back to
    the host: pass `clip` to sgd_step / adam_step.  max_norm >= 0; inf never clips."""
    fn = "grad_norm"
    max_norm = float(max_norm)
    if not max_norm >= 0.0:
        raise ValueError(f"{fn}: max_norm = {max_norm!r} (max_norm >= 0 is needed)")
    count, lens, arrs = _lists(fn, [("grads", grads)])
    both = newTensor(np.float32, 2)                # one allocation; the results are its two one-element views
    norm, clip = both[0:1], both[1:2]
    _lib.check(_lib.lib().laser_hip_grad_norm_f32_dev(C.c_void_p(_f32("norm", norm).ptr), C.c_void_p(_f32("clip", clip).ptr), arrs[0],
                                                      lens, count, max_norm, _stream()))
    return norm, clip


def _zeros_like(fn, params):
    state = []
    for k, p in enumerate(params):
        _flat(fn, f"params[{k}]", p)
        state.append(newTensor(np.float32, *(int(e) for e in p.shape)))
    return state


class SGD:
    """The state of sgd_step for one parameter list: the momentum tensors (zeros; none with mu = 0 and no nesterov).  The
    pointer lists of the parameters and the state are built once; a step reads the gradients' addresses only."""

    def __init__(self, params, lr, mu=0.0, wd=0.0, nesterov=False):
        self.params = list(params)
        self.lr, self.mu, self.wd, self.nesterov = lr, mu, wd, nesterov
        self.momentum = _zeros_like("SGD", self.params) if (float(mu) != 0.0 or nesterov) else None
        self.steps = 0
        named = [("params", self.params)] + ([("momentum", self.momentum)] if self.momentum is not None else [])
        self._count, self._lens, self._lists = _lists("SGD", named)

    def step(self, grads, clip=None, gscale=1.0):
        g, _ = _list("SGD.step", "grads", grads, self._lens)
        _sgd_call("SGD.step", self._count, self._lens, self._lists[0], g, self._lists[1] if self.momentum is not None else None, self.lr,
                  self.mu, self.wd, self.nesterov, gscale, clip)
        self.steps += 1


class Adam:
    """The state of adam_step for one parameter list: m and v (zeros) and the step count.  The pointer lists of the
    parameters and the state are built once; a step reads the gradients' addresses only."""

    def __init__(self, params, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False):
        self.params = list(params)
        self.lr, self.b1, self.b2, self.eps, self.wd, self.decoupled = lr, b1, b2, eps, wd, decoupled
        self.m = _zeros_like("Adam", self.params)
        self.v = _zeros_like("Adam", self.params)
        self.steps = 0
        self._count, self._lens, self._lists = _lists("Adam", [("params", self.params), ("m", self.m), ("v", self.v)])

    def step(self, grads, clip=None, gscale=1.0):
        g, _ = _list("Adam.step", "grads", grads, self._lens)
        _adam_call("Adam.step", self._count, self._lens, self._lists[0], g, self._lists[1], self._lists[2], self.steps + 1, self.lr, self.b1,
                   self.b2, self.eps, self.wd, self.decoupled, gscale, clip)
        self.steps += 1
