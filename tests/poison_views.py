"""Non-finite values where a GEMM or a convolution must not look, and a few where it must.  Used by tests/test_poison_cpu.py (the
helpers themselves, no device) and tests/test_gpu_poison.py.

The kernels discard data in one way: they load from a clamped or padded address and zero the value afterwards, or they multiply it
by a zero of the other operand.  With finite data both give +0, so the bit-exact tests on seeded data cannot tell them apart; with
Inf or NaN in the discarded place the second gives NaN.  The claim under test: a non-finite value reaches exactly the elements of C
(or of the convolution output) that IEEE arithmetic on the ADDRESSED operands says it reaches; every other element keeps the bits of
the clean run.

Two kinds of poison over the arenas of tests/batched_views.py (that module is not changed: its arenas, its expected() cache and the
recorded route sets stay as they are):

  gap_poisoned(c)      every element of the A and B arenas the views do not address (leading-dimension gaps, the elements between
                       strided ones, the slack on both sides) holds a NaN pattern, +Inf or -Inf: C must keep every bit
  element_poisoned(c)  a few addressed elements are NaN / +Inf: whole rows and columns of C become non-finite, the others keep
                       their bits.  `special` is the expected class of every C element, from a plain float64 evaluation.

conv_poison() does the same for an NCHW input, its filter and bias: guard bands around the dense operands, a few poisoned pixels, one
poisoned weight where there is no padding.
"""
import collections
import zlib

import numpy as np

from tests import batched_views as BV

FINITE, NAN, PINF, NINF = 0, 1, 2, 3
CAP = 0.6            # at least this share of every case's elements is expected finite, so still compared bit for bit
GUARD = 256          # elements of poison on each side of a convolution operand (a multiple of 64: the operand's alignment class stays)


def poison(n, dtype, phase=0):
    """n non-finite values: BV.nan_patterns (quiet and signalling, both signs, varying payloads) with every fifth and sixth
    element replaced by +Inf and -Inf"""
    out = np.array(BV.nan_patterns(n + phase, dtype)[phase:], copy=True)
    i = np.arange(n) + phase
    out[i % 6 == 4] = np.inf
    out[i % 6 == 5] = -np.inf
    return out


def classify(x):
    """the class of every element: FINITE, NAN, PINF or NINF"""
    x = np.asarray(x)
    out = np.full(x.shape, FINITE, dtype=np.int8)
    out[np.isnan(x)] = NAN
    out[np.isposinf(x)] = PINF
    out[np.isneginf(x)] = NINF
    return out


def addressed_mask(v, batch, rows, cols, n):
    mask = np.zeros(n, dtype=bool)
    mask[BV.element_offsets(v, batch, rows, cols).ravel()] = True
    return mask


_GAP = collections.OrderedDict()
_ELEMENT = collections.OrderedDict()
_PRODUCT = {}


def _keep(cache, key, value, n=4):
    cache[key] = value
    while len(cache) > n:
        cache.popitem(last=False)
    return value


def _key(c):
    return (c.layout, c.dtype.name, c.batch, c.M, c.N, c.K)


def gap_poisoned(c):
    """(A arena, B arena), read-only: BV.arenas(c) with every element the views do not address -- the complement of
    BV.element_offsets over the arena -- replaced by poison(); the addressed elements keep their bits"""
    key = _key(c)
    if key in _GAP:
        _GAP.move_to_end(key)
        return _GAP[key]
    a, b, _, _ = BV.arenas(c)
    out = []
    for arena, v, which in ((a, c.A, "A"), (b, c.B, "B")):
        rows, cols = BV.dims(c, which)
        mask = addressed_mask(v, c.batch, rows, cols, arena.size)
        buf = np.array(arena, copy=True)
        buf[~mask] = poison(int((~mask).sum()), c.dtype, phase=len(out))
        buf.setflags(write=False)
        out.append(buf)
    return _keep(_GAP, key, tuple(out))


def element_positions(c):
    """({(row, col): value} of A, the same of B): the addressed elements element_poisoned() makes non-finite in every entry.
    A NaN in A makes a row of C NaN, one in B a column; with N < 8 only rows are poisoned, with M < 8 only columns, with both
    nothing, so that the matrix-vector shapes take part without becoming all NaN."""
    pa, pb = {}, {}
    if c.M >= 8:
        pa[(c.M - 1, c.K - 1)] = np.nan         # the last element of the operand
        pa[(1, 0)] = np.nan                     # the element after a row's end
    if c.N >= 8:
        pb[(c.K - 1, c.N - 1)] = np.inf
        pb[(0, 2)] = np.nan
    return pa, pb


def element_poisoned(c):
    """(A arena, B arena, special), read-only: BV.arenas(c) with the elements of element_positions() made non-finite in every
    entry p, through the view's own offsets (an element that several entries share or slide over is poisoned for each of them);
    special [batch][M][N] = classify() of alpha * A @ B + beta * C0 in float64 on the gathered poisoned views, by a plain
    einsum (never BLAS, never the library)"""
    key = _key(c)
    if key in _ELEMENT:
        _ELEMENT.move_to_end(key)
        a, b = _ELEMENT[key]
        prod = _PRODUCT[key]
    else:
        a0, b0, _, _ = BV.arenas(c)
        a, b = np.array(a0, copy=True), np.array(b0, copy=True)
        pa, pb = element_positions(c)
        for buf, v, which, pos in ((a, c.A, "A", pa), (b, c.B, "B", pb)):
            rows, cols = BV.dims(c, which)
            off = BV.element_offsets(v, c.batch, rows, cols)
            for (r, k), value in pos.items():
                buf[off[:, r, k]] = value
        if key not in _PRODUCT:                  # the float64 product is computed once per (layout, shape, type) and kept
            A = BV.gather(a, c.A, c.batch, c.M, c.K).astype(np.float64)
            B = BV.gather(b, c.B, c.batch, c.K, c.N).astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                _PRODUCT[key] = np.einsum("pik,pkj->pij", A, B, optimize=False)
            _PRODUCT[key].setflags(write=False)
        prod = _PRODUCT[key]
        for x in (a, b):
            x.setflags(write=False)
        _keep(_ELEMENT, key, (a, b))
    _, _, C0 = BV.operands(c)
    with np.errstate(invalid="ignore", over="ignore"):
        full = float(c.alpha) * prod
        if c.beta != 0:                          # beta = 0 never reads C0
            full = full + float(c.beta) * np.asarray(C0, dtype=np.float64)
    special = classify(full)
    special.setflags(write=False)
    return a, b, special


def check_result(got, clean, special, tanh=False):
    """None, or what is wrong with `got` under the claim: where special is FINITE the bits of the clean result, where it is NAN a
    NaN of any payload, where it is PINF / NINF that infinity -- or, behind a fused tanh, exactly +1 / -1 (tanh(+-Inf) = +-1)"""
    got, clean = np.asarray(got), np.asarray(clean)
    assert got.shape == clean.shape == special.shape, (got.shape, clean.shape, special.shape)
    isp, isn = (np.isposinf, np.isneginf) if not tanh else (lambda x: x == 1, lambda x: x == -1)
    fin = special == FINITE
    bad = fin & (BV.bits(got) != BV.bits(clean))
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        return f"{int(bad.sum())} of {int(fin.sum())} elements expected finite lost their bits, first at {at}: got {got[at]!r} want {clean[at]!r}"
    for cls, test, name in ((NAN, np.isnan, "NaN"), (PINF, isp, "tanh(+Inf)" if tanh else "+Inf"), (NINF, isn, "tanh(-Inf)" if tanh else "-Inf")):
        bad = (special == cls) & ~test(got)
        if bad.any():
            at = tuple(int(v) for v in np.argwhere(bad)[0])
            return f"{int(bad.sum())} elements expected {name} are not, first at {at}: got {got[at]!r}"
    return None


def finite_share(special):
    return float((special == FINITE).mean())


# ---- convolution --------------------------------------------------------------------------------------------------------------
ConvPoison = collections.namedtuple("ConvPoison", "x w bias x_poison special w_poison w_special w_channel")


def guarded(x, phase=0):
    """(flat buffer, start): the dense operand between two guard bands of GUARD poison values; buffer[start:start + x.size] is x"""
    flat = np.ascontiguousarray(x).ravel()
    buf = np.concatenate([poison(GUARD, x.dtype, phase), flat, poison(GUARD, x.dtype, phase + 3)])
    return buf, GUARD


def conv_reference(x, w, pad, st, bias=None):
    """float64 direct convolution [n][c_out][oH][oW]: real zeros as padding, then the windows and one einsum"""
    x8 = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (pad[0], pad[0]), (pad[1], pad[1])))
    win = np.lib.stride_tricks.sliding_window_view(x8, w.shape[2:], axis=(2, 3))[:, :, ::st[0], ::st[1]]
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.einsum("nchwyx,ocyx->nohw", win, w.astype(np.float64), optimize=False)
        if bias is not None:
            out = out + bias.astype(np.float64).reshape(1, -1, 1, 1)
    return out


def conv_poison(ishape, kshape, pad, st, seed):
    """The clean float32 input, filter and bias (uniform(-1, 1), no zeros); a poisoned input with NaN at (0, 0, 0, 0), at the last
    element, at the first pixel of image 1 (when there is one) and at one interior pixel, and +Inf at one border pixel of another
    channel; `special`, the expected class of every output element from conv_reference() of the poisoned input.  With pad == (0,
    0) also w_poison, the filter with one NaN at w[w_channel, C - 1, kH - 1, kW - 1], and its classes w_special (output channel
    w_channel NaN everywhere, nothing else); None otherwise: what a NaN weight does against a zero-padded border is left
    undefined (the materialised im2col says NaN, a tap-skipping kernel says finite).  guarded() adds the guard bands."""
    n, C, H, W = ishape
    Co = kshape[0]
    rng = np.random.default_rng(seed)

    def draw(shape):
        v = rng.uniform(-1, 1, shape).astype(np.float32)
        v[v == 0] = 0.5
        return v
    x, w, bias = draw(ishape), draw(kshape), draw((Co,))
    xp = x.copy()
    xp[0, 0, 0, 0] = np.nan
    xp[n - 1, C - 1, H - 1, W - 1] = np.nan
    if n > 1:
        xp[1, 0, 0, 0] = np.nan
    xp[n // 2, C // 2, H // 2, W // 2] = np.nan
    xp[0, (C // 2 + 1) % C, H // 3, W - 1] = np.inf
    special = classify(conv_reference(xp, w, pad, st))
    wp = wspecial = co0 = None
    if tuple(pad) == (0, 0):
        co0 = Co // 2
        wp = w.copy()
        wp[co0, C - 1, kshape[2] - 1, kshape[3] - 1] = np.nan
        wspecial = classify(conv_reference(x, wp, pad, st))
    for v in (x, w, bias, xp, special, wp, wspecial):
        if v is not None:
            v.setflags(write=False)
    return ConvPoison(x, w, bias, xp, special, wp, wspecial, co0)


# (input shape, filter shape, padding, strides): one geometry per kernel class of conv2d_im2col (tests/test_gpu_poison.py says
# which options put each on its route)
CONV_GEOMETRIES = [
    ((2, 4, 17, 19), (7, 4, 5, 3), (2, 1), (2, 1)),         # the direct small-channel kernels
    ((2, 3, 20, 34), (3, 3, 3, 3), (0, 0), (1, 1)),         # their scalar-filter forms
    ((2, 12, 11, 13), (5, 12, 3, 3), (1, 1), (1, 1)),
    ((2, 8, 12, 16), (40, 8, 3, 3), (1, 1), (1, 1)),        # W % 4 == 0: the implicit loaders, the LDS input patch
    ((2, 8, 12, 15), (40, 8, 3, 2), (0, 0), (1, 2)),        # W % 4 != 0, no padding: the per-element gather
    ((1, 5, 20, 22), (33, 5, 6, 7), (2, 3), (1, 1)),        # the assembly loader, K = 210 padded
    ((2, 3, 30, 30), (64, 3, 7, 7), (3, 3), (2, 2)),        # the assembly loader, K = 147 padded to 148
    ((2, 60, 13, 14), (48, 60, 3, 3), (1, 1), (1, 1)),      # 182 pixels an image: one 128-pixel tile and a tail of 54; K = 540, two kc slices
    ((3, 32, 14, 16), (130, 32, 3, 3), (1, 1), (1, 1)),     # the unit walkers
    ((2, 16, 9, 11), (20, 16, 1, 1), (0, 0), (1, 1)),       # 1x1 / stride 1 / pad 0: the GEMM shortcut
]
