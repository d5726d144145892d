"""GEMM on operands whose spans reach and pass 2^31 / 2^32 bytes (tests/far_views.py): every hand-written 32-bit guard of the
launchers from both sides, and the 64-bit address arithmetic of whichever kernel takes the view behind a declined guard.
One arena per test holds every operand; each case checks the result in the C view against the oracle (bit for bit), that
nothing else in the arena changed (the int64 sum of the arena as int32 words moves by exactly the change inside C), and, on
the `inside` case of an assembly guard with the assembly kernels forced, that they really ran."""
import numpy as np
import pytest

from tests import exp_model
from tests import far_views as FV

pytestmark = pytest.mark.gpu

GIB = 2 ** 30


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import laser_amd
    assert laser_amd.lib().laser_hip_arch().decode().startswith("gfx950")
    return laser_amd


# ---- the arena ----------------------------------------------------------------------------------------------------------
def _arena(nbytes, seed):
    """One device buffer of int32 words with a reproducible random pattern; skips when the device has not that much free."""
    import torch
    assert nbytes <= FV.CAP and nbytes % 4 == 0
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes + 2 * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB free on the device, the arena needs {nbytes / GIB:.1f} + 2 GiB")
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (nbytes // 4,), dtype=torch.int32, device="cuda", generator=g)


def _free(la):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    la.tensor.trimStorageCache()


def _typed(arena, dtype):
    import torch
    return arena.view(getattr(torch, np.dtype(dtype).name))


def _tview(typed, v):
    """torch view of a far_views.View, and the axes to flip (torch has no negative strides: the view is taken from its lowest
    address and flipped on the host side)"""
    off, strides, flips = v.offset, [], []
    for ax, (n, s) in enumerate(zip(v.shape, v.strides)):
        if s < 0:
            off += (n - 1) * s
            flips.append(ax)
        strides.append(abs(s))
    return typed.as_strided(v.shape, strides, off), flips


def _put(typed, v, host):
    import torch
    t, flips = _tview(typed, v)
    host = np.flip(host, flips) if flips else host
    if 0 in v.strides:           # a shared batch operand: write one matrix
        idx = tuple(0 if s == 0 else slice(None) for s in v.strides)
        t[idx].copy_(torch.from_numpy(np.array(host[idx], order="C")).cuda())
    else:
        t.copy_(torch.from_numpy(np.array(host, order="C")).cuda())


def _get(typed, v):
    t, flips = _tview(typed, v)
    host = t.cpu().numpy()
    return np.flip(host, flips) if flips else host


def _ptr(typed, v):
    """what the caller passes: a tensor whose data pointer is the view's first element"""
    return typed.narrow(0, v.offset, 1)


def _words(arena, v, size):
    """the int32 words that cover the view (a superset of its bytes that shares no word with anything else used)"""
    if size >= 4:
        w = size // 4
        return arena.as_strided(tuple(v.shape) + (w,), tuple(s * w for s in v.strides) + (1,), v.offset * w)
    per = 4 // size
    assert (v.offset * size) % 4 == 0 and all((s * size) % 4 == 0 for s in v.strides[:-1]) and v.strides[-1] in (1, 2)
    row = -(-((v.shape[-1] - 1) * v.strides[-1] + 1) // per)
    return arena.as_strided(tuple(v.shape[:-1]) + (row,), tuple(s // per for s in v.strides[:-1]) + (1,), v.offset // per)


# ---- which kernels, by element type ---------------------------------------------------------------------------------------
DEFAULTS = dict(f32_asm=1, asm_tile=-1, slice_parallel=1, f64_asm=1, i32_asm=1, i32_mfma=1, i64_mfma=1, narrow_mfma=1, skinny=1,
                small_path=1)


def runs(dtype):
    """(name, options, f32 config, diagnostic that must be nonzero on the inside case of an assembly guard)"""
    dt = np.dtype(dtype)
    plain = ("no skinny / small-matrix kernels", dict(skinny=0, small_path=0), -1, None)
    if dt == np.float32:
        return ([("assembly 256x128 family", dict(f32_asm=2, asm_tile=0), -1, "last_f32_asm"),
                 ("assembly 16x16-block family", dict(f32_asm=2, asm_tile=5), -1, "last_f32_asm")] +
                [(f"compiler kernels, config {i}", dict(), i, None) for i in range(5)] +
                [("compiler kernels, the launcher's choice", dict(f32_asm=0), -1, None),
                 ("compiler kernels, no slice-parallel form", dict(f32_asm=0, slice_parallel=0), -1, None), plain])
    if dt == np.float64:
        return [("assembly", dict(f64_asm=2, slice_parallel=0), -1, "last_f64_asm"),
                ("compiler kernels", dict(f64_asm=0), -1, None),
                ("compiler kernels, no slice-parallel form", dict(f64_asm=0, slice_parallel=0), -1, None), plain]
    if dt.itemsize >= 4:
        return [("assembly limb kernel", dict(i32_asm=2), -1, "last_i32_asm"), ("compiler limb kernel", dict(i32_asm=0), -1, None),
                ("VALU kernel", dict(i32_mfma=0, i64_mfma=0), -1, None), plain]
    return [("matrix cores", dict(), -1, None), ("VALU kernel", dict(narrow_mfma=0), -1, None), plain]


RUNS = [(dt, r) for dt in FV.DTYPES for r in runs(dt)]

# ---- references, computed once per (element type, case, mode) and shared by the runs ---------------------------------------
_REF = {}


def _reference(oracle, c, fast):
    key = (c.dtype.name, c.name, fast)
    if key in _REF:
        return _REF[key]
    A, B, C0, bias = FV.fast_operands(c) if fast else FV.laser_operands(c)
    alpha, beta = FV.scalars(c, fast)
    if c.dtype.kind == "f" and c.extra.get("nan_c"):
        C0 = FV.nan_patterns(C0.shape, c.dtype)

    def one(a, b, c0, bi):
        if fast:        # exact in any order: the float64 product is the bar
            w = alpha * (a.astype(np.float64) @ b.astype(np.float64)) + (beta * c0.astype(np.float64) if beta else 0.0)
            return (w + (bi.astype(np.float64) if bi is not None else 0.0)).astype(c.dtype)
        if c.dtype.itemsize < 4:
            from tests.test_gpu_narrow_int import reference
            return reference(a, b, alpha, beta, c0)
        # (beta = 0 never reads C: the oracle gets zeros where the device C holds NaN patterns)
        w = oracle.matmul(np.ascontiguousarray(a), np.ascontiguousarray(b), alpha, beta, np.ascontiguousarray(c0).copy() if beta else np.zeros_like(c0))
        return oracle.apply_epilogue(w, bi, None) if bi is not None else w

    want = np.stack([one(A[i], B[i], C0[i], None) for i in range(A.shape[0])]) if A.ndim == 3 else one(A, B, C0, bias)
    for x in (A, B, C0, want) + (() if bias is None else (bias,)):
        x.setflags(write=False)
    _REF[key] = (A, B, C0, bias, alpha, beta, want)
    return _REF[key]


def _launch(la, typed, c, alpha, beta):
    A, B, C = c.A, c.B, c.C
    kind = c.extra.get("kind", "gemm")
    pA, pB, pC = _ptr(typed, A), _ptr(typed, B), _ptr(typed, C)
    if kind == "batched":
        la.gemm_strided_batched(c.extra["batch"], c.M, c.N, c.K, alpha, pA, A.strides[1], A.strides[2], A.strides[0],
                                pB, B.strides[1], B.strides[2], B.strides[0], beta, pC, C.strides[1], C.strides[2], C.strides[0])
    elif kind == "prepacked":
        import torch
        pa = torch.empty(la.gemm_prepackA_mem_required(c.dtype, c.M, c.N, c.K), dtype=torch.uint8, device="cuda")
        pb = torch.empty(la.gemm_prepackB_mem_required(c.dtype, c.M, c.N, c.K), dtype=torch.uint8, device="cuda")
        la.gemm_prepackA(pa, c.M, c.N, c.K, pA, *A.strides)
        la.gemm_prepackB(pb, c.M, c.N, c.K, pB, *B.strides)
        la.gemm_packed(c.M, c.N, c.K, alpha, pa, pb, beta, pC, *C.strides)
        torch.cuda.synchronize()
    elif "bias" in c.extra:
        b = c.extra["bias"]
        la.gemm_strided(c.M, c.N, c.K, alpha, pA, *A.strides, pB, *B.strides, beta, pC, *C.strides, bias=_ptr(typed, b),
                        rowStrideBias=b.strides[0], colStrideBias=b.strides[1])
    else:
        la.gemm_strided(c.M, c.N, c.K, alpha, pA, *A.strides, pB, *B.strides, beta, pC, *C.strides)


def _bits(x):
    return x.view(np.dtype(f"u{x.dtype.itemsize}")) if x.dtype.kind == "f" else x


@pytest.mark.parametrize("dtype,run", RUNS, ids=[f"{np.dtype(dt)}-{r[0].replace(' ', '_')}" for dt, r in RUNS])
def test_far_views(la, oracle, dtype, run):
    import torch
    name, options, cfg, diag = run
    cases = FV.cases(dtype)
    size = np.dtype(dtype).itemsize
    arena = _arena(FV.arena_bytes(cases), 1000 + size)
    typed = _typed(arena, dtype)
    fails = []
    try:
        for k, v in options.items():
            la.set_option(k, v)
        if cfg >= 0:
            la.set_f32_config(cfg)
        for fast in ((False, True) if np.dtype(dtype).kind == "f" else (False,)):
            la.set_float_mode(1 if fast else 0)
            for c in cases:
                A, B, C0, bias, alpha, beta, want = _reference(oracle, c, fast)
                what = f"{np.dtype(dtype)} {c.name} [{name}] {'one-chain' if fast else 'laser-order'} A={c.A} B={c.B} C={c.C}"
                _put(typed, c.A, A); _put(typed, c.B, B); _put(typed, c.C, C0)
                if bias is not None:
                    _put(typed, c.extra["bias"], bias)
                gap = None
                if c.C.strides[-1] == 2:         # the elements between C's columns keep their bytes
                    gap = FV.View(c.C.shape, c.C.strides, c.C.offset + 1)
                    gap_before = _get(typed, gap)
                cw = _words(arena, c.C, size)
                sum0, csum0 = arena.sum(dtype=torch.int64), cw.sum(dtype=torch.int64)
                _launch(la, typed, c, alpha, beta)
                used = la.get_option(diag) if diag else None
                got = _get(typed, c.C)
                delta, cdelta = arena.sum(dtype=torch.int64) - sum0, cw.sum(dtype=torch.int64) - csum0
                # (a wrong number is collected and the next case still runs; a device error raises and ends the test)
                bad = np.argwhere(_bits(got) != _bits(want))
                if bad.size or not np.array_equal(got, want):
                    fails.append(f"{what}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")
                if int(delta) != int(cdelta):
                    fails.append(f"{what}: wrote outside the C view (arena sum moved by {int(delta)}, C by {int(cdelta)})")
                if gap is not None and not np.array_equal(_bits(_get(typed, gap)), _bits(gap_before)):
                    fails.append(f"{what}: wrote between C's columns")
                if diag and c.guard in FV.ASM_GUARDS and c.side == "inside" and used == 0:
                    fails.append(f"{what}: the assembly kernels declined a view inside their guard ({diag} = 0)")
                if c.guard.startswith("gemm_small") and c.side == "inside" and dtype == np.float32 and cfg < 0 and options.get("small_path", 1) \
                        and la.last_f32_config() != -2:
                    fails.append(f"{what}: the small-matrix kernel did not run")
                if diag and c.guard in FV.ASM_GUARDS:
                    print(f"{np.dtype(dtype)} {c.name} [{name}] mode={int(fast)}: {diag} = {used}")
        assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails)
    finally:
        for k, v in DEFAULTS.items():
            la.set_option(k, v)
        la.set_f32_config(-1)
        la.set_float_mode(0)
        del typed, arena
        _free(la)


# ---- exp and softmax on far views ---------------------------------------------------------------------------------------------
EXP_SRC = FV.View((1025, 512), (2 ** 20, 2), FV.FAR0 // 4 + 3)           # shaped like BIG_VIEWS[0] of test_gpu_strided_movers.py: 2^32 bytes
EXP_DST = FV.View((1025, 512), (2 ** 20, 2), FV.FAR0 // 4 + 2048)
SM_SRC = FV.View((3, 1025), (2 ** 29, 1), FV.FAR0 // 4 + 5)
SM_DST = FV.View((3, 1025), (2 ** 29, 1), FV.FAR0 // 4 + 4096)


def _float_case(la, src, dst, fn, model, seed, edges):
    import torch
    nbytes = max(FV.byte_span(v, 4)[1] for v in (src, dst))
    nbytes = -(-nbytes // (64 << 20)) * (64 << 20)
    assert nbytes > 2 ** 32 and min(FV.byte_span(v, 4)[0] for v in (src, dst)) >= FV.FAR0
    assert np.intersect1d(FV.element_offsets(src).ravel(), FV.element_offsets(dst).ravel()).size == 0
    arena = _arena(nbytes, seed)
    typed = _typed(arena, np.float32)
    try:
        rng = np.random.default_rng(seed)
        x = rng.uniform(-30, 30, src.shape).astype(np.float32)
        if edges:
            e = exp_model.edges()
            x.reshape(-1)[:e.size] = e
            x[-1, -e.size:] = e
        _put(typed, src, x)
        want = model(x)
        # into a dense tensor
        dense = torch.full(src.shape, 7.0, dtype=torch.float32, device="cuda")
        fn(_tview(typed, src)[0], out=dense)
        assert exp_model.same_bits(dense.cpu().numpy(), want), "far source, dense destination"
        # into the far destination: nothing else in the arena moves
        dw = _words(arena, dst, 4)
        sum0, dsum0 = arena.sum(dtype=torch.int64), dw.sum(dtype=torch.int64)
        fn(_tview(typed, src)[0], out=_tview(typed, dst)[0])
        got = _get(typed, dst)
        delta, ddelta = arena.sum(dtype=torch.int64) - sum0, dw.sum(dtype=torch.int64) - dsum0
        assert exp_model.same_bits(got, want), "far source, far destination"
        assert int(delta) == int(ddelta), "wrote outside the destination view"
    finally:
        del typed, arena
        _free(la)


def test_exp_on_a_far_strided_view(la):
    u32, i32 = FV.has_teeth(EXP_SRC, 4)
    assert u32 and i32
    _float_case(la, EXP_SRC, EXP_DST, la.exp, exp_model.lexp, 2001, True)


def test_softmax_on_far_rows(la):
    u32, i32 = FV.has_teeth(SM_SRC, 4)
    assert u32 and i32
    _float_case(la, SM_SRC, SM_DST, la.softmax, exp_model.softmax_rows, 2002, False)
