"""Non-finite values where the GEMM and convolution kernels must not look (tests/poison_views.py): every kernel here discards
data -- k beyond K, a convolution's padding, rows past a tile's edge, a padded filter row -- by loading it from a clamped or padded
address and zeroing it afterwards.  A path that zeroes only ONE operand of a product passes every test on finite data (finite x 0
= +0) and returns NaN as soon as the neighbouring value is Inf or NaN.

The claim: a non-finite value reaches exactly the elements of C (or of the convolution output) that IEEE arithmetic on the ADDRESSED
operands says it reaches; every other element keeps the bits of the clean run.  Every comparison is on bit patterns (BV.bits): where
the expected class is finite the clean run's bits, where it is NaN a NaN of any payload, where it is an infinity that infinity.  Under
a fused tanh an infinity becomes +-1 exactly (C's Annex F: tanh(+-Inf) = +-1), a NaN stays a NaN.

(a) the batched catalogue of tests/batched_views.py on every route tests/test_gpu_batched.py drives, the kernel that ran a member of
    that file's recorded ROUTE_SETS entry;
(b) single products on the routes only a single product reaches: one-entry `padded` views (leading dimensions + 3 / + 5 / + 7, bases
    1 / 3 / 5 elements past a 64-byte boundary, slack on both sides), `b_transposed` for the transposed-B kernels;
(c) conv2d_im2col with and without bias + tanh, one geometry per kernel class, guard bands around the input, the filter and the bias.

The clean reference is the oracle in laser-order mode.  In FAST mode, and wherever a tanh is fused (the device's tanh is within a few
ulp of numpy's, not bit-defined), it is the clean launch of the same route under the same options: those results repeat bit for bit.
Every FAST clean launch, float32 and float64, every alpha / beta, is tied to the true value by fast_accuracy(): the element-wise
forward error bound of the number format, and for float32 the mode's bar, oracle.mean_relative_error <= 1e-5, or twice the
laser-order oracle's own figure where cancellation puts that above 1e-5.

The streaming (M <= 8 / N <= 8) kernel, the slice-parallel form, the peeled rows / columns, the pre-packed path and the host-pointer
row-panel pipeline leave no `last_*` diagnostic: they run under the host-side rules restated next to each test (gemm_route.cpp,
capi.cpp), and where an option switches them off both settings run.  The same holds for the convolution's loaders: the LDS input
patch and the per-element gather (conv_patch), the explicit im2col + batched GEMM (conv_implicit = 0), the 1x1 GEMM shortcut and its
implicit twin (conv_1x1_implicit) all report a compiler-scheduled configuration and nothing else, so their route assertion cannot tell
them apart: each runs under its option, and launch_conv_implicit_f32 / launch_conv_cfg (gemm_mfma.hip) and capi.cpp are the rule.
"""
import contextlib

import numpy as np
import pytest

from tests import batched_views as BV
from tests import poison_views as PV
from tests import test_gpu_batched as TB

pytestmark = pytest.mark.gpu

SCALARS = [(1, 0), (0.5, 0.25)]


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import laser_amd
    assert laser_amd.lib().laser_hip_arch().decode().startswith("gfx950")
    return laser_amd


@contextlib.contextmanager
def options(la, mode=0, **opts):
    """set the options and the float mode, put everything back afterwards"""
    before = {k: la.get_option(k) for k in opts}
    try:
        la.set_float_mode(mode)
        for k, v in opts.items():
            la.set_option(k, v)
        yield
    finally:
        for k, v in before.items():
            la.set_option(k, v)
        la.set_float_mode(0)
        la.set_f32_config(-1)


def _sync():
    import torch
    torch.cuda.synchronize()


def _same(x, y):
    return np.array_equal(BV.bits(np.asarray(x)), BV.bits(np.asarray(y)))


# ---- (a) the batched catalogue ------------------------------------------------------------------------------------------------
def run_poison_cases(la, route, case_list, allowed, check=None):
    """Two launches per case under the options already set: (1) gap-poisoned operands, C equal to BV.expected(c) bit for bit;
    (2) element-poisoned operands, C as PV.check_result says.  After both the C arena outside the view holds its sentinel; after a
    group (the alpha / beta variants share their arenas) the A and B arenas are unchanged; every kernel that ran is in `allowed`.
    Returns (failures, what ran)."""
    fails, seen = [], set()
    group, dev, host = None, None, None

    def close_group():
        if group is not None:
            for kind in dev:
                for name, h, d in zip("AB", host[kind], dev[kind]):
                    if not _same(d.cpu().numpy(), h):
                        fails.append(f"[{route}] {BV.describe(group)}: the {kind}-poisoned {name} arena changed")

    for c in case_list:
        key = (c.layout, c.batch, c.M, c.N, c.K)
        ea, eb, special = PV.element_poisoned(c)
        if group is None or key != (group.layout, group.batch, group.M, group.N, group.K):
            close_group()
            group = c
            host = {"gap": PV.gap_poisoned(c), "element": (ea, eb)}
            dev = {kind: (TB._dev(h[0]), TB._dev(h[1])) for kind, h in host.items()}
        want = BV.expected(c)
        off = BV.element_offsets(c.C, c.batch, c.M, c.N)
        _, _, cbuf, mask = BV.arenas(c)
        share = PV.finite_share(special)
        if share < PV.CAP:
            fails.append(f"[{route}] {BV.describe(c)}: only {share:.3f} of C is expected finite")
        for kind in ("gap", "element"):
            what = f"[{route}] {BV.describe(c)}, {kind} poison"
            dA, dB = dev[kind]
            dC = TB._dev(cbuf)
            TB._prime(la, c.dtype)
            TB._call(la, c, dA, dB, dC)
            _sync()
            ran = TB._ran(la, c.dtype)
            seen.add(ran)
            hC = dC.cpu().numpy()
            bad = PV.check_result(hC[off], want, special if kind == "element" else np.zeros_like(special))
            if bad:
                fails.append(f"{what} (ran {ran}): {bad}")
            if not _same(hC[~mask], cbuf[~mask]):
                fails.append(f"{what} (ran {ran}): elements outside the C view lost their sentinel")
            if ran not in allowed:
                fails.append(f"{what}: ran {ran}, not in the route's recorded set {sorted(allowed, key=repr)}")
            msg = check(c, ran) if check else None
            if msg:
                fails.append(f"{what} (ran {ran}): {msg}")
    close_group()
    return fails, seen


def _finish(route, fails, seen):
    print(f"POISON_ROUTE {route!r}: {sorted(seen, key=repr)!r}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("route", list(TB.F32_ROUTES))
def test_f32_routes(la, route):
    opts, asm_mode = TB.F32_ROUTES[route]
    case_list = BV.cases(np.float32, scalar_list=SCALARS)
    fails, seen = TB._with_options(la, opts, lambda: run_poison_cases(la, route, case_list, TB.ROUTE_SETS[route], TB._f32_rule(asm_mode)))
    _finish(route, fails, seen)


def _config_routes():
    return sorted(r for r in TB.ROUTE_SETS if r.startswith("f32 config "))


@pytest.mark.parametrize("route", _config_routes())
def test_f32_every_pinned_compiler_configuration(la, route):
    i = int(route.split()[2])
    assert route == f"f32 config {i} {la.f32_configs()[i]}"
    case_list = BV.cases(np.float32, layouts=["padded", "transposed", "reversed_batches", "interleaved"], scalar_list=SCALARS)

    def body():
        la.set_f32_config(i)
        return run_poison_cases(la, route, case_list, TB.ROUTE_SETS[route],
                                lambda c, ran: None if ran[0] == 0 and ran[1] >= 0 else "not a compiler-scheduled kernel")
    fails, seen = TB._with_options(la, {}, body)
    _finish(route, fails, seen)


def test_f32_pinned_configurations_are_all_here(la):
    assert len(_config_routes()) == len(la.f32_configs())


@pytest.mark.parametrize("small_path", [1, 0])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_small_matrix_kernel_on_and_off(la, dtype, small_path):
    """(the defaults but for small_path: float32 ran what "f32 heuristic" records, without the small-matrix kernel when it is
    off; float64 a kernel of its recorded routes)"""
    is32 = dtype == np.float32
    route = f"{np.dtype(dtype).name} small_path={small_path}"
    allowed = (TB.ROUTE_SETS["f32 heuristic"] - (set() if small_path else {(0, -2)})) if is32 else set().union(*(TB.ROUTE_SETS[r] for r in TB.F64_ROUTES))
    case_list = BV.cases(dtype, scalar_list=SCALARS)
    rule = TB._f32_rule(1, bool(small_path)) if is32 else None
    fails, seen = TB._with_options(la, dict(small_path=small_path), lambda: run_poison_cases(la, route, case_list, allowed, rule))
    _finish(route, fails, seen)
    if is32:
        assert ((0, -2) in seen) == bool(small_path)


@pytest.mark.parametrize("pin", range(10))
def test_f32_each_assembly_tile_class(la, pin):
    route = f"f32 asm_tile {pin}"
    case_list = BV.cases(np.float32, shape_list=[(3, 200, 136, 260), (3, 130, 70, 517)], scalar_list=SCALARS)
    fails, seen = TB._with_options(la, dict(f32_asm=2, asm_tile=pin),
                                   lambda: run_poison_cases(la, route, case_list, TB.ROUTE_SETS[route], TB._f32_rule(2, True, pin)))
    _finish(route, fails, seen)
    assert any(k for k, _ in seen), "no hand-scheduled kernel ran"


@pytest.mark.parametrize("route", list(TB.F64_ROUTES))
def test_f64_routes(la, route):
    opts = TB.F64_ROUTES[route]

    def check(c, ran):
        if opts.get("f64_asm") == 2 and TB.asm_takes(c) and not TB.small_takes(c):
            return None if ran else "the hand-scheduled launcher declined a view it accepts"
        return None if ran == 0 else "a hand-scheduled kernel ran where its launcher declines"
    case_list = BV.cases(np.float64, scalar_list=SCALARS)
    fails, seen = TB._with_options(la, opts, lambda: run_poison_cases(la, route, case_list, TB.ROUTE_SETS[route], check))
    _finish(route, fails, seen)


# ---- (b) single products ------------------------------------------------------------------------------------------------------
def single(layout, dtype, M, N, K, alpha=1, beta=0):
    return BV.make_case(layout, dtype, (1, M, N, K), alpha, beta)


def _launch(la, c, dA, dB, dC, **kw):
    la.gemm_strided(c.M, c.N, c.K, c.alpha, dA[c.A.offset:], c.A.strides[1], c.A.strides[2], dB[c.B.offset:], c.B.strides[1], c.B.strides[2],
                    c.beta, dC[c.C.offset:], c.C.strides[1], c.C.strides[2], **kw)


def _wide_value(c):
    """alpha A B + beta C0 and the sum of the terms' magnitudes, one precision up: float64 for float32, long double for float64"""
    wide = np.float64 if c.dtype == np.float32 else np.longdouble
    A, B, C0 = (x[0].astype(wide) for x in BV.operands(c))
    al, be = wide(c.alpha), wide(c.beta)
    return al * (A @ B) + be * C0, abs(al) * (np.abs(A) @ np.abs(B)) + abs(be) * np.abs(C0)


def fast_accuracy(oracle, c, got, what):
    """What ties a FAST clean launch, which is then its own reference, to the true value; asserted on EVERY such launch.
    (1) Element by element the standard forward bound of a sum of K products in any order (Higham, Accuracy and Stability of
    Numerical Algorithms, 3.1): |got - value| <= gamma_n (|alpha| |A| |B| + |beta| |C0|), gamma_n = n u / (1 - n u), u the unit
    roundoff of the element type, n = K + 8 roundings (K fused multiply-adds, the folds of up to four partial sums, alpha, beta, their
    sum).  A kernel or plan that takes alpha, beta or one k wrong misses it by orders of magnitude.
    (2) float32: the mode's bar, oracle.mean_relative_error <= 1e-5 against the float64 value.  Where alpha A B + beta C0 cancels
    to nearly zero in a few elements the mean is theirs and the bar says nothing about the arithmetic -- on 259x251x516 and 131x251x544
    at (0.5, 0.25) the laser-order oracle itself has 1.198e-05 and 1.218e-05 -- so a launch above 1e-5 must stay within twice the
    figure of the oracle's result on the same operands: the same roundings in another order.  Returns the failures."""
    fails = []
    value, mag = _wide_value(c)
    u = 2.0 ** -24 if c.dtype == np.float32 else 2.0 ** -53
    n = c.K + 8
    over = np.abs(got.astype(value.dtype) - value) > (n * u / (1 - n * u)) * mag
    if over.any():
        at = tuple(int(v) for v in np.argwhere(over)[0])
        fails.append(f"{what}: {int(over.sum())} elements of the clean FAST launch are beyond the forward error bound, first at {at}: "
                     f"got {got[at]!r}, value {float(value[at])!r}")
    if c.dtype == np.float32:
        mre = oracle.mean_relative_error(got, value)
        bar = 1e-5
        if mre > bar:
            bar = max(bar, 2 * oracle.mean_relative_error(BV.expected(c)[0], value))
        print(f"POISON_MRE {what}: {mre:.3e} (bar {bar:.3e})")
        if not mre <= bar:
            fails.append(f"{what}: the clean FAST launch has mean relative error {mre:.3e}, the bar is {bar:.3e}")
    return fails


def poison_single(la, oracle, c, what, route=None, fast=False, element=True, want=None, tanh=False, launch=_launch, prime=True):
    """The clean (FAST mode, or `want` is "clean"), gap-poisoned and element-poisoned launches of one single product under the
    options already set; route() -> message or None is asked after every launch.  Returns the failures."""
    fails = []
    a, b, cbuf, mask = BV.arenas(c)
    off = BV.element_offsets(c.C, 1, c.M, c.N)

    def run(kind, ha, hb):
        dA, dB, dC = TB._dev(ha), TB._dev(hb), TB._dev(cbuf)
        if prime:
            TB._prime(la, c.dtype)
        launch(la, c, dA, dB, dC)
        _sync()
        msg = route() if route else None
        if msg:
            fails.append(f"{what}, {kind}: {msg}")
        hC = dC.cpu().numpy()
        if not (_same(dA.cpu().numpy(), ha) and _same(dB.cpu().numpy(), hb)):
            fails.append(f"{what}, {kind}: an operand arena changed")
        if not _same(hC[~mask], cbuf[~mask]):
            fails.append(f"{what}, {kind}: elements outside the C view lost their sentinel")
        return hC[off]

    if fast or (isinstance(want, str) and want == "clean"):
        want = run("clean", a, b)
        if fast and not tanh:
            fails += fast_accuracy(oracle, c, want[0], what)
    elif want is None:
        want = BV.expected(c)
    ea, eb, special = PV.element_poisoned(c)
    assert PV.finite_share(special) >= PV.CAP, (what, PV.finite_share(special))
    bad = PV.check_result(run("gap poison", *PV.gap_poisoned(c)), want, np.zeros_like(special))
    if bad:
        fails.append(f"{what}, gap poison: {bad}")
    if element:
        bad = PV.check_result(run("element poison", ea, eb), want, special, tanh=tanh)
        if bad:
            fails.append(f"{what}, element poison: {bad}")
    return fails


def _done(fails, notes=()):
    for n in notes:
        print(n)
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# (laser-order kernel, one-chain kernel, tile, B transposed, 16x16-block class): one kernel per family, the indices of
# test_hybrid_plan_bit_identical and test_one_chain_cut_launches_within_tolerance_and_deterministic (asm_kernels.h kKernels)
ASM_FAMILIES = {"256x128": (0, 8, (256, 128), False, False), "128x128x16": (2, 3, (128, 128), False, False), "64x64": (12, 13, (64, 64), False, False),
                "128x128x32": (30, 31, (128, 128), False, False), "96x96": (46, 47, (96, 96), False, True),
                "128x128x16_nt": (6, 7, (128, 128), True, False), "160x160": (62, 63, (160, 160), False, True),
                "256x256": (None, 1, (256, 256), False, False), "256x128_nt": (4, 9, (256, 128), True, False)}
# (the one-chain 256x256 tile has no laser-order row)
ASM_RUNS = [(mode, family) for family, f in ASM_FAMILIES.items() for mode in (0, 1) if f[mode] is not None]


def _plan_runs(bm, bn, x16):
    """(plan, asm_wgs, asm_noseed, M, N, K): M = bm + 3 and N = 2 bn - 5 are four ragged tiles; K = 516 is one kc slice and a
    4-element tail, 517 an odd tail (not on the 16x16-block classes: K % 4 == 0), 1029 / 1028 three slices for the K-cut plan, 544 =
    17 whole K-tiles for the strided plan's pipelined transitions; plans 3 and 4 get the fewest tiles that exceed the forced
    workgroup count: 4 tiles on 2 workgroups, 18 tiles on 10 (8 left to the hybrid plan's K-cut launch, its minimum)"""
    M, N = bm + 3, 2 * bn - 5
    tails = (516,) if x16 else (516, 517)
    long_k = 1028 if x16 else 1029
    runs = [(1, 0, 0, M, N, k) for k in tails]
    runs += [(2, 3, late, M, N, long_k) for late in (0, 1)]
    runs += [(3, 2, 0, M, N, k) for k in (544, tails[-1])]
    runs += [(4, 10, 0, 2 * bm + 3, 6 * bn - 5, k) for k in (1056, long_k)]
    return runs


@pytest.mark.parametrize("mode,family", ASM_RUNS, ids=[f"{('laser-order', 'fast')[m]}-{f}" for m, f in ASM_RUNS])
def test_f32_assembly_kernels_under_every_launch_plan(la, oracle, mode, family):
    """What each plan must report as (last_asm_wgs, last_asm_slices, last_asm_rem), on `tiles` tiles: plan 1 (tiles, 1, 0); plan 2
    (asm_wgs, 3, 0), three K slices in both modes; plans 3 and 4 pipeline tile transitions, which needs whole K-tiles (K % 32 == 0)
    and beta == 0 (include/laser_hip.h "asm_plan"): then (asm_wgs, 1, 0) and (asm_wgs, slices, 8) -- 8 of 18 tiles left to the K-cut
    launch, its slices 3 in laser-order mode and 1 with one chain -- and otherwise the launcher falls back to one workgroup per
    tile, (tiles, 1, 0): the ragged K and the beta != 0 runs of plans 3 and 4 are that fallback, asserted as such."""
    kern = ASM_FAMILIES[family][mode]
    _, _, (bm, bn), nt, x16 = ASM_FAMILIES[family]
    fails, notes = [], []
    for plan, wgs, late, M, N, K in _plan_runs(bm, bn, x16):
        for alpha, beta in SCALARS:
            c = single("b_transposed" if nt else "padded", np.float32, M, N, K, alpha, beta)
            what = f"kernel {kern} ({family}) mode {mode} plan {plan} wgs {wgs} noseed {late} {M}x{N}x{K} alpha {alpha} beta {beta}"
            diag = []

            def route():
                d = (la.last_f32_asm(), la.get_option("last_asm_wgs"), la.get_option("last_asm_slices"), la.get_option("last_asm_rem"))
                diag.append(d)
                tiles = -(-M // bm) * -(-N // bn)
                if d[0] != kern + 1:
                    return f"last_f32_asm = {d[0]}, wanted {kern + 1}"
                pipelined = K % 32 == 0 and beta == 0
                want = {1: (tiles, 1, 0), 2: (wgs, 3, 0), 3: (wgs, 1, 0) if pipelined else (tiles, 1, 0),
                        4: (wgs, 1 if mode else 3, 8) if pipelined else (tiles, 1, 0)}[plan]
                if d[1:] != want:
                    return f"plan {plan} ran (wgs, slices, rem) = {d[1:]}, wanted {want}"
                return None
            with options(la, mode, f32_asm=2, asm_kernel=kern, asm_plan=plan, asm_wgs=wgs, asm_noseed=late, slice_parallel=0):
                fails += poison_single(la, oracle, c, what, route, fast=bool(mode))
            notes.append(f"POISON_ASM {what}: (last_f32_asm, wgs, slices, rem) = {sorted(set(diag))}")
    _done(fails, notes)


def test_f32_assembly_fused_prologue_kernel_gap_poison_only(la, oracle):
    """a `_pre` kernel (relu on A and B in the staging registers): relu maps NaN to 0 by its documented rule, so only the gaps are
    poisoned; the reference is the oracle on relu(A), relu(B)"""
    relu = lambda x: np.where(x > 0, x, 0).astype(x.dtype)
    fails = []
    for K in (516, 517):
        c = single("padded", np.float32, 259, 251, K, 1, 0)
        A, B, _ = BV.operands(c)
        want = oracle.matmul(relu(np.ascontiguousarray(A[0])), relu(np.ascontiguousarray(B[0])))[None]
        with options(la, 0, f32_asm=2, asm_tile=0):
            fails += poison_single(la, oracle, c, f"_pre kernel K={K}", lambda: None if 35 <= la.last_f32_asm() <= 46 else f"last_f32_asm = {la.last_f32_asm()}",
                                   element=False, want=want, launch=lambda la_, c_, dA, dB, dC: _launch(la_, c_, dA, dB, dC, pre=la.PRE_RELU_A | la.PRE_RELU_B))
    _done(fails)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_streaming_kernel_rows_and_columns(la, oracle, dtype):
    """M <= 8 or N <= 8 with option skinny on: the streaming kernel is the first rung of run_gemm_core (gemm_route.cpp); off, the
    same shapes are one-row / one-column tiles of the tiled kernels.  K spans several kc slices with an odd tail."""
    fails = []
    for skinny in (1, 0):
        for M, N, K in ((300, 5, 517), (7, 300, 1029), (3, 8, 516), (1, 131, 1541)):
            for alpha, beta in SCALARS:
                c = single("padded", dtype, M, N, K, alpha, beta)
                with options(la, 0, skinny=skinny):
                    fails += poison_single(la, oracle, c, f"skinny={skinny} {np.dtype(dtype).name} {M}x{N}x{K} alpha {alpha} beta {beta}")
    _done(fails)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_slice_parallel_form(la, oracle, dtype):
    """few tiles x long K (gemm_slice_parallel: at most 150 tiles of 64x64, three slices or more when the last is ragged, no batch,
    no epilogue): the kc slices as one batched launch + the ragged last slice + an ordered combine; off, the sequential K loop"""
    kc = 512 if dtype == np.float32 else 256
    fails = []
    for on in (1, 0):
        for M, N, K in ((67, 131, 3 * kc + 5), (67, 131, 3 * kc + 4), (131, 59, 2 * kc)):
            for alpha, beta in SCALARS:
                c = single("padded", dtype, M, N, K, alpha, beta)
                with options(la, 0, slice_parallel=on):
                    fails += poison_single(la, oracle, c, f"slice_parallel={on} {np.dtype(dtype).name} {M}x{N}x{K} alpha {alpha} beta {beta}")
    _done(fails)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_peeled_rows_and_columns(la, oracle, dtype):
    """run_gemm_peeled: M = 1027 and N = 1029 are 3 rows and 5 columns past a multiple of 64 (M >= 1024, N >= 1024, K >= 256, split_tail
    and skinny on, laser-order): the whole tiles run tiled, the extra rows and columns on the streaming kernel -- which then starts
    at row 1024 of A and column 1024 of B, inside the operands; split_tail = 0 is the single launch"""
    kc = 512 if dtype == np.float32 else 256
    fails = []
    for split in (1, 0):
        for alpha, beta in SCALARS:
            c = single("padded", dtype, 1027, 1029, kc + 5, alpha, beta)
            with options(la, 0, split_tail=split):
                fails += poison_single(la, oracle, c, f"split_tail={split} {np.dtype(dtype).name} 1027x1029x{kc + 5} alpha {alpha} beta {beta}")
    _done(fails)


# (shape, scalars) per float mode: the smallest shapes gemm_mfma.hip plan_split cuts (its model needs a round of 256 tiles of the main
# configuration and a badly filled last one: 899 x 9835 in laser-order arithmetic -- K > kc -- and 899 x 8747 with one chain, both cut
# at column 8192).  Eight million elements of C: these two are the slowest tests of the file.
SPLIT_CASES = {0: ((899, 9835, 517), SCALARS), 1: ((899, 8747, 517), SCALARS)}


@pytest.mark.parametrize("mode", [0, 1], ids=["laser-order", "fast"])
def test_main_and_tail_split(la, oracle, mode):
    """the compiler-scheduled kernels' main + tail cut: the tail launch starts at column n_cut of B and of C; last_split tells the
    cut"""
    (M, N, K), scalars = SPLIT_CASES[mode]
    fails, cuts = [], set()
    for alpha, beta in scalars:
        c = single("padded", np.float32, M, N, K, alpha, beta)

        def route():
            cuts.add(la.last_split())
            if la.last_f32_asm() != 0:
                return f"last_f32_asm = {la.last_f32_asm()}"
            return None if 0 < la.last_split() < N else f"last_split = {la.last_split()}: the planner made no cut"
        with options(la, mode, f32_asm=0, skinny=0, split_tail=1):
            fails += poison_single(la, oracle, c, f"main + tail mode {mode} {M}x{N}x{K} alpha {alpha} beta {beta}", route, fast=bool(mode), prime=False)
    _done(fails, [f"POISON_SPLIT mode {mode}: last_split = {sorted(cuts)}"])


def _padded_host(rng, rows, cols, ld, dtype, lead=3):
    """(flat poisoned buffer, view [rows][cols] with leading dimension ld inside it, starting `lead` elements in)"""
    buf = PV.poison(lead + (rows - 1) * ld + cols + 5, dtype)
    v = np.lib.stride_tricks.as_strided(buf[lead:], (rows, cols), (ld * buf.itemsize, buf.itemsize))
    d = rng.uniform(-0.5, 0.5, (rows, cols)).astype(dtype)
    d[d == 0] = 0.25
    v[:] = d
    return buf, v


def _host_special(A, B, alpha, beta, C0):
    with np.errstate(invalid="ignore", over="ignore"):
        full = float(alpha) * np.einsum("ik,kj->ij", A.astype(np.float64), B.astype(np.float64), optimize=False)
        if beta != 0:
            full = full + float(beta) * C0.astype(np.float64)
    return PV.classify(full)


def _poke(A, B):
    """PV.element_positions on host views"""
    M, K = A.shape
    N = B.shape[1]
    A[M - 1, K - 1] = np.nan
    A[1, 0] = np.nan
    B[K - 1, N - 1] = np.inf
    B[0, 2] = np.nan


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_prepacked_path(la, oracle, dtype):
    """gemm_prepackA / gemm_prepackB from strided host views inside poisoned buffers (A column-major, B row-major, as
    test_prepacked_ragged_shapes), then gemm_packed: the packing pass pads the panels to whole tiles"""
    rng = np.random.default_rng(71)
    M, N, K = 130, 77, 600
    _, At = _padded_host(rng, K, M, M + 3, dtype)          # column-major A: element (i, k) at k * (M + 3) + i
    _, B = _padded_host(rng, K, N, N + 5, dtype, lead=1)
    A = At.T
    want = oracle.matmul(np.ascontiguousarray(A), np.ascontiguousarray(B))

    def product():
        pa = la.aligned_host_buffer(la.gemm_prepackA_mem_required(dtype, M, N, K))
        pb = la.aligned_host_buffer(la.gemm_prepackB_mem_required(dtype, M, N, K))
        la.gemm_prepackA(pa, M, N, K, A, 1, M + 3)
        la.gemm_prepackB(pb, M, N, K, B, N + 5, 1)
        Cbuf = BV.sentinel(dtype, M * (N + 7)).reshape(M, N + 7).copy()
        try:
            la.gemm_packed(M, N, K, 1, pa, pb, 0, Cbuf[:, :N], N + 7, 1)
        finally:
            la.gemm_prepack_release(pa)
            la.gemm_prepack_release(pb)
        assert _same(Cbuf[:, N:], BV.sentinel(dtype, M * 7).reshape(M, 7)), "wrote outside C"
        return Cbuf[:, :N]
    assert _same(product(), want), "gap poison: C lost bits"
    _poke(A, B)
    special = _host_special(A, B, 1, 0, None)
    assert PV.finite_share(special) >= PV.CAP
    bad = PV.check_result(product(), want, special)
    assert bad is None, f"element poison: {bad}"


# (the hand-scheduled kernels fuse a bias and relu; tanh and sigmoid are the compiler-scheduled kernels' -- choose_gemm_f32_asm)
EPILOGUE_ROUTES = {"float32 compiler-scheduled": (np.float32, dict(f32_asm=0), lambda la, act: la.last_f32_asm() == 0),
                   "float32 hand-scheduled": (np.float32, dict(f32_asm=2), lambda la, act: (la.last_f32_asm() != 0) == (act is None)),
                   "float64": (np.float64, dict(), lambda la, act: True)}


@pytest.mark.parametrize("name", list(EPILOGUE_ROUTES))
def test_fused_epilogue_bias_views_and_tanh(la, oracle, name):
    """act(alpha A B + beta C + bias) with the bias a strided view (row stride, column stride) = (1, 0) one value per row, (0, 1)
    one per column, (ld, 1) a full matrix with a leading-dimension gap, everything around and between its elements poisoned.
    Without an activation the clean launch equals oracle.apply_epilogue of the oracle's product; with tanh the clean launch is
    the reference, a +-Inf of the product is +-1 and a NaN a NaN."""
    import torch
    dtype, opts, ran = EPILOGUE_ROUTES[name]
    M, N, K = 131, 251, 517
    rng = np.random.default_rng(83)
    fails = []
    for alpha, beta in SCALARS:
        c = single("padded", dtype, M, N, K, alpha, beta)
        for bname, (rows, cols, rs, cs) in {"(1, 0)": (M, 1, 1, 0), "(0, 1)": (1, N, 0, 1), "(ld, 1)": (M, N, N + 7, 1)}.items():
            hb, bias = _padded_host(rng, rows, cols, max(rs, 1), dtype, lead=64 + 3)
            db = torch.from_numpy(hb).cuda()
            for act in (None, "tanh"):
                what = f"{name} bias {bname} activation {act} alpha {alpha} beta {beta}"
                launch = lambda la_, c_, dA, dB, dC: _launch(la_, c_, dA, dB, dC, bias=db[64 + 3:], rowStrideBias=rs, colStrideBias=cs, activation=act)
                want = "clean" if act else oracle.apply_epilogue(BV.expected(c)[0], bias)[None]
                with options(la, 0, **opts):
                    fails += poison_single(la, oracle, c, what, lambda act=act: None if ran(la, act) else f"last_f32_asm = {la.last_f32_asm()}",
                                           want=want, tanh=bool(act), launch=launch)
            if not _same(db.cpu().numpy(), hb):
                fails.append(f"{name} bias {bname}: the bias buffer changed")
    _done(fails)


F64_SINGLE = {"matrix cores": (dict(f64_asm=0, slice_parallel=0), lambda v: v == 0), "hand-scheduled": (dict(f64_asm=2, slice_parallel=0), lambda v: v != 0),
              "VALU": (dict(f64_mfma=0), lambda v: v == 0)}


@pytest.mark.parametrize("name", list(F64_SINGLE))
def test_f64_single_products(la, oracle, name):
    """float64 on the compiler-scheduled matrix-core kernels, the hand-scheduled kernels (K even) and the VALU kernel: 131 x 251 are
    ragged tiles of 128x128 and of 64x64, K = 262 one kc slice and a 6-element tail, 263 an odd tail, 518 two slices and a tail"""
    opts, ok = F64_SINGLE[name]
    fails, seen = [], set()
    for mode in (0, 1):
        for K in ((262, 518) if name == "hand-scheduled" else (262, 263, 518)):
            for alpha, beta in SCALARS:
                c = single("padded", np.float64, 131, 251, K, alpha, beta)

                def route():
                    v = la.get_option("last_f64_asm")
                    seen.add(v)
                    return None if ok(v) else f"last_f64_asm = {v}"
                with options(la, mode, **opts):
                    fails += poison_single(la, oracle, c, f"float64 {name} mode {mode} K={K} alpha {alpha} beta {beta}", route, fast=bool(mode))
    _done(fails, [f"POISON_F64 {name}: last_f64_asm = {sorted(seen)}"])


def test_host_pointer_row_panel_pipeline(la, oracle):
    """numpy operands in NaN-padded buffers on the row-panel pipeline, the twin of test_host_pointer_2d_pipelined_path's 2-D case:
    pageable memory, M >= 2048 and operand spans of 64 MiB together (capi.cpp gemm_host) -- the spans are mostly padding, the product is
    small.  Every row panel of A and strip of C is a span copy that carries the padding with it."""
    rng = np.random.default_rng(29)
    M, N, K = 2051, 131, 517
    _, A = _padded_host(rng, M, K, 4096, np.float32)
    _, B = _padded_host(rng, K, N, 8192, np.float32, lead=1)
    assert (A.strides[0] // 4 * (M - 1) + K + B.strides[0] // 4 * (K - 1) + N + 2100 * (M - 1) + N) * 4 >= 64 << 20
    C0 = rng.uniform(-0.5, 0.5, (M, N)).astype(np.float32)
    sent = BV.sentinel(np.float32, M * 2100).reshape(M, 2100)
    clean = {}
    for poke in (False, True):
        if poke:
            _poke(A, B)
        for alpha, beta in SCALARS:
            Cbuf = sent.copy()
            Cbuf[:, :N] = C0
            la.matmul(A, B, alpha, beta, Cbuf[:, :N])
            assert _same(Cbuf[:, N:], sent[:, N:]), "the gaps of C changed"
            if not poke:
                clean[(alpha, beta)] = oracle.matmul(np.ascontiguousarray(A), np.ascontiguousarray(B), alpha, beta, C0.copy())
                assert _same(Cbuf[:, :N], clean[(alpha, beta)]), (alpha, beta, "gap poison: C lost bits")
            else:
                special = _host_special(A, B, alpha, beta, C0)
                assert PV.finite_share(special) >= PV.CAP
                bad = PV.check_result(Cbuf[:, :N], clean[(alpha, beta)], special)
                assert bad is None, (alpha, beta, bad)


# ---- (c) convolution ----------------------------------------------------------------------------------------------------------
G = PV.CONV_GEOMETRIES
DIRECT = lambda d: d["cfg"] == -3
COMPILER = lambda d: d["cfg"] >= 0 and d["asm"] == 0
ASM_CONV = lambda d: 0 < d["asm"] < 67


def _cut(form):
    """the assembly main launch, the cut at the last whole 128-pixel tile, the tail as `form` (last_conv_tail)"""
    return lambda d: ASM_CONV(d) and d["split"] == 128 and d["tail"] == form


# name -> (geometry, options, what the diagnostics of a launch WITHOUT the epilogue must say: cfg = last_f32_config, asm =
# last_f32_asm, tail = last_conv_tail, split = last_split).  With bias + tanh every route ends on the compiler-scheduled implicit
# kernels (COMPILER): the direct kernels take no epilogue (launch_conv_direct_small_f32), the assembly loader bias and relu only
# (conv_asm_classify), the K-slice tail none.  The tail forms at K = 540: the direct tail kernel (1); kc slices + combine (2) in
# both modes, two slices; one compiler-kernel launch (3).
CONV_ROUTES = {
    "direct 1": (G[0], dict(conv_direct=1), DIRECT),
    "direct 2": (G[0], dict(conv_direct=2), DIRECT),
    "direct scalar-filter 1": (G[1], dict(conv_direct=1), DIRECT),
    "direct scalar-filter 3": (G[1], dict(conv_direct=3), DIRECT),
    "direct 12 channels": (G[2], dict(conv_direct=1), DIRECT),
    "direct 12 channels 2": (G[2], dict(conv_direct=2), DIRECT),
    "implicit W%4==0 patch": (G[3], dict(conv_direct=0, conv_patch=1, f32_asm=0), COMPILER),
    "implicit W%4==0 gather": (G[3], dict(conv_direct=0, conv_patch=0, f32_asm=0), COMPILER),
    "implicit W%4!=0 patch": (G[4], dict(conv_direct=0, conv_patch=1, f32_asm=0), COMPILER),
    "implicit W%4!=0 gather": (G[4], dict(conv_direct=0, conv_patch=0, f32_asm=0), COMPILER),
    "explicit im2col": (G[3], dict(conv_direct=0, conv_implicit=0, f32_asm=0), COMPILER),
    "explicit im2col W%4!=0": (G[4], dict(conv_direct=0, conv_implicit=0, f32_asm=0), COMPILER),
    "assembly K=210": (G[5], dict(f32_asm=2), ASM_CONV),
    "assembly K=147": (G[6], dict(f32_asm=2), ASM_CONV),
    "cut tail=1 kslice=1": (G[7], dict(f32_asm=2, conv_cut_always=1, conv_tail=1, conv_kslice=1), _cut(1)),
    "cut tail=1 kslice=0": (G[7], dict(f32_asm=2, conv_cut_always=1, conv_tail=1, conv_kslice=0), _cut(1)),
    "cut tail=0 kslice=1": (G[7], dict(f32_asm=2, conv_cut_always=1, conv_tail=0, conv_kslice=1), _cut(2)),
    "cut tail=0 kslice=0": (G[7], dict(f32_asm=2, conv_cut_always=1, conv_tail=0, conv_kslice=0), _cut(3)),
    "walkers 2": (G[8], dict(f32_asm=2, conv_walk=2), lambda d: d["asm"] >= 67),
    "walkers 3": (G[8], dict(f32_asm=2, conv_walk=3), lambda d: d["asm"] >= 67),
    "1x1 shortcut": (G[9], dict(), COMPILER),
    "1x1 implicit": (G[9], dict(conv_1x1_implicit=1, conv_direct=0, f32_asm=0), COMPILER),
}


def _guarded_dev(x, phase):
    import torch
    buf, start = PV.guarded(x, phase)
    d = torch.from_numpy(buf).cuda()
    return buf, d, d[start:start + x.size]


@pytest.mark.parametrize("name", list(CONV_ROUTES))
@pytest.mark.parametrize("mode", [0, 1], ids=["laser-order", "fast"])
def test_conv2d_im2col(la, oracle, mode, name):
    """Per route and float mode, without an epilogue and with bias + tanh: (1) a clean launch, the route asserted, equal to
    oracle.conv2d_im2col in laser-order mode without the epilogue; (2) the same operands between poisoned guard bands: identical
    output; (3) the poisoned input: the clean bits where the float64 convolution is finite, NaN / +-Inf exactly where it has them;
    (4) without padding, one NaN weight: its output channel NaN everywhere, nothing else changes."""
    import torch
    (ishape, kshape, pad, st), opts, ok = CONV_ROUTES[name]
    p = PV.conv_poison(ishape, kshape, pad, st, seed=11)
    oshape = la.conv2d_out_shape(ishape, kshape, pad, st)
    assert tuple(oshape) == p.special.shape and PV.finite_share(p.special) >= PV.CAP
    assert p.w_special is None or PV.finite_share(p.w_special) >= PV.CAP
    nout = int(np.prod(oshape))
    sent = BV.sentinel(np.float32, nout + 2 * PV.GUARD)
    fails, seen = [], set()

    def conv(what, dx, dw, db, act):
        dout = torch.from_numpy(sent.copy()).cuda()
        la.conv2d_im2col(dout[PV.GUARD:PV.GUARD + nout], oshape, dx, ishape, dw, kshape, pad, st, None, bias=db, activation=act)
        _sync()
        d = dict(cfg=la.get_option("last_f32_config"), asm=la.last_f32_asm(), tail=la.get_option("last_conv_tail"), split=la.last_split())
        seen.add((act,) + tuple(d.values()))
        if not (COMPILER if act else ok)(d):
            fails.append(f"{what}: not on its route: {d}")
        out = dout.cpu().numpy()
        if not (_same(out[:PV.GUARD], sent[:PV.GUARD]) and _same(out[PV.GUARD + nout:], sent[:PV.GUARD])):
            fails.append(f"{what}: wrote outside the output")
        return out[PV.GUARD:PV.GUARD + nout].reshape(oshape)

    with options(la, mode, **opts):
        plain = [torch.from_numpy(np.array(v)).cuda() for v in (p.x, p.w, p.bias)]
        hx, gx, vx = _guarded_dev(p.x, 0)
        hw, gw, vw = _guarded_dev(p.w, 1)
        hb, gb, vb = _guarded_dev(p.bias, 2)
        hxp, gxp, vxp = _guarded_dev(p.x_poison, 0)
        if p.w_poison is not None:
            hwp, gwp, vwp = _guarded_dev(p.w_poison, 1)
        for epilogue in (False, True):
            act = "tanh" if epilogue else None
            what = f"{name} mode {mode} {'bias + tanh' if epilogue else 'plain'}"
            clean = conv(f"{what}, clean", plain[0], plain[1], plain[2] if epilogue else None, act)
            if mode == 0 and not epilogue:
                if not _same(clean, oracle.conv2d_im2col(p.x, p.w, pad, st, isa=oracle.fused_isa(np.float32))):
                    fails.append(f"{what}: the clean launch differs from the oracle")
            elif not epilogue:
                mre = oracle.mean_relative_error(clean, PV.conv_reference(p.x, p.w, pad, st))
                if not mre <= 1e-5:
                    fails.append(f"{what}: the clean FAST launch has mean relative error {mre:.3e}")
            got = conv(f"{what}, guard bands", vx, vw, vb if epilogue else None, act)
            if not _same(got, clean):
                fails.append(f"{what}: the guard bands reached the output: {PV.check_result(got, clean, np.zeros_like(p.special))}")
            got = conv(f"{what}, poisoned input", vxp, vw, vb if epilogue else None, act)
            bad = PV.check_result(got, clean, p.special, tanh=epilogue)
            if bad:
                fails.append(f"{what}, poisoned input: {bad}")
            if p.w_poison is not None:
                got = conv(f"{what}, poisoned filter", vx, vwp, vb if epilogue else None, act)
                bad = PV.check_result(got, clean, p.w_special, tanh=epilogue)
                if bad:
                    fails.append(f"{what}, poisoned filter: {bad}")
        for h, g in ((hx, gx), (hw, gw), (hb, gb), (hxp, gxp)):
            if not _same(g.cpu().numpy(), h):
                fails.append(f"{name}: an operand buffer changed")
    _done(fails, [f"POISON_CONV {name!r} mode {mode}: (activation, cfg, asm, tail, split) = {sorted(seen, key=repr)}"])
