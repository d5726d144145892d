"""laser_hip_gemm_strided_batched_*_dev on every kernel family, element type, layout and alpha / beta (tests/batched_views.py):
each family indexes the batch in its own code -- the compiler-scheduled tiled kernels and the small-matrix kernel by grid y, the
VALU kernel by grid z, the hand-scheduled kernels through byte batch strides in their kernel arguments -- and the host side picks
vector / edge / scalar loaders from the batch strides.

Every comparison is bit-exact against the references cached in tests/batched_views.py (the CPU oracle per entry for float32 /
float64 / int32 / int64, wrapping 64-bit arithmetic for the narrow and unsigned types); the library stays in laser-order mode.
Per case: (1) the gathered C equals the reference, (2) every element of the C arena the view does not address still holds the
sentinel, (3) the A and B arenas are unchanged (checked once per (layout, shape): the alpha / beta variants share them), (4) with a
negative batch stride the hand-scheduled kernels did not run.  (5) Every route is held to the same cached reference, so the routes
are equal to each other; small_path on / off is compared directly as well.

Which kernel ran.  The `last_*` diagnostics are process state that some rungs never reset (scripts/route_fingerprint.py records
them as such), so before every float launch a tiny single product puts them into a known state: float32 with configuration 3
pinned leaves (last_f32_asm, last_f32_config) = (0, 3); float64 with f64_asm = 0 leaves last_f64_asm = 0.  After the launch under
test the pair is normalised to what ran: (k, -1) = hand-scheduled kernel k, (0, -2) = the small-matrix kernel, (0, c) =
compiler-scheduled configuration c.  The integer routes prime last_i32_asm once, with a single 128^3 product on the compiler
limb kernel.

Coverage.  ROUTE_SETS holds, per route, the set of kernels observed on the MI355X; every run asserts it, so the file cannot pass
with everything on one kernel.  Over the routes with f32_asm = 2 the set holds the large tile, the 128x128 tile, the 64x64 tile,
a transposed-B variant and a 16x16-block tile (the index ranges tests/test_gpu_parity.py documents for last_f32_asm: 1 / 2 large,
3 / 4 128x128, + 4 B transposed, 13..16 64x64, 31..34 128x128x32, 47..66 the 16x16-block tiles).  The transposed-B variants are
reached through the layout `b_transposed` only: `transposed` has a column-major A, which the hand-scheduled launchers decline.
The one-chain 256x128 tile (9 / 10) cannot be reached in laser-order mode: class 1 has no laser-order row and the launcher
takes class 0 instead.
"""
import numpy as np
import pytest

from tests import batched_views as BV

pytestmark = pytest.mark.gpu

DEFAULTS = dict(f32_asm=1, asm_tile=-1, f64_asm=1, f64_mfma=1, small_path=1)


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import laser_amd
    assert laser_amd.lib().laser_hip_arch().decode().startswith("gfx950")
    return laser_amd


# ---- the launchers' rules, restated -----------------------------------------------------------------------------------------
def small_takes(c, small_path=True):
    """gemm_small_takes (device-resident) and launch_gemm_small's stride limits, which no view of the catalogue reaches"""
    fits = all(abs(s) * c.dtype.itemsize < 2 ** 31 for s in (c.A.strides[2], c.B.strides[1]))
    return bool(small_path) and c.dtype.kind == "f" and c.batch > 1 and c.M <= 64 and c.N <= 64 and c.K <= 128 and fits


def asm_takes(c, pin=-1):
    """choose_gemm_f32_asm / choose_gemm_f64_asm on a plain batched problem of these sizes, the kernels forced (f32_asm / f64_asm =
    2): no negative batch stride, A row-major, B row-major or k-contiguous, C with rows as the slow direction (float64: unit
    column stride, K even); the 16x16-block tile classes need K % 4 == 0"""
    (bsA, rsA, csA), (bsB, rsB, csB), (bsC, rsC, csC) = c.A.strides, c.B.strides, c.C.strides
    if c.batch > 1 and min(bsA, bsB, bsC) < 0:
        return False
    if csA != 1 or csC < 1 or rsC < (c.N - 1) * csC + 1:
        return False
    nt = csB != 1 and rsB == 1
    if not nt and csB != 1:
        return False
    ldb = csB if nt else rsB
    if rsA < c.K or ldb < (c.K if nt else c.N):
        return False
    if c.dtype == np.float64:
        return csC == 1 and c.K >= 2 and c.K % 2 == 0
    return not (pin >= 5 and c.K % 4 != 0)


def asm_class(last):
    """(tile class of option "asm_tile", B transposed) of last_f32_asm = 1 + the kernel's index"""
    k = last - 1
    if k in (0, 1, 4, 5):
        return 0, k >= 4
    if k in (2, 3, 6, 7):
        return 2, k >= 6
    if k in (8, 9):
        return 1, k == 9
    if 12 <= k <= 15:
        return 4, k >= 14
    if 30 <= k <= 33:
        return 3, k >= 32
    if 46 <= k <= 65:
        return 5 + (k - 46) // 4, (k - 46) % 4 >= 2
    raise AssertionError(f"last_f32_asm = {last} is no float32 GEMM kernel")


# ---- the kernels observed per route on the MI355X, asserted on every run ---------------------------------------------------
ROUTE_SETS = {
    # at these sizes the compiler-scheduled kernels' model always takes the 64x64 configuration (3), and f32_asm = 1 keeps the
    # hand-scheduled kernels for problems of 5 / 8 of a round of tiles and more: the heuristic route is the compiler-scheduled one
    "f32 heuristic": {(0, -2), (0, 3)},
    "f32 hand-scheduled": {(0, -2), (0, 3), (13, -1), (15, -1)},
    "f32 compiler-scheduled": {(0, -2), (0, 3)},
    "f32 asm_tile 0": {(0, 3), (1, -1), (5, -1)},
    "f32 asm_tile 1": {(0, 3), (1, -1), (5, -1)},          # (no laser-order row in class 1: class 0's tile)
    "f32 asm_tile 2": {(0, 3), (3, -1), (7, -1)},
    "f32 asm_tile 3": {(0, 3), (31, -1), (33, -1)},
    "f32 asm_tile 4": {(0, 3), (13, -1), (15, -1)},
    "f32 asm_tile 5": {(0, 3), (47, -1), (49, -1)},
    "f32 asm_tile 6": {(0, 3), (51, -1), (53, -1)},
    "f32 asm_tile 7": {(0, 3), (55, -1), (57, -1)},
    "f32 asm_tile 8": {(0, 3), (59, -1), (61, -1)},
    "f32 asm_tile 9": {(0, 3), (63, -1), (65, -1)},
    # a pinned configuration without the scalar loaders hands the views that need them to 3, and one without laser-order
    # accumulators hands K > kc to 4 (launch_mfma_cfg, launch_mfma)
    "f32 config 0 256x256x16_w2x4_s3": {(0, 0), (0, 3), (0, 4)},
    "f32 config 1 256x128x16_w4x2_s3": {(0, 1), (0, 3)},
    "f32 config 2 128x128x16_w2x2_s3": {(0, 2)},
    "f32 config 3 64x64x32_w2x2_s2": {(0, 3)},
    "f32 config 4 256x128x32_w4x2_s3": {(0, 3), (0, 4)},
    # last_f64_asm: 0 = the small-matrix, compiler-scheduled or VALU kernels; 19 / 28 = lh_f64_exact_64x64x16 / its transposed-B
    # variant (at K = 260 and 1028: laser-order slices; K = 128 and below is the small-matrix kernel's, K = 517 and 1 are odd)
    "f64 hand-scheduled": {0, 19, 28},
    "f64 compiler-scheduled": {0},
    "f64 VALU": {0},
}


# ---- running a case ---------------------------------------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()


def _call(la, c, dA, dB, dC, batch=None, K=None):
    la.gemm_strided_batched(c.batch if batch is None else batch, c.M, c.N, c.K if K is None else K, c.alpha,
                            dA[c.A.offset:], c.A.strides[1], c.A.strides[2], c.A.strides[0],
                            dB[c.B.offset:], c.B.strides[1], c.B.strides[2], c.B.strides[0], c.beta,
                            dC[c.C.offset:], c.C.strides[1], c.C.strides[2], c.C.strides[0])


_PRIMERS = {}


def _prime(la, dt):
    """put the diagnostics of the element type into a known state (module docstring)"""
    import torch
    if dt.kind != "f":
        return
    if dt.name not in _PRIMERS:
        _PRIMERS[dt.name] = tuple(torch.ones((16, 16), dtype=getattr(torch, dt.name), device="cuda") for _ in range(3))
    x, y, z = _PRIMERS[dt.name]
    if dt == np.float32:
        cfg = la.get_f32_config()
        la.set_f32_config(3)
        try:
            la.matmul(x, y, out=z)
        finally:
            la.set_f32_config(cfg)
    else:
        before = [(o, la.get_option(o)) for o in ("f64_mfma", "f64_asm")]
        la.set_option("f64_mfma", 1); la.set_option("f64_asm", 0)
        try:
            la.matmul(x, y, out=z)
        finally:
            for o, v in before:
                la.set_option(o, v)


def _ran(la, dt):
    """what ran, normalised (module docstring); None for the integer types"""
    if dt == np.float32:
        asm, cfg = la.last_f32_asm(), la.last_f32_config()
        return (asm, -1) if asm else (0, cfg)
    if dt == np.float64:
        return la.get_option("last_f64_asm")
    return None


def _first_bad(got, want):
    bad = np.argwhere(BV.bits(got) != BV.bits(want))
    if not bad.size:
        return None
    p, i, j = (int(v) for v in bad[0])
    return f"{len(bad)} elements differ, first at (p, i, j) = ({p}, {i}, {j}): got {got[p, i, j]!r} want {want[p, i, j]!r}"


def run_cases(la, route, case_list, check=None, results=None):
    """Run the cases (grouped by layout and shape as batched_views.cases yields them) under the options already set; returns
    (failures, set of what ran).  check(case, ran) -> message or None adds the route's own rule; results[key] collects the gathered
    C per case."""
    import torch
    fails, seen = [], set()
    group, dA, dB = None, None, None

    def close_group():
        if group is not None:
            a, b, _, _ = BV.arenas(group)
            for name, host, d in (("A", a, dA), ("B", b, dB)):
                if not np.array_equal(BV.bits(d.cpu().numpy()), BV.bits(host)):
                    fails.append(f"[{route}] {BV.describe(group)}: the {name} arena changed")

    for c in case_list:
        key = (c.layout, c.batch, c.M, c.N, c.K)
        if group is None or key != (group.layout, group.batch, group.M, group.N, group.K):
            close_group()
            group = c
            a, b, _, _ = BV.arenas(c)
            dA, dB = _dev(a), _dev(b)
        want = BV.expected(c)
        off = BV.element_offsets(c.C, c.batch, c.M, c.N)
        for nan_c in ((False, True) if (c.dtype.kind == "f" and (c.alpha, c.beta) == (1, 0)) else (False,)):
            what = f"[{route}] {BV.describe(c)}{' over a C of NaNs' if nan_c else ''}"
            _, _, cbuf, mask = BV.arenas(c, nan_c)
            dC = _dev(cbuf)
            _prime(la, c.dtype)
            _call(la, c, dA, dB, dC)
            torch.cuda.synchronize()
            ran = _ran(la, c.dtype)
            seen.add(ran)
            hC = dC.cpu().numpy()
            got = hC[off]
            bad = _first_bad(got, want)
            if bad:
                fails.append(f"{what} (ran {ran}): {bad}")
            if not np.array_equal(BV.bits(hC)[~mask], BV.bits(cbuf)[~mask]):
                n = int((BV.bits(hC)[~mask] != BV.bits(cbuf)[~mask]).sum())
                fails.append(f"{what} (ran {ran}): {n} elements outside the C view lost their sentinel")
            if min(c.A.strides[0], c.B.strides[0], c.C.strides[0]) < 0 and c.dtype.kind == "f" and (ran[0] if c.dtype == np.float32 else ran) != 0:
                fails.append(f"{what}: a hand-scheduled kernel ({ran}) took a negative batch stride")
            msg = check(c, ran) if check else None
            if msg:
                fails.append(f"{what} (ran {ran}): {msg}")
            if results is not None:
                results[(c.layout, c.batch, c.M, c.N, c.K, c.alpha, c.beta, nan_c)] = got
    close_group()
    return fails, seen


def _with_options(la, options, body):
    try:
        for k, v in options.items():
            la.set_option(k, v)
        return body()
    finally:
        for k, v in DEFAULTS.items():
            la.set_option(k, v)
        la.set_f32_config(-1)
        la.set_float_mode(0)


def _finish(route, fails, seen):
    print(f"ROUTE_SET {route!r}: {sorted(seen, key=repr)!r}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])
    assert route in ROUTE_SETS and seen == ROUTE_SETS[route], f"route {route!r} ran {sorted(seen, key=repr)}, recorded {sorted(ROUTE_SETS.get(route, ()), key=repr)}"


# ---- float32 ----------------------------------------------------------------------------------------------------------------
def _f32_rule(asm_mode, small_path=True, pin=-1):
    """what must have run on a float32 case: the small-matrix kernel exactly where it applies, then the hand-scheduled kernels
    exactly where their launcher accepts (forced) or nowhere (off; at the default, f32_asm = 1, these few tiles are below the
    launcher's floor of 5 / 8 of a round)"""
    def check(c, ran):
        if small_takes(c, small_path):
            return None if ran == (0, -2) else "the small-matrix kernel did not run"
        if ran == (0, -2):
            return "the small-matrix kernel ran outside its class"
        if asm_mode == 2 and asm_takes(c, pin):
            if ran[0] == 0:
                return "the hand-scheduled launcher declined a view it accepts"
            cls, nt = asm_class(ran[0])
            if pin >= 0 and cls != (0 if pin == 1 else pin):
                return f"asm_tile = {pin} ran a kernel of class {cls}"
            if nt != (c.B.strides[2] != 1 and c.B.strides[1] == 1):
                return "the transposed-B variant does not match B's strides"
            return None
        return None if ran[0] == 0 else "a hand-scheduled kernel ran where its launcher declines"
    return check


F32_ROUTES = {"f32 heuristic": (dict(), 1), "f32 hand-scheduled": (dict(f32_asm=2), 2), "f32 compiler-scheduled": (dict(f32_asm=0), 0)}


@pytest.mark.parametrize("route", list(F32_ROUTES))
def test_f32_routes(la, route):
    options, asm_mode = F32_ROUTES[route]
    fails, seen = _with_options(la, options, lambda: run_cases(la, route, BV.cases(np.float32), _f32_rule(asm_mode)))
    _finish(route, fails, seen)


def test_f32_every_pinned_compiler_configuration(la):
    """set_f32_config(i) switches every rung off but the compiler-scheduled kernels; a configuration without the scalar loaders
    hands a view that needs them to one that has them (launch_mfma_cfg), so the configuration that ran is recorded, not assumed"""
    names = la.f32_configs()
    case_list = BV.cases(np.float32, layouts=["padded", "transposed", "reversed_batches", "interleaved"], scalar_list=[(0.5, 0.25)])
    fails, seen = [], {}
    for i in range(len(names)):
        route = f"f32 config {i} {names[i]}"

        def body():
            la.set_f32_config(i)
            return run_cases(la, route, case_list, lambda c, ran: None if ran[0] == 0 and ran[1] >= 0 else "not a compiler-scheduled kernel")
        f, seen[route] = _with_options(la, {}, body)
        fails += f
    for route in seen:
        print(f"ROUTE_SET {route!r}: {sorted(seen[route], key=repr)!r}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])
    assert seen == {r: k for r, k in ROUTE_SETS.items() if r.startswith("f32 config ")}, seen


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_small_matrix_kernel_on_and_off(la, dtype):
    """the small-matrix kernel takes a batch as grid y: every layout at every shape, `small_path` on (it runs exactly where
    gemm_small_takes and the stride limits say so: last_f32_config == -2) and off (it never runs); equal bits on the shapes it takes"""
    on, off = {}, {}
    case_list = BV.cases(dtype)
    name = np.dtype(dtype).name
    is32 = dtype == np.float32
    f1, s1 = _with_options(la, dict(small_path=1), lambda: run_cases(la, f"{name} small_path=1", case_list, _f32_rule(1, True) if is32 else None, on))
    f0, s0 = _with_options(la, dict(small_path=0), lambda: run_cases(la, f"{name} small_path=0", case_list, _f32_rule(1, False) if is32 else None, off))
    taken = [c for c in case_list if small_takes(c)]
    assert {(c.batch, c.M, c.N, c.K) for c in taken} >= set(BV.SMALL_SHAPES)
    fails = f1 + f0
    for key in on:
        if not np.array_equal(BV.bits(on[key]), BV.bits(off[key])):
            fails.append(f"{name} {key}: small_path on and off differ")
    print(f"ROUTE_SET '{name} small_path=1': {sorted(s1, key=repr)!r}\nROUTE_SET '{name} small_path=0': {sorted(s0, key=repr)!r}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])
    if is32:
        assert (0, -2) in s1 and (0, -2) not in s0


@pytest.mark.parametrize("pin", range(10))
def test_f32_each_assembly_tile_class(la, pin):
    """f32_asm = 2 with option asm_tile pinning each class, on the two tiled shapes at and past kc: where the launcher accepts
    (asm_takes) a kernel of that class ran, where it declines -- every negative or non-unit stride it cannot do, K % 4 != 0 on
    the 16x16-block tiles -- last_f32_asm == 0 and the compiler-scheduled kernels give the same bits"""
    route = f"f32 asm_tile {pin}"
    case_list = BV.cases(np.float32, shape_list=[(3, 200, 136, 260), (3, 130, 70, 517)])
    fails, seen = _with_options(la, dict(f32_asm=2, asm_tile=pin), lambda: run_cases(la, route, case_list, _f32_rule(2, True, pin)))
    _finish(route, fails, seen)


def test_recorded_f32_assembly_routes_cover_every_kernel_class():
    """over the routes with f32_asm = 2: the large tile, the 128x128 tile, the 64x64 tile, a transposed-B variant, a 16x16-block tile"""
    seen = set()
    for route, kernels in ROUTE_SETS.items():
        if route == "f32 hand-scheduled" or route.startswith("f32 asm_tile"):
            seen |= {asm_class(k) for k, _ in kernels if k}
    classes = {cls for cls, _ in seen}
    assert {0, 2, 4} <= classes and classes & {5, 6, 7, 8, 9} and any(nt for _, nt in seen), sorted(seen)


# ---- float64 ----------------------------------------------------------------------------------------------------------------
F64_ROUTES = {"f64 hand-scheduled": dict(f64_asm=2), "f64 compiler-scheduled": dict(f64_asm=0), "f64 VALU": dict(f64_mfma=0)}


@pytest.mark.parametrize("route", list(F64_ROUTES))
def test_f64_routes(la, route):
    """the hand-scheduled kernels (forced: they run exactly where their launcher accepts and the small-matrix kernel does not come
    first), the compiler-scheduled matrix-core kernels, and the VALU kernel, which takes the batch as grid z"""
    options = F64_ROUTES[route]

    def check(c, ran):
        if options.get("f64_asm") == 2 and asm_takes(c) and not small_takes(c):
            return None if ran else "the hand-scheduled launcher declined a view it accepts"
        return None if ran == 0 else "a hand-scheduled kernel ran where its launcher declines"
    fails, seen = _with_options(la, options, lambda: run_cases(la, route, BV.cases(np.float64), check))
    _finish(route, fails, seen)


# ---- integers ---------------------------------------------------------------------------------------------------------------
INTS = [dt for dt in BV.DTYPES if np.dtype(dt).kind != "f"]


@pytest.mark.parametrize("dtype", INTS, ids=[np.dtype(t).name for t in INTS])
def test_integer_batches_run_on_the_valu_kernel(la, dtype):
    """all eight integer types at the defaults: a batch goes to the VALU kernel (grid z), never to the limb kernels on the matrix
    cores -- last_narrow_mfma (reset by every integer launch) and last_i32_asm (primed to 0 here) stay 0"""
    import torch
    x = torch.ones((128, 128), dtype=torch.int32, device="cuda")
    la.set_option("i32_asm", 0)
    try:
        la.matmul(x, x)                          # a single product on the compiler-scheduled limb kernel: last_i32_asm = 0
    finally:
        la.set_option("i32_asm", 1)
    assert la.get_option("last_i32_asm") == 0

    def check(c, ran):
        if la.get_option("last_narrow_mfma") != 0 or la.get_option("last_i32_asm") != 0:
            return "a batch ran on the limb kernels"
        return None
    name = np.dtype(dtype).name
    fails, _ = _with_options(la, {}, lambda: run_cases(la, f"{name} defaults", BV.cases(dtype), check))
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ---- the batch-count limit ----------------------------------------------------------------------------------------------------
LIMIT_RUNS = [("float32 small_path=1", np.float32, dict(small_path=1)), ("float32 small_path=0", np.float32, dict(small_path=0)),
              ("float64", np.float64, dict()), ("int32", np.int32, dict())]


@pytest.mark.parametrize("name,dtype,options", LIMIT_RUNS, ids=[r[0].replace(" ", "-") for r in LIMIT_RUNS])
def test_batch_count_limit(la, name, dtype, options):
    """batch = 65535, the largest accepted (grid y of the small-matrix and tiled kernels, grid z of the VALU kernel), A shared,
    values that are exact in any order: all 65535 entries against one einsum; 65536 is refused and leaves C as it was; batch = 0
    and K = 0 leave C untouched"""
    import torch
    M, N, K = BV.LIMIT_SHAPE
    A, B, C0, alpha, beta, want = BV.limit_operands(dtype, BV.LIMIT_BATCH + 1)
    guard = M * N
    cbuf = np.concatenate([BV.sentinel(dtype, guard), C0.ravel(), BV.sentinel(dtype, guard)])
    dA, dB = _dev(A), _dev(B)

    def launch(batch, k=K, refused=False):
        dC = _dev(cbuf)
        try:
            la.gemm_strided_batched(batch, M, N, k, alpha, dA, K, 1, 0, dB, N, 1, K * N, beta, dC[guard:], N, 1, M * N)
            assert not refused, f"{name}: batch = {batch} was accepted"
        except la.LaserHipError:
            assert refused, f"{name}: batch = {batch}, K = {k} was refused"
        torch.cuda.synchronize()
        return dC.cpu().numpy()

    def body():
        _prime(la, np.dtype(dtype))
        got = launch(BV.LIMIT_BATCH)
        ran = _ran(la, np.dtype(dtype))
        n = BV.LIMIT_BATCH * M * N
        bad = _first_bad(got[guard:guard + n].reshape(-1, M, N), want[:-1])
        assert bad is None, f"{name}: {bad}"
        assert np.array_equal(BV.bits(got[:guard]), BV.bits(cbuf[:guard])) and np.array_equal(BV.bits(got[guard + n:]), BV.bits(cbuf[guard + n:])), \
            f"{name}: wrote outside the 65535 entries"
        if dtype == np.float32:
            assert (ran == (0, -2)) == bool(options["small_path"]), ran
        for batch, k, refused in ((BV.LIMIT_BATCH + 1, K, True), (0, K, False), (7, 0, False)):
            assert np.array_equal(BV.bits(launch(batch, k, refused)), BV.bits(cbuf)), f"{name}: batch = {batch}, K = {k} touched C"
    _with_options(la, options, body)


# ---- the Python mirror ----------------------------------------------------------------------------------------------------------
def test_mirror_refuses_operands_of_another_element_type(la):
    """gemm_strided_batched checks A and B like gemm_strided does: a float64 A would otherwise be read as float32"""
    import torch
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    C = torch.full((2, 4, 4), 3.0, dtype=torch.float32, device="cuda")
    for A, B in ((f64(2, 4, 4), f32(2, 4, 4)), (f32(2, 4, 4), f64(2, 4, 4)), (f32(2, 4, 4), torch.zeros((2, 4, 4), dtype=torch.int32, device="cuda"))):
        with pytest.raises(TypeError):
            la.gemm_strided_batched(2, 4, 4, 4, 1.0, A, 4, 1, 16, B, 4, 1, 16, 0.0, C, 4, 1, 16)
    torch.cuda.synchronize()
    assert (C == 3.0).all()
    la.gemm_strided_batched(2, 4, 4, 4, 1.0, f32(2, 4, 4), 4, 1, 16, f32(2, 4, 4), 4, 1, 16, 0.0, C, 4, 1, 16)
    torch.cuda.synchronize()
    assert (C == 0.0).all()
