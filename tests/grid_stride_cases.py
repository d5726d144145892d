"""The capped launches of the library, each run past its cap: the table of shapes, their data and their models.

Nearly every device kernel launches a capped grid (2048 workgroups for the row, strip and column kernels, 8 per compute unit
for the scan, 16384 for the sampler and the lane-per-item kernels of scan.hip, 65536 for the embedding) and walks its rows,
strips or units with a grid-sized stride.  What can go wrong there -- LDS scratch reused while a slow wave still reads it, a
maximum or an accumulator carried from one row of a workgroup into its next, a unit walk that wraps wrongly -- shows on the
second trip of that loop and not on the first.  Which family runs a second trip, and where:

    family                                   past the cap in
    ---------------------------------------  --------------------------------------------------------------------------------
    pointwise / activation                   test_gpu_activation.py (CAP = 2048 * 256 * 4)
    random fill                              test_gpu_random.py
    log-softmax / logsumexp / cross-entropy  test_gpu_log_softmax.py (wave and workgroup kernels); the long-row kernel: here
    softmax rows                             here: wave, workgroup and long-row kernels, both instances
    softmax along an axis (strip kernels)    here: resident and streaming kernels, 2052 strips over 3 outer indices
    layer norm forward and dx                here: wave, workgroup and long-row kernels, both instances (tests/cpp/layer_norm_mirror.cpp
                                             crosses the wave kernels' cap by the way, with the 16389 rows of its column sums)
    layer norm dgamma / dbeta                here: 2050 units in one chunk (the walk stops), 2052 in two (the walk wraps)
    bias gradient / dense backward           here: the same two walks, the second with the fold launch behind it
    row cumsum                               here: wave and workgroup variants, f32 and i64
    searchsorted, CDF draws (scan.hip)       here: 16387 x 257 lanes; draw-and-remove: 2^22 + 3 rows (a lane per row)
    sampler build                            here: both launches of the segment kernel, and the LDS kernel
    sampler sample / update / remove         here: 16387 x 257 lanes; update and remove on 2^22 + 3 rows (a lane per row)
    embedding gather                         here: 65539 tokens of 1024 columns; columns past 1024 (a second lane trip)
    embedding grouping                       here: tile 1024 with 2049 workgroups a pass; 4 passes and `starts` past 65536
    embedding short and long sums            here: 65539 ids; 2 and 3 column blocks; 65 and more strips; 2049 position tiles
    GEMM, convolution                        test_gpu_scheduler.py (persistent plans; not a grid-stride loop over rows)
    reductions                               the grid is the chunk count: no stride loop

A new capped kernel gets a row above and a case below.  Left out, with the reason:
    sampler update on the 16387-row tree     update and draw-and-remove give a lane to a ROW, not to a draw: their lane count
                                             passes 16384 * 256 only with 2^22 + 3 rows, so they have a tree of 3 weights
    embedding grid y (65535 blocks)          needs dim > 16 * 65535 columns per row next to 65 ids: past 1 GB; the column loops
                                             `q += gridDim.y * lpr` and `strip += gridDim.y` take one trip in every case here
    scan on more compute units               the launcher plans with cus = 0, that is 256: the cap is 2048 on every device

Every case is built from a base of PERIOD = 13 vectors (rows for the row kernels, columns for the column and strip kernels),
tiled: operand vector i is base vector i mod 13 (for the strips (i + 5 o) mod 13 with the outer index o).  13 is coprime to
4, 8, 16, 2048, 1022, 1026, 16384 and 65536, so the vectors a workgroup meets on its trips differ.  Base vector k is scaled by
2^(k - 6); vector NAN_AT holds a NaN, vector EQUAL_AT is constant and, for the softmax families, vector NINF_AT is all -Inf:
a maximum, a sum or a row that survives from the previous trip then changes the next result's bits.  The models run on the
base alone; test_grid_stride_cpu.py checks that their results for the 13 vectors differ pairwise in bits, which is what makes
"trip two got trip one's vector" visible, and that every shape exceeds its cap in the plan.  test_gpu_grid_stride.py runs them.

No GPU import here: the plans are asked of the library handle the caller passes in."""
import ctypes as C
import functools
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
F = np.float32
PERIOD = 13
NAN_AT, EQUAL_AT, NINF_AT = 3, 7, 10
FWD, DX, PARAMS = 0, 1, 2                      # laser_hip_layer_norm_plan's `what`
TOP = F(1) - F(2.0 ** -24)                     # the largest float32 below 1


def text_of(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def define(header, name):
    """an integer #define of a header of laser_amd/csrc"""
    return int(re.search(r"#define " + name + r" (\d+)\b", text_of(header)).group(1))


def constant(source, name):
    """an integer `constexpr int name = value` of a source file of laser_amd/csrc"""
    return int(re.search(r"\b" + name + r" = (\d+)\b", text_of(source)).group(1))


# ---- the constants the shapes are computed from: read from the plan headers, held against the plans by the CPU test --------------
ROW_CAP = define("softmax_rows_plan.h", "LH_SOFTMAX_ROWS_MAX_WORKGROUPS")
WAVE_N = define("softmax_rows_plan.h", "LH_SOFTMAX_ROWS_WAVE_N")          # the longest row of the wave kernels
CHUNK_N = define("softmax_rows_plan.h", "LH_SOFTMAX_ROWS_CHUNK_N")        # the longest row of the workgroup kernels
LN_CAP = define("layer_norm_plan.h", "LH_LAYER_NORM_MAX_WORKGROUPS")
LN_CW = define("layer_norm_plan.h", "LH_LAYER_NORM_CW")
LN_CHUNK = define("layer_norm_plan.h", "LH_LAYER_NORM_CHUNK")
BG_CAP = define("bias_grad_plan.h", "LH_BIAS_GRAD_MAX_WORKGROUPS")
BG_CW = define("bias_grad_plan.h", "LH_BIAS_GRAD_CW")
BG_CHUNK = define("bias_grad_plan.h", "LH_BIAS_GRAD_CHUNK")
AXIS_CAP = define("softmax_axis_plan.h", "LH_SOFTMAX_MAX_WORKGROUPS")
AXIS_CW = define("softmax_axis_plan.h", "LH_SOFTMAX_AXIS_CW")
_m = re.search(r"#define LH_SOFTMAX_AXIS_RESIDENT_N \(LH_SOFTMAX_AXIS_CW == (\d+) \? (\d+) : (\d+)\)", text_of("softmax_axis_plan.h"))
AXIS_BOUND = int(_m.group(2)) if AXIS_CW == int(_m.group(1)) else int(_m.group(3))      # the longest axis of the resident kernel
SCAN_RUN = define("scan_core.h", "LH_SCAN_RUN")
SCAN_WAVE_N = define("scan_plan.h", "LH_SCAN_WAVE") * SCAN_RUN                         # the last n of the wave variant
SCAN_CUS = define("scan_plan.h", "LH_SCAN_DEFAULT_CUS")
SCAN_CAP = define("scan_plan.h", "LH_SCAN_WGS_PER_CU") * SCAN_CUS
SCAN_LANE_CAP = constant("scan.hip", "kMaxGrid")                                       # searchsorted and the CDF draws
SAMPLER_CAP = define("sampler_plan.h", "LH_SAMPLER_MAX_WORKGROUPS")
SAMPLER_SMALL_P = define("sampler_plan.h", "LH_SAMPLER_SMALL_P")
SAMPLER_SMALL_LEAVES = define("sampler_plan.h", "LH_SAMPLER_SMALL_LEAVES")
SAMPLER_SEG = define("sampler_plan.h", "LH_SAMPLER_SEG")
EMB_CAP = constant("embedding.hip", "kGridX")
EMB_MIN_TILE = define("embedding_plan.h", "LH_EMBEDDING_MIN_TILE")
EMB_SHORT = define("embedding_plan.h", "LH_EMBEDDING_SHORT")
EMB_PTILE = define("embedding_plan.h", "LH_EMBEDDING_PTILE")
EMB_MAX_TILES = 1 << 14                                                                 # LH_EMBEDDING_MAX_TILES (1ll << 14)
LANES = 256                                                                             # lanes of a workgroup, everywhere


def cdiv(a, b):
    return -(-a // b)


# `plan`: (the library's plan entry point, its arguments before the output array, the index of the workgroups in the output),
# or None where the launcher computes its grid itself; `units`: what the capped launch walks (rows, row groups, strips,
# chunks x strips, lane blocks), one number per capped launch of the call; all of them exceed `cap`
Case = namedtuple("Case", "id family entry shape plan cap units period note")
CASES = []


def add(id, family, entry, shape, plan, cap, units, note=""):
    CASES.append(Case(id, family, entry, dict(shape), plan, cap, tuple(units), PERIOD, note))


# ---- row kernels: the same three shapes for each family -------------------------------------------------------------------------
def row_shapes(cap, wave_n, chunk_n):
    """(kernel name, kernel code, rows, n, units): the smallest shapes whose launch loops, one per lane mapping"""
    return [("wave", 0, 4 * cap + 5, 5, cdiv(4 * cap + 5, 4)), ("block", 1, cap + 2, wave_n + 1, cap + 2),
            ("long", 2, cap + 2, chunk_n + 1, cap + 2)]


for _k, _code, _rows, _n, _units in row_shapes(ROW_CAP, WAVE_N, CHUNK_N):
    add(f"softmax-{_k}", "softmax_rows", "laser_hip_softmax_rows_f32_dev", dict(rows=_rows, n=_n, code=_code),
        ("laser_hip_softmax_rows_plan", (_rows, _n, 1), 1), ROW_CAP, [_units])
    if _k == "long":    # (test_gpu_log_softmax.py::test_more_rows_than_the_grid_has_workgroups has the other two)
        add(f"log-softmax-{_k}", "log_softmax_rows", "laser_hip_{logsumexp,log_softmax,softmax_xent}_rows_f32_dev",
            dict(rows=_rows, n=_n, code=_code), ("laser_hip_softmax_rows_plan", (_rows, _n, 1), 1), ROW_CAP, [_units])
for _k, _code, _rows, _n, _units in row_shapes(LN_CAP, define("layer_norm_plan.h", "LH_LAYER_NORM_WAVE_N"), LN_CHUNK):
    add(f"layer-norm-forward-{_k}", "layer_norm_forward", "laser_hip_layer_norm_f32_dev", dict(rows=_rows, n=_n, code=_code),
        ("laser_hip_layer_norm_plan", (_rows, _n, 1, FWD), 1), LN_CAP, [_units])
    add(f"layer-norm-dx-{_k}", "layer_norm_dx", "laser_hip_layer_norm_grad_f32_dev", dict(rows=_rows, n=_n, code=_code),
        ("laser_hip_layer_norm_plan", (_rows, _n, 1, DX), 1), LN_CAP, [_units])

# ---- strip kernels of the axis softmax: 3 outer indices, just over cap / 3 strips each, the last strip ragged ------------------------
_per_outer = AXIS_CAP // 3 + 2                           # 3 * 684 = 2052 > 2048 >= 3 * 682
_inner = AXIS_CW * (_per_outer - 1) + 5
for _k, _code, _n in (("resident", 8, 5), ("streaming", 9, AXIS_BOUND + 1)):
    add(f"softmax-axis-{_k}", "softmax_axis", "laser_hip_softmax_axis_f32_dev", dict(outer=3, n=_n, inner=_inner, code=_code),
        ("laser_hip_softmax_axis_plan", (3, _n, _inner, 1, 256), 2), AXIS_CAP, [3 * cdiv(_inner, AXIS_CW)])

# ---- column kernels: (a) one chunk, two strips more than the grid; (b) two chunks of half the grid plus two strips -----------------
#      (a): step_chunks = 0, step_strips = cap: workgroup 2's second unit wraps past the last chunk and the walk must stop
#      (b): step_chunks = 1, step_strips = cap - strips: workgroups 0 .. 3 reach the last four units in the second chunk; every
#           wrap `strip -= strips; ++ch` still leaves the matrix; the launch is two-level, the fold launch behind it
#      (c): the same strips over three chunks: workgroups 4 and up wrap INTO the third chunk.  A wrap can land on a unit only
#           with three chunks and more than cap / 2 strips, so this is the smallest such shape (0.54 GB an operand, 1.08 GB for
#           the bias gradient's wider strips)
for _fam, _entry, _pl, _cap, _cw, _chunk, _args in (
        ("bias_grad", "laser_hip_bias_grad_f32_dev", "laser_hip_bias_grad_plan", BG_CAP, BG_CW, BG_CHUNK, (1, 256)),
        ("layer_norm_params", "laser_hip_layer_norm_grad_f32_dev", "laser_hip_layer_norm_plan", LN_CAP, LN_CW, LN_CHUNK, (1, PARAMS))):
    for _k, _rows, _strips in (("a", 5, _cap + 2), ("b", _chunk + 1, _cap // 2 + 2), ("c", 2 * _chunk + 1, _cap // 2 + 2)):
        _n = _cw * (_strips - 1) + 3
        _chunks = cdiv(_rows, _chunk)
        add(f"{_fam.replace('_', '-')}-{_k}", _fam, _entry,
            dict(rows=_rows, n=_n, chunks=_chunks, strips=_strips, step_chunks=_cap // _strips, step_strips=_cap % _strips),
            (_pl, (_rows, _n) + _args, 1), _cap, [_chunks * _strips])

# ---- scan.hip ------------------------------------------------------------------------------------------------------------------------
for _sfx, _elem in (("f32", 4), ("i64", 8)):
    for _k, _variant, _rows, _n, _units in (("wave", 0, 4 * SCAN_CAP + 5, 5, cdiv(4 * SCAN_CAP + 5, 4)),
                                            ("block", 1, SCAN_CAP + 2, SCAN_WAVE_N + 1, SCAN_CAP + 2)):
        add(f"cumsum-{_sfx}-{_k}", "cumsum", f"laser_hip_cumsum_{_sfx}_dev", dict(sfx=_sfx, rows=_rows, n=_n, variant=_variant),
            ("laser_hip_cumsum_plan", (_rows, _n, _elem, SCAN_CUS), 2), SCAN_CAP, [_units])
_lane_rows, _lane_m = SCAN_LANE_CAP + 3, LANES + 1        # 16387 x 257 lanes > 16384 x 256
add("searchsorted", "scan_lanes", "laser_hip_searchsorted_f32_dev", dict(rows=_lane_rows, n=5, m=_lane_m), None, SCAN_LANE_CAP,
    [cdiv(_lane_rows * _lane_m, LANES)], "a lane per value")
add("cdf-sample", "scan_lanes", "laser_hip_cdf_sample_f32_dev", dict(rows=_lane_rows, n=5, m=_lane_m), None, SCAN_LANE_CAP,
    [cdiv(_lane_rows * _lane_m, LANES)], "a lane per draw")
_many = SCAN_LANE_CAP * LANES + 3                         # a lane per row: 2^22 + 3 rows, of 3 weights
add("cdf-sample-remove", "scan_lanes", "laser_hip_cdf_sample_remove_f32_dev", dict(rows=_many, n=3, k=2), None, SCAN_LANE_CAP,
    [cdiv(_many, LANES)], "a lane per row; its two scans walk 2^20 row groups with the grid of the cumsum")

# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
def leaves(n):
    """P: the next power of two >= n"""
    p = 1
    while p < n:
        p *= 2
    return p


_srows, _sn = SAMPLER_CAP + 3, SAMPLER_SEG + 1            # 2 segments a row: 32774 units, then 16387 rows
add("sampler-build-segments", "sampler_build", "laser_hip_sampler_build_f32_dev", dict(rows=_srows, n=_sn, code=1),
    ("laser_hip_sampler_plan", (_srows, _sn), (2, 3)), SAMPLER_CAP, [_srows * (leaves(_sn) // SAMPLER_SEG), _srows])
_per = SAMPLER_SMALL_LEAVES // SAMPLER_SMALL_P            # rows of one workgroup of the LDS kernel at its longest row
_lrows = _per * SAMPLER_CAP + 3
add("sampler-build-lds", "sampler_build", "laser_hip_sampler_build_f32_dev", dict(rows=_lrows, n=SAMPLER_SMALL_P, code=0),
    ("laser_hip_sampler_plan", (_lrows, SAMPLER_SMALL_P), (2,)), SAMPLER_CAP, [cdiv(_lrows, _per)])
add("sampler-sample", "sampler_lanes", "laser_hip_sampler_sample_f32_dev", dict(rows=_srows, n=_sn, m=LANES + 1), None, SAMPLER_CAP,
    [cdiv(_srows * (LANES + 1), LANES)], "a lane per draw, on the trees of sampler-build-segments")
_smany = SAMPLER_CAP * LANES + 3
add("sampler-update-remove", "sampler_lanes", "laser_hip_sampler_{build,update,sample_remove}_f32_dev", dict(rows=_smany, n=3, k=2),
    ("laser_hip_sampler_plan", (_smany, 3), (2,)), SAMPLER_CAP, [cdiv(_smany, SAMPLER_SMALL_LEAVES // leaves(3)), cdiv(_smany, LANES)],
    "a lane per row; the build is the LDS kernel with 256 rows a workgroup")


# ---- the embedding -------------------------------------------------------------------------------------------------------------------
def lanes_per_row(dim):
    """the lanes that span a row of `dim`: the power of two at or above its quads, at most 256 (embedding.hip)"""
    lpr = 1
    while lpr < LANES and lpr < cdiv(dim, 4):
        lpr *= 2
    return lpr


for _dim, _kind in ((WAVE_N + 1, "mixed"), (WAVE_N + 4, "mostly0"), (2 * WAVE_N + 4, "mixed")):
    # quads past 256 lanes: the gather's and the short kernel's lane trips, grid y = 2 and 3, 65 and more strips
    add(f"embedding-columns-{_dim}", "embedding_columns", "laser_hip_embedding_{f32,grad_f32}_dev",
        dict(tokens=300, vocab=13, dim=_dim, kind=_kind), None, LANES, [cdiv(_dim, 4)],
        "the units are the quads of a row, the cap the lanes that span it")
_tok = EMB_CAP + 3
add("embedding-gather-cap", "embedding_gather", "laser_hip_embedding_f32_dev", dict(tokens=_tok, vocab=13, dim=WAVE_N), None, EMB_CAP,
    [cdiv(_tok, LANES // lanes_per_row(WAVE_N))])
add("embedding-short-cap", "embedding_short", "laser_hip_embedding_grad_f32_dev", dict(tokens=3000, vocab=EMB_CAP + 3, dim=WAVE_N),
    None, EMB_CAP, [cdiv(EMB_CAP + 3, LANES // lanes_per_row(WAVE_N))])
_ttok = EMB_MIN_TILE * EMB_MAX_TILES + 5                  # one tile of 512 more than a pass takes: the tile doubles
add("embedding-tile", "embedding_tile", "laser_hip_embedding_{group_i32,grad_f32}_dev", dict(tokens=_ttok, vocab=257, dim=1, tile=1024),
    ("laser_hip_embedding_plan", (_ttok, 257, 1, 1, 256), 2), ROW_CAP, [cdiv(cdiv(_ttok, 1024), 4), cdiv(_ttok, EMB_PTILE)],
    "no launch is capped here: 2049 workgroups a pass and 2049 position tiles, one more than the other kernels' 2048")
add("embedding-group-4-passes", "embedding_group", "laser_hip_embedding_group_i32_dev", dict(tokens=1500, vocab=(1 << 24) + 5, passes=4),
    ("laser_hip_embedding_plan", (1500, (1 << 24) + 5, 0, 1, 256), 0), EMB_CAP, [((1 << 24) + 5 + LANES) // LANES],
    "the `starts` kernel, a lane per id")

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def of(family):
    return [c for c in CASES if c.family == family]


def plan_of(L, case):
    """the output array of the case's plan call"""
    name, args, _ = case.plan
    size = 8 if "embedding" in name else 3 if "softmax_rows" in name else 4
    out = (C.c_int64 * size)()
    assert getattr(L, name)(*args, out) == 0, (case.id, name, args)
    return list(out)


def planned_workgroups(L, case):
    """the workgroups the plan reports for the capped launches of the case"""
    where = case.plan[2]
    p = plan_of(L, case)
    return [p[i] for i in (where if isinstance(where, tuple) else (where,))]


# ---- the data: 13 base vectors and their models, computed once ----------------------------------------------------------------------
def scales():
    return (2.0 ** (np.arange(PERIOD) - 6)).astype(F)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def key_rows(a):
    """one bytes key per base vector of `a` (the first axis), every NaN the same NaN; None for a vector that is all NaN"""
    a = np.ascontiguousarray(a)
    a = a.reshape(a.shape[0], -1)
    out = []
    for r in a:
        if r.dtype.kind == "f":
            if np.isnan(r).all():
                out.append(None)
                continue
            r = np.where(np.isnan(r), r.dtype.type(np.nan), r)
        out.append(r.tobytes())
    return out


def pairwise_distinct(a):
    """the results of the base vectors differ pairwise in bits, apart from the all-NaN ones among themselves"""
    keys = [k for k in key_rows(a) if k is not None]
    return len(keys) >= PERIOD - 3 and len(set(keys)) == len(keys)


@functools.lru_cache(maxsize=None)
def softmax_base(n, seed=0):
    """13 rows for the softmax families: uniform on [-20, 20] scaled by 2^(k - 6), one with a NaN, one constant, one all -Inf"""
    rng = np.random.default_rng(7000 + 31 * n + seed)
    x = (rng.uniform(-20, 20, (PERIOD, n)).astype(F) * scales()[:, None]).astype(F)
    x[NAN_AT, n // 2] = np.nan
    x[EQUAL_AT] = F(2.5)
    x[NINF_AT] = -np.inf
    return frozen(x)


@functools.lru_cache(maxsize=None)
def softmax_model(n):
    from tests import exp_model as E
    return frozen(E.softmax_rows(softmax_base(n)))


@functools.lru_cache(maxsize=None)
def log_softmax_model(n):
    """(labels, logsumexp, log_softmax, loss, grad) of the 13 rows: one label -1 (ignored), one n (NaN), the others valid"""
    from tests import log_model as G
    x = softmax_base(n)
    lab = np.random.default_rng(n).integers(0, n, PERIOD).astype(np.int32)
    lab[1], lab[5] = -1, n
    loss, grad = G.xent_rows(x, lab)
    return frozen(lab, G.logsumexp_rows(x), G.log_softmax_rows(x), loss, grad)


@functools.lru_cache(maxsize=None)
def layer_norm_base(n):
    """(x, dy, gamma, beta): 13 rows each of x and dy at different magnitudes, one x row with a NaN, one constant"""
    rng = np.random.default_rng(8000 + n)
    x = (rng.normal(3, 2, (PERIOD, n)).astype(F) * scales()[:, None]).astype(F)
    dy = (rng.normal(0, 1, (PERIOD, n)).astype(F) * np.roll(scales(), 5)[:, None]).astype(F)
    x[NAN_AT, n // 2] = np.nan
    x[EQUAL_AT] = F(2.5)
    gamma = rng.normal(1, 0.5, n).astype(F)
    beta = rng.normal(0, 1, n).astype(F)
    return frozen(x, dy, gamma, beta)


LN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def layer_norm_model(n):
    """(y, mean, rstd, dx) of the 13 rows, with gamma and beta"""
    from tests import layer_norm_model as M
    x, dy, gamma, beta = layer_norm_base(n)
    y, mean, rstd = M.forward(x, gamma, beta, LN_EPS)
    return frozen(y, mean, rstd, M.dx_of(dy, x, mean, rstd, gamma))


@functools.lru_cache(maxsize=None)
def column_base(rows, seed=0):
    """(dy, other, mean, rstd): 13 columns of `rows` values each for dy (scaled by 2^(k - 6), one with a NaN, one constant) and
    for the second operand (the forward output y in (-1, 1) of the bias gradient as `other`, x of the layer norm as 3 + 2
    other), and one mean and rstd per row"""
    rng = np.random.default_rng(9000 + rows + seed)
    dy = (rng.normal(0, 3, (rows, PERIOD)).astype(F) * scales()[None, :]).astype(F)
    dy[rows // 2, NAN_AT] = np.nan
    dy[:, EQUAL_AT] = F(0.75)
    other = rng.uniform(-0.95, 0.95, (rows, PERIOD)).astype(F)
    mean = rng.normal(3, 0.2, rows).astype(F)
    rstd = rng.uniform(0.3, 0.8, rows).astype(F)
    return frozen(dy, other, mean, rstd)


@functools.lru_cache(maxsize=None)
def bias_grad_model(rows, kind):
    """(dz, db) of the 13 columns"""
    from tests import act_model as A
    from tests import reduce_model as R
    dy, y, _, _ = column_base(rows)
    dz = np.array(dy) if kind is None else A.activation_grad(dy, y, kind)
    db = np.array([R.model_sum(np.ascontiguousarray(dz[:, j])) for j in range(PERIOD)], F).reshape(PERIOD)
    return frozen(dz, db)


def layer_norm_x_columns(rows):
    return frozen((F(3) + F(2) * column_base(rows)[1]).astype(F))


@functools.lru_cache(maxsize=None)
def layer_norm_params_model(rows):
    """(dgamma, dbeta) of the 13 columns"""
    from tests import layer_norm_model as M
    dy, _, mean, rstd = column_base(rows)
    return frozen(*M.param_grads(dy, layer_norm_x_columns(rows), mean, rstd))


@functools.lru_cache(maxsize=None)
def cumsum_base(sfx, n):
    rng = np.random.default_rng(10000 + n)
    if sfx == "i64":
        x = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, (PERIOD, n), dtype=np.int64, endpoint=True)   # the sums wrap
        x[EQUAL_AT] = 3
        return frozen(x)
    x = (rng.uniform(0, 1, (PERIOD, n)).astype(F) * scales()[:, None]).astype(F)
    x[NAN_AT, n // 2] = np.nan
    x[EQUAL_AT] = F(0.5)
    return frozen(x)


@functools.lru_cache(maxsize=None)
def cumsum_model(sfx, n):
    from tests import scan_model as S
    return frozen(S.cumsum(cumsum_base(sfx, n)))


def uniforms(m, seed):
    """(13, m) uniform numbers in [0, 1), the first 0 and the last the largest below 1"""
    u = np.random.default_rng(seed).random((PERIOD, m), dtype=F)
    u[:, 0], u[:, -1] = 0, TOP
    return u


@functools.lru_cache(maxsize=None)
def weights_base(n, seed=0):
    """13 rows of n positive weights at different magnitudes, one with a NaN (its draws are -1), one constant"""
    rng = np.random.default_rng(11000 + n + seed)
    w = (rng.uniform(0.1, 1, (PERIOD, n)).astype(F) * scales()[:, None]).astype(F)
    w[NAN_AT, n // 2] = np.nan
    w[EQUAL_AT] = F(0.5)
    return frozen(w)


@functools.lru_cache(maxsize=None)
def searchsorted_model(n, m):
    """(a, v, left, right): 13 sorted rows with equal neighbours, 13 rows of values (one NaN), the indices on both sides"""
    from tests import scan_model as S
    rng = np.random.default_rng(12000 + n + m)
    a = np.sort(rng.integers(-8, 8, (PERIOD, n)), axis=1).astype(F)
    v = rng.integers(-9, 9, (PERIOD, m)).astype(F)
    v[NAN_AT, m // 2] = np.nan
    return frozen(a, v, S.searchsorted(a, v, right=False), S.searchsorted(a, v, right=True))


@functools.lru_cache(maxsize=None)
def cdf_sample_model(n, m):
    """(cdf, u, idx)"""
    from tests import scan_model as S
    cdf = S.cumsum(weights_base(n))
    u = uniforms(m, 13000 + n + m)
    return frozen(cdf, u, S.draw(cdf, u))


@functools.lru_cache(maxsize=None)
def cdf_remove_model(n, k):
    """(w, u, idx, w afterwards)"""
    from tests import scan_model as S
    w = weights_base(n, seed=1)
    u = uniforms(k, 14000 + n + k)
    after = np.array(w)
    idx = S.draw_remove(after, u)
    return frozen(w, u, idx, after)


@functools.lru_cache(maxsize=None)
def sampler_build_model(n):
    """(w, trees)"""
    from tests import fplus_tree_model as T
    w = weights_base(n, seed=2)
    return frozen(w, T.build(w))


@functools.lru_cache(maxsize=None)
def sampler_sample_model(n, m):
    """(u, idx) on the trees of sampler_build_model(n)"""
    from tests import fplus_tree_model as T
    u = uniforms(m, 15000 + n + m)
    return frozen(u, T.draw(sampler_build_model(n)[1], u))


@functools.lru_cache(maxsize=None)
def sampler_update_model(n, k):
    """(elem, weight, trees after the update, u, idx of k draws without replacement, trees after them)"""
    from tests import fplus_tree_model as T
    rng = np.random.default_rng(16000 + n + k)
    elem = rng.integers(0, n, PERIOD).astype(np.int32)
    elem[2], elem[9] = -1, n                              # nothing to do; outside the row: skipped
    weight = (rng.uniform(0.1, 1, PERIOD).astype(F) * np.roll(scales(), 4)).astype(F)
    updated = T.update(np.array(sampler_build_model(n)[1]), elem, weight, n)
    u = uniforms(k, 17000 + n + k)
    drawn = np.array(updated)
    idx = T.draw_remove(drawn, u)
    return frozen(elem, weight, updated, u, idx, drawn)


# ---- the embedding's data ------------------------------------------------------------------------------------------------------------
INVALID_IDS = (-1, -2, 2 ** 31 - 1)                       # -1: a row of +0; the others, and `vocab`: a row of NaN


@functools.lru_cache(maxsize=None)
def embedding_columns_base(tokens, vocab, kind):
    """(idx, 13 columns of dy, 13 columns of the table): ids with some invalid ones (kind "mixed"), or one id for nearly every
    token -- a long segment -- and a short one ("mostly0")"""
    rng = np.random.default_rng(18000 + tokens + vocab + len(kind))
    idx = rng.integers(0, vocab, tokens).astype(np.int32)
    if kind == "mostly0":
        idx[:] = 0
        idx[5::40] = 1
    else:
        idx[rng.integers(0, tokens, tokens // 20)] = -1
        for k, bad in enumerate((vocab,) + INVALID_IDS[1:]):
            idx[3 + 11 * k::97] = bad
    dy = (rng.normal(0, 1, (tokens, PERIOD)) * 2.0 ** rng.uniform(-8, 8, (tokens, PERIOD))).astype(F) * scales()[None, :]
    dy = dy.astype(F)
    dy[tokens // 2, NAN_AT] = np.nan
    dy[:, EQUAL_AT] = F(0.75)
    w = (rng.normal(0, 1, (vocab, PERIOD)).astype(F) * scales()[None, :]).astype(F)
    w[vocab // 2, NAN_AT] = np.nan
    w[:, EQUAL_AT] = F(0.75)
    return frozen(idx, dy, w)


@functools.lru_cache(maxsize=None)
def embedding_columns_model(tokens, vocab, kind):
    """(y, order, starts, dw) of the 13 columns"""
    from tests import embedding_model as M
    idx, dy, w = embedding_columns_base(tokens, vocab, kind)
    order, starts = M.group(idx, vocab)
    return frozen(M.gather(w, idx), order, starts, M.grad(dy, idx, vocab, order, starts))


@functools.lru_cache(maxsize=None)
def embedding_gather_model(vocab, dim):
    """(ids, table, rows): 13 ids (-1, `vocab` and another invalid one among them, no valid one twice) and the rows they gather"""
    from tests import embedding_model as M
    rng = np.random.default_rng(19000 + vocab + dim)
    ids = rng.permutation(vocab)[:PERIOD].astype(np.int32)
    ids[1], ids[5], ids[8] = -1, vocab, INVALID_IDS[2]
    w = (rng.normal(0, 1, (vocab, dim)).astype(F) * scales()[np.arange(vocab) % PERIOD, None]).astype(F)
    return frozen(ids, w, M.gather(w, ids))


@functools.lru_cache(maxsize=None)
def embedding_short_model(tokens, vocab, cap):
    """(idx, 13 columns of dy, the ids that occur, their rows of dw): about 150 ids, among them the first and the last three
    and both sides of the cap, so that the workgroups 0 .. 2 have work on both of their trips"""
    from tests import embedding_model as M
    rng = np.random.default_rng(20000 + tokens + vocab)
    pool = np.unique(np.concatenate([[0, 1, 2, 3, cap - 1, cap, cap + 1, cap + 2, vocab - 1], rng.integers(0, vocab, 140)]))
    idx = pool[rng.integers(0, pool.size, tokens)].astype(np.int32)
    idx[rng.integers(0, tokens, 50)] = -1
    idx[7::500] = vocab
    dy = ((rng.normal(0, 1, (tokens, PERIOD)) * 2.0 ** rng.uniform(-8, 8, (tokens, PERIOD))).astype(F) * scales()[None, :]).astype(F)
    order, starts = M.group(idx, vocab)
    seen = np.nonzero(np.diff(starts))[0]
    dw = np.zeros((seen.size, PERIOD), F)
    from tests import reduce_model as R
    for i, v in enumerate(seen):
        seg = dy[order[starts[v]:starts[v + 1]]]
        for j in range(PERIOD):
            dw[i, j] = R.model_sum(np.ascontiguousarray(seg[:, j]))
    return frozen(idx, dy, seen, dw)


@functools.lru_cache(maxsize=None)
def embedding_tile_model(tokens, vocab):
    """(idx, 13 values of dy, order, starts, dw): random ids with some invalid ones; dy[t] = the base value t mod 13"""
    from tests import embedding_model as M
    from tests import reduce_model as R
    rng = np.random.default_rng(21000 + vocab)
    idx = rng.integers(0, vocab, tokens, dtype=np.int32)
    idx[11::1000] = -1
    idx[13::7001] = vocab
    dy = (rng.normal(0, 1, PERIOD) * 2.0 ** rng.uniform(-8, 8, PERIOD)).astype(F)
    order, starts = M.group(idx, vocab)
    dw = np.zeros((vocab, 1), F)
    for v in range(vocab):
        dw[v, 0] = R.model_sum(np.ascontiguousarray(dy[order[starts[v]:starts[v + 1]] % PERIOD]))
    return frozen(idx, dy, order, starts, dw)


@functools.lru_cache(maxsize=None)
def embedding_group_model(tokens, vocab):
    """(idx, order, starts): ids over the whole range, so that every digit of the four passes varies"""
    from tests import embedding_model as M
    rng = np.random.default_rng(22000 + tokens)
    idx = rng.integers(0, vocab, tokens).astype(np.int32)
    idx[:6] = [0, vocab - 1, vocab, -1, 1 << 24, (1 << 24) - 1]
    idx[rng.integers(6, tokens, 40)] = idx[6:46]          # some ids twice: stability shows
    order, starts = M.group(idx, vocab)
    return frozen(idx, order, starts)
