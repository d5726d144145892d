"""Random strided views for the data-movement kernels, and a Python restatement of their host launchers' rules.

A `View` is a recipe: a flat buffer, a start offset of 0-3 elements, a row-major base array of rank <= 6 from there on, then
a list of view operations replayed identically on a numpy array (`numpy`) and on a laser_amd.Tensor over a device copy of
the same buffer (`tensor`).  The operations are those of Tensor's own view code: an axis permutation, slices with steps
(negative ones included), integer indices that drop axes, and, for read-only operands, broadcast axes of stride 0.

The case lists are drawn with fixed seeds and steered to the thresholds of the launchers in
laser_amd/csrc/data_movement.hip (launch_copy_strided, launch_transpose_t) and laser_amd/csrc/map_strided.hip
(launch_map_strided): inner extents around the 1024-element chunk, short-row grids that end on a partial workgroup, views
that merge to one dimension, dense matrices read through .T, vector-sized transposes on aligned and misaligned bases.
`copy_branch`, `map_branch` and `transpose_branch` restate which kernel each launcher picks; tests/test_strided_views_cpu.py
checks that the case lists reach every branch, tests/test_gpu_strided_movers.py runs them against numpy.
"""
import math

import numpy as np

MAXRANK = 6
CHUNK = 1024                                   # elements per workgroup of the row kernels (256 lanes x 4)
INNER_EXTENTS = (1, 2, 3, 5, 255, 1023, 1024, 1025, 2049)
TILE_SWITCH = 1 << 24                          # launch_transpose_t: 16x256 tile up to this many elements, 32x256 above


def _prod(xs):
    p = 1
    for x in xs:
        p *= int(x)
    return p


# ---- views --------------------------------------------------------------------------------------------------------
class View:
    """flat[offset : offset + prod(base_shape)].reshape(base_shape), then `ops`:
        ("T", axes)      transpose(axes)
        ("ix", index)    a tuple of slices and integers
        ("bc", axis, n)  a new axis of extent n and stride 0 inserted at `axis` (read-only operands only)
    `base_len` = the flat buffer's length: the base plus 0-3 elements of tail."""

    def __init__(self, base_shape, offset, ops, tail=0):
        self.base_shape = tuple(int(n) for n in base_shape)
        self.offset = int(offset)
        self.ops = list(ops)
        self.base_len = self.offset + _prod(self.base_shape) + int(tail)
        flat = np.zeros(self.base_len, np.uint8)                    # 1-byte elements: byte strides = element strides
        probe = self.numpy(flat)
        self.shape = probe.shape
        self.strides = tuple(int(s) for s in probe.strides)
        self.elem_offset = int(probe.__array_interface__["data"][0] - flat.__array_interface__["data"][0])
        self.broadcast = any(op[0] == "bc" for op in self.ops)

    def numpy(self, flat):
        """the view of the numpy array `flat` (length base_len); writable unless it broadcasts"""
        v = flat[self.offset:self.offset + _prod(self.base_shape)].reshape(self.base_shape)
        for op in self.ops:
            if op[0] == "T":
                v = v.transpose(op[1])
            elif op[0] == "ix":
                v = v[op[1] + (Ellipsis,)]             # (the Ellipsis keeps a 0-d result a view, not a scalar)
            else:
                _, axis, n = op
                v = np.lib.stride_tricks.as_strided(v, v.shape[:axis] + (n,) + v.shape[axis:],
                                                    v.strides[:axis] + (0,) + v.strides[axis:], writeable=False)
        return v

    def tensor(self, Tensor, storage, dtype):
        """the same view as a laser_amd.Tensor over `storage` (a device copy of the flat buffer), built with Tensor's own
        transpose / __getitem__; a broadcast axis is a Tensor with a stride of 0 (Tensor has no expand)"""
        st, run = [], 1
        for n in reversed(self.base_shape):
            st.append(run)
            run *= n
        t = Tensor(self.base_shape, tuple(reversed(st)), self.offset, storage, dtype)
        for op in self.ops:
            if op[0] == "T":
                t = t.transpose(op[1])
            elif op[0] == "ix":
                t = t[op[1]]
            else:
                _, axis, n = op
                t = Tensor(t.shape[:axis] + (n,) + t.shape[axis:], t.strides[:axis] + (0,) + t.strides[axis:], t.offset,
                           t.storage, t.dtype)
        return t

    def __repr__(self):
        return (f"View(shape={self.shape}, strides={self.strides}, offset={self.elem_offset}, base={self.base_shape}"
                f"+{self.offset}, ops={self.ops})")


def layout(rng, shape, *, broadcast=False, steps=None, pads=None, drops=None, permute=True, offset=None, max_base=1 << 21):
    """A random View of logical shape `shape`.  Every axis is a slice (step from `steps` or drawn, negative steps included)
    of a longer base axis; `drops` extra base axes (drawn: 0-2) are removed by integer indices; the base axes are stored in
    a random order (permute) from a start offset of 0-3 elements.  With broadcast, some axes of extent > 1 become stride-0
    axes instead.  Redrawn with unit steps while the base would exceed max_base elements."""
    shape = tuple(int(n) for n in shape)
    r = len(shape)
    for attempt in range(8):
        bc = [broadcast and n > 1 and rng.random() < 0.3 for n in shape]
        nreal = r - sum(bc)
        ndrop = int(rng.integers(0, 3)) if drops is None else drops
        ndrop = max(0, min(ndrop, MAXRANK - nreal))
        axes = []                                      # logical base axes: (extent, index)
        for d, n in enumerate(shape):
            if bc[d]:
                continue
            if steps is not None:
                s = steps[d]
            elif attempt >= 4:
                s = 1
            else:
                s = int(rng.choice([1, 1, 1, 2, -1, -2, 3]))
            pad = int(rng.integers(0, 3)) if pads is None else pads[d]
            B = abs(s) * (n - 1) + 1 + pad
            lo = int(rng.integers(0, pad + 1))
            if s > 0:
                ix = slice(lo, lo + s * (n - 1) + 1, s)
            else:
                start = B - 1 - lo
                stop = start + s * (n - 1) - 1
                ix = slice(start, stop if stop >= 0 else None, s)
            axes.append((B, ix))
        for _ in range(ndrop):
            k = int(rng.integers(2, 4))
            axes.insert(int(rng.integers(0, len(axes) + 1)), (k, int(rng.integers(0, k))))
        if _prod(a[0] for a in axes) <= max_base:
            break
    m = len(axes)
    phys = list(rng.permutation(m)) if permute and m > 1 else list(range(m))   # memory order of the logical base axes
    base_shape = [axes[a][0] for a in phys]
    ops = []
    if phys != list(range(m)):
        ops.append(("T", tuple(phys.index(j) for j in range(m))))
    ops.append(("ix", tuple(a[1] for a in axes)))
    for d in range(r):
        if bc[d]:
            ops.append(("bc", d, shape[d]))
    off = int(rng.integers(0, 4)) if offset is None else offset
    v = View(base_shape, off, ops, tail=int(rng.integers(0, 4)))
    assert v.shape == shape, (v, shape)
    return v


def merged_layout(shape, step, offset=0):
    """A View of `shape` that every launcher merges into ONE dimension of stride `step`: a dense base whose inner axis is
    walked with `step` (and every other axis reversed too when step < 0)."""
    base = tuple(shape[:-1]) + (abs(step) * (shape[-1] - 1) + 1,)
    ix = tuple(slice(None, None, -1 if step < 0 else 1) for _ in shape[:-1]) + (slice(None, None, step),)
    return View(base, offset, [("ix", ix)])


def dense_layout(shape, offset=0, tail=0):
    return View(shape, offset, [("ix", tuple(slice(None) for _ in shape))], tail=tail)


def transposed_layout(R, C, offset=0):
    """a dense R x C matrix read through .T: copy_strided's transpose shortcut when the destination is dense"""
    return View((R, C), offset, [("T", (1, 0))])


def outer_extents(rng, rank, inner, max_elems):
    """rank - 1 outer extents in 1..6 whose product with `inner` stays under max_elems"""
    out = []
    for _ in range(rank - 1):
        cap = max(1, max_elems // (inner * max(1, _prod(out))))
        out.append(int(rng.integers(1, min(6, cap) + 1)))
    return tuple(out)


# ---- the launchers' rules -----------------------------------------------------------------------------------------
def merge_dims(shape, *strides):
    """extent-1 dimensions dropped, neighbours (outer o, inner i) merged when stride_o == stride_i * extent_i on EVERY
    operand: the loop at the top of launch_copy_strided and launch_map_strided"""
    sh, st = [], [[] for _ in strides]
    for d, n in enumerate(shape):
        if n == 1:
            continue
        if sh and all(s[-1] == x[d] * n for s, x in zip(st, strides)):
            sh[-1] *= n
            for s, x in zip(st, strides):
                s[-1] = x[d]
        else:
            sh.append(n)
            for s, x in zip(st, strides):
                s.append(x[d])
    return sh, st


def _row_branch(sh):
    """the row kernels shared by copy_strided and map_strided: short rows packed 1024 >> log2p per workgroup, else
    1024-element chunks of one row per workgroup"""
    r = len(sh)
    rows, inner = _prod(sh[:-1]), sh[-1]
    if inner < CHUNK and r > 1:
        log2p = max(0, math.ceil(math.log2(inner)))
        per = CHUNK >> log2p
        return {"kernel": "rows", "rank": r, "inner": inner, "rows": rows, "rows_per_wg": per,
                "workgroups": -(-rows // per), "partial_wg": rows % per != 0}
    chunks = -(-inner // CHUNK)
    return {"kernel": "long", "rank": r, "inner": inner, "rows": rows, "chunks": chunks, "partial_chunk": inner % CHUNK != 0}


def copy_branch(shape, dstrides, sstrides, dst_byte_addr=0, src_byte_addr=0, itemsize=4):
    """which path laser_hip_copy_strided_*_dev takes: "empty", "memcpy" (both sides C-contiguous, copy_strided_api),
    "transpose" (a dense matrix read through swapped strides; "tr_kernel" says which transpose kernel), "rows" or "long"
    (copy_strided_rows_kernel / copy_strided_kernel)"""
    if _prod(shape) == 0:
        return {"kernel": "empty"}
    run, contiguous = 1, True
    for d in range(len(shape) - 1, -1, -1):
        if shape[d] != 1 and (dstrides[d] != run or sstrides[d] != run):
            contiguous = False
        run *= shape[d]
    if contiguous:
        return {"kernel": "memcpy"}
    sh, (ds, ss) = merge_dims(shape, dstrides, sstrides)
    if not sh:
        sh, ds, ss = [1], [1], [1]
    if len(sh) == 2 and ds[1] == 1 and ds[0] == sh[1] and ss[0] == 1 and ss[1] == sh[0]:
        return {"kernel": "transpose", "rank": 2,
                "tr_kernel": transpose_branch(1, sh[1], sh[0], itemsize, dst_byte_addr, src_byte_addr)}
    return _row_branch(sh)


def map_branch(shape, dstrides, astrides=None, bstrides=None):
    """which traversal launch_map_strided takes ("rows" or "long"); operands not read pass None (stride 0 everywhere)"""
    if _prod(shape) == 0:
        return {"kernel": "empty"}
    z = [0] * len(shape)
    sh, _ = merge_dims(shape, dstrides, astrides or z, bstrides or z)
    return _row_branch(sh or [1])


def transpose_branch(N, NR, NC, itemsize, dst_byte_addr=0, src_byte_addr=0):
    """launch_transpose_t with dense pitches: the 16-byte vector kernel ("vec16x256" up to 2^24 elements, "vec32x256"
    above) when NR, NC and the pitches are multiples of the vector and both bases are 16-byte aligned, else "scalar" """
    V = 16 // itemsize
    vec = NR % V == 0 and NC % V == 0 and (dst_byte_addr | src_byte_addr) % 16 == 0
    if not vec:
        return "scalar"
    return "vec16x256" if N * NR * NC <= TILE_SWITCH else "vec32x256"


def transpose_tiles_partial(N, NR, NC, kernel):
    """(rows, columns): does the last tile of the source rows / columns stick out of the matrix?"""
    TR, TC = {"vec16x256": (16, 256), "vec32x256": (32, 256), "scalar": (64, 64)}[kernel]
    return NR % TR != 0, NC % TC != 0


# ---- the fixed-seed case lists ------------------------------------------------------------------------------------
def copy_cases(seed=20261016, draws=2):
    """[(name, src View, dst View)] of equal shapes: src may broadcast, dst never does"""
    rng = np.random.default_rng(seed)
    cases = []
    for inner in INNER_EXTENTS:                                   # threshold inner extents at random ranks and layouts
        for k in range(draws):
            rank = int(rng.integers(1, MAXRANK + 1))
            shape = outer_extents(rng, rank, inner, 40_000) + (inner,)
            cases.append((f"inner{inner}-r{rank}-{k}", layout(rng, shape, broadcast=True), layout(rng, shape)))
    for inner, rows in ((2, 700), (3, 300), (5, 200), (255, 7), (100, 3)):   # short-row grids ending on a partial workgroup
        a = rows // 3 + 1
        shape = (a, 3, inner)
        # an unpadded inner step of 2: the inner axis merges with no outer one
        cases.append((f"partial-wg-inner{inner}", layout(rng, shape, steps=(1, 1, 2), pads=(0, 0, 0), drops=0, permute=False),
                      layout(rng, shape, steps=(1, -1, 1), drops=0, permute=False)))
    for shape, step in (((4, 5, 7), 2), ((3, 700), -1), ((2, 2, 1025), 3), ((6, 50), 2)):   # everything merges: r == 1
        cases.append((f"merged-{'x'.join(map(str, shape))}-step{step}", merged_layout(shape, step, offset=1),
                      dense_layout(shape, offset=2, tail=3)))
    for R, C, off in ((64, 256, 0), (37, 1029, 1), (256, 260, 0), (8, 12, 2), (3, 2049, 0)):   # dense matrix through .T
        cases.append((f"dotT-{R}x{C}-off{off}", transposed_layout(R, C, off), dense_layout((C, R), offset=0, tail=2)))
    return cases


def map_cases(seed=20261017):
    """[(name, dst View, a View, b View)]: a and b may broadcast; `a is dst` in the in-place cases"""
    rng = np.random.default_rng(seed)
    cases = []
    for inner in INNER_EXTENTS:
        for k in range(2):
            rank = int(rng.integers(1, MAXRANK + 1))
            shape = outer_extents(rng, rank, inner, 20_000) + (inner,)
            d = layout(rng, shape)
            a = d if k == 1 else layout(rng, shape, broadcast=True)
            cases.append((f"inner{inner}-r{rank}" + ("-inplace" if k == 1 else ""), d, a, layout(rng, shape, broadcast=True)))
    for inner, rows in ((3, 300), (5, 200), (255, 7)):
        shape = (rows, inner)
        d = layout(rng, shape, steps=(1, 2), pads=(0, 0), drops=0, permute=False)
        cases.append((f"partial-wg-inner{inner}", d, layout(rng, shape, steps=(-1, 1), drops=0, permute=False),
                      layout(rng, shape, broadcast=True)))
    for shape, step in (((4, 5, 7), 2), ((2, 2, 1025), -1)):
        d = merged_layout(shape, step, offset=3)
        name = f"merged-{'x'.join(map(str, shape))}-step{step}"
        cases.append((name, d, merged_layout(shape, step, offset=1), merged_layout(shape, step)))
        cases.append((name + "-inplace", d, d, merged_layout(shape, step)))
    return cases


def transpose_cases(itemsize):
    """[(fn, N, NR, NC, src_off, dst_off)] for one element size: fn is "batched", "copy", "nchw2nhwc" (NR = C, NC = H*W)
    or "nhwc2nchw" (NR = H*W, NC = C); offsets in elements from a 16-byte aligned buffer"""
    V = 16 // itemsize
    mis = [k for k in (1, 2, 3) if (k * itemsize) % 16]            # element offsets that leave 16-byte alignment
    cases = [("batched", 3, 32, 512, 0, 0),                         # vector kernel, N > 1, whole tiles
             ("batched", 2, 32 + V, 256 + V, 0, 0),                 # vector kernel, N > 1, partial tiles
             ("batched", 2, 9 * V, 3 * V, 0, 0)]
    cases += [("batched", 2, 32 + V, 256 + V, k, 0) for k in mis]   # vector-sized, misaligned source: scalar kernel
    cases += [("batched", 3, 9 * V, 3 * V, 0, mis[0]),              # misaligned destination
              ("batched", 2, 45, 70, 0, 0),                         # scalar kernel, partial 64x64 tiles on both axes
              ("batched", 2, 1, 300, 0, 0), ("batched", 3, 129, 1, 0, 0), ("batched", 1, 1, 1, 0, 0),
              ("batched", 2, V, V, 0, 0), ("batched", 2, V, 1, 0, 0),
              ("copy", 1, 9 * V, 33 * V, 0, 0), ("copy", 1, 100, 37, 0, 0), ("copy", 1, 16 * V, V, mis[-1], 0),
              ("nchw2nhwc", 2, 2 * V, 4 * V, 0, 0), ("nchw2nhwc", 2, 3, 35, 0, 0),
              ("nhwc2nchw", 2, 4 * V, 2 * V, 0, 0), ("nhwc2nchw", 3, 35, 3, 0, 0)]
    return cases


def split_hw(hw):
    """(H, W) with H * W = hw for the nchw2nhwc / nhwc2nchw cases"""
    W = 7 if hw % 7 == 0 else (hw // 4 if hw % 4 == 0 else hw)
    return hw // W, W


# 4-byte elements above 2^24 elements: the 32x256 tile, batched and single (4104 rows: a partial 32-row tile)
BIG_TRANSPOSES = ((4, 2304, 2048), (1, 4104, 4096))
