"""CPU checks of tests/strided_views.py: its views are the same under numpy and under laser_amd.Tensor's own view code, the
Python restatement of the launchers picks the kernels it should on hand-made layouts, and the fixed-seed case lists of
tests/test_gpu_strided_movers.py reach every branch of launch_copy_strided, launch_map_strided and launch_transpose_t --
so that a change to the lists cannot quietly drop one."""
import numpy as np

from laser_amd.tensor import Tensor
from tests import strided_views as SV

COPY_BRANCHES = {"memcpy", "transpose:vec16x256", "transpose:scalar", "rows", "rows:partial-wg", "long:1-chunk",
                 "long:multi-chunk", "long:partial-chunk", "long:r1", "src-broadcast"}
MAP_BRANCHES = {"rows", "rows:partial-wg", "long:1-chunk", "long:multi-chunk", "long:partial-chunk", "long:r1",
                "broadcast", "in-place"}
TRANSPOSE_BRANCHES = {"vec16x256:N>1", "vec16x256:N=1", "vec32x256:N>1", "vec32x256:N=1", "vec:partial-rows",
                      "vec:partial-cols", "scalar:misaligned-vec-extents", "scalar:partial-both", "NR=1", "NC=1",
                      "fn:batched", "fn:copy", "fn:nchw2nhwc", "fn:nhwc2nchw"}


def _labels(b):
    k = b["kernel"]
    if k == "transpose":
        return {"transpose:" + b["tr_kernel"]}
    if k == "rows":
        return {"rows"} | ({"rows:partial-wg"} if b["partial_wg"] and b["workgroups"] > 1 else set())
    if k == "long":
        s = {"long:1-chunk" if b["chunks"] == 1 else "long:multi-chunk"}
        if b["chunks"] > 1 and b["partial_chunk"]:
            s.add("long:partial-chunk")
        if b["rank"] == 1:
            s.add("long:r1")
        return s
    return {k}


def _row_major(shape):
    st, run = [], 1
    for n in reversed(shape):
        st.append(run)
        run *= n
    return tuple(reversed(st))


def copy_labels(src, dst, itemsize):
    """branches of deepCopy(src) (a fresh row-major destination) and copyFrom(dst, src); bases 16-byte aligned"""
    fresh = SV.copy_branch(src.shape, _row_major(src.shape), src.strides, 0, src.elem_offset * itemsize, itemsize)
    into = SV.copy_branch(src.shape, dst.strides, src.strides, dst.elem_offset * itemsize, src.elem_offset * itemsize, itemsize)
    return _labels(fresh) | _labels(into) | ({"src-broadcast"} if src.broadcast else set())


def test_views_match_numpy_and_tensor_view_code():
    """shape, element strides and offset of every case view agree between numpy and Tensor's transpose / __getitem__"""
    views = [v for c in SV.copy_cases() for v in c[1:]] + [v for c in SV.map_cases() for v in c[1:]]
    assert len(views) > 60
    for v in views:
        flat = np.arange(v.base_len, dtype=np.int64)
        nv = v.numpy(flat)
        t = v.tensor(Tensor, None, np.int64)           # no storage needed: views are metadata only
        assert (t.shape, t.strides, t.offset) == (v.shape, v.strides, v.elem_offset), v
        assert t.rank <= SV.MAXRANK and v.base_len >= 1
        # every element the view exposes lies inside the buffer: flat[offset + sum(i * stride)] is nv[i]
        if nv.size:
            idx = np.indices(nv.shape).reshape(len(nv.shape), -1).T
            pos = v.elem_offset + idx @ np.array(v.strides, dtype=np.int64)
            assert pos.min() >= 0 and pos.max() < v.base_len, v
            assert np.array_equal(flat[pos], nv.reshape(-1)), v


def test_restated_rules_on_hand_made_layouts():
    assert SV.merge_dims((2, 1, 3, 4), (12, 99, 4, 1), (1, 7, 2, 6)) == ([2, 3, 4], [[12, 4, 1], [1, 2, 6]])
    assert SV.merge_dims((2, 3, 4), (24, 8, 2), (-12, -4, -1)) == ([24], [[2], [-1]])
    assert SV.copy_branch((5, 7), (7, 1), (7, 1))["kernel"] == "memcpy"
    assert SV.copy_branch((7, 5), (5, 1), (1, 7))["kernel"] == "transpose"       # a dense 5 x 7 read through .T
    assert SV.copy_branch((7, 5), (5, 1), (1, 8))["kernel"] == "rows"            # a pitched one is not the shortcut
    assert SV.copy_branch((300, 3), (3, 1), (6, 2))["kernel"] == "long"          # contiguous on both: one row of 900
    b = SV.copy_branch((300, 3), (3, 1), (7, 2))
    assert (b["kernel"], b["rows_per_wg"], b["workgroups"], b["partial_wg"]) == ("rows", 256, 2, True)
    b = SV.map_branch((2, 2049), (4100, 2), (2049, 1), (0, 1))
    assert (b["kernel"], b["chunks"], b["rows"]) == ("long", 3, 2)
    assert SV.map_branch((4, 500), (500, 1), (500, 1))["kernel"] == "long"      # merges to one 2000-element row
    assert SV.transpose_branch(3, 8, 12, 4) == "vec16x256"
    assert SV.transpose_branch(3, 8, 12, 4, src_byte_addr=4) == "scalar"
    assert SV.transpose_branch(3, 8, 12, 8, dst_byte_addr=16) == "vec16x256"
    assert SV.transpose_branch(1, 4104, 4096, 4) == "vec32x256"
    assert SV.transpose_branch(1, 10, 16, 1) == "scalar"


def test_case_lists_are_steered_to_the_thresholds():
    for cases in (SV.copy_cases(), SV.map_cases()):
        assert set(SV.INNER_EXTENTS) <= {c[1].shape[-1] for c in cases}
        assert {len(c[1].shape) for c in cases} >= {1, 2, 3, 4, 5, 6}
        strides = {s for c in cases for v in c[1:] for s in v.strides}
        assert any(s < 0 for s in strides) and 0 in strides
        assert {v.elem_offset % 4 for c in cases for v in c[1:]} == {0, 1, 2, 3}
        assert any(op[0] == "ix" and any(isinstance(i, int) for i in op[1]) for c in cases for v in c[1:] for op in v.ops)
        assert any(op[0] == "T" for c in cases for v in c[1:] for op in v.ops)


def test_copy_cases_reach_every_copy_strided_branch():
    for itemsize in (4, 8):
        got = set()
        for name, src, dst in SV.copy_cases():
            assert src.shape == dst.shape and not dst.broadcast, name
            got |= copy_labels(src, dst, itemsize)
        assert COPY_BRANCHES <= got, f"itemsize {itemsize}: not reached: {sorted(COPY_BRANCHES - got)}"


def test_map_cases_reach_every_map_strided_branch():
    got = set()
    for name, d, a, b in SV.map_cases():
        assert d.shape == a.shape == b.shape and not d.broadcast, name
        for nin in (0, 1, 2):                       # fill, unary, binary ops
            got |= _labels(SV.map_branch(d.shape, d.strides, a.strides if nin else None, b.strides if nin == 2 else None))
        got |= {"broadcast"} if a.broadcast or b.broadcast else set()
        got |= {"in-place"} if a is d else set()
    assert MAP_BRANCHES <= got, f"not reached: {sorted(MAP_BRANCHES - got)}"


def test_transpose_cases_reach_every_transpose_branch():
    got = set()
    entries = [(it, c) for it in (1, 2, 4, 8) for c in SV.transpose_cases(it)]
    entries += [(4, ("batched", N, NR, NC, 0, 0)) for N, NR, NC in SV.BIG_TRANSPOSES]
    for itemsize, (fn, N, NR, NC, so, do) in entries:
        V = 16 // itemsize
        k = SV.transpose_branch(N, NR, NC, itemsize, do * itemsize, so * itemsize)
        pr, pc = SV.transpose_tiles_partial(N, NR, NC, k)
        got.add(f"fn:{fn}")
        if k != "scalar":
            got.add(f"{k}:{'N>1' if N > 1 else 'N=1'}")
            got |= ({"vec:partial-rows"} if pr else set()) | ({"vec:partial-cols"} if pc else set())
        elif NR % V == 0 and NC % V == 0:
            got.add("scalar:misaligned-vec-extents")
        elif pr and pc and max(NR, NC) > 64:
            got.add("scalar:partial-both")
        got |= ({"NR=1"} if NR == 1 else set()) | ({"NC=1"} if NC == 1 else set())
        if fn in ("nchw2nhwc", "nhwc2nchw"):
            H, W = SV.split_hw(NC if fn == "nchw2nhwc" else NR)
            assert H * W == (NC if fn == "nchw2nhwc" else NR)
    assert TRANSPOSE_BRANCHES <= got, f"not reached: {sorted(TRANSPOSE_BRANCHES - got)}"
