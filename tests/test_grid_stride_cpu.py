"""The table of tests/grid_stride_cases.py holds, without a device: every shape exceeds its cap in the plan the library
reports (the plan entry points need no device), the two column walks have the steps the table states, the embedding cases
have the tile and the passes they were chosen for, the constants the shapes were computed from are the plans', and the data
can tell a wrong vector from a right one: the models' results for the 13 base vectors differ pairwise in bits."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import grid_stride_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
IDS = [c.id for c in G.CASES]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    from laser_amd import _lib
    return _lib.lib()


def plan(L, name, *args, size=4):
    out = (C.c_int64 * size)()
    assert getattr(L, name)(*args, out) == 0, (name, args)
    return list(out)


def test_the_constants_are_the_plans(L):
    """what the shapes were computed from, read from the headers, against what the plans do at those values"""
    for name, what in (("laser_hip_softmax_rows_plan", None), ("laser_hip_layer_norm_plan", G.FWD), ("laser_hip_layer_norm_plan", G.DX)):
        tail = () if what is None else (what,)
        size = 3 if what is None else 4
        code = lambda n: plan(L, name, 1, n, 1, *tail, size=size)[0]
        assert [code(G.WAVE_N), code(G.WAVE_N + 1), code(G.CHUNK_N), code(G.CHUNK_N + 1)] == [0, 1, 1, 2]
        groups = lambda n: plan(L, name, 1 << 40, n, 1, *tail, size=size)[1]
        assert groups(5) == groups(G.CHUNK_N + 1) == G.ROW_CAP
    assert G.ROW_CAP == G.LN_CAP
    # the strip kernels: CW and the resident bound as test_gpu_softmax_axis.py finds them
    axis = lambda n: plan(L, "laser_hip_softmax_axis_plan", 1, n, 2, 1, 256)
    assert axis(1)[1] == G.AXIS_CW and axis(G.AXIS_BOUND)[0] == 8 and axis(G.AXIS_BOUND + 1)[0] == 9
    assert plan(L, "laser_hip_softmax_axis_plan", 1 << 20, 5, 1 << 20, 1, 256)[2] == G.AXIS_CAP
    # the column kernels: the strip width is where the workgroup count of one chunk steps
    for name, tail, cw, cap, chunk in (("laser_hip_bias_grad_plan", (1, 256), G.BG_CW, G.BG_CAP, G.BG_CHUNK),
                                       ("laser_hip_layer_norm_plan", (1, G.PARAMS), G.LN_CW, G.LN_CAP, G.LN_CHUNK)):
        groups = lambda rows, n: plan(L, name, rows, n, *tail)[1]
        assert [groups(5, cw), groups(5, cw + 1), groups(5, 2 * cw), groups(5, 2 * cw + 1)] == [1, 2, 2, 3]
        assert [groups(chunk, cw), groups(chunk + 1, cw)] == [1, 2] and groups(5, 1 << 26) == cap
    # the scan: the run, the switch between the variants, the cap on 256 compute units (what cus = 0 means)
    scan = lambda rows, n, cus=G.SCAN_CUS: plan(L, "laser_hip_cumsum_plan", rows, n, 4, cus)
    assert scan(1, G.SCAN_WAVE_N)[0] == 0 and scan(1, G.SCAN_WAVE_N + 1)[0] == 1
    assert scan(1 << 30, 5)[2] == scan(1 << 30, 5, 0)[2] == scan(1 << 30, G.SCAN_WAVE_N + 1)[2] == G.SCAN_CAP
    from tests import scan_model
    assert scan_model.run() == G.SCAN_RUN
    # the sampler: the longest row of the LDS kernel, the segment, the cap of both launches
    samp = lambda rows, n: plan(L, "laser_hip_sampler_plan", rows, n)
    assert samp(1, G.SAMPLER_SMALL_P)[:2] == [0, G.SAMPLER_SMALL_LEAVES] and samp(1, G.SAMPLER_SMALL_P + 1)[:2] == [1, G.SAMPLER_SEG]
    assert samp(1 << 30, 3)[2] == G.SAMPLER_CAP and samp(1 << 30, G.SAMPLER_SEG + 1)[2:] == [G.SAMPLER_CAP, G.SAMPLER_CAP]
    # the embedding: the tile doubles one tile of 512 past 2^14 tiles
    emb = lambda tokens, vocab: plan(L, "laser_hip_embedding_plan", tokens, vocab, 1, 1, 256, size=8)
    full = G.EMB_MIN_TILE * G.EMB_MAX_TILES
    assert emb(full, 5)[1] == G.EMB_MIN_TILE and emb(full + 1, 5)[1] == 2 * G.EMB_MIN_TILE
    assert [emb(5, v)[0] for v in (255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)] == [1, 2, 2, 3, 3, 4]


@pytest.mark.parametrize("cid", IDS)
def test_every_case_exceeds_its_cap(L, cid):
    c = G.BY_ID[cid]
    assert c.period == G.PERIOD == 13 and c.units and all(u > c.cap for u in c.units), (c.units, c.cap)
    if c.family == "embedding_tile":
        p = G.plan_of(L, c)
        assert p[1] == c.shape["tile"] == 1024 and p[2] == c.units[0] == c.cap + 1 and p[0] == 2
        return
    if c.family == "embedding_group":
        assert G.plan_of(L, c)[0] == c.shape["passes"] == 4
        return
    if c.plan is None:
        return
    groups = G.planned_workgroups(L, c)
    assert groups == [c.cap] * len(groups), (groups, c.cap)
    assert len(groups) == len(c.units) or c.family == "sampler_lanes"
    if "code" in c.shape:
        assert G.plan_of(L, c)[0] == c.shape["code"]
    if c.family == "cumsum":
        assert G.plan_of(L, c)[0] == c.shape["variant"]
        name, args, _ = c.plan
        assert plan(L, name, *args[:3], 0)[2] == c.cap                     # what the launcher asks: cus = 0


@pytest.mark.parametrize("cid", [c.id for c in G.CASES if c.family in ("bias_grad", "layer_norm_params")])
def test_the_unit_walks_are_the_ones_stated(L, cid):
    """step_chunks and step_strips recomputed from the plan's grid as the launchers do, and the walk itself: every unit is
    visited once, (a) ends on a wrap past the last chunk, (b) wraps inside the matrix"""
    c = G.BY_ID[cid]
    s = c.shape
    grid = G.planned_workgroups(L, c)[0]
    cw, chunk = (G.BG_CW, G.BG_CHUNK) if c.family == "bias_grad" else (G.LN_CW, G.LN_CHUNK)
    strips, chunks = G.cdiv(s["n"], cw), G.cdiv(s["rows"], chunk)
    assert (strips, chunks) == (s["strips"], s["chunks"]) and s["n"] % cw == 3
    assert (grid // strips, grid % strips) == (s["step_chunks"], s["step_strips"])
    if cid.endswith("-a"):
        assert (chunks, strips, s["step_chunks"], s["step_strips"]) == (1, grid + 2, 0, grid)
    else:
        assert (chunks, strips, s["step_chunks"], s["step_strips"]) == (3 if cid.endswith("-c") else 2, grid // 2 + 2, 1, grid // 2 - 2)
    seen, second, stopped, landed = [], 0, 0, 0
    for b in range(grid):                                                    # the kernels' walk, as written there
        ch, strip = (b // strips, b % strips) if b >= strips else (0, b)
        trip = 0
        while ch < chunks:
            if strip >= strips:
                strip -= strips
                ch += 1
                if ch >= chunks:
                    stopped += 1
                    break
                landed += 1
            seen.append(ch * strips + strip)
            second += trip == 1
            trip += 1
            ch += s["step_chunks"]
            strip += s["step_strips"]
    assert sorted(seen) == list(range(chunks * strips))
    if cid.endswith("-a"):          # workgroups 0 and 1 take a second unit; every other one wraps past the only chunk and stops
        assert (second, stopped, landed) == (2, grid, 0)
    elif cid.endswith("-b"):        # workgroups 0 .. 3 take a second unit in chunk 1; the others of chunk 0 wrap out of the matrix
        assert (second, stopped, landed) == (4, strips - 4, 0)
    else:                           # the wrap lands: a workgroup's second unit is in the chunk after the next
        assert second == chunks * strips - grid and landed == strips - 4 and stopped > 0


# ---- the data can tell a wrong vector from a right one -----------------------------------------------------------------------------
def results_of(c):
    """the model's results for the case's 13 base vectors, each with the base vector on its first axis"""
    s = c.shape
    if c.family == "softmax_rows":
        return [G.softmax_model(s["n"])]
    if c.family == "log_softmax_rows":
        return list(G.log_softmax_model(s["n"])[1:])
    if c.family == "softmax_axis":
        return [G.softmax_model(s["n"])]
    if c.family == "layer_norm_forward":
        return list(G.layer_norm_model(s["n"])[:3])
    if c.family == "layer_norm_dx":
        return [G.layer_norm_model(s["n"])[3]]
    if c.family == "bias_grad":
        dz, db = G.bias_grad_model(s["rows"], "tanh" if c.id.endswith("-a") else None)
        return [dz.T, db]
    if c.family == "layer_norm_params":
        return list(G.layer_norm_params_model(s["rows"]))
    if c.family == "cumsum":
        return [G.cumsum_model(s["sfx"], s["n"])]
    if c.id == "searchsorted":
        return list(G.searchsorted_model(s["n"], s["m"])[2:])
    if c.id == "cdf-sample":
        return [G.cdf_sample_model(s["n"], s["m"])[2]]
    if c.id == "cdf-sample-remove":
        return [G.cdf_remove_model(s["n"], s["k"])[3]]
    if c.family == "sampler_build":
        return [G.sampler_build_model(s["n"])[1]]
    if c.id == "sampler-sample":
        return [G.sampler_sample_model(s["n"], s["m"])[1]]
    if c.id == "sampler-update-remove":
        m = G.sampler_update_model(s["n"], s["k"])
        return [m[2], m[5]]
    if c.family == "embedding_columns":
        y, _, _, dw = G.embedding_columns_model(s["tokens"], s["vocab"], s["kind"])
        return [y.T, dw.T]
    if c.family == "embedding_gather":
        return [G.embedding_gather_model(s["vocab"], s["dim"])[2]]
    if c.family == "embedding_short":
        return [G.embedding_short_model(s["tokens"], s["vocab"], c.cap)[3].T]
    raise AssertionError(c.family)


@pytest.mark.parametrize("cid", [c.id for c in G.CASES if c.family not in ("embedding_tile", "embedding_group")])
def test_the_models_results_for_the_base_vectors_differ_pairwise(cid):
    c = G.BY_ID[cid]
    for k, r in enumerate(results_of(c)):
        assert r.shape[0] == G.PERIOD and G.pairwise_distinct(r), (cid, k)


def test_the_base_vectors_have_the_special_ones():
    x = G.softmax_base(5)
    assert np.isnan(x[G.NAN_AT]).sum() == 1 and (x[G.EQUAL_AT] == x[G.EQUAL_AT][0]).all() and (x[G.NINF_AT] == -np.inf).all()
    mags = np.abs(np.delete(G.softmax_base(1025), [G.NAN_AT, G.EQUAL_AT, G.NINF_AT], axis=0)).max(axis=1)
    assert (np.diff(mags) > 0).all() and mags[-1] > 1000 * mags[0]            # the magnitudes 2^(k - 6)
    y = G.softmax_model(5)
    assert np.isnan(y[G.NAN_AT]).all() and np.isnan(y[G.NINF_AT]).all() and np.isnan(y).sum() == 10
    lx = G.layer_norm_base(5)[0]
    assert np.isnan(lx[G.NAN_AT]).sum() == 1 and (lx[G.EQUAL_AT] == lx[G.EQUAL_AT][0]).all()
    dy = G.column_base(5)[0]
    assert np.isnan(dy[:, G.NAN_AT]).sum() == 1 and (dy[:, G.EQUAL_AT] == dy[0, G.EQUAL_AT]).all()


def test_the_short_sums_have_work_on_both_trips_of_the_first_workgroups():
    """ids v and v + cap belong to the same workgroup of the short-segment kernel: both occur, with different sums"""
    c = G.BY_ID["embedding-short-cap"]
    idx, dy, seen, dw = G.embedding_short_model(c.shape["tokens"], c.shape["vocab"], c.cap)
    where = {int(v): i for i, v in enumerate(seen)}
    for v in (0, 1, 2):
        assert v in where and v + c.cap in where
        assert not np.array_equal(dw[where[v]].view(np.uint32), dw[where[v + c.cap]].view(np.uint32))
    counts = np.bincount(idx[(idx >= 0) & (idx < c.shape["vocab"])])
    assert 0 < counts[counts > 0].min() and (counts[counts > 0] <= G.EMB_SHORT).sum() > 100


def test_the_tile_and_group_cases_sort_what_they_claim():
    """the tile case: every id has more than a chunk of occurrences (the two-level fold of the long sums) and their sums differ
    pairwise; the group case: every one of the four digits varies, and some ids occur twice"""
    c = G.BY_ID["embedding-tile"]
    idx, dy, order, starts, dw = G.embedding_tile_model(c.shape["tokens"], c.shape["vocab"])
    assert np.diff(starts).min() > 8192 and starts[-1] < c.shape["tokens"]
    assert len(set(dw.view(np.uint32)[:, 0].tolist())) == c.shape["vocab"]
    g = G.BY_ID["embedding-group-4-passes"]
    idx, order, starts = G.embedding_group_model(g.shape["tokens"], g.shape["vocab"])
    ok = idx[(idx >= 0) & (idx < g.shape["vocab"])]
    for shift in (0, 8, 16, 24):
        assert len(set(((ok >> shift) & 255).tolist())) > 1, shift
    assert np.bincount(np.unique(ok, return_counts=True)[1])[2] > 10
