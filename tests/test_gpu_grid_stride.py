"""Every capped launch of the library run past its cap on an MI355X, bit for bit (any NaN equals any NaN) against the numpy
models: the cases, their data and the reasons are in tests/grid_stride_cases.py.  An operand is 13 base vectors tiled on
the device with an index gather, so the models run on 13 vectors and the large operands never exist on the host; every
output is filled with a sentinel first, so a unit no trip reached shows; results are compared on the device against the
tiled model result and only the count and the place of the first difference come back.  Every case asserts that its shape
took the path it was chosen for: the kernel the library recorded (or the plan's, where none is recorded) and a plan whose
workgroups equal the cap."""
import ctypes as C

import numpy as np
import pytest
import torch

import laser_amd
from laser_amd import _lib
from laser_amd.tensor import _stream
from tests import grid_stride_cases as G

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
P = G.PERIOD
ITYPE = {torch.float32: torch.int32, torch.int64: torch.int64, torch.int32: torch.int32}


def L():
    return _lib.lib()


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the shared base arrays are read-only


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    rc = getattr(L(), name)(*args, _stream())
    assert rc == 0, (name, L().laser_hip_last_error())


def opt(name):
    return laser_amd.primitives.get_option(name)


def tiled(count):
    """which base vector operand vector i is: i mod 13"""
    return torch.arange(count, device="cuda") % P


def up4(v):
    return (v + 3) // 4 * 4


def ids(family):
    return [c.id for c in G.of(family)]


def past_the_cap(c):
    """the plan's workgroups equal the cap, for every capped launch the plan reports"""
    groups = G.planned_workgroups(L(), c)
    assert groups == [c.cap] * len(groups) and all(u > c.cap for u in c.units), (c.id, groups, c.units)


def assert_bits(got, want, what):
    """device tensors, compared as integers; only the count and the first difference come to the host"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = got.contiguous(), want.contiguous()
    same = g.view(ITYPE[g.dtype]) == w.view(ITYPE[w.dtype])
    if g.dtype.is_floating_point:
        same |= torch.isnan(g) & torch.isnan(w)
    count = int((~same).sum())
    if count:
        first = int(torch.nonzero(~same.reshape(-1))[0])
        where = tuple(int(i) for i in np.unravel_index(first, tuple(g.shape)))
        raise AssertionError(f"{what}: {count} elements differ, first at {where}: {g.reshape(-1)[first].item()!r} vs "
                             f"{w.reshape(-1)[first].item()!r}")


def rows_buffer(rows, n, stride, off, fill=None, dtype=torch.float32):
    """a buffer full of the sentinel and its (rows, n) view with the given row stride, `off` elements in, holding `fill`"""
    buf = torch.full((off + rows * stride + 8,), SENTINEL if dtype.is_floating_point else int(SENTINEL), dtype=dtype, device="cuda")
    view = torch.as_strided(buf, (rows, n), (stride, 1), off)
    if fill is not None:
        view.copy_(fill)
    return buf, view


def gaps_hold(buf, off, rows, n, stride):
    """the sentinel before the first row, between the rows and after the last survived"""
    body = buf[off:off + rows * stride].view(rows, stride)
    return bool((buf[:off] == SENTINEL).all() & (body[:, n:] == SENTINEL).all() & (buf[off + rows * stride:] == SENTINEL).all())


def row_layouts(n, elems=4):
    """(name, row stride, base offset in elements, vector instance): rows padded to 16-byte boundaries (a gap after every row),
    and contiguous rows with the base one element off its alignment"""
    pad = (n + elems - 1) // elems * elems
    return [("padded rows on 16-byte boundaries", pad if pad > n else n + elems, 0, 1), ("base one element off", n, 1, 0)]


# ---- softmax rows and the log-softmax family -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids("softmax_rows"))
def test_softmax_rows(cid):
    c = G.BY_ID[cid]
    rows, n, code = c.shape["rows"], c.shape["n"], c.shape["code"]
    past_the_cap(c)
    idx = tiled(rows)
    x, want = dev(G.softmax_base(n))[idx], dev(G.softmax_model(n))[idx]
    for name, stride, off, vec in row_layouts(n):
        sbuf, src = rows_buffer(rows, n, stride, off, x)
        dbuf, dst = rows_buffer(rows, n, stride, off)
        laser_amd.softmax(src, out=dst)
        assert opt("last_softmax_kernel") == code + 4 * (1 - vec), name
        assert_bits(dst, want, f"{cid}, {name}")
        assert gaps_hold(dbuf, off, rows, n, stride), name
        assert_bits(src, x, f"{cid}, {name}: the source")
        laser_amd.softmax(src, out=src)
        assert_bits(src, want, f"{cid}, {name}, in place")
        assert gaps_hold(sbuf, off, rows, n, stride), name


@pytest.mark.parametrize("cid", ids("log_softmax_rows"))
def test_log_softmax_family_long_rows(cid):
    """the long-row kernel of logsumexp, log-softmax and the cross-entropy; their other two kernels run past the cap in
    test_gpu_log_softmax.py::test_more_rows_than_the_grid_has_workgroups.  These launches record no kernel: the plan's code is
    asserted"""
    c = G.BY_ID[cid]
    rows, n, code = c.shape["rows"], c.shape["n"], c.shape["code"]
    past_the_cap(c)
    assert G.plan_of(L(), c)[0] == code == 2
    idx = tiled(rows)
    lab13, lse13, lsm13, loss13, grad13 = G.log_softmax_model(n)
    x, labels = dev(G.softmax_base(n))[idx], dev(lab13)[idx].contiguous()
    want_lse, want_lsm, want_loss, want_grad = (dev(a)[idx] for a in (lse13, lsm13, loss13, grad13))
    for name, stride, off, vec in row_layouts(n):
        sbuf, src = rows_buffer(rows, n, stride, off, x)
        lse = torch.full((rows,), SENTINEL, device="cuda")
        laser_amd.logsumexp(src, out=lse)
        assert_bits(lse, want_lse, f"logsumexp, {name}")
        dbuf, dst = rows_buffer(rows, n, stride, off)
        laser_amd.log_softmax(src, out=dst)
        assert_bits(dst, want_lsm, f"log_softmax, {name}")
        assert gaps_hold(dbuf, off, rows, n, stride), name
        loss = torch.full((rows,), SENTINEL, device="cuda")
        gbuf, grad = rows_buffer(rows, n, stride, off)
        call("laser_hip_softmax_xent_rows_f32_dev", ptr(loss), 1, ptr(grad), stride, ptr(src), stride, ptr(labels), rows, n, 1.0)
        assert_bits(loss, want_loss, f"loss, {name}")
        assert_bits(grad, want_grad, f"grad, {name}")
        assert gaps_hold(gbuf, off, rows, n, stride), name
        assert_bits(src, x, f"{name}: the source")
        laser_amd.log_softmax(src, out=src)
        assert_bits(src, want_lsm, f"log_softmax, {name}, in place")
        assert gaps_hold(sbuf, off, rows, n, stride), name


# ---- layer normalization: the row kernels ------------------------------------------------------------------------------------------
def ln_last(what):
    return L().laser_hip_layer_norm_last_kernel(what)


@pytest.mark.parametrize("cid", ids("layer_norm_forward"))
def test_layer_norm_forward(cid):
    c = G.BY_ID[cid]
    rows, n, code = c.shape["rows"], c.shape["n"], c.shape["code"]
    past_the_cap(c)
    idx = tiled(rows)
    x13, _, gamma, beta = G.layer_norm_base(n)
    y13, mean13, rstd13, _ = G.layer_norm_model(n)
    x, gamma, beta = dev(x13)[idx], dev(gamma), dev(beta)
    want_y, want_mean, want_rstd = dev(y13)[idx], dev(mean13)[idx], dev(rstd13)[idx]
    for name, stride, off, vec in row_layouts(n):
        sbuf, src = rows_buffer(rows, n, stride, off, x)
        for in_place in (False, True):
            dbuf, dst = (sbuf, src) if in_place else rows_buffer(rows, n, stride, off)
            mean, rstd = (torch.full((rows,), SENTINEL, device="cuda") for _ in range(2))
            call("laser_hip_layer_norm_f32_dev", ptr(dst), stride, ptr(mean), 1, ptr(rstd), 1, ptr(src), stride, ptr(gamma), 1,
                 ptr(beta), 1, rows, n, G.LN_EPS)
            what = f"{cid}, {name}{', in place' if in_place else ''}"
            assert ln_last(G.FWD) == code + 4 * (1 - vec), what
            assert_bits(dst, want_y, f"y: {what}")
            assert_bits(mean, want_mean, f"mean: {what}")
            assert_bits(rstd, want_rstd, f"rstd: {what}")
            assert gaps_hold(dbuf, off, rows, n, stride), what
            if not in_place:
                assert_bits(src, x, f"the source: {what}")


@pytest.mark.parametrize("cid", ids("layer_norm_dx"))
def test_layer_norm_dx(cid):
    c = G.BY_ID[cid]
    rows, n, code = c.shape["rows"], c.shape["n"], c.shape["code"]
    past_the_cap(c)
    idx = tiled(rows)
    x13, dy13, gamma, _ = G.layer_norm_base(n)
    _, mean13, rstd13, dx13 = G.layer_norm_model(n)
    x, dy, gamma = dev(x13)[idx], dev(dy13)[idx], dev(gamma)
    mean, rstd, want = dev(mean13)[idx].contiguous(), dev(rstd13)[idx].contiguous(), dev(dx13)[idx]
    for name, stride, off, vec in row_layouts(n):
        xbuf, vx = rows_buffer(rows, n, stride, off, x)
        ybuf, vdy = rows_buffer(rows, n, stride, off, dy)
        for in_place in (False, True):                           # in place: dx over dy
            dbuf, dst = (ybuf, vdy) if in_place else rows_buffer(rows, n, stride, off)
            call("laser_hip_layer_norm_grad_f32_dev", ptr(dst), stride, None, 1, None, 1, ptr(vdy), stride, ptr(vx), stride, ptr(mean), 1,
                 ptr(rstd), 1, ptr(gamma), 1, rows, n)
            what = f"{cid}, {name}{', dx over dy' if in_place else ''}"
            assert ln_last(G.DX) == code + 4 * (1 - vec), what
            assert_bits(dst, want, f"dx: {what}")
            assert gaps_hold(dbuf, off, rows, n, stride), what
            assert_bits(vx, x, f"x: {what}")
            if not in_place:
                assert_bits(vdy, dy, f"dy: {what}")


# ---- the strip kernels of the softmax along an axis ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids("softmax_axis"))
def test_softmax_axis_strips(cid):
    """x[o, :, i] is base vector (i + 5 o) mod 13: the strips a workgroup meets on its two trips, 2048 strips apart and in
    different outer indices, hold different columns"""
    c = G.BY_ID[cid]
    outer, n, inner, code = (c.shape[k] for k in ("outer", "n", "inner", "code"))
    past_the_cap(c)
    assert G.plan_of(L(), c)[:2] == [code, G.AXIS_CW] and inner % G.AXIS_CW not in (0, 1)
    pat = (torch.arange(inner, device="cuda")[None, :] + 5 * torch.arange(outer, device="cuda")[:, None]) % P
    x = dev(G.softmax_base(n))[pat].permute(0, 2, 1)                # (outer, n, inner)
    want = dev(G.softmax_model(n))[pat].permute(0, 2, 1)
    for name, astride, off, vec in (("strip rows on 16-byte boundaries", up4(inner), 0, 1), ("base one element off", inner, 1, 0)):
        ostride = n * astride
        size = off + outer * ostride + 8
        view = lambda b: b.as_strided((outer, n, inner), (ostride, astride, 1), off)
        sbuf = torch.full((size,), SENTINEL, device="cuda")
        view(sbuf).copy_(x)
        for in_place in (False, True):
            dbuf = sbuf if in_place else torch.full((size,), SENTINEL, device="cuda")
            laser_amd.softmax(view(sbuf), out=view(dbuf), axis=1)
            what = f"{cid}, {name}{', in place' if in_place else ''}"
            assert opt("last_softmax_kernel") == code + 4 * (1 - vec), what
            assert_bits(view(dbuf), want, what)
            if not in_place:
                assert_bits(view(sbuf), x, f"the source: {what}")
            view(dbuf).fill_(SENTINEL)
            assert bool((dbuf == SENTINEL).all()), f"wrote outside the elements: {what}"
            del dbuf


# ---- the column kernels: the bias gradient and the layer norm's parameter gradients --------------------------------------------------
def column_layouts(n):
    return [("rows on 16-byte boundaries", up4(n) if up4(n) > n else n + 4, 0, 1), ("base one element off", n, 1, 0)]


@pytest.mark.parametrize("cid", ids("bias_grad"))
def test_bias_gradient(cid):
    """(a): dz stored and the tanh gradient, one chunk; (b), (c): db alone, two-level, no activation"""
    c = G.BY_ID[cid]
    rows, n = c.shape["rows"], c.shape["n"]
    past_the_cap(c)
    assert G.plan_of(L(), c)[2] == (1 if c.shape["chunks"] == 1 else 2)
    kind = "tanh" if cid.endswith("-a") else None
    idx = tiled(n)
    dy13, y13, _, _ = G.column_base(rows)
    dz13, db13 = G.bias_grad_model(rows, kind)
    dy13, y13, dz13, want_db = dev(dy13), dev(y13), dev(dz13), dev(db13)[idx]
    for name, stride, off, vec in column_layouts(n):
        ybuf, vdy = rows_buffer(rows, n, stride, off)
        vdy.copy_(dy13[:, idx])
        db = torch.full((n,), SENTINEL, device="cuda")
        if kind:
            _, vy = rows_buffer(rows, n, stride, off, y13[:, idx])
            zbuf, vdz = rows_buffer(rows, n, stride, off)
            laser_amd.bias_grad(vdy, vy, kind, dz=vdz, out=db)
            assert_bits(vdz, dz13[:, idx], f"dz: {cid}, {name}")
            assert gaps_hold(zbuf, off, rows, n, stride), name
        else:
            laser_amd.bias_grad(vdy, dz=False, out=db)
        assert L().laser_hip_bias_grad_last_kernel() == 1 - vec, name
        assert_bits(db, want_db, f"db: {cid}, {name}")
        assert gaps_hold(ybuf, off, rows, n, stride), name
        del ybuf, vdy


@pytest.mark.parametrize("cid", ids("layer_norm_params"))
def test_layer_norm_parameter_gradients(cid):
    """both sums from one launch, and each alone: three instances of the column kernel"""
    c = G.BY_ID[cid]
    rows, n = c.shape["rows"], c.shape["n"]
    past_the_cap(c)
    assert G.plan_of(L(), c)[2] == (1 if c.shape["chunks"] == 1 else 3)
    idx = tiled(n)
    dy13, _, mean, rstd = G.column_base(rows)
    g13, b13 = G.layer_norm_params_model(rows)
    dy13, x13, mean, rstd = dev(dy13), dev(G.layer_norm_x_columns(rows)), dev(mean), dev(rstd)
    want_g, want_b = dev(g13)[idx], dev(b13)[idx]
    for name, stride, off, vec in column_layouts(n):
        ybuf, vdy = rows_buffer(rows, n, stride, off)
        vdy.copy_(dy13[:, idx])
        xbuf, vx = rows_buffer(rows, n, stride, off)
        vx.copy_(x13[:, idx])
        for need_g, need_b in ((1, 1), (1, 0), (0, 1)):
            dg = torch.full((n,), SENTINEL, device="cuda") if need_g else None
            db = torch.full((n,), SENTINEL, device="cuda") if need_b else None
            call("laser_hip_layer_norm_grad_f32_dev", None, 0, ptr(dg), 1, ptr(db), 1, ptr(vdy), stride, ptr(vx), stride, ptr(mean), 1,
                 ptr(rstd), 1, None, 1, rows, n)
            what = f"{cid}, {name}, dgamma {need_g} dbeta {need_b}"
            assert ln_last(G.PARAMS) == 1 - vec, what
            if need_g:
                assert_bits(dg, want_g, f"dgamma: {what}")
            if need_b:
                assert_bits(db, want_b, f"dbeta: {what}")
        assert gaps_hold(ybuf, off, rows, n, stride) and gaps_hold(xbuf, off, rows, n, stride), name
        del ybuf, vdy, xbuf, vx


# ---- scan.hip ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids("cumsum"))
def test_cumsum(cid):
    c = G.BY_ID[cid]
    sfx, rows, n = c.shape["sfx"], c.shape["rows"], c.shape["n"]
    past_the_cap(c)
    plan = (C.c_int64 * 4)()
    assert L().laser_hip_cumsum_plan(rows, n, 4 if sfx == "f32" else 8, 0, plan) == 0            # cus = 0: what the launcher asks
    assert plan[0] == c.shape["variant"] and plan[2] == c.cap
    dtype = torch.float32 if sfx == "f32" else torch.int64
    idx = tiled(rows)
    x, want = dev(G.cumsum_base(sfx, n))[idx], dev(G.cumsum_model(sfx, n))[idx]
    for name, stride, off, vec in row_layouts(n, 4 if sfx == "f32" else 2):
        sbuf, src = rows_buffer(rows, n, stride, off, x, dtype)
        dbuf, dst = rows_buffer(rows, n, stride, off, None, dtype)
        call(f"laser_hip_cumsum_{sfx}_dev", ptr(dst), stride, ptr(src), stride, rows, n)
        assert_bits(dst, want, f"{cid}, {name}")
        assert gaps_hold(dbuf, off, rows, n, stride), name
        assert_bits(src, x, f"{cid}, {name}: the source")
        call(f"laser_hip_cumsum_{sfx}_dev", ptr(src), stride, ptr(src), stride, rows, n)
        assert_bits(src, want, f"{cid}, {name}, in place")
        assert gaps_hold(sbuf, off, rows, n, stride), name


def test_searchsorted_with_more_values_than_lanes():
    c = G.BY_ID["searchsorted"]
    rows, n, m = c.shape["rows"], c.shape["n"], c.shape["m"]
    assert c.units[0] == G.cdiv(rows * m, G.LANES) > c.cap
    idx = tiled(rows)
    a13, v13, left13, right13 = G.searchsorted_model(n, m)
    a, v = dev(a13)[idx].contiguous(), dev(v13)[idx].contiguous()
    for right, want in ((0, left13), (1, right13)):
        out = torch.full((rows, m), int(SENTINEL), dtype=torch.int32, device="cuda")
        call("laser_hip_searchsorted_f32_dev", ptr(out), ptr(a), n, ptr(v), rows, n, m, right)
        assert_bits(out, dev(want)[idx], f"searchsorted, right {right}")


def test_cdf_sample_with_more_draws_than_lanes():
    c = G.BY_ID["cdf-sample"]
    rows, n, m = c.shape["rows"], c.shape["n"], c.shape["m"]
    assert c.units[0] == G.cdiv(rows * m, G.LANES) > c.cap
    idx = tiled(rows)
    cdf13, u13, idx13 = G.cdf_sample_model(n, m)
    cdf, u = dev(cdf13)[idx].contiguous(), dev(u13)[idx].contiguous()
    out = torch.full((rows, m), int(SENTINEL), dtype=torch.int32, device="cuda")
    call("laser_hip_cdf_sample_f32_dev", ptr(out), ptr(cdf), n, ptr(u), rows, n, m)
    assert_bits(out, dev(idx13)[idx], "cdf_sample")
    assert bool((out[G.NAN_AT::P] == -1).all())                                   # the rows whose total is NaN
    assert_bits(cdf, dev(cdf13)[idx], "the CDF was only read")


def test_cdf_sample_and_remove_with_more_rows_than_lanes():
    """a lane per row; each of the two rounds also scans 2^22 + 3 rows, 2^20 row groups on a grid of 2048"""
    c = G.BY_ID["cdf-sample-remove"]
    rows, n, k = c.shape["rows"], c.shape["n"], c.shape["k"]
    assert c.units[0] == G.cdiv(rows, G.LANES) > c.cap
    idx = tiled(rows)
    w13, u13, idx13, after13 = G.cdf_remove_model(n, k)
    w, u = dev(w13)[idx].contiguous(), dev(u13)[idx].contiguous()
    cdf = torch.full((rows, n), SENTINEL, device="cuda")
    out = torch.full((rows, k), int(SENTINEL), dtype=torch.int32, device="cuda")
    call("laser_hip_cdf_sample_remove_f32_dev", ptr(out), ptr(w), n, ptr(cdf), n, ptr(u), rows, n, k)
    assert_bits(out, dev(idx13)[idx], "cdf_sample_remove")
    assert_bits(w, dev(after13)[idx], "the weights afterwards")
    assert not bool((cdf == SENTINEL).any())                                       # every row of the workspace was scanned


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids("sampler_build"))
def test_sampler_build(cid):
    c = G.BY_ID[cid]
    rows, n, code = c.shape["rows"], c.shape["n"], c.shape["code"]
    past_the_cap(c)
    assert G.plan_of(L(), c)[0] == code
    idx = tiled(rows)
    w13, trees13 = G.sampler_build_model(n)
    w, want = dev(w13)[idx], dev(trees13)[idx]
    elems = trees13.shape[1]
    for name, stride, off, vec in row_layouts(n):
        wbuf, vw = rows_buffer(rows, n, stride, off, w)
        tbuf, tree = rows_buffer(rows, elems, elems + 4, 0)                        # images on 16-byte boundaries, a gap after each
        call("laser_hip_sampler_build_f32_dev", ptr(tree), elems + 4, ptr(vw), stride, rows, n)
        assert_bits(tree, want, f"{cid}, {name}")
        assert gaps_hold(tbuf, 0, rows, elems, elems + 4), name
        assert_bits(vw, w, f"{cid}, {name}: the weights")
        del tbuf, tree


def test_sampler_sample_with_more_draws_than_lanes():
    c = G.BY_ID["sampler-sample"]
    rows, n, m = c.shape["rows"], c.shape["n"], c.shape["m"]
    assert c.units[0] == G.cdiv(rows * m, G.LANES) > c.cap
    idx = tiled(rows)
    trees13 = G.sampler_build_model(n)[1]
    u13, idx13 = G.sampler_sample_model(n, m)
    tree, u = dev(trees13)[idx].contiguous(), dev(u13)[idx].contiguous()
    out = torch.full((rows, m), int(SENTINEL), dtype=torch.int32, device="cuda")
    call("laser_hip_sampler_sample_f32_dev", ptr(out), ptr(tree), trees13.shape[1], ptr(u), rows, n, m)
    assert_bits(out, dev(idx13)[idx], "sample")
    assert bool((out[G.NAN_AT::P] == -1).all())
    assert_bits(tree, dev(trees13)[idx], "the trees were only read")


def test_sampler_update_and_remove_with_more_rows_than_lanes():
    """update and draw-and-remove give a lane to a row: 2^22 + 3 trees of 3 weights, built by the LDS kernel 256 rows a workgroup"""
    c = G.BY_ID["sampler-update-remove"]
    rows, n, k = c.shape["rows"], c.shape["n"], c.shape["k"]
    past_the_cap(c)
    assert all(u > c.cap for u in c.units)
    idx = tiled(rows)
    w13, trees13 = G.sampler_build_model(n)
    elem13, weight13, updated13, u13, idx13, drawn13 = G.sampler_update_model(n, k)
    elems = trees13.shape[1]
    w = dev(w13)[idx].contiguous()
    tree = torch.full((rows, elems), SENTINEL, device="cuda")
    call("laser_hip_sampler_build_f32_dev", ptr(tree), elems, ptr(w), n, rows, n)
    assert_bits(tree, dev(trees13)[idx], "build")
    elem, weight = dev(elem13)[idx].contiguous(), dev(weight13)[idx].contiguous()
    call("laser_hip_sampler_update_f32_dev", ptr(tree), elems, ptr(elem), ptr(weight), rows, n)
    assert_bits(tree, dev(updated13)[idx], "update")
    u = dev(u13)[idx].contiguous()
    out = torch.full((rows, k), int(SENTINEL), dtype=torch.int32, device="cuda")
    call("laser_hip_sampler_sample_remove_f32_dev", ptr(out), ptr(tree), elems, ptr(u), rows, n, k)
    assert_bits(out, dev(idx13)[idx], "sample_remove")
    assert_bits(tree, dev(drawn13)[idx], "the trees after the draws")


# ---- the embedding -------------------------------------------------------------------------------------------------------------------
def emb_last(what):
    return L().laser_hip_embedding_last_kernel(what)


def emb_layouts(dim):
    """(name, row stride, base offset, vector instances)"""
    return [("contiguous", dim, 0, int(dim % 4 == 0)), ("padded rows on 16-byte boundaries", up4(dim) + 4, 0, 1),
            ("base one element off", dim, 1, 0)]


@pytest.mark.parametrize("cid", ids("embedding_columns"))
def test_embedding_rows_wider_than_the_lanes_that_span_them(cid):
    """dim > 1024: the gather's lanes take a second trip along the row, the short-segment kernel has 2 or 3 column blocks and
    the long-segment kernel 65 strips and more; the 13 base columns are tiled along the rows"""
    c = G.BY_ID[cid]
    tokens, vocab, dim, kind = (c.shape[k] for k in ("tokens", "vocab", "dim", "kind"))
    assert G.lanes_per_row(dim) == c.cap == G.LANES < c.units[0] == G.cdiv(dim, 4)
    idx13, dy13, w13 = G.embedding_columns_base(tokens, vocab, kind)
    y13, order, starts, dw13 = G.embedding_columns_model(tokens, vocab, kind)
    counts = np.diff(starts)
    if kind == "mostly0":
        assert counts[0] > G.EMB_SHORT and 0 < counts[1] <= G.EMB_SHORT          # a long segment next to a short one
    cols = tiled(dim)
    didx = dev(idx13)
    w, dy, want_y, want_dw = dev(w13)[:, cols], dev(dy13)[:, cols], dev(y13)[:, cols], dev(dw13)[:, cols]
    o, s = laser_amd.embedding_group(didx, vocab)
    assert np.array_equal(o.to_numpy(), order) and np.array_equal(s.to_numpy(), starts)
    for name, stride, off, vec in emb_layouts(dim):
        _, vw = rows_buffer(vocab, dim, stride, off, w)
        ybuf, vy = rows_buffer(tokens, dim, stride, off)
        laser_amd.embedding(vw, didx, out=vy)
        assert emb_last(0) == 1 - vec, name
        assert_bits(vy, want_y, f"y: {cid}, {name}")
        assert gaps_hold(ybuf, off, tokens, dim, stride), name
        gbuf, vdy = rows_buffer(tokens, dim, stride, off, dy)
        dbuf, vdw = rows_buffer(vocab, dim, stride, off)
        laser_amd.embedding_backward(vdy, didx, vocab, out=vdw)
        assert emb_last(2) == 1 - vec, name
        assert_bits(vdw, want_dw, f"dw: {cid}, {name}")
        assert gaps_hold(dbuf, off, vocab, dim, stride) and gaps_hold(gbuf, off, tokens, dim, stride), name


def test_embedding_gather_with_more_tokens_than_workgroups():
    c = G.BY_ID["embedding-gather-cap"]
    tokens, vocab, dim = c.shape["tokens"], c.shape["vocab"], c.shape["dim"]
    assert c.units[0] == tokens > c.cap and G.lanes_per_row(dim) == G.LANES          # a workgroup per token
    ids13, w, rows13 = G.embedding_gather_model(vocab, dim)
    t = tiled(tokens)
    didx, want = dev(ids13)[t].contiguous(), dev(rows13)[t]
    for name, stride, off, vec in emb_layouts(dim):
        _, vw = rows_buffer(vocab, dim, stride, off, dev(w))
        ybuf, vy = rows_buffer(tokens, dim, stride, off)
        laser_amd.embedding(vw, didx, out=vy)
        assert emb_last(0) == 1 - vec, name
        assert_bits(vy, want, f"y: {name}")
        assert gaps_hold(ybuf, off, tokens, dim, stride), name
        del ybuf, vy


def test_embedding_short_sums_with_more_ids_than_workgroups():
    c = G.BY_ID["embedding-short-cap"]
    tokens, vocab, dim = c.shape["tokens"], c.shape["vocab"], c.shape["dim"]
    assert c.units[0] == vocab > c.cap and G.lanes_per_row(dim) == G.LANES           # a workgroup per id
    idx, dy13, seen, dw13 = G.embedding_short_model(tokens, vocab, c.cap)
    cols = tiled(dim)
    didx, dy = dev(idx), dev(dy13)[:, cols]
    want = torch.zeros((vocab, dim), device="cuda")                                   # +0 for an id that never occurs
    want[dev(seen)] = dev(dw13)[:, cols]
    for name, stride, off, vec in emb_layouts(dim):
        _, vdy = rows_buffer(tokens, dim, stride, off, dy)
        dbuf, vdw = rows_buffer(vocab, dim, stride, off)
        laser_amd.embedding_backward(vdy, didx, vocab, out=vdw)
        assert emb_last(2) == 1 - vec, name
        assert_bits(vdw, want, f"dw: {name}")
        assert gaps_hold(dbuf, off, vocab, dim, stride), name
        del dbuf, vdw


def test_embedding_sort_tile_above_512():
    """2^23 + 5 tokens: tiles of 1024 positions, 2049 workgroups a pass, 2049 position tiles of the long-segment kernel, every
    id a segment of four chunks"""
    c = G.BY_ID["embedding-tile"]
    tokens, vocab, dim = c.shape["tokens"], c.shape["vocab"], c.shape["dim"]
    p = G.plan_of(L(), c)
    assert p[:3] == [2, c.shape["tile"], c.cap + 1] and G.cdiv(tokens, G.EMB_PTILE) == c.cap + 1
    idx, dy13, order, starts, dw = G.embedding_tile_model(tokens, vocab)
    didx = dev(idx)
    dy = dev(dy13)[tiled(tokens)].reshape(tokens, 1).contiguous()
    o, s = laser_amd.embedding_group(didx, vocab)
    assert (emb_last(1), emb_last(3)) == (p[0], p[2])
    o, s = torch.as_tensor(o, device="cuda"), torch.as_tensor(s, device="cuda")
    assert_bits(o, dev(order), "order")
    assert_bits(s, dev(starts), "starts")
    out = torch.full((vocab, dim), SENTINEL, device="cuda")
    laser_amd.embedding_backward(dy, didx, vocab, out=out)                            # grouped again by the call itself
    assert_bits(out, dev(dw), "dw")


def test_embedding_group_with_four_passes_and_more_ids_than_lanes():
    c = G.BY_ID["embedding-group-4-passes"]
    tokens, vocab = c.shape["tokens"], c.shape["vocab"]
    assert G.plan_of(L(), c)[0] == 4 and c.units[0] == (vocab + G.LANES) // G.LANES > c.cap
    idx, order, starts = G.embedding_group_model(tokens, vocab)
    o, s = laser_amd.embedding_group(dev(idx), vocab)
    assert emb_last(1) == 4
    assert_bits(torch.as_tensor(o, device="cuda"), dev(order), "order")
    assert_bits(torch.as_tensor(s, device="cuda"), dev(starts), "starts")
