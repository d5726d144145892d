#!/usr/bin/env python3
"""forEach with a body (laser_amd.forEach) beside forEachMap and torch on the same device operands, in one process after
warm-up.  One JSON line per case:
  - contiguous `x = y + alpha * z` at n = 2^28: f32 (12 B per element, TB/s against the 8 TB/s HBM spec) beside
    forEachMap("axpy") and torch.add(y, z, alpha=...); the same body on f64 and int8 (the widest and narrowest vectors);
  - a strided case: x = y with y a transposed view, beside forEachMap("copy") on the same views;
  - first-call compile latency of a new body, and warm host time per call at 4096 elements beside forEachMap.
Event timings include launch overhead; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script.  usage: foreach_throughput.py [iters = 20] [log2 n = 28]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import laser_amd  # noqa: E402

SPEC_TBS = 8.0


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def row(case, n, nbytes, **times):
    out = {"case": case, "n": n, "bytes": nbytes}
    for k, t in times.items():
        out[k + "_ms"] = round(t * 1e3, 4)
        out[k + "_tbs"] = round(nbytes / t / 1e12, 3)
    if "foreach" in times:
        out["foreach_of_spec"] = round(nbytes / times["foreach"] / 1e12 / SPEC_TBS, 3)
    print(json.dumps(out), flush=True)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 28)
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    alpha = 0.5
    body = "x = y + alpha * z"

    # contiguous f32: forEach vs forEachMap("axpy") vs torch.add, identical results required
    y = torch.rand(n, device="cuda", generator=g)
    z = torch.rand(n, device="cuda", generator=g)
    x = torch.empty_like(y)
    ty, tz, tx = laser_amd.fromTorch(y), laser_amd.fromTorch(z), laser_amd.fromTorch(x)
    ref = torch.empty_like(y)
    prm = {"alpha": np.float32(alpha)}
    t_fe = timed(lambda: laser_amd.forEach(body, x=x, y=y, z=z, params=prm), iters)
    assert laser_amd.get_option("last_foreach_variant") == 0
    ref.copy_(x)
    t_map = timed(lambda: laser_amd.forEachMap("axpy", tx, tz, ty, alpha=alpha), iters)   # alpha * z + y
    assert torch.equal(x, ref), "forEach and forEachMap differ"
    t_torch = timed(lambda: torch.add(y, z, alpha=alpha, out=x), iters)
    row("contig_f32_axpy", n, 12 * n, foreach=t_fe, forEachMap=t_map, torch=t_torch)
    del y, z, x, ref, ty, tz, tx

    # the same body on f64 (E = 2) and int8 (E = 16), against torch on the same operands
    for dt, pv in ((torch.float64, np.float64(alpha)), (torch.int8, np.int8(3))):
        if dt.is_floating_point:
            y = torch.rand(n, dtype=dt, device="cuda", generator=g)
            z = torch.rand(n, dtype=dt, device="cuda", generator=g)
        else:
            y = torch.randint(-128, 128, (n,), dtype=dt, device="cuda", generator=g)
            z = torch.randint(-128, 128, (n,), dtype=dt, device="cuda", generator=g)
        x = torch.empty_like(y)
        t_fe = timed(lambda: laser_amd.forEach(body, x=x, y=y, z=z, params={"alpha": pv}), iters)
        assert laser_amd.get_option("last_foreach_variant") == 0
        t_torch = timed(lambda: torch.add(y, z, alpha=pv.item(), out=x), iters)
        row(f"contig_{str(dt).replace('torch.', '')}_axpy", n, 3 * y.element_size() * n, foreach=t_fe, torch=t_torch)
        del y, z, x

    # strided: x = y^T on an m x m f32 matrix, beside forEachMap("copy") on the same views
    m = 1 << 14
    y = torch.rand((m, m), device="cuda", generator=g)
    x = torch.empty((m, m), device="cuda")
    yt = y.t()
    t_fe = timed(lambda: laser_amd.forEach("x = y", x=x, y=yt), iters)
    assert laser_amd.get_option("last_foreach_variant") == 2
    got = x.clone()
    tx, tyt = laser_amd.fromTorch(x), laser_amd.fromTorch(y).transpose()
    t_map = timed(lambda: laser_amd.forEachMap("copy", tx, tyt), iters)
    torch.cuda.synchronize()
    assert torch.equal(got, x)
    row("strided_f32_transpose_copy", m * m, 8 * m * m, foreach=t_fe, forEachMap=t_map)
    del y, x, yt, got, tx, tyt

    # first-call compile latency and warm host overhead at 4096 elements
    k = 4096
    y = torch.rand(k, device="cuda", generator=g)
    z = torch.rand(k, device="cuda", generator=g)
    x = torch.empty_like(y)
    before = laser_amd.get_option("foreach_compiles")
    t0 = time.perf_counter()
    laser_amd.forEach("x = y * alpha - z", x=x, y=y, z=z, params=prm)
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    assert laser_amd.get_option("foreach_compiles") == before + 1
    tx, ty, tz = laser_amd.fromTorch(x), laser_amd.fromTorch(y), laser_amd.fromTorch(z)
    calls = 2000

    def host_us(fn):
        for _ in range(50):
            fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            fn()
        el = time.perf_counter() - t
        torch.cuda.synchronize()
        return el / calls * 1e6

    us_fe = host_us(lambda: laser_amd.forEach("x = y * alpha - z", x=x, y=y, z=z, params=prm))
    us_map = host_us(lambda: laser_amd.forEachMap("axpy", tx, tz, ty, alpha=-1.0))
    assert laser_amd.get_option("foreach_compiles") == before + 1
    print(json.dumps({"case": "call_overhead", "n": k, "first_call_ms": round(first * 1e3, 1),
                      "warm_host_us_foreach": round(us_fe, 2), "warm_host_us_forEachMap": round(us_map, 2)}), flush=True)


if __name__ == "__main__":
    main()
