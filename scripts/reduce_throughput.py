#!/usr/bin/env python3
"""Reductions (laser_amd.reduce_* / forEachReduce) beside torch on the same device operands, in one process after warm-up.
One JSON line per case:
  - f32 reduce_sum at n = 2^28 beside torch.sum (bytes read per second against the 8 TB/s HBM spec); f64 sum, f32 min / max
    and i32 sum at the same n;
  - a strided case: reduce_sum of a transposed 16384^2 f32 view beside torch.sum of the same view;
  - forEachReduce("acc += x * y") beside torch.dot on two f32 vectors of 2^28;
  - warm host time per call at 4096 elements (asynchronous, into a device scalar) beside torch.sum(out=).
Event timings include launch overhead; kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this
script.  usage: reduce_throughput.py [iters = 20] [log2 n = 28]"""
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
    if "laser" in times:
        out["laser_of_spec"] = round(nbytes / times["laser"] / 1e12 / SPEC_TBS, 3)
        if "torch" in times:
            out["laser_vs_torch_rate"] = round(times["torch"] / times["laser"], 3)
    print(json.dumps(out), flush=True)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    n = 1 << (int(sys.argv[2]) if len(sys.argv) > 2 else 28)
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)

    # f32 sum, then min / max, on one vector; results into a device scalar (no host synchronisation per call)
    x = torch.randn(n, device="cuda", generator=g)
    o = torch.empty(1, device="cuda")
    ot = torch.empty((), device="cuda")
    t_l = timed(lambda: laser_amd.reduce_sum(x, out=o), iters)
    assert laser_amd.get_option("last_reduce_variant") == 0
    t_t = timed(lambda: torch.sum(x, dim=0, out=ot), iters)
    row("sum_f32", n, 4 * n, laser=t_l, torch=t_t)
    for op, tf in (("min", torch.amin), ("max", torch.amax)):
        t_l = timed(lambda: getattr(laser_amd, f"reduce_{op}")(x, out=o), iters)
        t_t = timed(lambda: tf(x, dim=0, out=ot), iters)
        row(f"{op}_f32", n, 4 * n, laser=t_l, torch=t_t)

    # forEachReduce dot product beside torch.dot
    y = torch.randn(n, device="cuda", generator=g)
    f = np.float32(0)
    t_l = timed(lambda: laser_amd.forEachReduce("acc += x * y", merge="acc += other", init=f, x=x, y=y, out=o), iters)
    t_t = timed(lambda: torch.dot(x, y, out=ot), iters)
    row("dot_f32_forEachReduce", n, 8 * n, laser=t_l, torch=t_t)
    del x, y

    # f64 and i32 sums
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    o64, ot64 = torch.empty(1, dtype=torch.float64, device="cuda"), torch.empty((), dtype=torch.float64, device="cuda")
    t_l = timed(lambda: laser_amd.reduce_sum(x, out=o64), iters)
    t_t = timed(lambda: torch.sum(x, dim=0, out=ot64), iters)
    row("sum_f64", n, 8 * n, laser=t_l, torch=t_t)
    del x
    x = torch.randint(-1000, 1000, (n,), dtype=torch.int32, device="cuda", generator=g)
    oi = torch.empty(1, dtype=torch.int32, device="cuda")
    t_l = timed(lambda: laser_amd.reduce_sum(x, out=oi), iters)
    t_t = timed(lambda: torch.sum(x, dtype=torch.int32), iters)
    row("sum_i32", n, 4 * n, laser=t_l, torch=t_t)
    del x

    # strided: a transposed view
    m = 1 << 14
    x = torch.randn((m, m), device="cuda", generator=g)
    xt = x.t()
    t_l = timed(lambda: laser_amd.reduce_sum(xt, out=o), iters)
    assert laser_amd.get_option("last_reduce_variant") == 2
    t_t = timed(lambda: torch.sum(xt, dim=(0, 1), out=ot), iters)
    row("sum_f32_transposed", m * m, 4 * m * m, laser=t_l, torch=t_t)
    del x, xt

    # warm host time per call at 4096 elements
    k = 4096
    x = torch.randn(k, device="cuda", generator=g)
    hx = x.cpu().numpy()
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

    print(json.dumps({"case": "call_overhead", "n": k,
                      "warm_host_us_reduce_sum_dev": round(host_us(lambda: laser_amd.reduce_sum(x, out=o)), 2),
                      "warm_host_us_reduce_sum_sync": round(host_us(lambda: laser_amd.reduce_sum(x)), 2),
                      "warm_host_us_reduce_sum_host_array": round(host_us(lambda: laser_amd.reduce_sum(hx)), 2),
                      "warm_host_us_torch_sum": round(host_us(lambda: torch.sum(x, dim=0, out=ot)), 2)}), flush=True)


if __name__ == "__main__":
    main()
