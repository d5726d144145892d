#!/usr/bin/env python3
"""laser_hip_topk_rows_f32_dev and laser_hip_argmax_rows_f32_dev at the shapes of profiles/select/README.md beside torch.topk /
torch.argmax on the same operands, in one process after warm-up, the two interleaved and the order reversed every other
round.  Every round is reported on its own (ms per call, device events around `iters` back-to-back calls, so launch overhead
is included), with the median.  GB/s counts ONE read of the source (rows * n * 4 bytes) over the time: the streaming mapping
reads a row five times, and that is what the rate then shows.  The outputs (rows * k * 8 bytes) are noise beside it.
torch defines no tie order and its values are not bit-defined for NaN: it is a yardstick for time only; the indices are
compared on tie-free random data as a plausibility check, not as a test.
usage: select_throughput.py [iters = 10] [rounds = 5]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402

TOPK = ((4096, 32000, 50), (4096, 50257, 50), (64, 1 << 20, 1024))
ARGMAX = ((8192, 1000),)


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def ptr(t):
    return C.c_void_p(t.data_ptr())


def run(case, rows, n, k, fns, iters, rounds, L, same):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for r in range(rounds):
        order = list(fns.items())
        for name, fn in (order if r % 2 == 0 else order[::-1]):
            times[name].append(timed(fn, iters))
    out = {"case": case, "rows": rows, "n": n, "k": k, "iters": iters, "rounds": rounds, "kernel": L.laser_hip_topk_last_kernel(),
           "plan": list(laser_amd.topk_plan(rows, n, k)), "indices_equal_torch": bool(same())}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name + "_ms_rounds"] = [round(t, 4) for t in ts]
        out[name + "_ms"] = round(med, 4)
        out[name + "_gbs"] = round(rows * n * 4 / (med * 1e-3) / 1e9, 1)
    print(json.dumps(out), flush=True)
    return out


def main():
    args = sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 10
    rounds = int(args[1]) if len(args) > 1 else 5
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    L = laser_amd.lib()
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = []
    for rows, n, k in TOPK:
        x = torch.randn((rows, n), device="cuda", generator=g)
        vals = torch.empty((rows, k), device="cuda")
        idx = torch.empty((rows, k), dtype=torch.int32, device="cuda")
        keep = {}

        def ours():
            laser_amd._lib.check(L.laser_hip_topk_rows_f32_dev(ptr(vals), k, ptr(idx), k, ptr(x), n, rows, n, k, 1, st()))

        def theirs():
            keep["t"] = torch.topk(x, k, dim=1)

        table.append(run("topk", rows, n, k, {"laser": ours, "torch": theirs}, iters, rounds, L,
                         lambda: torch.equal(idx.long(), keep["t"].indices)))
        del x, vals, idx, keep
        torch.cuda.empty_cache()
    for rows, n in ARGMAX:
        x = torch.randn((rows, n), device="cuda", generator=g)
        idx = torch.empty((rows,), dtype=torch.int32, device="cuda")
        keep = {}

        def ours():
            laser_amd._lib.check(L.laser_hip_argmax_rows_f32_dev(ptr(idx), 1, None, 1, ptr(x), n, rows, n, 1, st()))

        def theirs():
            keep["t"] = torch.argmax(x, dim=1)

        table.append(run("argmax", rows, n, 1, {"laser": ours, "torch": theirs}, iters, rounds, L, lambda: torch.equal(idx.long(), keep["t"])))
    print("\n| case | rows x n x k | kernel | laser ms per call, each round | median ms | GB/s (one read) | torch ms per call, each round | median ms |"
          "\n|---|---|---|---|---|---|---|---|")
    for o in table:
        print(f"| {o['case']} | {o['rows']} x {o['n']} x {o['k']} | {o['kernel']} | {o['laser_ms_rounds']} | {o['laser_ms']} | {o['laser_gbs']} | "
              f"{o['torch_ms_rounds']} | {o['torch_ms']} |")


if __name__ == "__main__":
    main()
