#!/usr/bin/env python3
"""laser_amd.exp and laser_amd.softmax beside two yardsticks on the same device buffers, in one process after warm-up and
interleaved (laser, copy, torch, laser, copy, torch, ...; the median of the rounds is reported):
  - copy_strided_b32 of the same matrix (laser_amd.copyFrom): the project's own one-read, one-write HBM yardstick;
  - torch.exp / torch.softmax writing into the same output buffer.
One JSON line per case: exp at 2^26 elements; softmax at rows x n = 8192 x 1024, 8192 x 4096, 4096 x 8192 (a row read once
and written once: the traffic of a copy) and 64 x 2^20 (long rows: read three times).  GB/s counts 8 bytes per element for
every case.  Event timings include launch overhead; kernel times and counters come from separate rocprofv3 runs of this
script (profiles/softmax/README.md).  usage: softmax_throughput.py [iters = 20] [rounds = 5] [case ...]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402

CASES = {"exp_2^26": ("exp", 1, 1 << 26), "softmax_8192x1024": ("softmax", 8192, 1024),
         "softmax_8192x4096": ("softmax", 8192, 4096), "softmax_4096x8192": ("softmax", 4096, 8192),
         "softmax_64x2^20": ("softmax", 64, 1 << 20)}


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def main():
    args = sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 20
    rounds = int(args[1]) if len(args) > 1 else 5
    names = args[2:] or list(CASES)
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in names:
        kind, rows, n = CASES[name]
        x = (torch.rand((rows, n), device="cuda", generator=g) * 40 - 20)
        y = torch.empty_like(x)
        tx, ty = laser_amd.fromTorch(x), laser_amd.fromTorch(y)
        if kind == "exp":
            fns = {"laser": lambda: laser_amd.exp(x, out=y), "copy": lambda: laser_amd.copyFrom(ty, tx),
                   "torch": lambda: torch.exp(x, out=y)}
        else:
            fns = {"laser": lambda: laser_amd.softmax(x, out=y), "copy": lambda: laser_amd.copyFrom(ty, tx),
                   "torch": lambda: torch.softmax(x, dim=1, out=y)}
        for fn in fns.values():       # warm up every shape the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, iters))
        nbytes = 8 * rows * n
        out = {"case": name, "rows": rows, "n": n, "bytes": nbytes, "iters": iters, "rounds": rounds}
        if kind == "softmax":
            out["kernel"] = laser_amd.get_option("last_softmax_kernel")
        for k, ts in times.items():
            med = statistics.median(ts)
            out[k + "_ms"] = round(med * 1e3, 4)
            out[k + "_gbs"] = round(nbytes / med / 1e9, 1)
            out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
        out["laser_of_copy"] = round(out["laser_gbs"] / out["copy_gbs"], 3)
        out["laser_of_torch"] = round(out["laser_gbs"] / out["torch_gbs"], 3)
        print(json.dumps(out), flush=True)
        del x, y, tx, ty


if __name__ == "__main__":
    main()
