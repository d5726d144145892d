#!/usr/bin/env python3
"""laser_amd.bias_grad at three (rows, n) shapes beside its yardsticks on the same preallocated device buffers, in one process
after warm-up, the entries interleaved and the order reversed every other round (the median, the minimum and the maximum of
the rounds are reported):
  - bias_grad (tanh) with the dz store, without it, and the plain column sum (no activation, no dz);
  - the only device route without this kernel: activation_grad into dz, then reduce_sum over each of the n strided column
    views dz[:, j] into db[j] -- n + 1 launches.  (forEachReduce folds a whole view into ONE value, so it is no second
    route: it would also take n calls.)  It is timed with fewer iterations: it is hundreds of times slower;
  - copy_strided_b32 (laser_amd.copyFrom) of dy into dz: the one-read, one-write HBM yardstick the other elementwise kernels
    are held to.
One JSON line per shape, and a table in markdown after them.  GB/s counts the bytes a call must move per element: 12 with dz
(dy and y read, dz written), 8 without (two reads), 4 for the column sum, 8 for the copy; db and the chunk partials are
noise beside them.  Event timings include launch overhead.
usage: dense_grad_throughput.py [iters = 20] [rounds = 6] [iters of the column-by-column route = 1]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402

SHAPES = ((65536, 1024), (4096, 4096), (256, 8192))
BYTES = {"bias_grad_dz": 12, "bias_grad": 8, "column_sum": 4, "act_grad_then_column_sums": 12, "act_grad": 12, "copy": 8}


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
    rounds = int(args[1]) if len(args) > 1 else 6
    slow_iters = int(args[2]) if len(args) > 2 else 1
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    table = []
    for rows, n in SHAPES:
        dy = torch.randn((rows, n), device="cuda", generator=g)
        y = torch.tanh(torch.randn((rows, n), device="cuda", generator=g))
        dz = torch.empty_like(dy)
        db = torch.empty((n,), device="cuda")
        tdy, tdz = laser_amd.fromTorch(dy), laser_amd.fromTorch(dz)
        cols = [dz[:, j] for j in range(n)]
        outs = [db[j:j + 1] for j in range(n)]

        def by_columns():
            laser_amd.activation_grad(dy, y, "tanh", out=dz)
            for j in range(n):
                laser_amd.reduce_sum(cols[j], out=outs[j])

        fns = {"bias_grad_dz": lambda: laser_amd.bias_grad(dy, y, "tanh", dz=dz, out=db),
               "bias_grad": lambda: laser_amd.bias_grad(dy, y, "tanh", dz=False, out=db),
               "column_sum": lambda: laser_amd.bias_grad(dy, None, None, dz=False, out=db),
               "act_grad": lambda: laser_amd.activation_grad(dy, y, "tanh", out=dz),
               "copy": lambda: laser_amd.copyFrom(tdz, tdy),
               "act_grad_then_column_sums": by_columns}
        its = {k: (slow_iters if k == "act_grad_then_column_sums" else iters) for k in fns}
        for k, fn in fns.items():       # warm up everything the timed window uses
            for _ in range(1 if its[k] == slow_iters else 3):
                fn()
        torch.cuda.synchronize()
        # the two routes agree, bit for bit (the column-by-column one ran last in the warm-up)
        want = db.clone()
        fns["bias_grad_dz"]()
        torch.cuda.synchronize()
        same = bool(torch.equal(want.view(torch.int32), db.view(torch.int32)))
        times = {k: [] for k in fns}
        for r in range(rounds):
            order = list(fns.items())
            for k, fn in (order if r % 2 == 0 else order[::-1]):
                times[k].append(timed(fn, its[k]))
        out = {"case": "dense_grad", "rows": rows, "n": n, "iters": iters, "rounds": rounds, "slow_iters": slow_iters,
               "kernel": laser_amd.lib().laser_hip_bias_grad_last_kernel(), "routes_agree_bit_for_bit": same}
        for k, ts in times.items():
            med = statistics.median(ts)
            out[k + "_ms"] = round(med * 1e3, 4)
            out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
            out[k + "_gbs"] = round(BYTES[k] * rows * n / med / 1e9, 1)
        for k in fns:
            if k != "copy":     # per byte moved, so that 12, 8 and 4 bytes per element compare with the copy's 8
                out[f"{k}_rate_of_copy"] = round(out[k + "_gbs"] / out["copy_gbs"], 3)
        out["speedup_over_column_sums"] = round(out["act_grad_then_column_sums_ms"] / out["bias_grad_dz_ms"], 1)
        print(json.dumps(out), flush=True)
        table.append(out)
        del cols, outs, dy, y, dz, db
    print("\n| rows x n | entry | ms (min .. max) | GB/s | GB/s / copy |\n|---|---|---|---|---|")
    for out in table:
        for k in BYTES:
            lo, hi = out[k + "_ms_min_max"]
            print(f"| {out['rows']} x {out['n']} | {k} | {out[k + '_ms']} ({lo} .. {hi}) | {out[k + '_gbs']} | "
                  f"{out.get(k + '_rate_of_copy', '')} |")


if __name__ == "__main__":
    main()
