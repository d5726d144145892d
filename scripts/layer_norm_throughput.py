#!/usr/bin/env python3
"""laser_amd.layer_norm and layer_norm_backward at four (rows, n) shapes beside their yardstick on the same preallocated device
buffers, in one process after warm-up, the entries interleaved and the order reversed every other round (the median, the
minimum and the maximum of the rounds are reported):
  - forward (gamma, beta, statistics stored), dx alone, dgamma and dbeta alone;
  - copy_strided_b32 (laser_amd.copyFrom) of x into y: the one-read, one-write HBM yardstick -- the forward call must read x
    and write y;
  - torch.nn.functional.layer_norm forward and its autograd backward (dx, dgamma and dbeta together) on the same box, as
    context only: another summation order, other bits.
64 x 2^20 is launch-starved by design: a row is one workgroup's, so 64 of 256 compute units work.
One JSON line per shape, and a table in markdown after them.  GB/s counts the bytes a call must move per element: 8 forward
(x read, y written), 12 for dx (dy and x read, dx written), 8 for the parameter gradients (dy and x read), 8 for the copy;
gamma, beta, the statistics and the chunk partials are noise beside them.  A long row (n > 8192) is read once per pass, three
times forward and twice backward: that traffic is not counted, it is what the rate then shows.  Event timings include
launch overhead.
usage: layer_norm_throughput.py [iters = 20] [rounds = 6]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402

SHAPES = ((65536, 1024), (8192, 4096), (4096, 8192), (64, 1 << 20))
BYTES = {"forward": 8, "dx": 12, "param_grads": 8, "copy": 8, "torch_forward": 8, "torch_backward": 20}


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
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    L = laser_amd.lib()
    table = []
    for rows, n in SHAPES:
        x = torch.randn((rows, n), device="cuda", generator=g) * 2 + 3
        dy = torch.randn((rows, n), device="cuda", generator=g)
        gamma = torch.randn((n,), device="cuda", generator=g) * 0.5 + 1
        beta = torch.randn((n,), device="cuda", generator=g)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        tx, ty = laser_amd.fromTorch(x), laser_amd.fromTorch(y)
        _, mean, rstd = laser_amd.layer_norm(x, gamma, beta, out=y)
        xt, gt, bt = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
        yt = torch.nn.functional.layer_norm(xt, (n,), gt, bt, 1e-5)
        fns = {"forward": lambda: laser_amd.layer_norm(x, gamma, beta, out=y),
               "dx": lambda: laser_amd.layer_norm_backward(dy, x, mean, rstd, gamma, need_dx=dx, need_params=False),
               "param_grads": lambda: laser_amd.layer_norm_backward(dy, x, mean, rstd, gamma, need_dx=False),
               "copy": lambda: laser_amd.copyFrom(ty, tx),
               "torch_forward": lambda: torch.nn.functional.layer_norm(x, (n,), gamma, beta, 1e-5),
               "torch_backward": lambda: torch.autograd.grad(yt, (xt, gt, bt), dy, retain_graph=True)}
        for fn in fns.values():       # warm up everything the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for r in range(rounds):
            order = list(fns.items())
            for k, fn in (order if r % 2 == 0 else order[::-1]):
                times[k].append(timed(fn, iters))
        out = {"case": "layer_norm", "rows": rows, "n": n, "iters": iters, "rounds": rounds,
               "kernels": [L.laser_hip_layer_norm_last_kernel(w) for w in (0, 1, 2)]}
        for k, ts in times.items():
            med = statistics.median(ts)
            out[k + "_ms"] = round(med * 1e3, 4)
            out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
            out[k + "_gbs"] = round(BYTES[k] * rows * n / med / 1e9, 1)
        for k in fns:
            if k != "copy":     # per byte moved, so that 8 and 12 bytes per element compare with the copy's 8
                out[f"{k}_rate_of_copy"] = round(out[k + "_gbs"] / out["copy_gbs"], 3)
        print(json.dumps(out), flush=True)
        table.append(out)
        del x, dy, y, dx, tx, ty, xt, yt, mean, rstd, fns
        torch.cuda.empty_cache()
    print("\n| rows x n | entry | ms (min .. max) | GB/s | GB/s / copy |\n|---|---|---|---|---|")
    for out in table:
        for k in BYTES:
            lo, hi = out[k + "_ms_min_max"]
            print(f"| {out['rows']} x {out['n']} | {k} | {out[k + '_ms']} ({lo} .. {hi}) | {out[k + '_gbs']} | "
                  f"{out.get(k + '_rate_of_copy', '')} |")


if __name__ == "__main__":
    main()
