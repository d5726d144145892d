#!/usr/bin/env python3
"""laser_amd.activation (relu, tanh, sigmoid) and laser_amd.activation_grad at 2^26 contiguous float32 elements beside their
yardsticks on the same preallocated device buffers, in one process after warm-up, the entries interleaved and the order
reversed every other round (the median, the minimum and the maximum of the rounds are reported):
  - laser_hip_exp_f32_dev and laser_hip_log_f32_dev (laser_amd.exp / laser_amd.log): the bit-defined elementwise kernels the
    parent has, lexp all float32, llog float64 inside without a division;
  - copy_strided_b32 (laser_amd.copyFrom): the one-read, one-write HBM yardstick of the same byte count;
  - torch.tanh and torch.sigmoid for context (the device math library; not bit-defined).
One JSON line, and a table in markdown after it.  GB/s counts the bytes a call must move: 8 per element forward (one read, one
write), 12 per element for a gradient (two reads, one write).  Event timings include launch overhead.
usage: activation_throughput.py [iters = 20] [rounds = 6] [log2 of the element count = 26]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402

KINDS = ("relu", "tanh", "sigmoid")


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
    n = 1 << (int(args[2]) if len(args) > 2 else 26)
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((n,), device="cuda", generator=g) * 16 - 8            # the main path of ltanh and lsigmoid, both signs
    xl = torch.rand((n,), device="cuda", generator=g) * 40 + 1e-3        # positive: llog's main path
    dy = torch.randn((n,), device="cuda", generator=g)
    y = torch.empty_like(x)
    dx = torch.empty_like(x)
    outs = {k: torch.empty_like(x) for k in KINDS}                        # the forward outputs the gradients read
    for k in KINDS:
        laser_amd.activation(x, k, out=outs[k])
    tx, ty = laser_amd.fromTorch(x), laser_amd.fromTorch(y)
    fns = {}
    for k in KINDS:
        fns[k] = lambda k=k: laser_amd.activation(x, k, out=y)
    for k in KINDS:
        fns[k + "_grad"] = lambda k=k: laser_amd.activation_grad(dy, outs[k], k, out=dx)
    fns.update({"exp": lambda: laser_amd.exp(x, out=y), "log": lambda: laser_amd.log(xl, out=y),
                "copy": lambda: laser_amd.copyFrom(ty, tx), "torch_tanh": lambda: torch.tanh(x, out=y),
                "torch_sigmoid": lambda: torch.sigmoid(x, out=y)})
    nbytes = {k: (12 if k.endswith("_grad") else 8) * n for k in fns}
    for fn in fns.values():       # warm up everything the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for r in range(rounds):
        order = list(fns.items())
        for k, fn in (order if r % 2 == 0 else order[::-1]):
            times[k].append(timed(fn, iters))
    out = {"case": "activation", "n": n, "iters": iters, "rounds": rounds}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k + "_ms"] = round(med * 1e3, 4)
        out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
        out[k + "_gbs"] = round(nbytes[k] / med / 1e9, 1)
    for k in fns:
        if k != "exp":
            out[f"{k}_time_of_exp"] = round(out[k + "_ms"] / out["exp_ms"], 3)
        if k != "copy":     # per byte moved, so that the gradients' 12 bytes per element compare with the copy's 8
            out[f"{k}_rate_of_copy"] = round(out[k + "_gbs"] / out["copy_gbs"], 3)
    print(json.dumps(out), flush=True)
    print("\n| entry | ms (min .. max) | GB/s | time / lexp | GB/s / copy |\n|---|---|---|---|---|")
    for k in fns:
        lo, hi = out[k + "_ms_min_max"]
        print(f"| {k} | {out[k + '_ms']} ({lo} .. {hi}) | {out[k + '_gbs']} | {out.get(k + '_time_of_exp', 1.0)} | "
              f"{out.get(k + '_rate_of_copy', '')} |")


if __name__ == "__main__":
    main()
