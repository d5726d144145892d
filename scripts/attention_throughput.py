#!/usr/bin/env python3
"""laser_amd.attention (the fused forward) beside the composition the library could already run -- gemm_strided_batched
(alpha = scale) + softmax over the rows + gemm_strided_batched, the (B*H, T, T) scores in global memory -- at three
(B*H, T, d) shapes, causal and not, on the same preallocated device buffers, in one process after warm-up, the entries
interleaved and the order reversed every other round (the median, the minimum and the maximum of the rounds are reported).
The composition has no causal form: beside the causal fused run it computes the full rows, a different problem, and is there
as context only.  laser_amd.attention_backward is timed against nothing, as absolute figures.
One JSON line per (shape, causal), and a table in markdown after them.
  *_tflops         useful flops per second: 2 * BH * pairs * (d + dv) forward (pairs = T^2, or T (T + 1) / 2 causal), 2.5 times
                   that backward (five products to the forward's two); the f32 matrix peak is 157.3
  fused_mfma_tflops the flops the fused kernel executes: three score sweeps and one P V sweep over all keys
  extra_bytes      what the composition moves through HBM and the fused form does not: S written, read and written again
                   in place by the softmax, read by the second GEMM -- 4 * BH * T^2 * 4 bytes
  *_mem_bytes      device memory in use at the end of the entry's warm-up minus the operands' (hipMemGetInfo; the library's
                   allocator may keep freed blocks, so the backward's figure is what stays, not its peak)
  backward_scratch_bytes   the backward's peak beyond its results: P and dS, 2 * BH * T^2 * 4 bytes
Event timings include launch overhead.
usage: attention_throughput.py [iters = 5] [rounds = 4]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import laser_amd  # noqa: E402
from laser_amd import _lib  # noqa: E402

SHAPES = ((64, 1024, 64), (32, 2048, 128), (8, 8192, 64))
PEAK = 157.3


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def used():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def main():
    args = sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 5
    rounds = int(args[1]) if len(args) > 1 else 4
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    L = laser_amd.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = []
    for bh, t, d in SHAPES:
        q, k, v, do = (torch.randn((bh, t, d), device="cuda", generator=g) for _ in range(4))
        o = torch.empty_like(q)
        scale = float(np.float32(1 / np.sqrt(np.float64(d))))
        base = used()
        s = torch.empty((bh, t, t), device="cuda")
        oc = torch.empty_like(q)

        def composed():
            _lib.check(L.laser_hip_gemm_strided_batched_f32_dev(bh, t, t, d, C.c_float(scale), q.data_ptr(), d, 1, t * d, k.data_ptr(), 1, d,
                                                                t * d, C.c_float(0), s.data_ptr(), t, 1, t * t, stream))
            _lib.check(L.laser_hip_softmax_rows_f32_dev(s.data_ptr(), t, s.data_ptr(), t, bh * t, t, stream))
            _lib.check(L.laser_hip_gemm_strided_batched_f32_dev(bh, t, d, t, C.c_float(1), s.data_ptr(), t, 1, t * t, v.data_ptr(), d, 1,
                                                                t * d, C.c_float(0), oc.data_ptr(), d, 1, t * d, stream))
        for causal in (False, True):
            fns = {"fused": lambda: laser_amd.attention(q, k, v, causal=causal, out=o), "composed": composed,
                   "backward": lambda: laser_amd.attention_backward(do, q, k, v, causal=causal)}
            mem = {}
            for name, fn in fns.items():       # warm up everything the timed window uses
                for _ in range(2):
                    r = fn()
                mem[name] = used() - base - (0 if name == "composed" else (s.numel() + oc.numel()) * 4)
                del r
            if not causal:
                torch.cuda.synchronize()
                same = bool(((o == oc) | (torch.isnan(o) & torch.isnan(oc))).all())
            times = {name: [] for name in fns}
            for r in range(rounds):
                order = list(fns.items())
                for name, fn in (order if r % 2 == 0 else order[::-1]):
                    times[name].append(timed(fn, iters))
            pairs = t * (t + 1) // 2 if causal else t * t
            useful = 2 * bh * pairs * (d + d)
            out = {"case": "attention", "bh": bh, "t": t, "d": d, "causal": causal, "iters": iters, "rounds": rounds,
                   "kernel": L.laser_hip_attention_last_kernel(), "fused_equals_composed": same,
                   "extra_bytes": 4 * bh * t * t * 4, "backward_scratch_bytes": 2 * bh * t * t * 4}
            for name, ts in times.items():
                med = statistics.median(ts)
                out[name + "_ms"] = round(med * 1e3, 4)
                out[name + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
                flops = useful * 2.5 if name == "backward" else 2 * bh * t * t * 2 * d if name == "composed" else useful
                out[name + "_tflops"] = round(flops / med / 1e12, 2)
                out[name + "_of_peak"] = round(flops / med / 1e12 / PEAK, 4)
                out[name + "_mem_bytes"] = int(mem[name])
            executed = 2 * bh * d * (3 * (pairs if causal else t * t) + t * t)
            out["fused_mfma_tflops"] = round(executed / statistics.median(times["fused"]) / 1e12, 2)
            out["fused_speedup_over_composed"] = round(out["composed_ms"] / out["fused_ms"], 3)
            print(json.dumps(out), flush=True)
            table.append(out)
        del q, k, v, do, o, s, oc
        torch.cuda.empty_cache()
    print("\n| BH x T x d | causal | entry | ms (min .. max) | useful TFLOP/s | of 157.3 | memory MiB |\n|---|---|---|---|---|---|---|")
    for out in table:
        for name in ("fused", "composed", "backward"):
            lo, hi = out[name + "_ms_min_max"]
            print(f"| {out['bh']} x {out['t']} x {out['d']} | {out['causal']} | {name} | {out[name + '_ms']} ({lo} .. {hi}) | "
                  f"{out[name + '_tflops']} | {out[name + '_of_peak']} | {out[name + '_mem_bytes'] / 2**20:.0f} |")


if __name__ == "__main__":
    main()
