#!/usr/bin/env python3
"""The F+tree sampler at the reference's benchmark shape (bench_multinomial_samplers.nim: rows of 50 000 probabilities; 128
rows there, and 4096 here to fill the device), on preallocated device buffers through the C entry points, in one process
after warm-up, the entries interleaved (build, copy, draw1, draw10, remove10, build, ...; the median round is reported):
  - build:    laser_hip_sampler_build_f32_dev; GB/s counts 4 * rows * (n + 2 P) bytes (the weights read, the images written)
  - copy:     copy_strided_b32 (laser_amd.copyFrom) of a matrix that moves the same number of bytes: the HBM yardstick
  - draw1:    1 draw per row with replacement;  draw10: 10 draws per row with replacement
  - remove10: 10 draws per row without replacement.  It mutates the trees and they are not rebuilt between calls: after all
              timed calls a row has lost about a thousand of its 50 000 elements, the depth of every walk is the same.
Random weights (normalised rows), uniforms from torch.rand.  One JSON line per shape.  Event timings include launch overhead.
usage: sampler_throughput.py [iters = 20] [rounds = 5] [rows ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402
from laser_amd import sampling  # noqa: E402

N = 50000


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
    shapes = [int(a) for a in args[2:]] or [128, 4096]
    torch.cuda.set_device(0)
    L = laser_amd.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    for rows in shapes:
        elems = sampling.tree_elems(N)
        w = torch.rand((rows, N), device="cuda", generator=g)
        w /= w.sum(1, keepdim=True)
        tree = torch.empty((rows, elems), device="cuda")
        half = (N + elems) // 2
        a, b = torch.rand((rows, half), device="cuda", generator=g), torch.empty((rows, half), device="cuda")
        ta, tb = laser_amd.fromTorch(a), laser_amd.fromTorch(b)
        u1 = torch.rand((rows, 1), device="cuda", generator=g)
        u10 = torch.rand((rows, 10), device="cuda", generator=g)
        i1 = torch.empty((rows, 1), device="cuda", dtype=torch.int32)
        i10 = torch.empty((rows, 10), device="cuda", dtype=torch.int32)
        p = lambda t: C.c_void_p(t.data_ptr())
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def ok(rc):
            assert rc == 0, L.laser_hip_last_error()

        fns = {"build": lambda: ok(L.laser_hip_sampler_build_f32_dev(p(tree), elems, p(w), N, rows, N, st())),
               "copy": lambda: laser_amd.copyFrom(tb, ta),
               "draw1": lambda: ok(L.laser_hip_sampler_sample_f32_dev(p(i1), p(tree), elems, p(u1), rows, N, 1, st())),
               "draw10": lambda: ok(L.laser_hip_sampler_sample_f32_dev(p(i10), p(tree), elems, p(u10), rows, N, 10, st())),
               "remove10": lambda: ok(L.laser_hip_sampler_sample_remove_f32_dev(p(i10), p(tree), elems, p(u10), rows, N, 10, st()))}
        for fn in fns.values():       # warm up (the build first: the draws need trees)
            for _ in range(3):
                fn()
        fns["build"]()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, iters))
        plan = (C.c_int64 * 4)()
        ok(L.laser_hip_sampler_plan(rows, N, plan))
        nbytes = 4 * rows * (N + elems)
        out = {"rows": rows, "n": N, "tree_elems": elems, "iters": iters, "rounds": rounds, "plan": list(plan), "build_bytes": nbytes,
               "copy_bytes": 8 * rows * half}
        for k, ts in times.items():
            med = statistics.median(ts)
            out[k + "_ms"] = round(med * 1e3, 4)
            out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
        out["build_gbs"] = round(nbytes / (out["build_ms"] / 1e3) / 1e9, 1)
        out["copy_gbs"] = round(out["copy_bytes"] / (out["copy_ms"] / 1e3) / 1e9, 1)
        out["build_of_copy"] = round(out["build_gbs"] / out["copy_gbs"], 3)
        i10.fill_(-2)
        fns["remove10"]()
        torch.cuda.synchronize()
        out["remove10_all_valid"] = bool(((i10 >= 0) & (i10 < N)).all())
        print(json.dumps(out), flush=True)
        del w, tree, a, b, ta, tb


if __name__ == "__main__":
    main()
