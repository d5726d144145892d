#!/usr/bin/env python3
"""The row cumsum and the inverse-CDF sampler at the reference's benchmark shape (bench_multinomial_samplers.nim: rows of
50 000 probabilities; 128 rows there, 4096 here to fill the device) and on one row of 2^24 (the chain-bound case), beside the
F+tree on the same weights -- the benchmark's comparison, on the device.  Preallocated device buffers through the C entry
points, in one process after warm-up, the entries interleaved (cumsum, copy, cdf_draw1, ..., cumsum, ...; the median round is
reported):
  - cumsum:        laser_hip_cumsum_f32_dev; GB/s counts 8 bytes per element (read once, written once)
  - copy:          copy_strided_b32 (laser_amd.copyFrom) of the same bytes: the HBM yardstick
  - cdf_draw1:     cumsum + 1 draw per row (laser_hip_cdf_sample_f32_dev)
  - cdf_remove10:  10 draws per row without replacement (laser_hip_cdf_sample_remove_f32_dev: 10 scans) on a scratch copy
                   of the weights that is not refreshed between calls: after all timed calls a row has lost about a thousand
                   of its 50 000 elements, the work of every call is the same
  - ftree_draw1:   laser_hip_sampler_build_f32_dev + 1 draw;   ftree_remove10: build + 10 removals
Random weights (normalised rows), uniforms from torch.rand.  One JSON line per shape.  Event timings include launch overhead.
The line carries "run": LH_SCAN_RUN of the library that was loaded; --lib loads a diagnostic build (another run).
usage: scan_throughput.py [--lib path/to/liblaser_hip.so] [--cumsum-only] [iters = 20] [rounds = 5] [rows:n ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402
from laser_amd import _lib, sampling  # noqa: E402


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
    if args and args[0] == "--lib":
        _lib.LIB_PATH = os.path.abspath(args[1])
        args = args[2:]
    only = bool(args) and args[0] == "--cumsum-only"
    args = args[1:] if only else args
    iters = int(args[0]) if len(args) > 0 else 20
    rounds = int(args[1]) if len(args) > 1 else 5
    shapes = [tuple(int(v) for v in a.split(":")) for a in args[2:]] or [(128, 50000), (4096, 50000), (1, 1 << 24)]
    torch.cuda.set_device(0)
    L = laser_amd.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    for rows, n in shapes:
        plan = (C.c_int64 * 4)()
        assert L.laser_hip_cumsum_plan(rows, n, 4, 0, plan) == 0
        big = (C.c_int64 * 4)()
        assert L.laser_hip_cumsum_plan(1, 1 << 24, 4, 0, big) == 0
        run = (1 << 24) // big[3] // 256              # the run of the loaded library: 2^24 / tiles / 256 lanes
        elems = sampling.tree_elems(n)
        w = torch.rand((rows, n), device="cuda", generator=g)
        w /= w.sum(1, keepdim=True)
        cdf, scratch, b = torch.empty_like(w), w.clone(), torch.empty_like(w)
        tree = torch.empty((rows, elems), device="cuda")
        ta, tb = laser_amd.fromTorch(w), laser_amd.fromTorch(b)
        u1 = torch.rand((rows, 1), device="cuda", generator=g)
        u10 = torch.rand((rows, 10), device="cuda", generator=g)
        i1 = torch.empty((rows, 1), device="cuda", dtype=torch.int32)
        i10 = torch.empty((rows, 10), device="cuda", dtype=torch.int32)
        p = lambda t: C.c_void_p(t.data_ptr())
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def ok(rc):
            assert rc == 0, L.laser_hip_last_error()

        def cumsum():
            ok(L.laser_hip_cumsum_f32_dev(p(cdf), n, p(w), n, rows, n, st()))

        def cdf_draw1():
            cumsum()
            ok(L.laser_hip_cdf_sample_f32_dev(p(i1), p(cdf), n, p(u1), rows, n, 1, st()))

        def cdf_remove10():
            ok(L.laser_hip_cdf_sample_remove_f32_dev(p(i10), p(scratch), n, p(cdf), n, p(u10), rows, n, 10, st()))

        def build():
            ok(L.laser_hip_sampler_build_f32_dev(p(tree), elems, p(w), n, rows, n, st()))

        def ftree_draw1():
            build()
            ok(L.laser_hip_sampler_sample_f32_dev(p(i1), p(tree), elems, p(u1), rows, n, 1, st()))

        def ftree_remove10():
            build()
            ok(L.laser_hip_sampler_sample_remove_f32_dev(p(i10), p(tree), elems, p(u10), rows, n, 10, st()))

        fns = {"cumsum": cumsum, "copy": lambda: laser_amd.copyFrom(tb, ta)}
        if not only:
            fns.update({"cdf_draw1": cdf_draw1, "cdf_remove10": cdf_remove10, "ftree_draw1": ftree_draw1, "ftree_remove10": ftree_remove10})
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, iters))
        nbytes = 8 * rows * n
        out = {"rows": rows, "n": n, "run": run, "iters": iters, "rounds": rounds, "plan": list(plan), "bytes": nbytes}
        for k, ts in times.items():
            med = statistics.median(ts)
            out[k + "_ms"] = round(med * 1e3, 4)
            out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
        out["cumsum_gbs"] = round(nbytes / (out["cumsum_ms"] / 1e3) / 1e9, 1)
        out["copy_gbs"] = round(nbytes / (out["copy_ms"] / 1e3) / 1e9, 1)
        out["cumsum_of_copy"] = round(out["cumsum_gbs"] / out["copy_gbs"], 3)
        cumsum()
        torch.cuda.synchronize()
        out["cdf_monotone"] = bool((cdf[:, 1:] >= cdf[:, :-1]).all())
        if not only:
            i10.fill_(-2)
            scratch.copy_(w)
            cdf_remove10()
            torch.cuda.synchronize()
            out["remove10_all_valid"] = bool(((i10 >= 0) & (i10 < n)).all())
        print(json.dumps(out), flush=True)
        del w, cdf, scratch, b, tree, ta, tb


if __name__ == "__main__":
    main()
