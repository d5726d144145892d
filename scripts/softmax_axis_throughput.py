#!/usr/bin/env python3
"""laser_amd.softmax(t, axis=) along the middle axis of (outer, n, inner) operands beside three yardsticks on the same device
buffers, in one process after warm-up and interleaved (axis, composed, copy, torch, axis, ...; the median round is reported):
  - composed: what the library offered before the axis form -- transpose2D_batched into preallocated scratch (outer matrices
    n x inner -> inner x n), softmax over the rows, transpose2D_batched back: six matrix passes over HBM;
  - copy: copy_strided_b32 of the same operand (laser_amd.copyFrom): the one-read, one-write yardstick;
  - torch: torch.softmax(dim=1) into the same output buffer.
One JSON line per shape; GB/s counts 8 bytes per element for every entry.  The composed route and the axis form must give
the same bits, and the script checks that before it times anything.  Judged: the first four shapes; (1, 4096, 64) is the
few-strips case, reported only.  Event timings include launch overhead (profiles/softmax/README.md).
usage: softmax_axis_throughput.py [iters = 20] [rounds = 5] [shape-name ...]"""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402
from laser_amd import primitives  # noqa: E402

SHAPES = {"1x4096x4096": (1, 4096, 4096, True), "32x256x3136": (32, 256, 3136, True), "1x1024x8192": (1, 1024, 8192, True),
          "1x65536x256": (1, 65536, 256, True), "1x4096x64": (1, 4096, 64, False)}


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
    names = args[2:] or list(SHAPES)
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in names:
        outer, n, inner, judged = SHAPES[name]
        x = (torch.rand((outer, n, inner), device="cuda", generator=g) * 40 - 20)
        y = torch.empty_like(x)
        y2 = torch.empty_like(x)
        s1 = torch.empty((outer * inner, n), device="cuda")      # scratch of the composed route, allocated once
        s2 = torch.empty_like(s1)
        tx, ty = laser_amd.fromTorch(x), laser_amd.fromTorch(y)

        def composed(dst=y):
            primitives.transpose2D_batched(s1, x, outer, n, inner)
            laser_amd.softmax(s1, out=s2)
            primitives.transpose2D_batched(dst, s2, outer, inner, n)

        fns = {"axis": lambda: laser_amd.softmax(x, out=y, axis=1), "composed": composed, "copy": lambda: laser_amd.copyFrom(ty, tx),
               "torch": lambda: torch.softmax(x, dim=1, out=y)}
        composed(y2)
        fns["axis"]()
        kernel = laser_amd.get_option("last_softmax_kernel")
        torch.cuda.synchronize()
        same = bool(torch.equal(y.view(torch.int32), y2.view(torch.int32)))
        for fn in fns.values():       # warm up every shape the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                times[k].append(timed(fn, iters))
        nbytes = 8 * outer * n * inner
        out = {"shape": [outer, n, inner], "judged": judged, "bytes": nbytes, "iters": iters, "rounds": rounds, "kernel": kernel,
               "same_bits_as_composed": same}
        p = (ctypes.c_int64 * 4)()
        if laser_amd.lib().laser_hip_softmax_axis_plan(outer, n, inner, 1, 256, p) == 0:
            out["cw"], out["workgroups"] = p[1], p[2]
        for k, ts in times.items():
            med = statistics.median(ts)
            out[k + "_ms"] = round(med * 1e3, 4)
            out[k + "_gbs"] = round(nbytes / med / 1e9, 1)
            out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
        out["composed_over_axis"] = round(out["composed_ms"] / out["axis_ms"], 3)      # > 1: the axis form is faster
        out["axis_of_copy"] = round(out["axis_gbs"] / out["copy_gbs"], 3)
        out["axis_of_torch"] = round(out["axis_gbs"] / out["torch_gbs"], 3)
        print(json.dumps(out), flush=True)
        del x, y, y2, s1, s2, tx, ty


if __name__ == "__main__":
    main()
