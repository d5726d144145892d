#!/usr/bin/env python3
"""laser_amd.sin / cos / sincos at 2^26 contiguous float32 elements beside tanh through laser_hip_act_f32_dev on the same
tensor, and a 2^26-element normal fill beside the uniform float32 fill, on preallocated device buffers, in one process after
warm-up, the entries interleaved and the order reversed every other round (the median, the minimum and the maximum of the
rounds are reported).  Arguments of sin / cos are uniform in [-8, 8) (the three-part reduction); `sin_big` is the same kernel
on arguments of 2^20 .. 2^30 (Payne-Hanek).  copy_strided_b32 (laser_amd.copyFrom) is the one-read, one-write HBM yardstick.

Each entry is set beside two floors: its HBM time, bytes / 6.3 TB/s (the achievable bandwidth of the MI355X), and its float64
VALU time, float64 operations / 39.3e12 per second (the 78.6 TFLOP/s vector float64 peak counts a fused multiply-add as two;
these kernels hold none, so an instruction is one operation).  The operation counts per element are the v_mul_f64 + v_add_f64
of the compiled kernels on the three-part path (llvm-objdump of the library; profiles/sincos/README.md lists them).

Before timing, 2^22 normal draws are compared with numpy's correctly rounded float32 square root through the model of
tests/normal_model.py (the device's sqrt is the one step of the fill that the compiler, not the header, defines).

One JSON line, and a table in markdown after it.  Event timings include launch overhead.
usage: sincos_throughput.py [iters = 20] [rounds = 6] [log2 of the element count = 26]"""
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import laser_amd  # noqa: E402

HBM = 6.3e12            # bytes per second, achievable
F64 = 39.3e12           # float64 multiplies or adds per second, vector units
# float64 operations per element on the three-part path, counted in the compiled gfx950 kernels
F64_OPS = {"sin": 43, "cos": 43, "sin_big": 43, "sincos": 43, "tanh": 40, "normal": 24.5, "uniform": 0, "copy": 0}
BYTES = {"sin": 8, "cos": 8, "sin_big": 8, "sincos": 12, "tanh": 8, "normal": 4, "uniform": 4, "copy": 8}


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def check_normal_bits(n=1 << 22):
    from tests import normal_model
    got = laser_amd.randomNormalTensor(n, 0.0, 1.0, seed=99, subseq=3, offset=1).to_numpy()
    want = normal_model.fill(n, 0.0, 1.0, 99, 3, 1)
    return int((got.view(np.uint32) != want.view(np.uint32)).sum())


def main():
    args = sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 20
    rounds = int(args[1]) if len(args) > 1 else 6
    n = 1 << (int(args[2]) if len(args) > 2 else 26)
    torch.cuda.set_device(0)
    mismatches = check_normal_bits()
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand((n,), device="cuda", generator=g) * 16 - 8
    xb = (torch.rand((n,), device="cuda", generator=g) * 1023 + 1) * 2.0 ** 20
    y, y2 = torch.empty_like(x), torch.empty_like(x)
    tx, ty = laser_amd.fromTorch(x), laser_amd.fromTorch(y)
    L = laser_amd.lib()
    from laser_amd.tensor import _stream
    dst = C.c_void_p(y.data_ptr())
    fns = {"sin": lambda: laser_amd.sin(x, out=y), "cos": lambda: laser_amd.cos(x, out=y), "sin_big": lambda: laser_amd.sin(xb, out=y),
           "sincos": lambda: laser_amd.sincos(x, out=(y, y2)), "tanh": lambda: laser_amd.activation(x, "tanh", out=y),
           "normal": lambda: L.laser_hip_random_normal_f32_dev(dst, n, 0.0, 1.0, 7, 0, 0, _stream()),
           "uniform": lambda: L.laser_hip_random_uniform_f32_dev(dst, n, 0.0, 1.0, 7, 0, 0, _stream()),
           "copy": lambda: laser_amd.copyFrom(ty, tx)}
    for fn in fns.values():       # warm up everything the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for r in range(rounds):
        order = list(fns.items())
        for k, fn in (order if r % 2 == 0 else order[::-1]):
            times[k].append(timed(fn, iters))
    out = {"case": "sincos", "n": n, "iters": iters, "rounds": rounds, "normal_bits_differing_of_2^22": mismatches}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k + "_ms"] = round(med * 1e3, 4)
        out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
        out[k + "_gbs"] = round(BYTES[k] * n / med / 1e9, 1)
        out[k + "_hbm_ms"] = round(BYTES[k] * n / HBM * 1e3, 4)
        out[k + "_f64_ms"] = round(F64_OPS[k] * n / F64 * 1e3, 4)
    print(json.dumps(out), flush=True)
    print("\n| entry | ms (min .. max) | GB/s | HBM floor ms | float64 VALU floor ms | time / tanh |\n|---|---|---|---|---|---|")
    for k in fns:
        lo, hi = out[k + "_ms_min_max"]
        print(f"| {k} | {out[k + '_ms']} ({lo} .. {hi}) | {out[k + '_gbs']} | {out[k + '_hbm_ms']} | {out[k + '_f64_ms']} | "
              f"{round(out[k + '_ms'] / out['tanh_ms'], 3)} |")


if __name__ == "__main__":
    main()
