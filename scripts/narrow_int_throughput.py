#!/usr/bin/env python3
"""int8 / int16 GEMM throughput on the int8 matrix cores (packing pass included) beside the widen route in the same process:
cast to int32, the int32 GEMM, narrow the result.  Full-range random operands, device-resident.  One JSON line per (type, n):
Tint-op/s = 2 n^3 / time.  usage: narrow_int_throughput.py [iters = 10] [n ...] (default n: 8192 1920)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    sizes = [int(v) for v in sys.argv[2:]] or [8192, 1920]
    torch.cuda.set_device(0)
    for n in sizes:
        for dt, lo, hi in ((torch.int8, -128, 128), (torch.int16, -32768, 32768)):
            A = torch.randint(lo, hi, (n, n), dtype=dt, device="cuda")
            B = torch.randint(lo, hi, (n, n), dtype=dt, device="cuda")
            C = torch.empty((n, n), dtype=dt, device="cuda")
            C32 = torch.empty((n, n), dtype=torch.int32, device="cuda")

            def narrow():
                laser_amd.matmul(A, B, 1, 0, C)

            def widen():
                laser_amd.matmul(A.to(torch.int32), B.to(torch.int32), 1, 0, C32)
                C.copy_(C32)

            t_n = timed(narrow, iters)
            assert laser_amd.get_option("last_narrow_mfma") == 1
            ref = C.clone()
            t_w = timed(widen, iters)
            assert torch.equal(C, ref), "the widen route and the narrow kernel differ"
            ops = 2.0 * n ** 3
            print(json.dumps({"dtype": str(dt).replace("torch.", ""), "n": n, "narrow_ms": round(t_n * 1e3, 4),
                              "narrow_tops": round(ops / t_n / 1e12, 1), "widen_ms": round(t_w * 1e3, 4),
                              "widen_tops": round(ops / t_w / 1e12, 1), "speedup": round(t_w / t_n, 2)}), flush=True)


if __name__ == "__main__":
    main()
