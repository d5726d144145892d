#!/usr/bin/env python3
"""The uniform fills and the sampler's self-drawing entry points, on preallocated device buffers through the C entry points, in
one process after warm-up, the entries of a group interleaved (fill, memset, torch.rand, fill, ...; the median round is
reported, min and max are the spread the script itself saw).
Fills, float32 and float64, 2^20, 2^24 and 2^28 elements, lo = 0, hi = 1:
  - fill:    laser_hip_random_uniform_{f32,f64}_dev; GB/s counts the bytes written
  - memset:  hipMemsetAsync of the same bytes (through laser_hip_storage_set_zero, which is that call): the write-bandwidth
             yardstick
  - torch:   Tensor.uniform_() on a preallocated tensor of the same shape and element type, the kernel torch.rand runs after
             its allocation: the vendor's Philox
Sampler, at the shapes of profiles/sampler/sampler_throughput.jsonl (rows of 50 000, 128 and 4096 rows), 1 and 10 draws per row:
  - rng:      laser_hip_sampler_sample_rng_f32_dev
  - two_step: laser_hip_random_uniform_f32_dev into a (rows, m) buffer, then laser_hip_sampler_sample_f32_dev
One JSON line per fill shape and per sampler shape.  Event timings include launch overhead.
usage: random_throughput.py [rounds = 7] [out.jsonl]"""
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
SEED, SUBSEQ = 0x0123456789ABCDEF, 7


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def interleaved(fns, iters, rounds):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(timed(fn, iters))
    out = {}
    for k, ts in times.items():
        out[k + "_ms"] = round(statistics.median(ts) * 1e3, 5)
        out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 5), round(max(ts) * 1e3, 5)]
    return out


def main():
    args = sys.argv[1:]
    rounds = int(args[0]) if len(args) > 0 else 7
    sink = open(args[1], "w") if len(args) > 1 else None
    torch.cuda.set_device(0)
    L = laser_amd.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc):
        assert rc == 0, L.laser_hip_last_error()

    def emit(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    for sfx, dt in (("f32", torch.float32), ("f64", torch.float64)):
        entry = getattr(L, f"laser_hip_random_uniform_{sfx}_dev")
        for log2n in (20, 24, 28):
            n = 1 << log2n
            dst, ref = torch.empty(n, device="cuda", dtype=dt), torch.empty(n, device="cuda", dtype=dt)
            nbytes = n * dst.element_size()
            iters = max(10, min(1000, (1 << 34) // nbytes))
            fns = {"fill": lambda: ok(entry(p(dst), n, 0.0, 1.0, SEED, SUBSEQ, 0, st())),
                   "memset": lambda: ok(L.laser_hip_storage_set_zero(p(ref), nbytes, st())),
                   "torch": lambda: ref.uniform_()}
            out = {"what": "fill", "dtype": sfx, "n": n, "bytes": nbytes, "iters": iters, "rounds": rounds}
            out.update(interleaved(fns, iters, rounds))
            for k in fns:
                out[k + "_gbs"] = round(nbytes / (out[k + "_ms"] / 1e3) / 1e9, 1)
            out["fill_of_memset"] = round(out["memset_ms"] / out["fill_ms"], 3)
            out["fill_of_torch"] = round(out["torch_ms"] / out["fill_ms"], 3)
            plan = (C.c_int64 * 4)()
            ok(L.laser_hip_random_plan(n, dst.element_size() // 4, 0, 0, 256, plan))
            out["plan"] = list(plan)
            out["in_range"] = bool(((dst >= 0) & (dst < 1)).all())
            emit(out)
            del dst, ref

    g = torch.Generator(device="cuda").manual_seed(0)
    for rows in (128, 4096):
        elems = sampling.tree_elems(N)
        w = torch.rand((rows, N), device="cuda", generator=g)
        w /= w.sum(1, keepdim=True)
        tree = torch.empty((rows, elems), device="cuda")
        ok(L.laser_hip_sampler_build_f32_dev(p(tree), elems, p(w), N, rows, N, st()))
        out = {"what": "sampler", "rows": rows, "n": N, "iters": 50, "rounds": rounds}
        for m in (1, 10):
            u = torch.empty((rows, m), device="cuda")
            ia = torch.empty((rows, m), device="cuda", dtype=torch.int32)
            ib = torch.empty((rows, m), device="cuda", dtype=torch.int32)

            def two_step():
                ok(L.laser_hip_random_uniform_f32_dev(p(u), rows * m, 0.0, 1.0, SEED, SUBSEQ, 5, st()))
                ok(L.laser_hip_sampler_sample_f32_dev(p(ib), p(tree), elems, p(u), rows, N, m, st()))

            fns = {f"rng{m}": lambda: ok(L.laser_hip_sampler_sample_rng_f32_dev(p(ia), p(tree), elems, SEED, SUBSEQ, 5, rows, N, m, st())),
                   f"two_step{m}": two_step}
            out.update(interleaved(fns, 50, rounds))
            out[f"same_indices{m}"] = bool((ia == ib).all())
        emit(out)
        del w, tree


if __name__ == "__main__":
    main()
