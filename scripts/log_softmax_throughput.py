#!/usr/bin/env python3
"""laser_amd.log, logsumexp, log_softmax and the softmax cross-entropy (loss alone; loss and gradient) beside their yardsticks
on the same preallocated device buffers, in one process after warm-up, the entries interleaved and the order reversed every
other round (the minimum and the median of the rounds are reported):
  - log at 2^26 elements beside laser_amd.exp (the same bytes through lexp), copy_strided_b32 (laser_amd.copyFrom: the
    one-read, one-write HBM yardstick) and torch.log;
  - the row calls at the shapes of profiles/softmax/ (8192 x 1024, 8192 x 4096, 4096 x 8192: a row read once; 64 x 2^20: long
    rows) beside laser_amd.softmax (log_softmax moves the same bytes through the same lane mapping), the copy, and
    torch.log_softmax / torch.logsumexp for context.
One JSON line per case.  GB/s counts the bytes a call must move: 8 per element for log, softmax, log_softmax, the copy and
loss + gradient; 4 per element for logsumexp and the loss alone (one read; the per-row output is noise).  Event timings include
launch overhead.  "plan" is laser_hip_softmax_rows_plan of the shape: {kernel code, workgroups, LDS bytes}.
usage: log_softmax_throughput.py [iters = 20] [rounds = 6] [case ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import laser_amd  # noqa: E402

CASES = {"log_2^26": ("log", 1, 1 << 26), "rows_8192x1024": ("rows", 8192, 1024), "rows_8192x4096": ("rows", 8192, 4096),
         "rows_4096x8192": ("rows", 4096, 8192), "rows_64x2^20": ("rows", 64, 1 << 20)}


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
    names = args[2:] or list(CASES)
    torch.cuda.set_device(0)
    L = laser_amd.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ok(rc):
        assert rc == 0, L.laser_hip_last_error()

    for name in names:
        kind, rows, n = CASES[name]
        out = {"case": name, "rows": rows, "n": n, "iters": iters, "rounds": rounds}
        if kind == "log":
            x = torch.rand((rows, n), device="cuda", generator=g) * 40 + 1e-3           # positive: llog's main path
            xe = x - 20                                                                 # lexp's usual range
            y = torch.empty_like(x)
            tx, ty = laser_amd.fromTorch(x), laser_amd.fromTorch(y)
            fns = {"log": lambda: laser_amd.log(x, out=y), "exp": lambda: laser_amd.exp(xe, out=y),
                   "copy": lambda: laser_amd.copyFrom(ty, tx), "torch_log": lambda: torch.log(x, out=y)}
            nbytes = {k: 8 * rows * n for k in fns}
            base = "exp"
        else:
            x = torch.rand((rows, n), device="cuda", generator=g) * 40 - 20
            y = torch.empty_like(x)
            per = torch.empty((rows,), device="cuda")
            lab = torch.randint(0, n, (rows,), device="cuda", dtype=torch.int32, generator=g)
            tx, ty = laser_amd.fromTorch(x), laser_amd.fromTorch(y)
            plan = (C.c_int64 * 3)()
            ok(L.laser_hip_softmax_rows_plan(rows, n, 1, plan))
            out["plan"] = list(plan)
            fns = {"logsumexp": lambda: ok(L.laser_hip_logsumexp_rows_f32_dev(p(per), 1, p(x), n, rows, n, st())),
                   "log_softmax": lambda: ok(L.laser_hip_log_softmax_rows_f32_dev(p(y), n, p(x), n, rows, n, st())),
                   "xent_loss": lambda: ok(L.laser_hip_softmax_xent_rows_f32_dev(p(per), 1, None, n, p(x), n, p(lab), rows, n, 1.0, st())),
                   "xent_loss_grad": lambda: ok(L.laser_hip_softmax_xent_rows_f32_dev(p(per), 1, p(y), n, p(x), n, p(lab), rows, n, 1.0, st())),
                   "softmax": lambda: ok(L.laser_hip_softmax_rows_f32_dev(p(y), n, p(x), n, rows, n, st())),
                   "copy": lambda: laser_amd.copyFrom(ty, tx),
                   "torch_log_softmax": lambda: torch.log_softmax(x, dim=1, out=y),
                   "torch_logsumexp": lambda: torch.logsumexp(x, dim=1, out=per)}
            nbytes = {k: 8 * rows * n for k in fns}
            for k in ("logsumexp", "xent_loss", "torch_logsumexp"):
                nbytes[k] = 4 * rows * n
            base = "softmax"
        for fn in fns.values():       # warm up every shape the timed window uses
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for r in range(rounds):
            order = list(fns.items())
            for k, fn in (order if r % 2 == 0 else order[::-1]):
                times[k].append(timed(fn, iters))
        for k, ts in times.items():
            med = statistics.median(ts)
            out[k + "_ms"] = round(med * 1e3, 4)
            out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
            out[k + "_gbs"] = round(nbytes[k] / med / 1e9, 1)
        for k in fns:
            if k != base and not k.startswith("torch") and k != "copy":
                out[f"{k}_time_of_{base}"] = round(out[k + "_ms"] / out[base + "_ms"], 3)
        print(json.dumps(out), flush=True)
        del x, y, tx, ty


if __name__ == "__main__":
    main()
