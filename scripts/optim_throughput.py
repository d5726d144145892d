#!/usr/bin/env python3
"""laser_amd.sgd_step (with momentum), adam_step and grad_norm beside their yardsticks on the same preallocated device buffers,
in one process after warm-up, the entries interleaved and the order reversed every other round (the median, the minimum and
the maximum of the rounds are reported):
  - one tensor of 2^24 and of 2^26 elements: the achieved bytes per second beside copy_strided_b32 (laser_amd.copyFrom), the
    one-read, one-write HBM yardstick of the other profiles.  Bytes a call must move per element: SGD with momentum 20 (w and m
    read and written, g read), Adam 28 (w, m, v read and written, g read), grad_norm 4, the copy 8;
  - a parameter list shaped like a perceptron's (matrices, biases, gamma / beta), 64 and 256 tensors of 64 .. 65536 elements:
    one multi-tensor call against one forEach launch per tensor with the same body (the route before the optimizer steps
    existed), and torch.optim's fused SGD / Adam on the same shapes as context only: other operation orders, other bits;
  - grad_norm on both lists, beside the norm torch.nn.utils.clip_grad_norm_ computes (torch._foreach_norm, then the norm of
    the norms; nothing comes back to the host there either).
One JSON line per case, appended to the output file, and a table in markdown after them.  Event timings include launch
overhead: for the lists that is the point.
usage: optim_throughput.py [iters = 20] [rounds = 6] [out = profiles/optim/optim_throughput.jsonl]"""
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

F = np.float32
BYTES = {"sgd_momentum": 20, "adam": 28, "grad_norm": 4, "sgd_momentum_c_abi": 20, "adam_c_abi": 28, "grad_norm_c_abi": 4, "adam_holder": 28, "copy": 8, "foreach_sgd_momentum": 20, "foreach_adam": 28,
         "torch_fused_sgd": 20, "torch_fused_adam": 28, "torch_grad_norm": 4}
ADAM_BODY = "m = b1 * m + omb1 * g; v = b2 * v + (omb2 * g) * g; w = w - lr * ((m / bc1) / (sqrtf(v / bc2) + eps))"
SGD_BODY = "m = mu * m + g; w -= lr * m"


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def list_lens(count, seed):
    """`count` lengths of 64 .. 65536 elements, log-uniform: a few matrices among many vectors, as a deep perceptron's"""
    rng = np.random.default_rng(seed)
    return [int(n) for n in np.exp(rng.uniform(np.log(64), np.log(65536), count))]


def run_case(name, lens, iters, rounds, with_foreach):
    g = torch.Generator(device="cuda").manual_seed(len(lens))
    w, gr, m, v = ([torch.randn((n,), device="cuda", generator=g) * s for n in lens] for s in (1.0, 0.01, 0.01, 0.0))
    v = [t.abs() + 1e-4 for t in v]
    total = sum(lens)
    bc1, bc2 = laser_amd.adam_bias_correction(0.9, 10), laser_amd.adam_bias_correction(0.999, 10)
    fns = {"sgd_momentum": lambda: laser_amd.sgd_step(w, gr, m, lr=1e-3, mu=0.9),
           "adam": lambda: laser_amd.adam_step(w, gr, m, v, 10, lr=1e-3),
           "grad_norm": lambda: laser_amd.grad_norm(gr, 1.0)}
    holder = laser_amd.Adam(w, lr=1e-3)      # keeps the pointer lists of w, m and v: a step walks the gradients only
    fns["adam_holder"] = lambda: holder.step(gr)
    # the same three calls on the C-ABI with the pointer lists built once: what a caller that keeps its lists pays (the Python
    # functions walk every list on every call, a cost per tensor that forEach pays as well)
    count, clens, arrs = laser_amd.optim._lists("optim_throughput", [("w", w), ("g", gr), ("m", m), ("v", v)])
    L, stream = laser_amd.lib(), laser_amd.tensor._stream()
    dn, dc = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    fns["sgd_momentum_c_abi"] = lambda: L.laser_hip_sgd_step_f32_dev(arrs[0], arrs[1], arrs[2], clens, count, 1e-3, 0.9, 0.0, 0, 1.0, None, stream)
    fns["adam_c_abi"] = lambda: L.laser_hip_adam_step_f32_dev(arrs[0], arrs[1], arrs[2], arrs[3], clens, count, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0,
                                                              bc1, bc2, 1.0, None, stream)
    fns["grad_norm_c_abi"] = lambda: L.laser_hip_grad_norm_f32_dev(C.c_void_p(dn.data_ptr()), C.c_void_p(dc.data_ptr()), arrs[1], clens, count,
                                                                   1.0, stream)
    if len(lens) == 1:
        src, dst = laser_amd.fromTorch(w[0]), laser_amd.fromTorch(torch.empty_like(w[0]))
        fns["copy"] = lambda: laser_amd.copyFrom(dst, src)
    if with_foreach:
        sp = dict(lr=F(1e-3), mu=F(0.9))
        ap = dict(lr=F(1e-3), b1=F(0.9), b2=F(0.999), omb1=F(1) - F(0.9), omb2=F(1) - F(0.999), bc1=F(bc1), bc2=F(bc2), eps=F(1e-8))

        def foreach_sgd():
            for a, b, c in zip(w, gr, m):
                laser_amd.forEach(SGD_BODY, w=a, g=b, m=c, writable=("w", "m"), params=sp)

        def foreach_adam():
            for a, b, c, d in zip(w, gr, m, v):
                laser_amd.forEach(ADAM_BODY, w=a, g=b, m=c, v=d, writable=("w", "m", "v"), params=ap)
        fns["foreach_sgd_momentum"], fns["foreach_adam"] = foreach_sgd, foreach_adam
    tw = [t.clone().requires_grad_(True) for t in w]
    for t, gg in zip(tw, gr):
        t.grad = gg.clone()
    tsgd = torch.optim.SGD(tw, lr=1e-3, momentum=0.9, fused=True)
    tadam = torch.optim.Adam(tw, lr=1e-3, fused=True)
    fns["torch_fused_sgd"], fns["torch_fused_adam"] = tsgd.step, tadam.step
    tg = [t.grad for t in tw]
    fns["torch_grad_norm"] = lambda: torch.linalg.vector_norm(torch.stack(torch._foreach_norm(tg)))
    for fn in fns.values():       # warm up everything the timed window uses
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for r in range(rounds):
        order = list(fns.items())
        for k, fn in (order if r % 2 == 0 else order[::-1]):
            times[k].append(timed(fn, iters))
    plans = {}
    for what, key in ((0, "sgd"), (1, "adam"), (2, "grad_norm")):
        out4 = (C.c_int64 * 4)()
        assert L.laser_hip_optim_plan(what, (C.c_int64 * len(lens))(*lens), len(lens), out4) == 0
        plans[key] = list(out4)
    out = {"case": name, "tensors": len(lens), "elements": total, "iters": iters, "rounds": rounds, "plan": plans}
    for k, ts in times.items():
        med = statistics.median(ts)
        out[k + "_us"] = round(med * 1e6, 2)
        out[k + "_us_min_max"] = [round(min(ts) * 1e6, 2), round(max(ts) * 1e6, 2)]
        out[k + "_gbs"] = round(BYTES[k] * total / med / 1e9, 1)
    if "copy" in fns:
        for k in fns:
            if k != "copy":     # per byte moved, so that 20, 28 and 4 bytes per element compare with the copy's 8
                out[f"{k}_rate_of_copy"] = round(out[k + "_gbs"] / out["copy_gbs"], 3)
    if with_foreach:
        for k in ("adam", "sgd_momentum"):
            out[k + "_speedup_over_foreach"] = round(out[f"foreach_{k}_us"] / out[k + "_us"], 2)
            out[k + "_c_abi_speedup_over_foreach"] = round(out[f"foreach_{k}_us"] / out[k + "_c_abi_us"], 2)
    return out, list(fns)


def main():
    args = sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 20
    rounds = int(args[1]) if len(args) > 1 else 6
    path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "optim", "optim_throughput.jsonl")
    torch.cuda.set_device(0)
    cases = [("one tensor 2^24", [1 << 24], False), ("one tensor 2^26", [1 << 26], False),
             ("list of 64", list_lens(64, 64), True), ("list of 256", list_lens(256, 256), True)]
    table = []
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for name, lens, with_foreach in cases:
            out, keys = run_case(name, lens, iters * (10 if len(lens) > 1 else 1), rounds, with_foreach)   # short calls: longer windows
            line = json.dumps(out)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            table.append((out, keys))
            torch.cuda.empty_cache()
    print("\n| case | entry | us (min .. max) | GB/s | GB/s / copy |\n|---|---|---|---|---|")
    for out, keys in table:
        for k in keys:
            lo, hi = out[k + "_us_min_max"]
            print(f"| {out['case']} ({out['elements']} elements) | {k} | {out[k + '_us']} ({lo} .. {hi}) | {out[k + '_gbs']} | "
                  f"{out.get(k + '_rate_of_copy', '')} |")


if __name__ == "__main__":
    main()
