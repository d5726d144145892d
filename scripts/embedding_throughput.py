#!/usr/bin/env python3
"""laser_amd.embedding, embedding_group and embedding_backward at tokens 16384 / 131072, vocab 32768 / 131072, dim 1024 / 4096,
with ids drawn uniformly and from a Zipf-like law (weights 1 / (rank + 1), through the library's own multinomial), beside
their yardsticks on the same preallocated device buffers, in one process after warm-up, the entries interleaved and the order
reversed every other round (the median, the minimum and the maximum of the rounds are reported):
  - forward: the gather into a preallocated y; copy: the device-to-device copy of the same tokens * dim * 4 bytes;
  - group: the grouping alone (tokens per second);
  - grad: embedding_backward grouping by itself; grad_grouped: the same with the group given;
  - memset: writing dW once (zero fill of its bytes); read_dy: one read of dY by bias_grad (no dz), the dense-gradient
    interface's own reader.  memset + read_dy is the floor that interface allows: dW is written once and dY read once;
  - torch_backward: torch's own embedding backward (autograd of torch.nn.functional.embedding, int64 ids) on the same
    operands, as context only: atomic float adds in arrival order, other bits from run to run.  Nothing in the product calls it.
One JSON line per case, and a table in markdown after them.  Event timings include launch overhead.
usage: embedding_throughput.py [iters = 10] [rounds = 4]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import laser_amd  # noqa: E402

TOKENS, VOCABS, DIMS = (16384, 131072), (32768, 131072), (1024, 4096)
ENTRIES = ("forward", "copy", "group", "grad", "grad_grouped", "memset", "read_dy", "torch_backward")


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / 1e3 / iters


def draw_ids(tokens, vocab, law, g):
    if law == "uniform":
        return torch.randint(0, vocab, (tokens,), device="cuda", generator=g, dtype=torch.int32)
    w = (1.0 / torch.arange(1, vocab + 1, device="cuda", dtype=torch.float32)).reshape(1, vocab)
    ids = laser_amd.multinomial(w, tokens, replacement=True, rng=laser_amd.Rng(tokens + vocab))
    return torch.from_numpy(ids.to_numpy().reshape(-1)).cuda()


def main():
    args = sys.argv[1:]
    iters = int(args[0]) if len(args) > 0 else 10
    rounds = int(args[1]) if len(args) > 1 else 4
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    L = laser_amd.lib()
    table = []
    for tokens in TOKENS:
        for vocab in VOCABS:
            for dim in DIMS:
                for law in ("uniform", "zipf"):
                    idx = draw_ids(tokens, vocab, law, g)
                    counts = np.bincount(idx.cpu().numpy(), minlength=vocab)
                    w = torch.randn((vocab, dim), device="cuda", generator=g)
                    dy = torch.randn((tokens, dim), device="cuda", generator=g)
                    y, y2, dw = torch.empty_like(dy), torch.empty_like(dy), torch.empty_like(w)
                    group = laser_amd.embedding_group(idx, vocab)
                    wt = w.clone().requires_grad_(True)
                    yt = torch.nn.functional.embedding(idx.long(), wt)
                    fns = {"forward": lambda: laser_amd.embedding(w, idx, out=y),
                           "copy": lambda: y2.copy_(y),
                           "group": lambda: laser_amd.embedding_group(idx, vocab),
                           "grad": lambda: laser_amd.embedding_backward(dy, idx, vocab, out=dw),
                           "grad_grouped": lambda: laser_amd.embedding_backward(dy, idx, vocab, out=dw, group=group),
                           "memset": lambda: dw.zero_(),
                           "read_dy": lambda: laser_amd.bias_grad(dy, dz=False),
                           "torch_backward": lambda: torch.autograd.grad(yt, wt, dy, retain_graph=True)}
                    for fn in fns.values():       # warm up everything the timed window uses
                        for _ in range(2):
                            fn()
                    torch.cuda.synchronize()
                    times = {k: [] for k in fns}
                    for r in range(rounds):
                        order = list(fns.items())
                        for k, fn in (order if r % 2 == 0 else order[::-1]):
                            times[k].append(timed(fn, iters))
                    out = {"case": "embedding", "tokens": tokens, "vocab": vocab, "dim": dim, "ids": law, "iters": iters, "rounds": rounds,
                           "ids_used": int((counts > 0).sum()), "max_count": int(counts.max()), "ids_over_32": int((counts > 32).sum()),
                           "kernels": [L.laser_hip_embedding_last_kernel(k) for k in (0, 1, 2, 3)]}
                    for k, ts in times.items():
                        out[k + "_ms"] = round(statistics.median(ts) * 1e3, 4)
                        out[k + "_ms_min_max"] = [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]
                    out["forward_gbs"] = round(2 * tokens * dim * 4 / out["forward_ms"] / 1e6, 1)
                    out["copy_gbs"] = round(2 * tokens * dim * 4 / out["copy_ms"] / 1e6, 1)
                    out["forward_rate_of_copy"] = round(out["copy_ms"] / out["forward_ms"], 3)
                    out["group_mtokens_per_s"] = round(tokens / out["group_ms"] / 1e3, 1)
                    out["floor_ms"] = round(out["memset_ms"] + out["read_dy_ms"], 4)
                    out["grad_over_floor"] = round(out["grad_ms"] / out["floor_ms"], 2)
                    out["grad_grouped_over_floor"] = round(out["grad_grouped_ms"] / out["floor_ms"], 2)
                    print(json.dumps(out), flush=True)
                    table.append(out)
                    del w, dy, y, y2, dw, wt, yt, fns, group
                    torch.cuda.empty_cache()
    print("\n| tokens | vocab | dim | ids | max count | forward ms (/ copy) | group ms (Mtok/s) | grad ms | grouped ms | floor ms "
          "(memset + read) | grad / floor | torch ms |\n|---|---|---|---|---|---|---|---|---|---|---|---|")
    for o in table:
        print(f"| {o['tokens']} | {o['vocab']} | {o['dim']} | {o['ids']} | {o['max_count']} | {o['forward_ms']} ({o['forward_rate_of_copy']}) | "
              f"{o['group_ms']} ({o['group_mtokens_per_s']}) | {o['grad_ms']} | {o['grad_grouped_ms']} | {o['floor_ms']} "
              f"({o['memset_ms']} + {o['read_dy_ms']}) | {o['grad_over_floor']} | {o['torch_backward_ms']} |")


if __name__ == "__main__":
    main()
