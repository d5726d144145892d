#!/usr/bin/env python3
"""Fingerprint of the assembly launch planner (laser_amd/csrc/asm_plan.h): which kernel and which launch plan every problem gets.

Two parts, both device-free:
  entry: laser_hip_plan_f32 over a grid of dense row-major f32 shapes, CU counts and modes, under ten option settings;
  host:  the problem lines of host_cases() through the host program tests/cpp/asm_plan_host.cpp (f64, B transposed, fused
         prologue / epilogue, batches, tile pins, forced kernels, the convolution classifier and its pixel cut, and the 64 bytes
         fill_sched makes of every plan).
Blocks of lines are stored as a sha256 and a histogram, a few hundred named cases in full: tests/golden/asm_plans_parent.json,
which tests/test_asm_plan_cpu.py recomputes and compares exactly.

  plan_fingerprint.py --host-exe EXE --write OUT.json     record
  plan_fingerprint.py --host-exe EXE --diff OTHER.json    compare with a recording; prints the first differing lines of each block
  plan_fingerprint.py --time                              seconds for the entry grid (minimum of five runs)
  plan_fingerprint.py --cases                             print the host program's input lines
"""
import argparse
import collections
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUS = (32, 64, 128, 256, 304)
MS = (1, 64, 257, 640, 1000, 1536, 1920, 2048, 3072, 3328, 4100, 5120, 6656, 8192)
NS = (96, 640, 1920, 3000, 4608, 8192)
KS = (1, 3, 64, 510, 512, 516, 2048, 8192)
SETTINGS = [("default", None, None), ("asm_plan=1", "asm_plan", 1), ("asm_plan=2", "asm_plan", 2), ("asm_plan=3", "asm_plan", 3),
            ("asm_plan=4", "asm_plan", 4), ("f32_asm=0", "f32_asm", 0), ("f32_asm=2", "f32_asm", 2), ("asm_wgs=64", "asm_wgs", 64),
            ("asm_slice=8", "asm_slice", 8), ("split_tail=0", "split_tail", 0)]
PLAN_NAMES = ("plain", "cut", "strided", "hybrid")
# the shapes test_launch_plans_scale_with_the_device_cu_count names: their eight outputs are stored in full
NAMED_ENTRY = [(cus, laser, *shape) for cus in (32, 64, 128, 256)
               for shape in [(8192, 8192, 8192), (4096, 4096, 4096), (4100, 4100, 4100), (3072, 3072, 3072), (2048, 2048, 2048), (1920, 1920, 1920)]
               for laser in (1, 0)] + [(256, 1, 512, 512, 512), (32, 1, 512, 512, 512)]


def sha(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def entry_blocks():
    """[(block name, [line per shape], histogram)]: 10 settings x 5 CU counts x 2 modes blocks of 672 shapes"""
    import laser_amd as la
    from laser_amd import _lib
    f = _lib.lib().laser_hip_plan_f32
    out = (C.c_int64 * 8)()
    blocks = []
    for name, opt, val in SETTINGS:
        old = la.get_option(opt) if opt else None
        try:
            if opt:
                la.set_option(opt, val)
            for cus in CUS:
                for laser in (1, 0):
                    lines, hist = [], collections.Counter()
                    for M in MS:
                        for N in NS:
                            for K in KS:
                                rc = f(M, N, K, laser, cus, out)
                                o = list(out)
                                lines.append("%d %d %d -> %d %s" % (M, N, K, rc, " ".join(map(str, o))))
                                hist["%d:%s" % (o[0], PLAN_NAMES[o[1]] if o[0] else "-")] += 1
                    blocks.append(("%s cus=%d laser=%d" % (name, cus, laser), lines, dict(sorted(hist.items()))))
        finally:
            if opt:
                la.set_option(opt, old)
    return blocks


def entry_named():
    from laser_amd import _lib
    f = _lib.lib().laser_hip_plan_f32
    out = (C.c_int64 * 8)()
    named = {}
    for cus, laser, M, N, K in NAMED_ENTRY:
        assert f(M, N, K, laser, cus, out) == 0
        named["cus=%d laser=%d %d %d %d" % (cus, laser, M, N, K)] = list(out)
    return named


# ---- the host program's problem lines -------------------------------------------------------------------------------------

def kv(**kw):
    return " ".join("%s=%s" % (k, v) for k, v in kw.items())


def host_cases():
    """[(block name, [input line]), ...]; blocks whose name starts with "named:" are stored in full"""
    B = collections.OrderedDict()

    def add(block, **kw):
        B.setdefault(block, []).append(kv(**kw))

    # f32: layouts (B transposed, fused prologue on A / B), both modes, a partition and the full chip
    for cus in (32, 256):
        for laser in (1, 0):
            for nt in (0, 1):
                for pre in (0, 1, 2):
                    for M in (64, 257, 1000, 1920, 3072, 4100, 8192):
                        for N in (96, 1920, 3000, 8192):
                            for K in (3, 64, 512, 513, 516, 2048):
                                add("f32 layouts", t="f32", cus=cus, laser=laser, nt=nt, preA=pre & 1, preB=pre >> 1, M=M, N=N, K=K)
    # every tile class pinned: every f32 row is reached (class x laser-order x B transposed x prologue)
    for tile in range(10):
        for laser in (1, 0):
            for nt in (0, 1):
                for pre in (0, 1):
                    for M, N, K in [(2048, 2048, 2048), (1920, 1920, 300), (4096, 4096, 4096), (300, 200, 1026)]:
                        add("named: f32 tile pins", t="f32", cus=256, laser=laser, tile=tile, nt=nt, preA=pre, M=M, N=N, K=K)
    # batches (grid y), negative and zero batch strides, the 65535 limit
    for batch in (2, 8, 65535, 65536):
        for laser in (1, 0):
            for M, N, K in [(256, 256, 1024), (1920, 1920, 1920), (64, 64, 64), (3072, 3072, 516)]:
                for nt in (0, 1):
                    add("f32 batches", t="f32", cus=256, laser=laser, batch=batch, nt=nt, M=M, N=N, K=K)
    for bs in ("bsA", "bsB", "bsC"):
        add("f32 batches", t="f32", cus=256, laser=1, batch=4, M=1920, N=1920, K=1920, **{bs: -1})
        add("f32 batches", t="f32", cus=256, laser=1, batch=4, M=1920, N=1920, K=1920, **{bs: 0})
    # fused epilogue: bias views, activations, beta != 0 (laser-order rows only), a column stride on C
    for laser in (1, 0):
        for bias in (0, 1):
            for act in (0, 1, 2):
                for beta in (0, 1):
                    for csC in (1, 2):
                        for M, N, K in [(4096, 4096, 4096), (1920, 1920, 1920), (3072, 3072, 512), (8192, 8192, 2048)]:
                            add("f32 fused epilogue", t="f32", cus=256, laser=laser, bias=bias, act=act, beta=beta, csC=csC, M=M, N=N, K=K)
    for k in ("rsBias", "csBias"):
        for v in (-1, 0, 0x3fffffff, 0x40000000):
            add("f32 fused epilogue", t="f32", cus=256, laser=1, bias=1, M=1920, N=1920, K=1920, **{k: v})
    add("f32 fused epilogue", t="f32", cus=256, laser=1, bias=1, batch=2, bsBias=8, M=1920, N=1920, K=1920)
    # options the entry point's grid leaves at their defaults or cannot combine with a layout
    shapes = [(8192, 8192, 8192), (4608, 4608, 4608), (6656, 6656, 6656), (3072, 3072, 3072), (1920, 1920, 1920), (4100, 4100, 516), (1000, 3000, 2048)]
    for opt, vals in (("plan", (1, 2, 3, 4)), ("wgs", (8, 64, 100, 5000)), ("slice", (4, 8)), ("split_tail", (0,)), ("f32_asm", (0, 2)),
                      ("group_m", (1, 2, 16)), ("noseed", (1,)), ("giveup", (1,))):
        for v in vals:
            for laser in (1, 0):
                for nt in (0, 1):
                    for M, N, K in shapes:
                        add("f32 options", t="f32", cus=256, laser=laser, nt=nt, M=M, N=N, K=K, **{opt: v})
    for plan in (2, 4):
        for wgs in (64, 96):
            for laser in (1, 0):
                for M, N, K in shapes:
                    add("f32 options", t="f32", cus=304, laser=laser, plan=plan, wgs=wgs, noseed=1, giveup=1, M=M, N=N, K=K)
    for kernel in range(72):      # option asm_kernel: any row forced, for f32 and for f64 problems
        for laser in (1, 0):
            for nt in (0, 1):
                add("forced kernels", t="f32", cus=256, laser=laser, nt=nt, kernel=kernel, M=2048, N=2048, K=2048)
                add("forced kernels", t="f32", cus=256, laser=laser, nt=nt, kernel=kernel, preB=1, M=2048, N=2048, K=2048)
                add("forced kernels", t="f64", cus=256, laser=laser, nt=nt, kernel=kernel, M=2048, N=2048, K=2048)
    # f64
    for cus in (32, 256):
        for laser in (1, 0):
            for nt in (0, 1):
                for beta in (0, 1):
                    for batch in (1, 4):
                        for M in (64, 257, 1000, 1920, 4100, 8192):
                            for N in (96, 1920, 3000, 8192):
                                for K in (2, 3, 64, 256, 258, 2048):
                                    add("f64 grid", t="f64", cus=cus, laser=laser, nt=nt, beta=beta, batch=batch, M=M, N=N, K=K)
    for opt, vals in (("plan", (1, 2, 3, 4)), ("wgs", (64,)), ("slice", (8,)), ("split_tail", (0,)), ("f64_asm", (0, 2)), ("group_m", (2,)),
                      ("tile", (2,)), ("bias", (1,)), ("act", (1,)), ("csC", (2,)), ("noseed", (1,))):
        for v in vals:
            for laser in (1, 0):
                for nt in (0, 1):
                    for M, N, K in [(8192, 8192, 8192), (4096, 4096, 4096), (3072, 3072, 3072), (1920, 1920, 1920), (1000, 3000, 2048), (640, 640, 64)]:
                        add("f64 options", t="f64", cus=256, laser=laser, nt=nt, M=M, N=N, K=K, **{opt: v})
    # both sides of every threshold.  kc: 512 / 513 (f32), 256 / 257 / 258 (f64)
    for laser in (1, 0):
        for K in (511, 512, 513, 514, 516):
            add("named: thresholds", t="f32", cus=256, laser=laser, M=4096, N=4096, K=K)
        for K in (254, 256, 257, 258):
            add("named: thresholds", t="f64", cus=256, laser=laser, M=4096, N=4096, K=K)
    # 5/8 (3/8 for 64-row tiles) of a round: 160 / 96 tiles at 256 CUs, 20 / 12 at 32, by forced kernel and by the model's own pick
    for t, k128, k64, side in (("f32", 2, 12, 128), ("f64", 16, 18, 128)):
        for cus, big, small in ((256, [(3, 53), (16, 10)], [(5, 19), (8, 12)]), (32, [(1, 19), (4, 5)], [(1, 11), (3, 4)])):
            for tm, tn in big:
                for batch in (1, 2):
                    add("named: thresholds", t=t, cus=cus, laser=1, kernel=k128, batch=batch, M=side * tm, N=side * tn, K=1024)
                    add("named: thresholds", t=t, cus=cus, laser=1, batch=batch, M=side * tm, N=side * tn, K=1024)
            for tm, tn in small:
                add("named: thresholds", t=t, cus=cus, laser=1, kernel=k64, M=64 * tm, N=64 * tn, K=1024)
                add("named: thresholds", t=t, cus=cus, laser=0, kernel=k64 + 1, M=64 * tm, N=64 * tn, K=1024)
    # 32-bit byte offsets: 4.0e9 on A and B, 2^31 on C and the bias view
    for t, el, rows in (("f32", 4, 256), ("f64", 8, 128)):
        edge = 4000000000 // (el * rows)
        for lda in (edge - 1, edge):
            add("named: thresholds", t=t, cus=256, laser=1, lda=lda, M=4096, N=4096, K=2048)
            add("named: thresholds", t=t, cus=256, laser=1, nt=1, ldb=lda, M=4096, N=4096, K=2048)
        edge = 4000000000 // (el * 2048)
        for ldb in (edge, edge + 1):
            add("named: thresholds", t=t, cus=256, laser=1, ldb=ldb, M=4096, N=4096, K=2048)
        edge = (1 << 31) // (el * 2048)      # ((M - 1) ldc + N) el > 2^31 with M - 1 = N = 2048: ldc + 1 > edge
        for ldc in (edge - 2, edge - 1, edge):
            add("named: thresholds", t=t, cus=256, laser=1, ldc=ldc, M=2049, N=2048, K=2048)
    for rs in (262142, 262143, 262144):      # the bias view: >= 2^31
        add("named: thresholds", t="f32", cus=256, laser=1, bias=1, rsBias=rs, csBias=1, M=2049, N=2048, K=2048)
    for M in (448, 512):                     # t * 8 * tn >= 4.0e9 on forced 64x64 tiles; fill_sched's own range
        add("named: thresholds", t="f32", cus=256, laser=1, kernel=12, M=M, N=512000, K=1024)
        add("named: thresholds", t="f64", cus=256, laser=1, kernel=18, M=M, N=512000, K=1024)
    for t in ("i32", "i64"):
        add("named: thresholds", t=t)
    # convolutions: the classifier, then the pixel cut, over the same geometries
    geoms = [(1, 1, 0), (3, 1, 1), (3, 2, 1), (5, 1, 2), (7, 2, 3)]
    for what in ("conv", "cut"):
        for cus in (32, 256):
            for laser in (1, 0):
                for k, s, p in geoms:
                    for Cin in (3, 64, 128):
                        for Cout in (32, 64, 96, 128, 192, 256, 512):
                            for HW in (14, 28, 56, 112, 224):
                                for batch in (1, 8, 32):
                                    if what == "cut" and (cus == 32 or batch == 8):
                                        continue
                                    add("conv classes" if what == "conv" else "conv pixel cuts", t=what, cus=cus, laser=laser, kH=k, kW=k, sH=s, sW=s,
                                        pH=p, pW=p, Cin=Cin, M=Cout, H=HW, W=HW, batch=batch)
    for k, s, p in geoms:                    # the reference's first layers: C_in = 3, in full
        for laser in (1, 0):
            for Cout in (64, 96, 256):
                for what in ("conv", "cut"):
                    add("named: conv first layers", t=what, cus=256, laser=laser, kH=k, kW=k, sH=s, sW=s, pH=p, pW=p, Cin=3, M=Cout, H=224, W=224, batch=32)
    for kH, kW in ((31, 1), (32, 1), (4, 8), (7, 7), (50, 1), (5, 10)):      # taps = 31 / 32 / 49 / 50
        for Cout in (128, 256):
            for laser in (1, 0):
                add("named: conv thresholds", t="conv", cus=256, laser=laser, kH=kH, kW=kW, pH=kH // 2, pW=kW // 2, Cin=16, M=Cout, H=56, W=56, batch=32)
    for Cout in (95, 96, 97, 191, 192, 193, 48, 49):      # the 0.75 padding rule, with and without f32_asm = 2; main launches of whole tiles
        for f32_asm in (1, 2):
            for N in (0, 3072):
                add("named: conv thresholds", t="conv", cus=256, laser=1, f32_asm=f32_asm, kH=3, kW=3, pH=1, pW=1, Cin=64, M=Cout, H=56, W=56, batch=32,
                    **({"N": N} if N else {}))
    for extra in (dict(alpha=2), dict(beta=1), dict(act=1), dict(act=2), dict(bias=1), dict(bias=1, bsBias=4), dict(f32_asm=0), dict(batch=65536),
                  dict(sH=0), dict(pH=256), dict(kH=9, H=4, pH=0), dict(coW=55), dict(N=3000), dict(batch=1), dict(batch=2), dict(batch=4)):
        args = dict(t="conv", cus=256, laser=1, kH=3, kW=3, sH=1, sW=1, pH=1, pW=1, Cin=64, M=64, H=56, W=56, batch=32)
        args.update(extra)
        add("named: conv thresholds", **args)
    return list(B.items())


def run_host(exe, blocks):
    """the host program's answer for every line: [(block, ["input -> output", ...])]"""
    lines = [ln for _, lns in blocks for ln in lns]
    r = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s: exit %d\n%s" % (exe, r.returncode, (r.stdout[-2000:] + r.stderr[-4000:])))
    got = r.stdout.splitlines()
    if len(got) != len(lines):
        raise RuntimeError("%s: %d answers for %d lines" % (exe, len(got), len(lines)))
    out, i = [], 0
    for name, lns in blocks:
        out.append((name, ["%s -> %s" % (a, b) for a, b in zip(lns, got[i:i + len(lns)])]))
        i += len(lns)
    return out


def host_row(line):
    """rows of the kernel table a host answer names: "pick=K ..." and, for convolutions, "walker=K" """
    rows = []
    for tok in line.split(" -> ")[1].split():
        if tok.startswith(("pick=", "walker=", "row=")) and not tok.endswith("=-1"):
            rows.append(int(tok.split("=")[1]))
    return rows


def fingerprint(host_exe):
    fp = {"entry": {"shapes_per_block": len(MS) * len(NS) * len(KS), "blocks": {}, "named": entry_named()}, "host": {"blocks": {}, "named": {}, "rows": {}}}
    for name, lines, hist in entry_blocks():
        fp["entry"]["blocks"][name] = {"sha256": sha(lines), "hist": hist}
    rows = collections.Counter()
    for name, lines in run_host(host_exe, host_cases()):
        fp["host"]["blocks"][name] = {"sha256": sha(lines), "lines": len(lines)}
        for ln in lines:
            rows.update(host_row(ln))
        if name.startswith("named:"):
            fp["host"]["named"][name] = lines
    fp["host"]["rows"] = {str(k): rows[k] for k in range(72)}
    return fp


def diff(fp, other, host_exe, limit=8):
    """what differs, block by block; for a differing block the first lines that changed cannot be read back from a hash, so the
    block's lines are printed with the two histograms (entry) or against the stored full lines (named host blocks)"""
    bad = 0
    entry_lines = None
    for name, blk in other["entry"]["blocks"].items():
        mine = fp["entry"]["blocks"].get(name)
        if mine == blk:
            continue
        bad += 1
        print("entry block %r differs" % name)
        if mine is None:
            continue
        keys = sorted(set(mine["hist"]) | set(blk["hist"]))
        print("  kernel:plan histogram (now, recorded): " + ", ".join("%s %d/%d" % (k, mine["hist"].get(k, 0), blk["hist"].get(k, 0))
                                                                      for k in keys if mine["hist"].get(k, 0) != blk["hist"].get(k, 0)))
        if entry_lines is None:
            entry_lines = {n: ls for n, ls, _ in entry_blocks()}
        for ln in entry_lines[name][:limit]:
            print("  now: " + ln)
    for key, want in other["entry"]["named"].items():
        if fp["entry"]["named"].get(key) != want:
            bad += 1
            print("entry %s: now %s, recorded %s" % (key, fp["entry"]["named"].get(key), want))
    for name, blk in other["host"]["blocks"].items():
        if fp["host"]["blocks"].get(name) == blk:
            continue
        bad += 1
        print("host block %r differs" % name)
        want, shown = other["host"]["named"].get(name), 0
        for i, ln in enumerate(fp["host"]["named"].get(name) or dict(run_host(host_exe, host_cases()))[name]):
            if want is None or i >= len(want) or want[i] != ln:
                print("  now:      " + ln)
                if want is not None and i < len(want):
                    print("  recorded: " + want[i])
                shown += 1
                if shown >= limit:
                    break
    if fp["host"]["rows"] != other["host"]["rows"]:
        bad += 1
        print("host rows picked: " + ", ".join("%s: %d/%d" % (k, fp["host"]["rows"][k], v) for k, v in other["host"]["rows"].items() if fp["host"]["rows"].get(k) != v))
    print("%d difference(s)" % bad)
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--host-exe", help="tests/cpp/asm_plan_host.cpp, built")
    ap.add_argument("--write")
    ap.add_argument("--diff")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--cases", action="store_true")
    a = ap.parse_args()
    if a.cases:
        for _, lines in host_cases():
            print("\n".join(lines))
        return 0
    if a.time:
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            n = sum(len(lines) for _, lines, _ in entry_blocks())
            ts.append(time.perf_counter() - t0)
        print(json.dumps({"plans": n, "seconds_min": min(ts), "seconds": ts}))
        return 0
    if not a.host_exe:
        ap.error("--host-exe is needed to record or compare")
    fp = fingerprint(a.host_exe)
    if a.write:
        with open(a.write, "w") as f:
            json.dump(fp, f, indent=0, sort_keys=True)
            f.write("\n")
    if a.diff:
        return 1 if diff(fp, json.load(open(a.diff)), a.host_exe) else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
