#!/usr/bin/env python3
"""Which kernel family each GEMM shape takes, and the bits it produces: one JSON line per case.

    python scripts/route_fingerprint.py                 # print the fingerprint (needs the MI355X)
    python scripts/route_fingerprint.py --write PATH    # record it (tests/golden/routes_parent.json was made this way)

A fixed list of the smallest shapes that reach each rung of the GEMM routing (gemm_route.cpp), walked in a fixed order in a process
that has not used the library before: the `last_*` diagnostics are process state and some rungs never reset them, so a line depends
on the lines before it.  After each call: every `last_*` option except the forEach / reduction / softmax ones, and the sha256 of C's
bytes.  Inputs come from numpy.random.RandomState(seed), whose stream numpy keeps stable.  Every option a case sets is put back.
tests/test_gpu_routes.py compares the output with the recording, exactly.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAST = ["last_f32_config", "last_f32_asm", "last_f64_asm", "last_i32_asm", "last_narrow_mfma", "last_split", "last_conv_tail",
        "last_asm_wgs", "last_asm_rem", "last_asm_slices", "last_asm_group_m"]
NARROW_MAX_K = 16384      # laser_amd/csrc/common.h


def operands(seed, dtype, M, N, K, batch=None):
    rs = np.random.RandomState(seed)
    lead = () if batch is None else (batch,)
    if np.dtype(dtype).kind == "f":
        return [rs.uniform(-1, 1, lead + s).astype(dtype) for s in ((M, K), (K, N))]
    info = np.iinfo(dtype)
    return [rs.randint(info.min, info.max, size=lead + s, dtype=dtype) for s in ((M, K), (K, N))]


def main(out=sys.stdout):
    """print one line per case; returns the list of them"""
    import torch
    import laser_amd as la

    seed = [1000]
    lines = []

    def emit(name, C):
        torch.cuda.synchronize()
        host = C.cpu().numpy() if isinstance(C, torch.Tensor) else C
        line = {"case": name, "last": {n: la.get_option(n) for n in LAST},
                "sha256": hashlib.sha256(np.ascontiguousarray(host).tobytes()).hexdigest()}
        lines.append(line)
        out.write(json.dumps(line, sort_keys=True) + "\n")
        out.flush()

    def dev(name, dtype, M, N, K, options=(), fast=False, pre=0):
        """one device-resident product under `options`, each put back afterwards"""
        seed[0] += 1
        A, B = (torch.from_numpy(x).cuda() for x in operands(seed[0], dtype, M, N, K))
        before = [(o, la.get_option(o)) for o, _ in options]
        try:
            for o, v in options:
                la.set_option(o, v)
            if fast:
                la.set_float_mode(1)
            emit(name, la.matmul(A, B, pre=pre))
        finally:
            la.set_float_mode(0)
            for o, v in before:
                la.set_option(o, v)

    f32 = np.float32
    dev("f32 4x512x600 skinny", f32, 4, 512, 600)
    seed[0] += 1
    A, B = (torch.from_numpy(x).cuda() for x in operands(seed[0], f32, 32, 32, 32, batch=8))
    C = torch.zeros((8, 32, 32), dtype=torch.float32, device="cuda")
    la.gemm_strided_batched(8, 32, 32, 32, 1.0, A, 32, 1, 1024, B, 32, 1, 1024, 0.0, C, 32, 1, 1024)
    emit("f32 8 x 32x32x32 small", C)
    dev("f32 256x256x2048 slice-parallel", f32, 256, 256, 2048)
    dev("f32 640x640x640 assembly", f32, 640, 640, 640)
    dev("f32 640x640x640 f32_asm=0", f32, 640, 640, 640, [("f32_asm", 0)])
    dev("f32 1028x512x512 peeled rows", f32, 1028, 512, 512)
    dev("f32 640x640x64 relu(A) f32_asm=1", f32, 640, 640, 64, [("f32_asm", 1)], pre=la.PRE_RELU_A)
    dev("f32 640x640x64 relu(A) f32_asm=0", f32, 640, 640, 64, [("f32_asm", 0)], pre=la.PRE_RELU_A)
    dev("f32 640x640x640 FAST", f32, 640, 640, 640, fast=True)
    seed[0] += 1
    A, B = operands(seed[0], f32, 128, 128, 128)
    emit("f32 128x128x128 host pointers", la.matmul(A, B))

    f64 = np.float64
    dev("f64 4x512x300", f64, 4, 512, 300)
    dev("f64 256x256x1024", f64, 256, 256, 1024)
    dev("f64 640x640x320", f64, 640, 640, 320)
    dev("f64 64x64x64 f64_mfma=0", f64, 64, 64, 64, [("f64_mfma", 0)])

    for t in (np.int32, np.int64):
        n = np.dtype(t).name
        dev(f"{n} 4x512x64", t, 4, 512, 64)
        dev(f"{n} 32x32x32", t, 32, 32, 32)
        dev(f"{n} 256x256x64", t, 256, 256, 64)
        dev(f"{n} 256x256x64 i32_asm=2", t, 256, 256, 64, [("i32_asm", 2)])
        dev(f"{n} 256x256x8200 i32_asm=2", t, 256, 256, 8200, [("i32_asm", 2)])
    for t in (np.int8, np.int16):
        n = np.dtype(t).name
        dev(f"{n} 4x512x64", t, 4, 512, 64)
        dev(f"{n} 32x32x32", t, 32, 32, 32)
        dev(f"{n} 256x256x64", t, 256, 256, 64)
        dev(f"{n} 128x128x{NARROW_MAX_K + 8}", t, 128, 128, NARROW_MAX_K + 8)

    # pre-packed operands: the host form (self-contained buffers + the device panel cache) and the device form
    M, N, K = 300, 200, 100
    seed[0] += 1
    A, B = operands(seed[0], f32, M, N, K)
    na, nb = la.gemm_prepackA_mem_required(f32, M, N, K), la.gemm_prepackB_mem_required(f32, M, N, K)
    pa, pb = la.aligned_host_buffer(na), la.aligned_host_buffer(nb)
    la.gemm_prepackA(pa, M, N, K, A, K, 1)
    la.gemm_prepackB(pb, M, N, K, B, N, 1)
    C = np.zeros((M, N), f32)
    la.gemm_packed(M, N, K, 1.0, pa, pb, 0.0, C, N, 1)
    emit("f32 300x200x100 pre-packed host", C)
    la.gemm_prepack_release(pa)
    la.gemm_prepack_release(pb)
    dpa = torch.empty(na, dtype=torch.uint8, device="cuda")
    dpb = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    dC = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    la.gemm_prepackA(dpa, M, N, K, dA, K, 1)
    la.gemm_prepackB(dpb, M, N, K, dB, N, 1)
    la.gemm_packed(M, N, K, 1.0, dpa, dpb, 0.0, dC, N, 1)
    emit("f32 300x200x100 pre-packed device", dC)
    return lines


if __name__ == "__main__":
    result = main()
    if len(sys.argv) == 3 and sys.argv[1] == "--write":
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])), exist_ok=True)
        with open(sys.argv[2], "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(x, sort_keys=True) for x in result) + "\n]\n")
