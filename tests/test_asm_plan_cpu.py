"""The launch planner of the assembly kernels (laser_amd/csrc/asm_plan.h over asm_kernels.h) makes the recorded choices, without a
device: tests/golden/asm_plans_parent.json holds, from the commit before the planner moved into its own headers, every answer of
laser_hip_plan_f32 over a grid of shapes, CU counts, modes and option settings, and the answers of the planner's own functions to
the problem lines of scripts/plan_fingerprint.py (f64, B transposed, fused prologue and epilogue, batches, tile pins, forced kernels,
the convolution classifier, its pixel cut, the scheduler block of every plan) -- as a sha256 per block of lines, a histogram, and
several hundred lines in full.  `python scripts/plan_fingerprint.py --host-exe EXE --diff tests/golden/asm_plans_parent.json` shows
what moved."""
import importlib.util
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")
CSRC = os.path.join(ROOT, "laser_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "asm_plans_parent.json")
PLANNER_HEADERS = ("asm_plan.h", "asm_kernels.h", "gemm_args.h")


@pytest.fixture(scope="module")
def fp():
    if not os.path.exists(SO):
        import __graft_entry__ as g
        g.build()
    spec = importlib.util.spec_from_file_location("plan_fingerprint", os.path.join(ROOT, "scripts", "plan_fingerprint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) < 256 * 1024
    return json.load(open(GOLDEN))


def test_entry_point_plans_are_the_recorded_ones(fp, golden):
    import laser_amd as la
    before = {opt: la.get_option(opt) for _, opt, _ in fp.SETTINGS if opt}
    blocks = fp.entry_blocks()
    assert {opt: la.get_option(opt) for opt in before} == before          # every option is put back
    assert len(blocks) == 100 == len(golden["entry"]["blocks"]) and golden["entry"]["shapes_per_block"] == 672
    for name, lines, hist in blocks:
        assert len(lines) == 672, name
        want = golden["entry"]["blocks"][name]
        assert hist == want["hist"], (name, "kernel:plan histogram")
        assert fp.sha(lines) == want["sha256"], name
    # all four plan kinds under the default settings, and the shapes test_launch_plans_scale_with_the_device_cu_count names in full
    kinds = {k.split(":")[1] for name, _, hist in blocks if name.startswith("default") for k in hist}
    assert kinds == {"-", "plain", "cut", "strided", "hybrid"}
    assert fp.entry_named() == golden["entry"]["named"] and len(golden["entry"]["named"]) == len(fp.NAMED_ENTRY) == 50


def test_planner_headers_have_no_hip_dependency():
    for h in PLANNER_HEADERS:
        text = open(os.path.join(CSRC, h)).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert "hip/" not in code and not re.search(r"\bhip[A-Z]\w*", code), h
        assert not re.search(r"\bstd::atomic\b|\bthread_local\b|\bg_\w+", code), h
    assert '#include "gemm_args.h"' in open(os.path.join(CSRC, "common.h")).read()


def test_planner_as_a_host_program_under_the_sanitizers(fp, golden, tmp_path):
    """g++ alone builds the planner (no HIP header, nothing to link: it reads no global), ASan and UBSan see its integer arithmetic on
    the edge lines, and every answer is the recorded one"""
    from laser_amd import _lib
    import ctypes as C
    exe = tmp_path / "asm_plan_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "asm_plan_host.cpp"), "-o", str(exe)], check=True)
    cases = fp.host_cases()
    got = fp.run_host(str(exe), cases)
    assert sorted(n for n, _ in got) == sorted(golden["host"]["blocks"])
    rows = {k: 0 for k in range(72)}
    for name, lines in got:
        want = golden["host"]["blocks"][name]
        assert len(lines) == want["lines"], name
        if name.startswith("named:"):
            for a, b in zip(lines, golden["host"]["named"][name]):
                assert a == b, name
        assert fp.sha(lines) == want["sha256"], name
        for ln in lines:
            for r in fp.host_row(ln):
                rows[r] += 1
    assert sum(len(v) for v in golden["host"]["named"].values()) >= 300
    assert min(rows.values()) >= 1, [k for k, v in rows.items() if v == 0]      # every row of the kernel table is picked somewhere
    assert {str(k): v for k, v in rows.items()} == golden["host"]["rows"]
    # the dense row-major f32 lines under default options: the library's entry point gives the same answers
    f = _lib.lib().laser_hip_plan_f32
    out = (C.c_int64 * 8)()
    plans = {"plain": 0, "cut": 1, "strided": 2, "hybrid": 3}
    dense = 0
    for ln in dict(got)["f32 layouts"]:
        q, ans = ln.split(" -> ")
        kv = dict(t.split("=") for t in q.split())
        if kv["nt"] != "0" or kv["preA"] != "0" or kv["preB"] != "0":
            continue
        dense += 1
        assert f(int(kv["M"]), int(kv["N"]), int(kv["K"]), int(kv["laser"]), int(kv["cus"]), out) == 0
        if ans == "pick=-1":
            assert out[0] == 0, ln
            continue
        a = dict(t.split("=") for t in ans.split() if "=" in t)
        tm, tn = (int(v) for v in a["tiles"].split("x"))
        slices = int(a["rem"].split(",")[2]) if a["plan"] == "hybrid" else int(a["P"])
        assert list(out)[:7] == [1 + int(a["pick"]), plans[a["plan"]], int(a["G"]), slices, tm * tn, tm, tn], ln
    assert dense == 2 * 2 * 7 * 4 * 6
