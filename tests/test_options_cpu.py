"""laser_hip_set_option / laser_hip_get_option against the recording of the two if-chains they replaced (tests/golden/
options_parent.json, made by scripts/record_options.py on a machine without a GPU): every name, every probe value, value for value;
and the names the library accepts against the names include/laser_hip.h documents.  No device needed."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import record_options  # noqa: E402


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")):
        g.build()
    import laser_amd
    return laser_amd


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "options_parent.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def probed(built):
    """the probe in a process of its own: the diagnostics are process state, and this process may have run anything before.  (The probe
    puts every option it wrote back in a `finally`, and the child's state ends with the child.)"""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "scripts", "record_options.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads(r.stdout)


def test_table_names_are_the_recorded_names(recorded):
    names = record_options.option_names()
    assert len(names) == len(set(names)) == 51
    assert set(names) == set(recorded)


def test_every_option_behaves_as_recorded(built, recorded, probed):
    assert set(probed) == set(recorded)
    want = json.loads(json.dumps(recorded))
    if built.lib().laser_hip_device_count() > 0:
        # the one diagnostic that asks the device: -1 without one (the recording), 0 with one in a process that launched nothing
        want["asm_fixup_timeouts"]["get"] = [0, 0]
    for name in sorted(recorded):
        print(name, probed[name])
        assert probed[name] == want[name], name
    assert sum(1 for r in probed.values() if r["set"][0][1] == 0) == 34
    assert all(r["restored"] for r in probed.values() if "restored" in r)


def test_no_option_is_writable_but_unreadable(probed):
    for name, r in probed.items():
        if r["set"][0][1] == 0:
            assert r["get"][0] == 0, f"{name} can be set but not read"
    # and in the source: a row without a reader does not exist (the reader is every row's second field)
    src = open(record_options.CAPI).read()
    rows = re.findall(r'^\s*\{"(\w+)",\s*(\S+)', src, re.M)
    assert len(rows) == 51 and all(second not in ("nullptr,", "nullptr}") for _, second in rows)


def test_header_option_block_lists_exactly_the_accepted_names():
    h = open(os.path.join(ROOT, "include", "laser_hip.h")).read()
    start = h.index("/* ---- options:")
    block = h[start:h.index("*/", start)]
    documented = set(re.findall(r'"(\w+)"', block))
    accepted = set(record_options.option_names())
    assert accepted - documented == set(), "accepted by the library, missing from the header's option block"
    assert documented - accepted == set(), "quoted in the header's option block, unknown to the library"


def test_unknown_and_null_keep_their_error_texts(built):
    import ctypes as C
    L = built.lib()
    v = C.c_int64()
    assert L.laser_hip_set_option(b"no_such_option", 1) == 1 and L.laser_hip_last_error() == b"set_option: unknown option 'no_such_option'"
    assert L.laser_hip_set_option(b"last_f32_asm", 1) == 1 and L.laser_hip_last_error() == b"set_option: unknown option 'last_f32_asm'"
    assert L.laser_hip_get_option(b"no_such_option", C.byref(v)) == 1 and L.laser_hip_last_error() == b"get_option: unknown option 'no_such_option'"
    assert L.laser_hip_set_option(None, 1) == 1 and L.laser_hip_last_error() == b"set_option: null name"
    assert L.laser_hip_get_option(b"f32_asm", None) == 1 and L.laser_hip_last_error() == b"get_option: null argument"
    assert L.laser_hip_get_option(None, C.byref(v)) == 1 and L.laser_hip_last_error() == b"get_option: null argument"
