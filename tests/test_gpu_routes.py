"""Which kernel family each GEMM shape takes and the bits it produces, against the recording made before the routing moved into
gemm_route.cpp (tests/golden/routes_parent.json, made by scripts/route_fingerprint.py on an MI355X)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_every_route_and_every_result_is_the_recorded_one():
    """The fingerprint runs in a process of its own (the `last_*` diagnostics are process state and some rungs never reset them) and
    must print every recorded case, in order, with the same diagnostics and the same sha256 of C: none skipped, none filtered."""
    with open(os.path.join(ROOT, "tests", "golden", "routes_parent.json")) as f:
        want = json.load(f)
    assert len(want) == 34
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "scripts", "route_fingerprint.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert [g["case"] for g in got] == [w["case"] for w in want]
    for g, w in zip(got, want):
        assert g == w, w["case"]
