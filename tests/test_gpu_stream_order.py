"""Every `_dev` entry point issued while its stream is blocked (tests/stream_order.py): the call must return before the gate
opens, and the results, the operands updated in place and their guard elements must have the bits of the synchronised run --
in the buffers after the host has waited AND in clones queued on the same stream with no host wait.  Cases with scratch, a
workspace or more than one launch run a second time beside the same operation on another stream.  The harness first proves
that it can see: the stream pairs it uses are probed, and two broken calls must be reported, each for its own reason."""
import pytest

from tests import stream_order as SO

pytestmark = pytest.mark.gpu

T_HOST = {}     # family -> the largest host time of one synchronised call, seconds


@pytest.fixture(scope="module")
def la():
    import torch
    import laser_amd
    assert torch.cuda.is_available()
    return laser_amd


def test_the_probe_finds_independent_streams_and_the_spin_is_calibrated(la):
    import torch
    s, s2 = SO.streams()
    ticks = SO.ticks_per_ms()
    print(f"STREAM_ORDER ticks_per_ms = {ticks:.1f}")
    assert ticks > 0
    assert SO.probe(s, torch.cuda.default_stream()), "probe(S, NULL stream)"
    assert SO.probe(s, s2), "probe(S1, S2)"
    # the gate itself: closed right after it is queued, open once the stream has been waited for
    gate = SO.close_gate(s, SO.GATE_MIN_MS)
    closed = not gate.query()
    s.synchronize()
    assert closed and gate.query()


def test_control_a_launch_on_the_null_stream_is_reported_as_wrong_bits(la):
    with pytest.raises(SO.StreamOrderError) as e:
        SO.run_gated(SO.CONTROL_NULL_STREAM, la)
    assert e.value.kind == "bits", str(e.value)


def test_control_a_host_wait_inside_the_call_is_reported_as_an_open_gate(la):
    with pytest.raises(SO.StreamOrderError) as e:
        SO.run_gated(SO.CONTROL_HOST_SYNC, la)
    assert e.value.kind == "gate-open" and "gate open on return" in str(e.value), str(e.value)


@pytest.mark.parametrize("case", SO.CASES, ids=repr)
def test_gated_producer(la, case):
    try:
        SO.run_gated(case, la, T_HOST)
    finally:
        print(f"STREAM_ORDER t_host {case.family} {case.name} max so far {T_HOST.get(case.family, 0.0) * 1e3:.3f} ms")


@pytest.mark.parametrize("case", [c for c in SO.CASES if c.scratch], ids=repr)
def test_two_streams(la, case):
    SO.run_two_streams(case, la)


def test_report_the_host_times(la):
    for family, t in sorted(T_HOST.items()):
        print(f"STREAM_ORDER largest t_host {family}: {t * 1e3:.3f} ms (gate {max(SO.GATE_MIN_MS, SO.GATE_FACTOR * t * 1e3):.0f} ms)")
    assert all(SO.GATE_FACTOR * t * 1e3 <= SO.GATE_MAX_MS for t in T_HOST.values())
