"""The case table of tests/stream_order.py against include/laser_hip.h, without a device: every `_dev` entry point has a row
or a quoted exemption, and every decoy is a valid input of its operation."""
import os
import re

import numpy as np
import pytest

from tests import stream_order as SO
from tests.test_abi_cpu import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "laser_amd", "lib", "liblaser_hip.so")):
        g.build()
    import laser_amd
    return laser_amd


def test_every_dev_entry_point_has_a_row_or_a_quoted_exemption():
    declared = header_symbols()
    dev = {s for s in declared if s.endswith("_dev")}
    assert len(dev) == 115, len(dev)       # a new entry point changes this count, and needs a row
    named = {s for c in SO.CASES for s in c.symbols} | set(SO.EXEMPT)
    assert named <= declared, sorted(named - declared)
    assert {s for s in named if s.endswith("_dev")} == dev, (sorted(dev - named), sorted(named - dev))
    covered = {s for c in SO.CASES for s in c.symbols}
    assert not (covered & {s for s in SO.EXEMPT if s.endswith("_dev")}), "an exempted _dev entry point also has an asynchronous row"
    names = [c.name for c in SO.CASES]
    assert len(names) == len(set(names))


def test_every_exemption_quotes_the_header():
    text = open(os.path.join(ROOT, "include", "laser_hip.h")).read()
    flat = re.sub(r"\s+\*?\s*", " ", text)
    for name, sentence in SO.EXEMPT.items():
        assert sentence, name
        assert re.sub(r"\s+\*?\s*", " ", sentence) in flat, (name, sentence)
    # a row marked synchronous names only exempted entry points
    for c in SO.CASES:
        if c.sync:
            assert set(c.symbols) <= set(SO.EXEMPT), c.name


@pytest.mark.parametrize("case", SO.CASES + [SO.CONTROL_NULL_STREAM, SO.CONTROL_HOST_SYNC], ids=repr)
def test_the_decoy_is_a_valid_input_of_the_same_shapes(built, case):
    staged, decoy = case.build(1), case.build(2)
    assert list(staged) == list(decoy)
    for k in case.outputs + case.inplace + case.temps + case.host + tuple(case.rules):
        assert k in staged, (case.name, k)
    ops = case.operands(staged)
    assert ops or case.host, case.name
    differs = False
    for k in ops + list(case.host):
        a, b = np.asarray(staged[k]), np.asarray(decoy[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (case.name, k, a.shape, b.shape, a.dtype, b.dtype)
        differs = differs or a.tobytes() != b.tobytes()
    for k in ops:
        assert np.asarray(staged[k]).tobytes() != np.asarray(decoy[k]).tobytes(), (case.name, k, "the decoy equals the staged operand")
        for which, bufs in (("staged", staged), ("decoy", decoy)):
            assert SO.check_rule(k, bufs[k], case.rules.get(k)) is None, (case.name, which, SO.check_rule(k, bufs[k], case.rules.get(k)))
    assert differs, case.name
    for k in case.outputs + case.temps:
        assert np.asarray(staged[k]).shape == np.asarray(decoy[k]).shape


def test_check_rule_sees_an_invalid_decoy():
    assert SO.check_rule("x", np.array([1.0, np.nan], np.float32), None)
    assert SO.check_rule("ids", np.array([0, 7], np.int32), ("ids", 7))
    assert SO.check_rule("ids", np.array([-1, 3], np.int32), ("ids", 7))
    assert SO.check_rule("a", np.array([[1, 3, 2]], np.int32), "sorted")
    assert SO.check_rule("w", np.array([1.0, 0.0], np.float32), "positive")
    assert SO.check_rule("cdf", np.array([[0.5, 0.4]], np.float32), "cdf")
    assert SO.check_rule("u", np.array([0.5, 1.0], np.float32), "unit")
    assert SO.check_rule("u", np.array([0.0, 0.5], np.float32), "unit") is None
