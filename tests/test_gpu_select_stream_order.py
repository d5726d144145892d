"""Stream order and host asynchrony of the `_dev` entry points of include/laser_hip_select.h: one row per entry point, built
with the case machinery of tests/stream_order.py (the same decoy rule, the same gated-producer check).  The rows live here and
not in that module's table, which is pinned to include/laser_hip.h; tests/test_select_cpu.py holds them against the header
without a device."""
import numpy as np
import pytest

from tests import stream_order as SO

pytestmark = pytest.mark.gpu

CASES = []


def _topk_case():
    rows, n, k = 5, 8200, 50            # the streaming mapping: five passes over the row behind the gate

    def build(seed):
        x = SO._f(SO._rng(seed, 130), (rows, n), lo=-4, hi=4)
        return {"x": x, "vals": np.zeros((rows, k), np.float32), "idx": np.zeros((rows, k), np.int32),
                "small": np.zeros((rows, k), np.int32)}

    def call(la, b):
        L, s = SO._L(), SO._st()
        SO._ok(L.laser_hip_topk_rows_f32_dev(SO._ptr(b["vals"]), k, SO._ptr(b["idx"]), k, SO._ptr(b["x"]), n, rows, n, k, 1, s))
        SO._ok(L.laser_hip_topk_rows_f32_dev(None, k, SO._ptr(b["small"]), k, SO._ptr(b["x"]), n, rows, n, k, 0, s))

    CASES.append(SO.Case("select_topk", "select", ["laser_hip_topk_rows_f32_dev"], build, call, ("vals", "idx", "small")))


def _argmax_case():
    rows, n = 37, 1000

    def build(seed):
        x = SO._f(SO._rng(seed, 131), (rows, n), lo=-4, hi=4)
        return {"x": x, "idx": np.zeros((rows,), np.int32), "val": np.zeros((rows,), np.float32), "amin": np.zeros((rows,), np.int32)}

    def call(la, b):
        L, s = SO._L(), SO._st()
        SO._ok(L.laser_hip_argmax_rows_f32_dev(SO._ptr(b["idx"]), 1, SO._ptr(b["val"]), 1, SO._ptr(b["x"]), n, rows, n, 1, s))
        SO._ok(L.laser_hip_argmax_rows_f32_dev(SO._ptr(b["amin"]), 1, None, 1, SO._ptr(b["x"]), n, rows, n, 0, s))

    CASES.append(SO.Case("select_argmax", "select", ["laser_hip_argmax_rows_f32_dev"], build, call, ("idx", "val", "amin")))


def _take_case():
    rows, m, num = 9, 300, 70

    def build(seed):
        r = SO._rng(seed, 132)
        return {"src": r.integers(0, 1 << 20, (rows, m)).astype(np.int32), "j": r.integers(0, m, (rows, num)).astype(np.int32),
                "out": np.zeros((rows, num), np.int32)}

    def call(la, b):
        SO._ok(SO._L().laser_hip_take_rows_i32_dev(SO._ptr(b["out"]), num, SO._ptr(b["src"]), m, SO._ptr(b["j"]), num, rows, m, num, SO._st()))

    CASES.append(SO.Case("select_take_rows", "select", ["laser_hip_take_rows_i32_dev"], build, call, ("out",), rules={"j": ("ids", m)}))


def _sample_case():
    """the whole of sample_top_k behind one gate: top-k, softmax, cumsum, the draw and the gather, nothing waited for"""
    rows, n, k, num = 4, 3000, 40, 8

    def build(seed):
        r = SO._rng(seed, 133)
        return {"logits": SO._f(r, (rows, n), lo=-6, hi=6), "seed": np.int64(77 + seed), "ids": np.zeros((rows, num), np.int32)}

    def call(la, b):
        # (the generator, not a buffer of uniform numbers: the mirror checks a buffer's range on the host)
        SO._copy_out(la, b["ids"], la.sample_top_k(b["logits"], k, num, rng=la.Rng(int(b["seed"]), 3, 5)))

    CASES.append(SO.Case("select_sample_top_k", "select", ["laser_hip_topk_rows_f32_dev", "laser_hip_take_rows_i32_dev"], build, call,
                         ("ids",), host=("seed",)))


_topk_case()
_argmax_case()
_take_case()
_sample_case()


@pytest.fixture(scope="module")
def la():
    import torch
    import laser_amd
    assert torch.cuda.is_available()
    return laser_amd


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_gated_producer(la, case):
    SO.run_gated(case, la)
