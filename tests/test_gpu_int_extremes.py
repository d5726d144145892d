"""Integer GEMM with the int32 accumulator groups of the limb kernels at their documented bound (tests/int_extremes.py):
coherent same-sign extreme digits on both operands, K at, around and beyond the chunk that bounds a group, the value change at
and 5 elements before a chunk seam, every kernel path, against the closed form evaluated in Python integers.
Signed types run on device tensors, unsigned ones through the host-pointer entry points (the same kernels on the same bits)."""
import numpy as np
import pytest

from tests import int_extremes as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import laser_amd
    assert laser_amd.lib().laser_hip_arch().decode().startswith("gfx950")
    return laser_amd


def paths(la, n):
    """(name, enter, leave, check) for every kernel family of the width"""
    if n >= 32:
        mfma = la.set_i32_mfma if n == 32 else la.set_i64_mfma
        return [("assembly limb kernel", lambda: la.set_option("i32_asm", 2), lambda: la.set_option("i32_asm", 1),
                 lambda: la.get_option("last_i32_asm") != 0),
                ("compiler limb kernel", lambda: la.set_option("i32_asm", 0), lambda: la.set_option("i32_asm", 1),
                 lambda: la.get_option("last_i32_asm") == 0),
                ("VALU kernel", lambda: mfma(False), lambda: mfma(True), lambda: True)]
    return [("matrix cores", lambda: None, lambda: None, lambda: la.get_option("last_narrow_mfma") == 1),
            ("VALU kernel", lambda: la.set_option("narrow_mfma", 0), lambda: la.set_option("narrow_mfma", 1),
             lambda: la.get_option("last_narrow_mfma") == 0)]


def operands(case, colmajor):
    """A, B and a function giving a fresh C0 and reading the result back; device tensors for the signed types"""
    A, B, C0 = case.A(), case.B(), case.C0()
    if colmajor:                 # column-major A, B passed transposed (k-contiguous columns)
        A, B = np.asfortranarray(A), np.ascontiguousarray(B.T).T
    if case.dtype.kind == "u":
        return A, B, C0.copy, lambda c: c
    import torch
    dA = torch.from_numpy(np.ascontiguousarray(A.T)).cuda().t() if colmajor else torch.from_numpy(A).cuda()
    dB = torch.from_numpy(np.ascontiguousarray(B.T)).cuda().t() if colmajor else torch.from_numpy(B).cuda()
    dC0 = torch.from_numpy(C0).cuda()
    assert tuple(dA.stride()) == ((1, X.M) if colmajor else (case.K, 1))
    return dA, dB, dC0.clone, lambda c: c.cpu().numpy()


def check(la, dtype, K, colmajor=False):
    n = X.bits(dtype)
    pairs = X.scalars(n)
    for idx, K1 in enumerate(X.k1_list(n, K)):
        case = X.Case(dtype, K, K1)
        A, B, fresh, back = operands(case, colmajor)
        for alpha, beta in pairs[2 * (idx % 2):2 * (idx % 2) + 2]:      # (1, 0), (-1, 1) / (min, -1), the full-range pair
            want = case.closed_form(alpha, beta)
            for name, enter, leave, took in paths(la, n):
                enter()
                try:
                    C = fresh()
                    la.matmul(A, B, alpha, beta, C)
                    assert took(), f"{name} did not run: {np.dtype(dtype)} K={K} K1={K1}"
                finally:
                    leave()
                got = back(C)
                assert got.dtype == want.dtype
                bad = np.argwhere(got != want)
                assert bad.size == 0, (f"{name}: {np.dtype(dtype)} K={K} K1={K1} alpha={alpha} beta={beta} colmajor={colmajor}: "
                                       f"{len(bad)} elements differ, first at {tuple(bad[0])}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


CASES = [(dt, K) for dt in X.DTYPES for K in X.k_list(X.bits(dt))]


@pytest.mark.parametrize("dtype,K", CASES, ids=[f"{np.dtype(dt)}-{K}" for dt, K in CASES])
def test_coherent_extremes_against_the_closed_form(la, dtype, K):
    check(la, dtype, K)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=[str(np.dtype(dt)) for dt in X.DTYPES])
def test_coherent_extremes_column_major_a_transposed_b(la, dtype):
    check(la, dtype, X.CHUNK[X.bits(dtype)] + 1, colmajor=True)
