"""GEMM for every integer element type on the GPU: int8 / uint8 / int16 / uint16 on the int8 matrix cores
(gemm_narrow_mfma.hip) and on the VALU / streaming kernels, uint32 / uint64 on the int32 / int64 entry points.  Every case is
bit-exact against an exact reference: A*B from float64 products of 16-bit limbs (each limb product below 2^32, so every partial
sum is an integer below 2^53 up to K = 2^21), reduced mod 2^n, alpha and beta applied in wrapping 64-bit arithmetic."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NARROW = [np.int8, np.uint8, np.int16, np.uint16]
ALL = NARROW + [np.uint32, np.uint64]


@pytest.fixture(scope="module")
def la():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import laser_amd
    assert laser_amd.lib().laser_hip_arch().decode().startswith("gfx950")
    return laser_amd


def bits(dtype):
    return np.dtype(dtype).itemsize * 8


def rand(rng, shape, dtype):
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, shape, dtype=dtype, endpoint=True)


def as_u64(x):
    """the n-bit pattern of every element, zero-extended"""
    return x.view(np.dtype(f"u{x.dtype.itemsize}")).astype(np.uint64)


def exact_product(A, B):
    """A @ B mod 2^n as uint64 (n = the element width): sum over 16-bit limb products p + q < n / 16"""
    n = bits(A.dtype)
    a, b = as_u64(A), as_u64(B)
    nl = max(1, n // 16)
    out = np.zeros((A.shape[0], B.shape[1]), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for p in range(nl):
            ap = ((a >> np.uint64(16 * p)) & np.uint64(0xFFFF)).astype(np.float64)
            for q in range(nl - p):
                bq = ((b >> np.uint64(16 * q)) & np.uint64(0xFFFF)).astype(np.float64)
                out += (ap @ bq).astype(np.uint64) << np.uint64(16 * (p + q))
    return out


def reference(A, B, alpha, beta, C0):
    n = bits(A.dtype)
    mask = np.uint64((1 << n) - 1) if n < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    al, be = np.uint64(alpha % (1 << n)), np.uint64(beta % (1 << n))
    with np.errstate(over="ignore"):
        v = al * exact_product(A, B)
        if beta % (1 << n):
            v = v + be * as_u64(C0)
    u = np.dtype(f"u{A.dtype.itemsize}")
    return (v & mask).astype(u).view(A.dtype)


def last_narrow(la):
    return la.get_option("last_narrow_mfma")


def run(la, A, B, alpha=1, beta=0, C0=None):
    C = np.zeros((A.shape[0], B.shape[1]), dtype=A.dtype) if C0 is None else C0.copy()
    return la.matmul(A, B, alpha=alpha, beta=beta, out=C)


def full_range_scalar(rng, dtype):
    return int(rng.integers(0, (1 << bits(dtype)) - 1, dtype=np.uint64, endpoint=True))


@pytest.mark.parametrize("dtype", ALL)
def test_every_integer_type_full_range_with_every_kind_of_scalar(la, dtype):
    rng = np.random.default_rng(100 + bits(dtype) + np.iinfo(dtype).min % 7)
    M, N, K = 300, 260, 500
    A, B, C0 = rand(rng, (M, K), dtype), rand(rng, (K, N), dtype), rand(rng, (M, N), dtype)
    for alpha in (0, 1, -1, full_range_scalar(rng, dtype)):
        for beta in (0, 1, -1, full_range_scalar(rng, dtype)):
            got = run(la, A, B, alpha, beta, C0)
            if dtype in NARROW:
                assert last_narrow(la) == 1, "the narrow matrix-core kernel did not run"
            assert np.array_equal(got, reference(A, B, alpha, beta, C0)), (dtype, alpha, beta)


def test_scalars_are_reduced_mod_2n(la):
    rng = np.random.default_rng(101)
    A, B, C0 = rand(rng, (200, 300), np.int8), rand(rng, (300, 180), np.int8), rand(rng, (200, 180), np.int8)
    assert np.array_equal(run(la, A, B, 257, -255, C0), run(la, A, B, 1, 1, C0))
    A, B, C0 = rand(rng, (200, 300), np.uint16), rand(rng, (300, 180), np.uint16), rand(rng, (200, 180), np.uint16)
    assert np.array_equal(run(la, A, B, 65535, 65537 * 3, C0), run(la, A, B, -1, 3, C0))


SHAPES = [  # (M, N, K), matrix cores?
    ((1, 5, 300), 0),          # M = 1, N = 5: the VALU kernel
    ((2, 3000, 700), 0),       # M <= 8: the streaming kernel
    ((3000, 3, 700), 0),       # N <= 8: the streaming kernel
    ((1, 1, 1), 0),
    ((7, 9, 3), 0),
    ((1000, 1030, 999), 1),    # M, N not tile multiples
    ((300, 260, 20000), 1),    # K beyond one launch: chunked
]


@pytest.mark.parametrize("dtype", NARROW)
@pytest.mark.parametrize("shape,mfma", SHAPES)
def test_every_path_by_shape(la, dtype, shape, mfma):
    rng = np.random.default_rng(sum(shape) + bits(dtype))
    M, N, K = shape
    A, B, C0 = rand(rng, (M, K), dtype), rand(rng, (K, N), dtype), rand(rng, (M, N), dtype)
    alpha, beta = full_range_scalar(rng, dtype), full_range_scalar(rng, dtype)
    got = run(la, A, B, alpha, beta, C0)
    assert last_narrow(la) == mfma
    assert np.array_equal(got, reference(A, B, alpha, beta, C0))


@pytest.mark.parametrize("dtype", [np.int8, np.uint16])
def test_4096_cubed_on_the_matrix_cores(la, dtype):
    rng = np.random.default_rng(102)
    A, B = rand(rng, (4096, 4096), dtype), rand(rng, (4096, 4096), dtype)
    got = run(la, A, B)
    assert last_narrow(la) == 1
    assert np.array_equal(got, reference(A, B, 1, 0, None))


@pytest.mark.parametrize("dtype", NARROW)
def test_widened_int32_oracle_agrees(la, oracle, dtype):
    rng = np.random.default_rng(103)
    for (M, N, K) in [(256, 256, 512), (333, 129, 1001)]:
        A, B, C0 = rand(rng, (M, K), dtype), rand(rng, (K, N), dtype), rand(rng, (M, N), dtype)
        want = oracle.matmul(A.astype(np.int32), B.astype(np.int32), alpha=3, beta=-2, C_=C0.astype(np.int32)).astype(dtype)
        assert np.array_equal(run(la, A, B, 3, -2, C0), want)


@pytest.mark.parametrize("dtype", NARROW)
def test_valu_path_matches_the_matrix_cores(la, dtype):
    rng = np.random.default_rng(104)
    A, B, C0 = rand(rng, (700, 900), dtype), rand(rng, (900, 520), dtype), rand(rng, (700, 520), dtype)
    mfma = run(la, A, B, 5, 7, C0)
    assert last_narrow(la) == 1
    la.set_option("narrow_mfma", 0)
    try:
        valu = run(la, A, B, 5, 7, C0)
        assert last_narrow(la) == 0
    finally:
        la.set_option("narrow_mfma", 1)
    assert np.array_equal(mfma, valu)
    assert np.array_equal(mfma, reference(A, B, 5, 7, C0))


@pytest.mark.parametrize("dtype", NARROW)
def test_strided_transposed_and_gapped_operands(la, dtype):
    rng = np.random.default_rng(105)
    M, N, K = 600, 520, 700
    A = rand(rng, (M, K), dtype)
    B = rand(rng, (K, N), dtype)
    want = reference(A, B, 1, 0, None)
    layouts_a = [np.asfortranarray(A),                                              # column-major
                 np.ascontiguousarray(np.pad(A, ((0, 0), (0, 37))))[:, :K],         # row stride K + 37
                 rand(rng, (2 * M, 3 * K), dtype),                                 # both strides > 1 (filled below)
                 np.ascontiguousarray(A[::-1])[::-1]]                              # negative row stride
    layouts_a[2][::2, ::3] = A
    layouts_a[2] = layouts_a[2][::2, ::3]
    for a in layouts_a:
        assert np.array_equal(a, A)
        assert np.array_equal(run(la, a, B), want)
    Bt = np.ascontiguousarray(B.T)
    assert np.array_equal(run(la, A, Bt.T), want)                                   # transposed (k-contiguous) B
    # C with gaps: the gaps keep their bytes; beta = 0 never reads C (garbage in it)
    big = rand(rng, (M, N + 11), dtype)
    keep = big.copy()
    C = big[:, :N]
    la.gemm_strided(M, N, K, 1, A, K, 1, B, N, 1, 0, C, N + 11, 1)
    assert np.array_equal(C, want)
    assert np.array_equal(big[:, N:], keep[:, N:])
    assert last_narrow(la) == 1


def test_device_resident_torch_tensors(la):
    import torch
    rng = np.random.default_rng(106)
    for dtype, tdt in [(np.int8, torch.int8), (np.uint8, torch.uint8), (np.int16, torch.int16)]:
        for (M, N, K) in [(640, 384, 768), (5, 2000, 300), (33, 17, 9)]:
            A, B, C0 = rand(rng, (M, K), dtype), rand(rng, (K, N), dtype), rand(rng, (M, N), dtype)
            dA, dB, dC = (torch.from_numpy(x).cuda() for x in (A, B, C0))
            la.matmul(dA, dB, alpha=-3, beta=2, out=dC)
            torch.cuda.synchronize()
            assert dC.dtype == tdt
            assert np.array_equal(dC.cpu().numpy(), reference(A, B, -3, 2, C0)), (dtype, M, N, K)


@pytest.mark.parametrize("dtype", [np.int8, np.int16])
def test_batched_device_gemm(la, dtype):
    import torch
    rng = np.random.default_rng(107)
    b, M, N, K = 3, 96, 200, 130
    A = rand(rng, (M, K), dtype)
    B = rand(rng, (b, K, N), dtype)
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    dC = torch.zeros((b, M, N), dtype=dA.dtype, device="cuda")
    la.gemm_strided_batched(b, M, N, K, 7, dA, K, 1, 0, dB, N, 1, K * N, 0, dC, N, 1, M * N)
    torch.cuda.synchronize()
    for i in range(b):
        assert np.array_equal(dC[i].cpu().numpy(), reference(A, B[i], 7, 0, None))


@pytest.mark.parametrize("dtype", NARROW)
def test_prepacked_round_trip_host_and_device(la, dtype):
    import torch
    rng = np.random.default_rng(108)
    M, N, K = 530, 300, 650
    A, B, C0 = rand(rng, (M, K), dtype), rand(rng, (K, N), dtype), rand(rng, (M, N), dtype)
    want = reference(A, B, 3, -1, C0)
    na, nb = la.gemm_prepackA_mem_required(dtype, M, N, K), la.gemm_prepackB_mem_required(dtype, M, N, K)
    pa, pb = la.aligned_host_buffer(na), la.aligned_host_buffer(nb)
    la.gemm_prepackA(pa, M, N, K, np.asfortranarray(A), 1, M)
    la.gemm_prepackB(pb, M, N, K, B, N, 1)
    C = C0.copy()
    la.gemm_packed(M, N, K, 3, pa, pb, -1, C, N, 1)
    assert np.array_equal(C, want)
    assert last_narrow(la) == 1
    la.gemm_prepack_release(pa)
    la.gemm_prepack_release(pb)
    dpa = torch.empty(na, dtype=torch.uint8, device="cuda")
    dpb = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dA, dB, dC = (torch.from_numpy(x).cuda() for x in (A, B, C0))
    la.gemm_prepackA(dpa, M, N, K, dA, K, 1)
    la.gemm_prepackB(dpb, M, N, K, dB.t().contiguous().t(), 1, K)      # column-major B source
    la.gemm_packed(M, N, K, 3, dpa, dpb, -1, dC, N, 1)
    torch.cuda.synchronize()
    assert np.array_equal(dC.cpu().numpy(), want)
