"""GPU parity tests (-m gpu) for the encoder's GEMM kernels in isolation (mdr_test_gemm_f16): every kernel flavour
against a float64 matmul of the same fp16 operands. Tolerance: fp32 accumulation of K <= 4096 products (W is scaled by 1 / sqrt(K), so the
outputs stay O(1) at every K) -> 2e-3 absolute on f32 outputs; f16 outputs add half-precision rounding of the result (2^-11 relative)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _gemm(A, W, bias, epilogue, kernel, m_valid=None):
    from multihop_dense_retrieval_amd import _lib
    L = _lib.lib()
    M, K = A.shape
    N = W.shape[0]
    out = torch.full((M, N), float("nan"), device="cuda", dtype=torch.float32 if epilogue == 3 else torch.float16)
    m_dev = None
    if m_valid is not None:
        m_dev = torch.tensor([m_valid], device="cuda", dtype=torch.int32)
    _lib.check(L.mdr_test_gemm_f16(A.data_ptr(), W.data_ptr(), bias.data_ptr(), M, m_dev.data_ptr() if m_dev is not None else None, N, K,
                                   out.data_ptr(), epilogue, kernel, 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out


def _reference(A, W, bias, epilogue):
    ref = A.double() @ W.double().T + bias.double()
    if epilogue == 1:
        ref = 0.5 * ref * (1.0 + torch.erf(ref / 2 ** 0.5))
    return ref


SHAPES = [  # (M, N, K): encoder shapes incl. ragged M, one tile, many tiles per workgroup
    (187, 768, 768), (256, 2304, 768), (1000, 3072, 768), (2413, 768, 3072), (20611, 2304, 768), (33000, 768, 768), (9000, 3072, 768),
    (9000, 768, 3072), (70000, 768, 768),
    # shapes outside roberta-base: K of 4 and 6 K-tiles (the four-wave kernel's shortest loops), N = 256, roberta-large's 1024
    (300, 256, 256), (5000, 512, 384), (3000, 1024, 1024),
    # the answer reader at ELECTRA-large geometry, 3 x 512 and 64 x 512 tokens: FFN1 (N = 4096 is wider than kPersistBiasMax: one-tile-per-block kernels whatever
    # is asked for), FFN2 (K = 4096: the four-wave kernel's K >= 2048 branch), QKV, out-projection; FFN2 at the reader's M_est = 32768 - 32768 / 3 and at 256 * 80 + 1 rows
    (1536, 4096, 1024), (32768, 4096, 1024), (20000, 1024, 4096), (32768, 1024, 4096), (32768, 3072, 1024), (32768, 1024, 1024), (21846, 1024, 4096),
    (20481, 1024, 4096),
    # dX of the reader's fused QKV projection in training (N = 1024, K = 3072): on the one-tile kernels, and past the 12033 rows from which 256 compute
    # units hand it to a persistent kernel (K >= 2048: the four-wave kernel's branch)
    (2413, 1024, 3072), (12300, 1024, 3072),
]


def _hook_rejects(shape, kernel):
    """Why the test hook is not asked for this pair (None: it is)."""
    if kernel in (1, 2) and shape[0] > 10000:
        return "small-tile kernels are not used at this size"
    return None


@pytest.mark.parametrize("kernel", [0, 1, 2, 4, 6, 7])
@pytest.mark.parametrize("epilogue", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_gemm_matches_fp64(shape, epilogue, kernel):
    M, N, K = shape
    if _hook_rejects(shape, kernel):
        pytest.skip(_hook_rejects(shape, kernel))
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = torch.randn((M, K), generator=g, device="cuda").half()
    W = (torch.randn((N, K), generator=g, device="cuda") / K ** 0.5).half()
    bias = torch.randn((N,), generator=g, device="cuda")
    out = _gemm(A, W, bias, epilogue, kernel)
    ref = _reference(A, W, bias, epilogue)
    err = (out.double() - ref).abs()
    tol = 2e-3 if epilogue == 3 else 2e-3 + ref.abs() * 2 ** -10
    bad = ~(err <= tol)   # (not err > tol: a NaN is no larger than anything)
    assert not bool(bad.any()), f"{int(bad.sum())} bad of {M * N}; worst {err.max().item():.3e} at {np.unravel_index(int(err.argmax()), (M, N))}"


def test_the_readers_ffn2_shape_runs_on_the_256x256_kernels():
    """(M, 1024, 4096) on kernels 6 and 7 is the pair the answer reader depends on at large M: the cases above must not skip it, and launch_gemm's conditions for
    handing a forced 6 / 7 to gemm_big_kernel / gemm_quad_kernel (instead of falling through to another flavour) must hold for it."""
    shapes = [s for s in SHAPES if s[1:] == (1024, 4096)]
    assert len(shapes) >= 4 and max(s[0] for s in shapes) >= 32768
    for M, N, K in shapes:
        for kernel in (6, 7):
            assert _hook_rejects((M, N, K), kernel) is None
        assert N % 256 == 0 and N <= 3072 and K % 128 == 0 and K >= 256
        assert (M + 255) * N * 4 < 1 << 32 and (M + 255) * K * 2 < 1 << 32  # the buffer descriptors' 32-bit offsets (out32, a32)
    g = torch.Generator(device="cuda").manual_seed(11)
    M, N, K = 20481, 1024, 4096
    A = torch.randn((M, K), generator=g, device="cuda").half()
    W = (torch.randn((N, K), generator=g, device="cuda") / K ** 0.5).half()
    bias = torch.randn((N,), generator=g, device="cuda")
    ref = _gemm(A, W, bias, 3, 2)
    for kernel in (6, 7):
        assert torch.equal(_gemm(A, W, bias, 3, kernel), ref), kernel


def test_quad_kernel_is_bit_identical_to_the_eight_wave_kernel():
    """Kernel 7 (four waves of 128x128, hand-scheduled K-loop) accumulates K in the same order with the same MFMA as kernel 6."""
    for (M, N, K), epi in (((20611, 2304, 768), 0), ((9000, 3072, 768), 1), ((20611, 768, 3072), 3), ((2413, 768, 768), 3)):
        g = torch.Generator(device="cuda").manual_seed(7)
        A = torch.randn((M, K), generator=g, device="cuda").half()
        W = (torch.randn((N, K), generator=g, device="cuda") / K ** 0.5).half()
        bias = torch.randn((N,), generator=g, device="cuda")
        a, b = _gemm(A, W, bias, epi, 6), _gemm(A, W, bias, epi, 7)
        assert torch.equal(a, b), f"{(M, N, K)} epilogue {epi}: {(a.double() - b.double()).abs().max().item():.3e}"


@pytest.mark.parametrize("kernel", [0, 4, 6, 7])
def test_gemm_device_side_row_count(kernel):
    """Rows past *m_dev are neither computed into nor stored (the packed token count lives on the device)."""
    for M, N, K, valid in [(5000, 768, 768, 3333)] + ([(5000, 1024, 4096, 3333)] if kernel in (6, 7) else []):  # + the reader's FFN2
        g = torch.Generator(device="cuda").manual_seed(1)
        A = torch.randn((M, K), generator=g, device="cuda").half()
        W = (torch.randn((N, K), generator=g, device="cuda") / K ** 0.5).half()
        bias = torch.zeros((N,), device="cuda")
        out = _gemm(A, W, bias, 3, kernel, m_valid=valid)
        ref = _reference(A, W, bias, 3)
        assert (out[:valid].double() - ref[:valid]).abs().max().item() <= 2e-3, (N, K)
        assert bool(torch.isnan(out[valid:]).all()), (N, K)


# (M, N, K) a little over a whole number of rounds of 256x256 tiles on 256 workgroups: the last, partial round runs on 128x128 tiles inside the same
# persistent kernel (gemm_head_row_tiles / gemm_tail_tile). 86 row tiles: 258 / 774 / 1032 tiles for N = 768 / 2304 / 3072 (remainders 2 / 6 / 8);
# 171 x 3 = 513 (two complete rounds + 1); 43 x 12 = 516 (remainder 4, rows not a multiple of 128); a tail of several row tiles (N = 768: 90 x 3 = 270).
# The reader's shapes by the same rule: N = 1024 is 4 column tiles, 65 row tiles = 260 (remainder 4, K = 4096) and 130 = 520 (two rounds + 8, K = 1024), rows not a
# multiple of 128; N = 3072, K = 1024: 43 x 12 = 516.
TAIL_SHAPES = [(22013, 768, 768), (22013, 2304, 768), (22013, 3072, 768), (22013, 768, 3072), (43700, 768, 768), (10900, 3072, 768), (22990, 768, 768),
               (16600, 1024, 4096), (33100, 1024, 1024), (10900, 3072, 1024)]


@pytest.mark.parametrize("kernel", [6, 7])
@pytest.mark.parametrize("epilogue", [0, 1, 3])
@pytest.mark.parametrize("shape", TAIL_SHAPES)
def test_partial_last_round_on_small_tiles_is_bit_identical(shape, epilogue, kernel):
    """Every flavour accumulates K in the same order with the same MFMA: the 256x256 kernels with their 128x128 tail must return the bits of the
    one-tile-per-block 128x128 kernel (2), whose results the fp64 test above pins, for every row -- head tiles, tail tiles and the ragged last rows."""
    M, N, K = shape
    g = torch.Generator(device="cuda").manual_seed(M + N + K + 1)
    A = torch.randn((M, K), generator=g, device="cuda").half()
    W = (torch.randn((N, K), generator=g, device="cuda") / K ** 0.5).half()
    bias = torch.randn((N,), generator=g, device="cuda")
    out = _gemm(A, W, bias, epilogue, kernel)
    ref = _gemm(A, W, bias, epilogue, 2)
    assert bool(torch.isfinite(out.float()).all())
    assert torch.equal(out, ref), f"{shape} epilogue {epilogue} kernel {kernel}: {int((out != ref).sum())} elements differ, first rows {torch.nonzero((out != ref).any(1))[:5].flatten().tolist()}"
    err = (out.double() - _reference(A, W, bias, epilogue)).abs()
    assert err.max().item() <= (2e-3 if epilogue == 3 else 2e-2)


@pytest.mark.parametrize("kernel", [6, 7])
def test_tail_respects_the_device_side_row_count(kernel):
    """The split point is computed on the device from *m_dev: rows past it stay untouched whether they fall in the 256x256 walk or in the tail."""
    # N = 768: 86 row tiles (tail of one) ... 89 (tail of four); the reader's FFN2 (N = 1024, K = 4096): 65 row tiles (a tail of one row) ... 67
    for (M, N, K), valids in (((23000, 768, 768), (21761, 21900, 22016, 22017, 22700)), ((18000, 1024, 4096), (16385, 16500, 16640, 16641, 17000))):
        g = torch.Generator(device="cuda").manual_seed(3)
        A = torch.randn((M, K), generator=g, device="cuda").half()
        W = (torch.randn((N, K), generator=g, device="cuda") / K ** 0.5).half()
        bias = torch.zeros((N,), device="cuda")
        ref = _reference(A, W, bias, 3)
        for valid in valids:
            out = _gemm(A, W, bias, 3, kernel, m_valid=valid)
            assert (out[:valid].double() - ref[:valid]).abs().max().item() <= 2e-3, (N, K, valid)
            assert bool(torch.isnan(out[valid:]).all()), (N, K, valid)
