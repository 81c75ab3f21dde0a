"""CPU: the fp64 statement of the Linear backward (tests/linear_grad_ref.py) against torch.autograd in float64, the fp32 gelu' formula over
every finite fp16 pre-activation, the emulation of the kernels' dataflow against the derived bound, each mutation against the same bound,
and the header / binding / split contract of include/mdr_linear_grad.h. No device and no kernel runs here.

The emulation runs over every list of the GPU test -- SMALL_NK, MODEL_NK, READER_NK, POOLER_MNK, LARGE_MNK, TWO_CHUNK_MNK -- except
PERSIST_DX_MNK: (12300, 3072, 1024) and (12300, 4096, 1024) cost six times the largest case here (the numpy slab loop and three fp64 products
of 12300 x 4096 x 1024, about a minute a shape) and are left to the GPU test, which runs them on the exact grid, where no bound is needed."""

import numpy as np
import pytest
import torch

import linear_grad_ref as ref
from oracle import fp

OUTPUTS = ("dx", "dw", "db")


def _pre(x, w, b):
    """the fp16 pre-activation of the forward, on the host: fp16(x w^T + b) from an fp32 product"""
    return (x.astype(np.float32) @ w.astype(np.float32).T + b).astype(np.float16)


def _ratios(got, rb):
    return {k: fp.worst_ratio(g, *rb[k]) for k, g in zip(OUTPUTS, got)}


@pytest.mark.parametrize("gelu", [False, True])
def test_fp64_statement_agrees_with_torch_autograd(gelu):
    """Both sides are fp64 and differ only in summation order: |a - b| <= 1e-10 max|b| per output."""
    M, N, K = 37, 128, 64
    x, w, dy = ref.realistic(M, N, K, 1)
    w = (w.astype(np.float32) * 20).astype(np.float16)  # pre-activations of order 1, where gelu' is not flat
    b = ref.bias(N, 1)
    pre = _pre(x, w, b)
    tx, tw = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, w))
    tb = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    if gelu:
        # the statement takes the pre-activation as given: feed autograd the same u by making the Linear reproduce it exactly
        tu = torch.from_numpy(pre.astype(np.float64)).requires_grad_(True)
        y = torch.nn.functional.gelu(tu)
        (dz,) = torch.autograd.grad(y, tu, torch.from_numpy(dy.astype(np.float64)))
        want_dz = dz.numpy()
    else:
        want_dz = dy.astype(np.float64)
    lin = torch.nn.functional.linear(tx, tw, tb)
    want = [g.numpy() for g in torch.autograd.grad(lin, (tx, tw, tb), torch.from_numpy(want_dz))]
    rb = ref.reference_and_bound(x, w, dy, pre if gelu else None)
    assert np.abs(rb["dz"][0] - want_dz).max() <= 1e-10 * np.abs(want_dz).max()
    for k, wnt in zip(OUTPUTS, want):
        assert np.abs(rb[k][0] - wnt).max() <= 1e-10 * np.abs(wnt).max(), (k, np.abs(rb[k][0] - wnt).max())
    if gelu:  # and end to end through F.gelu(F.linear) with an exactly representable pre-activation: b = 0, u = x w^T in fp64
        tx2, tw2 = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x, w))
        y2 = torch.nn.functional.gelu(torch.nn.functional.linear(tx2, tw2))
        want2 = torch.autograd.grad(y2, (tx2, tw2), torch.from_numpy(dy.astype(np.float64)))
        u64 = x.astype(np.float64) @ w.astype(np.float64).T
        dz2 = dy.astype(np.float64) * ref.gelu_grad64(u64)
        assert np.abs(dz2 @ w.astype(np.float64) - want2[0].numpy()).max() <= 1e-10 * np.abs(want2[0].numpy()).max()
        assert np.abs(dz2.T @ x.astype(np.float64) - want2[1].numpy()).max() <= 1e-10 * np.abs(want2[1].numpy()).max()


def test_gelu_grad_formula_over_every_finite_fp16():
    """The fp32 formula of the kernel (Phi from the forward's tail polynomial, phi from one exp2) against fp64 over ALL finite fp16 u: inside the
    dZ term of the bound. This pins the forward's 2.1e-7 claim for the derivative, and the clamp of the polynomial's argument."""
    u = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    u = u[np.isfinite(u)]
    assert u.size == 63488
    got = ref.gelu_grad32(u).astype(np.float64)
    want = ref.gelu_grad64(u.astype(np.float64))
    err, bnd = np.abs(got - want), ref.gelu_grad_bound(u.astype(np.float64))
    i = int(np.argmax(err / bnd))
    print(f"RATIO gelu' worst |err| / bound = {err[i] / bnd[i]:.4f} at u = {float(u[i])} (|err| {err[i]:.3e}, largest |err| {err.max():.3e})")
    assert np.isfinite(got).all()
    assert (err <= bnd).all(), (float(u[i]), got[i], want[i], bnd[i])
    assert ref.gelu_grad32(np.zeros(1, np.float16))[0] == np.float32(0.5)  # the structural case of the GPU tests: exactly 1/2 at 0
    wrong = np.abs(ref.gelu_grad32(u, "gelu_no_uphi").astype(np.float64) - want)
    assert (wrong > bnd).any()


@pytest.mark.parametrize("M,N,K", [pytest.param(None, N, K, id=f"{N}-{K}") for N, K in ref.SMALL_NK + ref.MODEL_NK + ref.READER_NK] +
                         [pytest.param(M, N, K, id=f"M{M}-{N}-{K}") for M, N, K in ref.POOLER_MNK + ref.LARGE_MNK + ref.TWO_CHUNK_MNK])
def test_emulation_stays_inside_the_bound(M, N, K):
    """A second implementation of the listed dataflow, on every shape the GPU tests use, identity and GELU, unit and loss scale (the shapes
    of LARGE_MNK, where the slab loop and the chunk reduction add thousands of terms: under the loss scale, as in training)."""
    for M in ([M] if M is not None else ref.M_SWEEP if (N, K) in ref.SMALL_NK else [300]):
        for scale in ((1.0, 256.0) if M <= 300 else (256.0,)):
            x, w, dy = ref.realistic(M, N, K, 11, scale)
            pre = _pre(x, w, ref.bias(N, 11))
            old_dw, old_db = ref.realistic(N, 64, K, 12)[0].astype(np.float32), ref.bias(N, 12)
            for p, m, odw, odb in ((None, None, None, None), (pre, None, None, None), (pre, max(M - 1, 0), old_dw, old_db)):
                rb = ref.reference_and_bound(x, w, dy, p, m, odw, odb)
                for k, (worst, at) in _ratios(ref.emulate(x, w, dy, p, m, odw, odb), rb).items():
                    assert worst <= 1.0, (M, N, K, scale, k, worst, at)


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_each_mutation_leaves_the_bound(mutation):
    """The bound is worth something: every row-count, chunk, index, accumulate and gelu' defect is thrown out."""
    M, N, K = 200, 128, 128
    assert ref.chunks(M, N, K)[0] > 1
    x, w, dy = ref.realistic(M, N, K, 21)
    w = (w.astype(np.float32) * 20).astype(np.float16)
    pre = _pre(x, w, ref.bias(N, 21))
    old_dw, old_db = ref.realistic(N, 64, K, 22)[0].astype(np.float32), ref.bias(N, 22)
    m = M - 1
    rb = ref.reference_and_bound(x, w, dy, pre, m, old_dw, old_db)
    assert max(v[0] for v in _ratios(ref.emulate(x, w, dy, pre, m, old_dw, old_db), rb).values()) <= 1.0
    r = _ratios(ref.emulate(x, w, dy, pre, m, old_dw, old_db, mutation), rb)
    print(f"mutation {mutation}: worst |err| / bound " + ", ".join(f"{k} {v[0]:.3g}" for k, v in r.items()))
    assert max(v[0] for v in r.values()) > 1.0, mutation


def test_split_is_a_function_of_the_shape_and_workspace_covers_it():
    """mdr_linear_backward_chunks equals the helper's restatement, S > 1 on a tested shape, the workspace holds what the header says."""
    from multihop_dense_retrieval_amd import linear
    lib = linear.lib()
    some_split = False
    for N, K in ref.SMALL_NK + ref.MODEL_NK + ref.READER_NK:
        for M in ref.M_SWEEP + [8608, 20000, 32768]:
            S, rpc = linear.backward_chunks(M, N, K)
            assert (S, rpc) == ref.chunks(M, N, K) and S >= 1 and rpc % 64 == 0 and (S - 1) * rpc < M <= S * rpc, (M, N, K, S, rpc)
            some_split |= S > 1
            full = lib.mdr_linear_backward_workspace_bytes(M, N, K, 15)
            assert full >= M * N * 2 + N * K * 2 + K * 4 + (S * N * K * 4 + S * N * 4 if S > 1 else 0)
            assert lib.mdr_linear_backward_workspace_bytes(M, N, K, 4) == (0 if S == 1 else (S * N * 4 + 255) // 256 * 256)
    assert some_split
    # the large shapes, and the reader's FFN shapes with their two long chunks, keep their properties under the LIBRARY's split
    for M, N, K, S, rpc, _ in ref.assert_large(chunks_of=linear.backward_chunks) + ref.assert_two_chunks(chunks_of=linear.backward_chunks):
        assert (S, rpc) == ref.chunks(M, N, K)
        assert lib.mdr_linear_backward_workspace_bytes(M, N, K, 15) >= M * N * 2 + N * K * 2 + K * 4 + S * N * K * 4 + S * N * 4
    assert ref.assert_two_chunks(chunks_of=linear.backward_chunks) == [(2051, 4096, 1024, 2, 1088, 963), (2051, 1024, 4096, 2, 1088, 963)]
    for M in ref.M_SWEEP + [2051, 12300, 32768]:  # the reader's FFN shapes: 256 dW tiles, so never more than two chunks, and two from 65 rows on
        for N, K in ((4096, 1024), (1024, 4096)):
            assert linear.backward_chunks(M, N, K)[0] == (2 if M > ref.SLAB else 1), (M, N, K)
    for M, N, K in ref.POOLER_MNK:  # the pooler's row counts fit one slab: one chunk, no partials
        assert linear.backward_chunks(M, N, K) == ref.chunks(M, N, K) == (1, ref.SLAB)
    for M, N, K in ref.PERSIST_DX_MNK:
        assert linear.backward_chunks(M, N, K) == ref.chunks(M, N, K)
    assert linear.backward_chunks(12300, 4096, 1024) == (2, 97 * ref.SLAB)
    for M, N, K in ((0, 64, 64), (-1, 64, 64), (5, 0, 64), (5, 64, 0), (5, 96, 64), (5, 64, 100), (5, -64, 64)):
        assert lib.mdr_linear_backward_workspace_bytes(M, N, K, 15) == 0
        assert linear.backward_chunks(M, N, K) == (0, 0)


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import linear
    x, w, b = torch.zeros(4, 64, dtype=torch.float16), torch.zeros(64, 64), torch.zeros(64)
    with pytest.raises(RuntimeError):
        linear.packed_linear(x, w, b)
    with pytest.raises(RuntimeError):
        linear.linear_backward(x, w.half(), torch.zeros(4, 64, dtype=torch.float16))


def test_the_exponent_field_term_covers_subnormal_columns_and_is_zero_otherwise():
    """line 1 of the derivation: an fp16 MFMA cuts the products it adds at 24 bits below their largest exponent FIELD, and a subnormal's field
    is 2^-14. The model of that (ref.aligned_dw) leaves the bound without the term F on the case the chain test met, stays inside with it, and
    F is exactly zero where no operand is subnormal or zero."""
    x, w, dy = ref.subnormal_columns_case()
    r, bnd = ref.reference_and_bound(x, w, dy)["dw"]
    f = ref.field_floor_term(np.abs(dy.astype(np.float64)).T, np.abs(x.astype(np.float64)))
    got = ref.aligned_dw(x, dy)
    with_f, without_f = fp.worst_ratio(got, r, bnd)[0], fp.worst_ratio(got, r, bnd - f)[0]
    print(f"aligned model, subnormal columns: share of the bound {with_f:.3f}, without F {without_f:.3f}, {int((np.abs(got - r) > bnd - f).sum())} elements over")
    assert with_f <= 1.0 < without_f
    xn, _, dyn = ref.realistic(4, 256, 384, 18)
    assert not (np.abs(xn) < fp.N16).any() and not (np.abs(dyn) < fp.N16).any()
    assert not ref.field_floor_term(np.abs(dyn.astype(np.float64)).T, np.abs(xn.astype(np.float64))).any()
    assert fp.worst_ratio(ref.aligned_dw(xn, dyn), *ref.reference_and_bound(xn, _, dyn)["dw"])[0] <= 1.0  # normal operands: inside the ulp count
