"""GPU (-m gpu): the head Linear with an fp32 output in isolation (multihop_dense_retrieval_amd/head.py, mdr_head_backward of
include/mdr_head_grad.h) against the fp64 statement and the derived bound of tests/head_grad_ref.py. EVERY element of dX, dW and db is
compared; nothing is averaged, and no tolerance here was read off a device.

Every output starts as a finite sentinel with 64 guard rows (dx) or 64 guard elements (dw, db) on both sides, which must keep their bits in
every call of this file. Shapes: head_grad_ref.M_SWEEP x head_grad_ref.NK -- one row, the batch sizes of the chain tests, one row past a
64-row tile, the training batch of 150 (two chunks of the dW / db sums, the second ragged); one tile, several tiles, non-square, the model's."""
import numpy as np
import pytest
import torch

import head_grad_ref as ref
from guarded import Guarded, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import fp

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = [pytest.param(N, K, id=f"N{N}-K{K}") for N, K in ref.NK]


def run(x, w, dy, outs="xwb", old_dw=None, old_db=None, accumulate=False):
    """One raw call on numpy inputs. Outputs start as SENTINEL (dw / db: the old values if given) inside guards; returns {"dx", "dw", "db"} as
    numpy for the outputs asked for, after asserting MDR_OK, that the guards kept their bits and that an output not asked for was not written."""
    from multihop_dense_retrieval_amd import _lib, head
    M, K = x.shape
    N = w.shape[0]
    bx = Guarded(M, (K,), torch.float16, GUARD, GUARD, name="dx")
    bw = Guarded(N * K, (), torch.float32, GUARD, GUARD, None if old_dw is None else old_dw.astype(np.float32), "dw", "elements")
    bb = Guarded(N, (), torch.float32, GUARD, GUARD, None if old_db is None else old_db.astype(np.float32), "db", "elements")
    want = (1 if "x" in outs else 0) | (2 if "w" in outs else 0) | (4 if "b" in outs else 0)
    need = int(head.lib().mdr_head_backward_workspace_bytes(M, N, K, want))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    tx, tw, tdy = dev(x), dev(w), dev(dy)
    _lib.check(head.lib().mdr_head_backward(ptr(tx), ptr(tw), ptr(tdy), M, N, K, bx.ptr("x" in outs), bw.ptr("w" in outs), bb.ptr("b" in outs),
                                            1 if accumulate else 0, ptr(ws), need, 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    return {"dx": bx.checked(asked="x" in outs), "dw": bw.checked(asked="w" in outs).reshape(N, K), "db": bb.checked(asked="b" in outs)}


def check_bound(got, rb, label, names=("dx", "dw", "db")):
    for name in names:
        worst = fp.assert_within(got[name], *rb[name], f"{label}: {name}")
        print(f"RATIO {label} {name} worst |err| / bound = {worst:.4f}")


@pytest.mark.parametrize("N,K", SHAPES)
def test_forward_bits_are_the_encoder_gemms(N, K):
    """packed_head_linear's output is mdr_test_gemm_f16 with epilogue 3 bit for bit, with the cast inside and with a caller's fp16 copy; and it
    is NOT the fp16 Linear's output widened (the rounding this brick removes)."""
    from multihop_dense_retrieval_amd import _lib, head, linear
    for M in ref.M_SWEEP:
        x, w, _ = ref.realistic(M, N, K, 3)
        b = ref.bias(N, 3)
        tx, tw16, tb = dev(x), dev(w), dev(b)
        want = torch.full((M, N), 777.0, dtype=torch.float32, device="cuda")
        _lib.check(_lib.lib().mdr_test_gemm_f16(ptr(tx), ptr(tw16), ptr(tb), M, None, N, K, ptr(want), 3, 0, 0, _lib.current_stream_ptr()))
        w32 = tw16.float()
        y = head.packed_head_linear(tx, w32, tb)
        y2 = head.packed_head_linear(tx, w32, tb, tw16)
        y16 = linear.packed_linear(tx, w32, tb)
        torch.cuda.synchronize()
        assert y.dtype == torch.float32 and fp.same_bits(y.cpu().numpy(), want.cpu().numpy()), (M, N, K)
        assert fp.same_bits(y2.cpu().numpy(), want.cpu().numpy()), (M, N, K)
        assert fp.same_bits(y16.cpu().numpy(), want.cpu().numpy().astype(np.float16))
        assert not np.array_equal(y16.float().cpu().numpy(), y.cpu().numpy())


@pytest.mark.parametrize("N,K", SHAPES)
def test_backward_inside_the_bound(N, K):
    """all three outputs together, overwrite and accumulate, unit and loss scale, at every M of the sweep"""
    for M in ref.M_SWEEP:
        for scale in (1.0, 256.0):
            x, w, dy = ref.realistic(M, N, K, 11, scale)
            check_bound(run(x, w, dy), ref.reference_and_bound(x, w, dy), f"M={M} N={N} K={K} x{scale:g}")
        old_dw, old_db = ref.old_values(N, K, 12)
        got = run(x, w, dy, old_dw=old_dw, old_db=old_db, accumulate=True)
        check_bound(got, ref.reference_and_bound(x, w, dy, old_dw, old_db), f"accumulate M={M} N={N} K={K}")
        got = run(x, w, dy, old_dw=old_dw, old_db=old_db, accumulate=False)  # the old values are overwritten, not added
        check_bound(got, ref.reference_and_bound(x, w, dy), f"overwrite M={M} N={N} K={K}")


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_each_output_alone_has_the_bits_of_the_joint_call_and_two_runs_agree(N, K, accumulate):
    for M in ref.M_SWEEP:
        x, w, dy = ref.realistic(M, N, K, 13, 256.0)
        old = ref.old_values(N, K, 14) if accumulate else (None, None)
        rb = ref.reference_and_bound(x, w, dy, *old)
        both = run(x, w, dy, "xwb", *old, accumulate)
        again = run(x, w, dy, "xwb", *old, accumulate)
        for name in ("dx", "dw", "db"):
            assert fp.same_bits(both[name], again[name]), f"{name}: two runs differ (M={M} N={N} K={K})"
        for outs, name in (("x", "dx"), ("w", "dw"), ("b", "db")):
            alone = run(x, w, dy, outs, *old, accumulate)  # (run() asserts that the two others were not written)
            check_bound(alone, rb, f"{name} alone M={M} N={N} K={K}", (name,))
            assert fp.same_bits(alone[name], both[name]), f"{name} alone differs from the joint call (M={M} N={N} K={K})"


@pytest.mark.parametrize("M", [6, 150])
def test_a_non_finite_dy_arrives_in_its_row_and_column_only(M):
    """one +Inf and one NaN in dY: dX is non-finite in exactly those two rows (every element: each reads the whole row of dY), dW in exactly
    those two rows n (every element), db in exactly those two elements. x and w hold zeros too: Inf * 0 is NaN, still non-finite."""
    N, K = 128, 192
    x, w, dy = ref.realistic(M, N, K, 15, 256.0)
    x[:, 5], w[:, 7] = 0, 0
    (mi, ni), (mn, nn) = (M - 1, 3), (M // 2, N - 1)
    dy[mi, ni], dy[mn, nn] = np.inf, np.nan
    for accumulate in (False, True):
        old = ref.old_values(N, K, 16) if accumulate else (None, None)
        got = run(x, w, dy, "xwb", *old, accumulate)
        bad_rows, bad_cols = np.zeros(M, bool), np.zeros(N, bool)
        bad_rows[[mi, mn]] = True
        bad_cols[[ni, nn]] = True
        assert np.array_equal(~np.isfinite(got["dx"]), np.broadcast_to(bad_rows[:, None], (M, K)))
        assert np.array_equal(~np.isfinite(got["dw"]), np.broadcast_to(bad_cols[:, None], (N, K)))
        assert np.array_equal(~np.isfinite(got["db"]), bad_cols)
        clean = dy.copy()
        clean[[mi, mn]] = 0
        rb = ref.reference_and_bound(x, w, clean, *old)
        fp.assert_within(got["dx"][~bad_rows], rb["dx"][0][~bad_rows], rb["dx"][1][~bad_rows], "the finite rows of dx")


def test_autograd_function_hands_back_the_bricks_gradients():
    """packed_head_linear under autograd: the three gradients are head_backward's on the same tensors, bit for bit, and the weight16 path
    sends its gradient to the fp32 master"""
    from multihop_dense_retrieval_amd import head
    M, N, K = 150, 256, 256
    x, w, dy = ref.realistic(M, N, K, 17, 256.0)
    tx = dev(x).requires_grad_(True)
    w16 = dev(w)
    tw, tb = w16.float().requires_grad_(True), dev(ref.bias(N, 17)).requires_grad_(True)
    g = dev(dy)
    y = head.packed_head_linear(tx, tw, tb, w16)
    y.backward(g)
    dx, dw, db = head.head_backward(tx.detach(), w16, g, True, torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda"))
    torch.cuda.synchronize()
    for name, a, b in (("dx", tx.grad, dx), ("dw", tw.grad, dw), ("db", tb.grad, db)):
        assert a.dtype == b.dtype and fp.same_bits(a.cpu().numpy(), b.cpu().numpy()), name
    check_bound({"dx": dx.cpu().numpy(), "dw": dw.cpu().numpy(), "db": db.cpu().numpy()}, ref.reference_and_bound(x, w, dy), "autograd")
