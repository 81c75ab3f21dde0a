"""GPU (-m gpu): mdr_reader_loss_forward / mdr_reader_loss_backward (include/mdr_reader_loss.h) against the fp64 statement of
tests/reader_loss_ref.py. The loss and every element of the four score gradients must sit inside that helper's DERIVED bound (fp32 evaluation
in any order; the one fp16 rounding of a gradient may flip only where a rounding boundary lies within the fp32 error; the `log_prob == 0`
decision may go either way only where fp32(lse) depends on the summation order). Every call writes into tests/guarded.py buffers.

The gradients are fp16, so the tests run with a loss scale, as an amp run has one: g0 = 64 and sp_weight = 1. g0 * sp_weight * offset must stay
finite in fp16 for offsets up to 511 (64 * 511 = 32704 < 65504); a larger scale overflows d_sp, which test_an_overflowing_scale_... asserts."""
import contextlib

import numpy as np
import pytest
import torch

import reader_loss_ref as ref
from guarded import Guarded, dev
from oracle import fp

pytestmark = pytest.mark.gpu

G0, SPW = 64.0, 1.0
# (B, L, A, NS): every B of {1, 3, 4, 5, 97}, every L of {1, 63, 64, 65, 256, 257, 512} (one wave of positions, its edges, 256 = one position per
# thread, 257 = the second position of thread 0, 512 = the LDS rows full), every A of {1, 3, 64, 65, 256, 257, 300, 513} and every NS of
# {0, 1, 5, 30} appear. reader_loss_grad_kernel stages the candidates in LDS in tiles of 256 (the `a0` loop): A <= 65 stays inside the first
# tile (65: past one wave of candidates). 256 = exactly one tile, the smallest A at which n = min(256, A - a0) is the whole tile; 257 = one
# candidate into the second trip, the smallest at which ts / te / tp are written again behind the barrier; 513 = one into the third, the
# smallest with two re-uses, at L = 512 (LDS rows full); 300 = a ragged second tile of 44 at L = 512 with the most markers and the most rows
SHAPES = [(1, 1, 1, 0), (3, 63, 3, 1), (4, 64, 64, 5), (5, 65, 65, 30), (97, 256, 3, 5), (4, 257, 1, 30), (3, 512, 65, 5),
          (4, 300, 256, 1), (3, 64, 257, 0), (2, 512, 513, 5), (5, 512, 300, 30)]
KEYS = ("start", "end", "rank", "sp")


def run(inp, g0=G0, spw=SPW, stream=None):
    """(loss, {start, end, rank, sp} gradients as numpy) from one forward + backward through the C entry points, outputs in guarded buffers"""
    from multihop_dense_retrieval_amd import _lib, reader_loss
    L_ = reader_loss.lib()
    B, L = inp["start"].shape
    A = inp["starts"].shape[1]
    has_sp = inp.get("sp") is not None
    NS = inp["sp"].shape[1] if has_sp else 0
    f16 = lambda a: dev(np.asarray(a, np.float16))  # noqa: E731
    i64 = lambda a: dev(np.asarray(a, np.int64))  # noqa: E731
    t = [f16(inp["start"]), f16(inp["end"]), f16(inp["rank"]), f16(inp["sp"]) if has_sp else None, i64(inp["starts"]), i64(inp["ends"]), i64(inp["label"]),
         i64(inp["sent_offsets"]) if has_sp else None, i64(inp["sent_labels"]) if has_sp else None]
    g = dev(np.array([g0], np.float32))
    out = {"loss": Guarded(1, (), torch.float32, 1, 1, name="loss"), "start": Guarded(B, (L,), torch.float16, 2, 2, name="d_start"),
           "end": Guarded(B, (L,), torch.float16, 2, 2, name="d_end"), "rank": Guarded(B, (), torch.float16, 3, 3, name="d_rank")}
    if has_sp:
        out["sp"] = Guarded(B, (NS,), torch.float16, 2, 2, name="d_sp")
    need = int(L_.mdr_reader_loss_workspace_bytes(B, L, A, NS))
    ws = _lib.workspace(need, torch.device("cuda", torch.cuda.current_device()))
    p = _lib.ptr
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        st = _lib.current_stream_ptr()
        _lib.check(L_.mdr_reader_loss_forward(*[p(x) for x in t], B, L, A, NS, spw, out["loss"].ptr(), p(ws), need, torch.cuda.current_device(), st))
        _lib.check(L_.mdr_reader_loss_backward(*[p(x) for x in t], B, L, A, NS, spw, p(g), out["start"].ptr(), out["end"].ptr(), out["rank"].ptr(),
                                               out["sp"].ptr() if has_sp else None, torch.cuda.current_device(), st))
    torch.cuda.synchronize()
    res = {k: o.checked() for k, o in out.items()}
    return float(res.pop("loss")[0]), res


def check(inp, g0, spw, label, rows=None, keys=KEYS):
    r = ref.loss_and_grads(inp, g0, spw)
    loss, grads = run(inp, g0, spw)
    worst = {}
    if rows is None:
        worst["loss"] = abs(loss - r["loss"]) / r["loss_bound"]
        assert worst["loss"] <= 1.0, (label, loss, r["loss"], r["loss_bound"])
    for k, g in grads.items():
        if k not in keys:
            continue
        sel = slice(None) if rows is None else rows
        worst[k] = fp.assert_within(g[sel], r["grads"][k][sel], r["bounds"][k][sel], f"{label} d_{k}")
    print(label, "worst |got - ref| / bound:", {k: f"{v:.3f}" for k, v in worst.items()})
    return loss, grads, r


@pytest.mark.parametrize("B,L,A,NS", SHAPES)
def test_loss_and_gradients_within_the_derived_bound(B, L, A, NS):
    inp = ref.make_loss_case(B, L, A, NS, seed=B + L + A + NS)
    loss, grads, r = check(inp, G0, SPW, f"B={B} L={L} A={A} NS={NS}")
    pad = ~np.isfinite(inp["start"])
    assert (grads["start"][pad] == 0).all() and (grads["end"][pad] == 0).all()  # written in full, 0 at -inf logits and on padding
    if B >= 3 and L > 1:
        assert r["counted"].any()
    if B >= 7:
        assert (~r["counted"]).any()


def test_loss_without_a_scale():
    """g0 = 1 and a fractional sp_weight: the loss value does not depend on g0, the gradients scale with it"""
    inp = ref.make_loss_case(5, 40, 6, 4, seed=2)
    check(inp, 1.0, 0.25, "g0=1")


def margin_case(L, target, others=0.0):
    inp = ref.make_loss_case(3, L, 2, 0, seed=1)
    for k in ("start", "end"):
        inp[k][1] = others
        inp[k][1, 2 % L] = target
    inp["starts"][1], inp["ends"][1] = [2 % L, -1], [2 % L, -1]
    return inp


def test_a_large_margin_gives_exactly_zero():
    """target logit 40 (fp16-exact), every other 0: the fp32 lse is exactly 40, so log_prob == 0: the candidate is masked and the row uncounted"""
    inp = margin_case(64, 40.0)
    loss, grads = run(inp)
    off = dict(inp, starts=inp["starts"].copy(), ends=inp["ends"].copy())
    off["starts"][1], off["ends"][1] = -1, -1
    loss_off, grads_off = run(off)
    assert loss == loss_off  # the span loss of the row is exactly 0
    assert (grads["start"][1] == 0).all() and (grads["end"][1] == 0).all()
    r = ref.loss_and_grads(inp, G0, SPW)
    assert not r["counted"][1] and abs(loss - r["loss"]) <= r["loss_bound"]


@pytest.mark.parametrize("L", [3, 4])
def test_a_candidate_on_the_mask_boundary_stays_inside_the_widened_bound(L):
    """target 15.5, L - 1 others at 0: the true ls = log(1 + (L - 1) e^-15.5) is 3.7e-7 (L = 3) or 5.6e-7 (L = 4), either side of half an fp32 ulp of
    15.5 (4.8e-7), and within the lse's error of it: the helper evaluates both decisions"""
    inp = margin_case(L, 15.5)
    check(inp, G0, SPW, f"mask boundary L={L}")


def test_an_all_ignored_batch_has_no_span_loss():
    inp = ref.make_loss_case(4, 33, 3, 2, seed=9)
    inp["starts"][:], inp["ends"][:] = -1, -1
    loss, grads, r = check(inp, G0, SPW, "all ignored")
    assert not r["counted"].any()
    assert (grads["start"] == 0).all() and (grads["end"] == 0).all()
    assert np.abs(grads["rank"]).min() > 0


@pytest.mark.parametrize("both", [False, True])
def test_a_row_of_minus_infinity_stays_in_its_row(both):
    """row 1's start logits (and, `both`, its end logits) are all -inf and its candidates are real: the row's loss is NaN, so the total is; with
    finite end logits that row's d_end is non-finite too (d_start is 0: every entry sits at a -inf logit). The other rows are inside the bound."""
    inp = ref.make_loss_case(4, 48, 3, 2, seed=5)
    inp["start"][1] = -np.inf
    if both:
        inp["end"][1] = -np.inf
    inp["starts"][1], inp["ends"][1] = [7, 8, -1], [9, 8, -1]
    loss, grads, _ = check(inp, G0, SPW, f"-inf row both={both}", rows=[0, 2, 3])
    assert not np.isfinite(loss)
    assert (grads["start"][1] == 0).all()
    fin = np.isfinite(inp["end"][1])
    assert both or not np.isfinite(grads["end"][1][fin]).any()
    assert np.isfinite(grads["rank"]).all() and np.isfinite(grads["sp"]).all()


def test_an_overflowing_scale_arrives_as_infinity_of_the_right_sign():
    """g0 = 4096: g0 * offset * (sigmoid - label) leaves the fp16 range for the larger offsets; the fp32 value's sign survives"""
    inp = ref.make_loss_case(5, 512, 3, 30, seed=3)
    inp["label"][:] = 1
    loss, grads, r = check(inp, 4096.0, SPW, "g0=4096", keys=("start", "end", "rank"))
    want, got = r["grads"]["sp"], grads["sp"]
    assert np.isposinf(want).any() and np.isneginf(want).any()
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert not np.isnan(got).any() and fin.any()
    fp.assert_within(got[fin], want[fin], r["bounds"]["sp"][fin], "g0=4096 finite d_sp")


def test_two_runs_and_a_side_stream_give_the_same_bits():
    """(the second case: three trips through the candidate tiles, the LDS rows written three times)"""
    for B, L, A, NS in ((5, 257, 65, 5), (2, 512, 513, 5)):
        inp = ref.make_loss_case(B, L, A, NS, seed=11)
        a = run(inp)
        b = run(inp)
        c = run(inp, stream=torch.cuda.Stream())
        for other in (b, c):
            assert fp.same_bits(np.float32(a[0]), np.float32(other[0])), (A,)
            for k in a[1]:
                assert fp.same_bits(a[1][k], other[1][k]), (A, k)


@pytest.mark.parametrize("has_sp", [True, False])
def test_qa_loss_is_the_same_call_with_autograd(has_sp):
    """reader_loss.qa_loss: a [1] fp32 tensor, differentiable in the four score tensors, the bits of the C entry points; rank_score [B, 1] and label
    [B, 1] as the model and qa_collate shape them"""
    from multihop_dense_retrieval_amd import reader_loss
    inp = ref.make_loss_case(5, 65, 3, 5 if has_sp else 0, seed=13)
    loss_raw, grads_raw = run(inp)
    t = {k: dev(np.asarray(inp[k], np.float16)).requires_grad_(True) for k in KEYS if inp.get(k) is not None}
    t["rank"] = t["rank"].detach().reshape(-1, 1).requires_grad_(True)
    batch = {k: dev(inp[k]) for k in ("starts", "ends", "sent_offsets", "sent_labels")}
    batch["label"] = dev(inp["label"]).reshape(-1, 1)
    loss = reader_loss.qa_loss(t["start"], t["end"], t["rank"], t.get("sp"), batch, SPW)
    assert tuple(loss.shape) == (1,) and loss.dtype == torch.float32
    (loss * G0).sum().backward()
    torch.cuda.synchronize()
    assert fp.same_bits(np.float32(loss_raw), np.float32(loss.item()))
    for k, v in t.items():
        assert v.grad.dtype == torch.float16 and v.grad.shape == v.shape
        assert fp.same_bits(v.grad.cpu().numpy().reshape(grads_raw[k].shape), grads_raw[k]), k
