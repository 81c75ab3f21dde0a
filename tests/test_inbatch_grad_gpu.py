"""GPU (-m gpu): mdr_inbatch_loss_forward / mdr_inbatch_loss_backward (include/mdr_inbatch_loss.h) through criterions.mhop_loss_outputs, against the
fp64 statement of tests/mhop_loss_ref.py. Every element of the loss and of the six gradients must sit inside that helper's DERIVED bound (fp32
accumulation in any order; mode O1: the listed fp16 rounding points applied in the helper, a flipped rounding allowed only where a rounding
boundary lies within the fp32 accumulation error). Inputs are LayerNorm-like rows scaled so that scores are O(1-10) (mhop_loss_ref.make_inputs).
Mode O1 runs with a loss scale g0 = 2^12, as an amp run has one: without it g = p / B is below the smallest fp16 number for most columns of the
queue (2^16, amp's starting value, overflows fp16 at B = 1, where amp would skip the step: tests/test_overflow_gpu.py asserts both halves of that).
"""
import contextlib
import os
import types

import numpy as np
import pytest
import torch

import mhop_loss_ref as ref

pytestmark = pytest.mark.gpu

F32, O1 = 0, 1
O1_SCALE = 4096.0
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mhop_loss_grad_ref.npz")

# B covers the 16-column tile and the 32-row workgroup edges, d the smallest, the shipping and the largest width, K the 16-row queue tile edges and
# (4097 = 257 tiles) three chunks of 128 tiles. Every B, every d and every K appears; (33, 768) meets every K and (17, .., 17) every d.
SHAPES = [(1, 32, 0), (2, 768, 1), (15, 1024, 15), (16, 32, 17), (17, 768, 4097), (31, 1024, 0), (32, 32, 1), (33, 768, 15), (150, 1024, 17),
          (33, 768, 0), (33, 768, 1), (33, 768, 17), (33, 768, 4097), (17, 32, 17), (17, 1024, 17), (150, 768, 4097), (150, 32, 0)]


def run(inp, queue, mode, g0=1.0, stream=None):
    """(loss, grads) as numpy from one forward + backward on the device."""
    from multihop_dense_retrieval_amd import criterions
    t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda().requires_grad_(True) for k, v in inp.items()}
    qd = torch.from_numpy(np.ascontiguousarray(queue, dtype=np.float32)).cuda() if queue is not None else None
    args = types.SimpleNamespace(fp16=mode == O1)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
        loss = criterions.mhop_loss_outputs(t, args, queue=qd)
        (loss * g0).backward()
    torch.cuda.synchronize()
    return float(loss), {k: v.grad.cpu().numpy() for k, v in t.items()}


def check(inp, queue, mode, g0, label):
    r = ref.loss_and_grads(inp, queue, g0=g0, o1=mode == O1)
    loss, grads = run(inp, queue, mode, g0)
    print(label, {k: f"{v[0]:.2e}/{v[1]:.2e}={v[2]:.3f}" for k, v in ref.worst(r, loss, grads).items()})
    assert ref.violations(r, loss, grads) == [], label
    return loss, grads


@pytest.mark.parametrize("mode", [F32, O1])
@pytest.mark.parametrize("B,d,K", SHAPES)
def test_loss_and_gradients_within_the_derived_bound(B, d, K, mode):
    inp, queue = ref.make_inputs(B, d, K, seed=7 * B + d + K)
    check(inp, queue, mode, 1.0 if mode == F32 else O1_SCALE, f"B={B} d={d} K={K} mode={mode}")


@pytest.mark.parametrize("mode", [F32, O1])
def test_readme_shape(mode):
    """B = 150, K = 76800, d = 768: stage 2 of the README (the queue of 76800 earlier passages)."""
    inp, queue = ref.make_inputs(150, 768, 76800, seed=5)
    check(inp, queue, mode, 1.0 if mode == F32 else O1_SCALE, f"README shape mode={mode}")


def margin_inputs(B, d, K):
    """Rows of +-1: q_i = qsp_i = c1_i = c2_i = e_i-like sign patterns that are mutually orthogonal (Hadamard rows), everything else orthogonal to all
    of them or zero: the target scores d = 256 (exact in fp16), every other score 0, so every other exp(0 - 256) underflows to 0 in fp32."""
    H = np.array([[1.0]])
    while H.shape[0] < d:
        H = np.block([[H, H], [H, -H]])
    rows = H[1:B + 1].astype(np.float32)
    inp = {"q": rows, "q_sp1": rows.copy(), "c1": rows.copy(), "c2": rows.copy(), "neg_1": np.zeros((B, d), np.float32), "neg_2": np.zeros((B, d), np.float32)}
    queue = H[B + 1:B + 1 + K].astype(np.float32) if K else None
    return inp, queue


@pytest.mark.parametrize("mode", [F32, O1])
def test_a_large_margin_gives_exactly_zero(mode):
    """(a) hop 1: target c1_i scores 256, its twin c2_i is the masked column; hop 2: c1_i and c2_i both score 256 -- so hop 2 uses q_sp rows that only
    c2 matches: c1 is moved to other Hadamard rows for it. All other scores are 0 and exp(-256) is 0 in fp32."""
    B, d, K = 17, 256, 33
    inp, queue = margin_inputs(B, d, K)
    H = margin_inputs(2 * B + K + 40, d, 0)[0]["q"]
    inp["q_sp1"] = H[B + K + 2:2 * B + K + 2].copy()
    inp["c2"] = inp["q_sp1"].copy()  # hop 1 sees c2 as 0-score columns (and masks its own), hop 2 sees c1 as 0-score columns
    loss, grads = run(inp, queue, mode, 1.0)
    assert loss == 0.0
    for k, g in grads.items():
        assert np.all(g == 0.0), k


@pytest.mark.parametrize("mode", [F32, O1])
def test_the_masked_column_gives_nothing_to_dc2(mode):
    """(b) q_sp = 0 makes every hop-2 score 0; with g0 fixed, hop 2 then sends g2_ij q_sp_i = 0 to dctx, so dc2 holds hop 1 alone. Row i of hop 1 must
    not reach dc2[i]: with B = 1 that is the only row there is, so dc2 is exactly 0 even though c2[0] would score highest; and for B = 19 the helper with
    the mask (accepted) and without it (rejected) differ in dc2."""
    inp, queue = ref.make_inputs(1, 64, 9, seed=3)
    inp["q_sp1"][:] = 0
    inp["c2"] = (3.0 * inp["q"]).copy()
    _, grads = run(inp, queue, mode, 1.0)
    assert np.all(grads["c2"] == 0.0) and np.any(grads["c1"] != 0.0)
    inp, queue = ref.make_inputs(19, 64, 9, seed=4)
    inp["q_sp1"][:] = 0
    inp["c2"] = (0.5 * inp["q"] + inp["c2"]).astype(np.float32)
    g0 = 1.0 if mode == F32 else O1_SCALE
    _, grads = check(inp, queue, mode, g0, f"masked column mode={mode}")
    wrong = ref.loss_and_grads(inp, queue, g0=g0, o1=mode == O1, mutate="no_mask")
    assert "c2" in ref.violations(wrong, None, grads)


@pytest.mark.parametrize("mode", [F32, O1])
def test_identical_rows(mode):
    """The structural case: every question, passage and negative is the same vector. All scores are equal, p = 1 / (number of unmasked columns)."""
    B, d, K = 5, 64, 3
    v = ref.layernorm_like(np.random.default_rng(1), 1, d)
    inp = {k: np.repeat(v, B, axis=0) for k in ref.KEYS}
    check(inp, np.repeat(v, K, axis=0), mode, 1.0 if mode == F32 else O1_SCALE, f"identical rows mode={mode}")


@pytest.mark.parametrize("mode", [F32, O1])
def test_queue_untouched_same_bits_twice_and_on_a_second_stream(mode):
    """(c) the queue keeps its bits through forward and backward; two runs agree bit for bit (no atomics); a side stream gives the same bits."""
    from multihop_dense_retrieval_amd import criterions
    inp, queue = ref.make_inputs(33, 768, 4097, seed=11)
    t = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in inp.items()}
    qd = torch.from_numpy(queue).cuda()
    loss = criterions.mhop_loss_outputs(t, types.SimpleNamespace(fp16=mode == O1), queue=qd)
    loss.backward()
    torch.cuda.synchronize()
    assert np.array_equal(qd.cpu().numpy().view(np.uint32), queue.view(np.uint32))
    a = run(inp, queue, mode, 3.0)
    b = run(inp, queue, mode, 3.0)
    c = run(inp, queue, mode, 3.0, stream=torch.cuda.Stream())
    for other in (b, c):
        assert a[0] == other[0]
        for k in ref.KEYS:
            assert np.array_equal(a[1][k].view(np.uint32), other[1][k].view(np.uint32)), k


def test_doubling_g0_doubles_every_f32_gradient_exactly():
    """(d)"""
    inp, queue = ref.make_inputs(33, 768, 17, seed=12)
    a = run(inp, queue, F32, 1.5)
    b = run(inp, queue, F32, 3.0)
    for k in ref.KEYS:
        assert np.array_equal((2.0 * a[1][k]).view(np.uint32), b[1][k].view(np.uint32)), k


@pytest.mark.parametrize("mode", [F32, O1])
@pytest.mark.parametrize("B,d", [(1, 32), (33, 768), (150, 1024)])
def test_without_a_queue_the_forward_equals_the_rank_step_bit_for_bit(B, d, mode):
    from multihop_dense_retrieval_amd import criterions
    inp, _ = ref.make_inputs(B, d, 0, seed=13)
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    r = criterions.inbatch_rank(t["q"], t["q_sp1"], t["c1"], t["c2"], t["neg_1"], t["neg_2"], mode)
    L = criterions.lib()
    ctx = torch.cat([t["c1"], t["c2"]])
    neg = torch.stack([t["neg_1"], t["neg_2"]], dim=1).contiguous()
    out = torch.empty(4, B, dtype=torch.float32, device="cuda")
    p = criterions._ptr
    from multihop_dense_retrieval_amd import _lib
    assert L.mdr_inbatch_loss_workspace_bytes(B, d, 0, mode) > 0
    ws = torch.empty(int(L.mdr_inbatch_loss_workspace_bytes(B, d, 0, mode)), dtype=torch.uint8, device="cuda")
    _lib.check(L.mdr_inbatch_loss_forward(p(t["q"]), p(t["q_sp1"]), p(ctx), p(neg), None, 0, B, d, mode, p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(ws),
                                          ws.numel(), _lib.current_stream_ptr(out.device)))
    torch.cuda.synchronize()
    for i, k in enumerate(("tscore1", "tscore2", "lse1", "lse2")):
        assert np.array_equal(out[i].cpu().numpy().view(np.uint32), r[k].cpu().numpy().view(np.uint32)), k


def test_bad_shapes_return_an_error_and_launch_nothing():
    from multihop_dense_retrieval_amd import criterions
    L = criterions.lib()
    x = torch.zeros(64, 48, device="cuda")
    p = criterions._ptr
    assert L.mdr_inbatch_loss_workspace_bytes(4, 48, 0, 0) == 0 and L.mdr_inbatch_loss_workspace_bytes(4, 64, -1, 0) == 0
    for B, d, K, mode, queue in ((0, 64, 0, 0, None), (4, 48, 0, 0, None), (4, 2048, 0, 0, None), (4, 64, -1, 0, None), (4, 64, 0, 2, None), (4, 64, 8, 0, None)):
        rc = L.mdr_inbatch_loss_forward(p(x), p(x), p(x), p(x), queue, K, B, d, mode, p(x), p(x), p(x), p(x), p(x), x.numel() * 4, None)
        assert rc != 0, (B, d, K, mode)
        rc = L.mdr_inbatch_loss_backward(p(x), p(x), p(x), p(x), queue, K, B, d, mode, p(x), p(x), p(x), p(x), p(x), p(x), p(x), p(x), x.numel() * 4, None)
        assert rc != 0, (B, d, K, mode)
    assert L.mdr_inbatch_loss_backward(p(x), p(x), p(x), p(x), None, 0, 4, 32, 0, p(x), p(x), p(x), p(x), p(x), p(x), p(x), p(x), 16, None) != 0  # workspace too small
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0


@pytest.mark.parametrize("mode", [F32, O1])
def test_a_nan_row_of_q_stays_in_its_own_row_of_dq(mode):
    inp, queue = ref.make_inputs(33, 64, 17, seed=14)
    g0 = 1.0 if mode == F32 else O1_SCALE
    clean = run(inp, queue, mode, g0)
    bad = {k: v.copy() for k, v in inp.items()}
    bad["q"][5, 3] = np.nan
    loss, grads = run(bad, queue, mode, g0)
    assert np.isnan(loss)
    assert np.all(np.isnan(grads["q"][5])) and np.all(np.isnan(grads["neg_1"][5])) and np.all(np.isnan(grads["c1"]))  # IEEE propagation, nothing else
    keep = np.arange(33) != 5
    assert np.array_equal(grads["q"][keep].view(np.uint32), clean[1]["q"][keep].view(np.uint32))
    assert np.array_equal(grads["q_sp1"].view(np.uint32), clean[1]["q_sp1"].view(np.uint32))  # hop 2 never sees q


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


class StubModel:
    def __init__(self, outputs, bank=None):
        self.outputs = outputs
        if bank is not None:
            self.queue, self.dequeue_and_enqueue, self.bank = bank.queue, bank.dequeue_and_enqueue, bank

    def __call__(self, batch):
        return self.outputs


@pytest.mark.parametrize("B,K", [(B, K) for B in (1, 3, 17) for K in (0, 5, 40)])
def test_the_reference_fixture_on_the_device(gold, B, K):
    """What gradcheck would be for (fp32 makes it useless): the reference's own loss, six gradients and queue after the step, through mhop_loss(model,
    batch, args) with a stub model. With --momentum the queue is scored first and enqueued afterwards; without it no queue is touched."""
    from multihop_dense_retrieval_amd import criterions
    pre = f"B{B}_K{K}."
    inp = {k: gold[pre + k] for k in ref.KEYS}
    t = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in inp.items()}
    args = types.SimpleNamespace(fp16=False, momentum=K > 0)
    bank = None
    if K:
        bank = criterions.MemoryBank(K, 32, "cuda")
        bank.queue.copy_(torch.from_numpy(gold[pre + "queue_before"]))
        bank.queue_ptr[0] = int(gold[pre + "ptr_before"])
    model = StubModel(t, bank)
    loss = criterions.mhop_loss(model, None, args)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    loss.backward()  # after the enqueue: the gradients must still be those of the queue that was scored
    torch.cuda.synchronize()
    r = ref.loss_and_grads(inp, gold[pre + "queue_before"] if K else None)
    grads = {k: v.grad.cpu().numpy() for k, v in t.items()}
    assert ref.violations(r, float(loss), grads) == []
    assert ref.violations(r, float(gold[pre + "loss"]), {k: gold[pre + "grad." + k] for k in ref.KEYS}) == []  # and so is the reference: same bound
    if K:
        assert np.array_equal(bank.queue.cpu().numpy(), gold[pre + "queue_after"])
        assert int(bank.queue_ptr) == int(gold[pre + "ptr_after"])
    else:
        assert not hasattr(model, "queue")
