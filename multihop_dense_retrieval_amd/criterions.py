"""In-batch-negative evaluation of a retriever checkpoint (mdr/retrieval/criterions.py of the reference):

    mhop_eval(outputs, args)         :153-182  -> {"rrs_1": [...], "rrs_2": [...]}, on the device (include/mdr_inbatch.h)
    mhop_loss_value(outputs, fp16)   :114-151  the forward value of mhop_loss from the same kernel's log-sum-exp outputs
    mhop_loss_outputs(outputs, args, queue)    the loss as a 0-d device tensor WITH gradients for the six matrices, over 2B + 2 + K
                                     columns (K rows of a memory bank): mdr_inbatch_loss_forward / _backward, a torch.autograd.Function
    mhop_loss(model, batch, args)    :114-151  the reference's signature, with its --momentum branch (score, then enqueue)
    MemoryBank(k, d, device)         queue / queue_ptr / dequeue_and_enqueue of RobertaMomentumRetriever (mhop_retriever.py:64-106)
    mhop_eval_host(outputs, fp16)    the reference formula stated on the CPU (tests; not a fallback: mhop_eval never calls it)

`outputs` is what RobertaRetriever.forward returns: six [B, d] fp32 matrices q, q_sp1, c1, c2, neg_1, neg_2. Row i of a hop is
scored against 2B + 2 columns -- [c1; c2] and the row's own two negatives -- with column B + i masked to -inf in hop 1; the
targets are column i (hop 1) and B + i (hop 2); the reciprocal rank is 1 / rank of the target.

Ties. The reference ranks with `argsort(descending=True)`, which is not stable: the target's rank among EQUAL scores is whatever
the sort happens to do. Here the rule is rank = 1 + #{j : s_j > s_t} + #{j < t : s_j == s_t}, what a stable descending sort
gives (score descending, column ascending, as everywhere in this package). With fp16 scores of magnitude 10^2..10^3 (spacing
0.06..0.5) ties are not rare.

Numerics. Without --fp16 the scores are fp32 products. With --fp16 the reference runs under apex `amp.initialize(opt_level="O1")`,
which patches torch.mm / torch.bmm process-wide to cast their operands to fp16; the embeddings leave a LayerNorm in fp32, so every
score is fp16(fp32 accumulation of fp16(q) * fp16(c)), and the `.float().masked_fill(-inf).type_as(...)` round trip keeps it fp16.
CrossEntropyLoss runs in fp32 under O1, so the log-sum-exp is taken in fp32 over those fp16 values. This is apex behaviour as
remembered (apex is not installable offline, so no O1 run of the reference could be captured): the rounding points are pinned by
construction and by the exact-grid tests (tests/test_inbatch_rank_gpu.py), as reader.py does for its heads. The backward under O1
(equally remembered, not captured) rounds g = (p - onehot) * g0 / B to fp16 once, rounds the result of each mm / bmm backward to fp16
once and adds the terms of one leaf in fp32; csrc/mdr_inbatch_grad.hip lists the points, tests/mhop_loss_ref.py states them in fp64.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MDR_INBATCH_F32, MDR_INBATCH_O1 = 0, 1

_c = ctypes
# include/mdr_inbatch.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_inbatch_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "mdr_inbatch_rank": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                    _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
# include/mdr_inbatch_loss.h (which include/mdr_inbatch.h ends by including): a table of its own, so that each header is pinned against its own list
LOSS_SIGNATURES = {
    "mdr_inbatch_loss_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int64, _c.c_int]),
    "mdr_inbatch_loss_forward": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int64, _c.c_int, _c.c_int, _c.c_int] + [_c.c_void_p] * 5 + [_c.c_size_t, _c.c_void_p]),
    "mdr_inbatch_loss_backward": (_c.c_int, [_c.c_void_p] * 5 + [_c.c_int64, _c.c_int, _c.c_int, _c.c_int] + [_c.c_void_p] * 8 + [_c.c_size_t, _c.c_void_p]),
}
LOSS_EXPORTED_SYMBOLS = tuple(LOSS_SIGNATURES)
lib = _lib.binder(SIGNATURES, LOSS_SIGNATURES)  # libmdrhip.so with include/mdr_inbatch.h and include/mdr_inbatch_loss.h bound
_ptr = _lib.ptr


def inbatch_rank(q, q_sp, c1, c2, neg_1, neg_2, mode):
    """mdr_inbatch_rank on device tensors: {"rank1", "rank2"} int32 [B] (1-based), {"tscore1", "tscore2", "lse1", "lse2"} fp32 [B], all on
    the device, enqueued on the current stream (no synchronisation)."""
    if not (torch.is_tensor(q) and q.is_cuda):
        raise RuntimeError("the in-batch rank step runs on a HIP device only (there is no CPU fallback)")
    dev = q.device
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    q, q_sp = f(q), f(q_sp)
    B, d = q.shape
    ctx = torch.cat([f(c1), f(c2)], dim=0)
    neg = torch.stack([f(neg_1), f(neg_2)], dim=1).contiguous()
    if q_sp.shape != (B, d) or ctx.shape != (2 * B, d) or neg.shape != (B, 2, d):
        raise ValueError(f"q {tuple(q.shape)}, q_sp {tuple(q_sp.shape)}, [c1; c2] {tuple(ctx.shape)} and the negatives {tuple(neg.shape)} do not fit one batch")
    out = {k: torch.empty(B, dtype=torch.int32, device=dev) for k in ("rank1", "rank2")}
    out.update({k: torch.empty(B, dtype=torch.float32, device=dev) for k in ("tscore1", "tscore2", "lse1", "lse2")})
    L, p = lib(), _ptr
    need = int(L.mdr_inbatch_workspace_bytes(B, d, mode))
    ws = _lib.workspace(need, dev)
    _lib.call(L.mdr_inbatch_rank, p(q), p(q_sp), p(ctx), p(neg), B, d, int(mode), p(out["rank1"]), p(out["rank2"]), p(out["tscore1"]), p(out["tscore2"]),
              p(out["lse1"]), p(out["lse2"]), p(ws), need, dev=dev, device_arg=False)
    return out


def _mode(args_or_flag):
    fp16 = args_or_flag if isinstance(args_or_flag, bool) else bool(getattr(args_or_flag, "fp16", False))
    return MDR_INBATCH_O1 if fp16 else MDR_INBATCH_F32


def mhop_eval(outputs, args):
    """criterions.py:153-182 on the device: reciprocal ranks as Python floats. args.fp16 selects apex O1's fp16 scores."""
    r = inbatch_rank(outputs["q"], outputs["q_sp1"], outputs["c1"], outputs["c2"], outputs["neg_1"], outputs["neg_2"], _mode(args))
    ranks = torch.stack([r["rank1"], r["rank2"]]).cpu().tolist()  # one copy, one synchronisation
    return {"rrs_1": [1 / k for k in ranks[0]], "rrs_2": [1 / k for k in ranks[1]]}


def mhop_loss_value(outputs, fp16=False):
    """Forward value of mhop_loss (criterions.py:114-151; no backward is built): CrossEntropyLoss(mean) of hop 1 plus that of hop 2 =
    mean(lse1 - t1) + mean(lse2 - t2). Device tensors go through mdr_inbatch_rank; CPU tensors are evaluated by the host formula."""
    if outputs["q"].is_cuda:
        r = inbatch_rank(outputs["q"], outputs["q_sp1"], outputs["c1"], outputs["c2"], outputs["neg_1"], outputs["neg_2"], _mode(bool(fp16)))
        return float(((r["lse1"] - r["tscore1"]).mean() + (r["lse2"] - r["tscore2"]).mean()).item())
    s1, s2 = host_scores(outputs, fp16)
    B = s1.shape[0]
    t = torch.arange(B)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1)
    return float((ce(s1.float(), t) + ce(s2.float(), t + B)).item())


class _InbatchLoss(torch.autograd.Function):
    """loss = mean(lse1 - t1) + mean(lse2 - t2) over 2B + 2 + K columns. forward: mdr_inbatch_loss_forward; backward:
    mdr_inbatch_loss_backward with the upstream gradient passed as a device scalar (no synchronisation in either)."""

    @staticmethod
    def forward(ctx, q, q_sp, c1, c2, neg_1, neg_2, queue, mode):
        dev = q.device
        f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        q, q_sp = f(q), f(q_sp)
        B, d = q.shape
        cc = torch.cat([f(c1), f(c2)], dim=0)
        neg = torch.stack([f(neg_1), f(neg_2)], dim=1).contiguous()
        if q_sp.shape != (B, d) or cc.shape != (2 * B, d) or neg.shape != (B, 2, d):
            raise ValueError(f"q {tuple(q.shape)}, q_sp {tuple(q_sp.shape)}, [c1; c2] {tuple(cc.shape)} and the negatives {tuple(neg.shape)} do not fit one batch")
        if queue is not None:
            if not (queue.is_cuda and queue.device == dev and queue.dim() == 2 and queue.shape[1] == d):
                raise ValueError(f"the queue must be a [K, {d}] tensor on {dev}, got {tuple(queue.shape)} on {queue.device}")
            queue = f(queue) if queue.shape[0] else None  # a view of the caller's tensor when it is fp32 and contiguous: never written
        K = int(queue.shape[0]) if queue is not None else 0
        L = lib()
        out = torch.empty(4, B, dtype=torch.float32, device=dev)  # tscore1, tscore2, lse1, lse2
        need = int(L.mdr_inbatch_loss_workspace_bytes(B, d, K, int(mode)))
        ws = _lib.workspace(need, dev)
        _lib.call(L.mdr_inbatch_loss_forward, _ptr(q), _ptr(q_sp), _ptr(cc), _ptr(neg), _ptr(queue), K, B, d, int(mode), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]),
                  _ptr(out[3]), _ptr(ws), need, dev=dev, device_arg=False)
        ctx.save_for_backward(q, q_sp, cc, neg, out)
        ctx.queue, ctx.mode, ctx.ws, ctx.need = queue, int(mode), ws, need
        return (out[2] - out[0]).mean() + (out[3] - out[1]).mean()

    @staticmethod
    def backward(ctx, grad):
        q, q_sp, cc, neg, out = ctx.saved_tensors
        dev = q.device
        B, d = q.shape
        queue = ctx.queue
        K = int(queue.shape[0]) if queue is not None else 0
        g0 = grad.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        dq, dqsp, dctx, dneg = torch.empty_like(q), torch.empty_like(q_sp), torch.empty_like(cc), torch.empty_like(neg)
        _lib.call(lib().mdr_inbatch_loss_backward, _ptr(q), _ptr(q_sp), _ptr(cc), _ptr(neg), _ptr(queue), K, B, d, ctx.mode, _ptr(out[2]), _ptr(out[3]), _ptr(g0),
                  _ptr(dq), _ptr(dqsp), _ptr(dctx), _ptr(dneg), _ptr(ctx.ws), ctx.need, dev=dev, device_arg=False)
        return dq, dqsp, dctx[:B], dctx[B:], dneg[:, 0], dneg[:, 1], None, None


def mhop_loss_outputs(outputs, args, queue=None):
    """The loss of criterions.py:114-151 as a 0-d fp32 device tensor that differentiates with respect to q, q_sp1, c1, c2, neg_1, neg_2 (whichever
    carry grad). args.fp16 selects apex O1's numerics; `queue` is a [K, d] device tensor of further negatives (never written, no gradient) or None."""
    q = outputs["q"]
    if not (torch.is_tensor(q) and q.is_cuda):
        raise RuntimeError("the in-batch loss runs on a HIP device only (there is no CPU fallback)")
    return _InbatchLoss.apply(q, outputs["q_sp1"], outputs["c1"], outputs["c2"], outputs["neg_1"], outputs["neg_2"], queue, _mode(args))


def mhop_loss(model, batch, args):
    """criterions.py:114-151. With args.momentum the K rows of model.queue are scored as further negatives and the batch's [c1; c2] is enqueued
    afterwards, in the reference's order (score first, enqueue after). `model` is the callable that returns the six matrices; the queue is looked
    up on model.module first, as the reference does for its DataParallel-wrapped model, then on model."""
    outputs = model(batch)
    if not getattr(args, "momentum", False):
        return mhop_loss_outputs(outputs, args)
    bank = getattr(model, "module", model)
    # the backward reads the queue again, after the enqueue below has overwritten rows of it: score a copy, as the reference does (.clone().detach())
    loss = mhop_loss_outputs(outputs, args, queue=bank.queue.clone())
    bank.dequeue_and_enqueue(torch.cat([outputs["c1"], outputs["c2"]], dim=0).detach())
    return loss


class MemoryBank:
    """queue / queue_ptr / dequeue_and_enqueue of RobertaMomentumRetriever (mhop_retriever.py:64-68, :85-106): k earlier passage embeddings,
    initialised with torch.randn. A batch that would pass the end is TRUNCATED, not wrapped, and the pointer moves by what was written, modulo k."""

    def __init__(self, k, d, device="cpu"):
        self.k = int(k)
        self.queue = torch.randn(self.k, int(d)).to(device)
        self.queue_ptr = torch.zeros(1, dtype=torch.long)

    @torch.no_grad()
    def dequeue_and_enqueue(self, embeddings):
        n = embeddings.shape[0]
        ptr = int(self.queue_ptr)
        if ptr + n > self.k:
            n = self.k - ptr
            embeddings = embeddings[:n]
        self.queue[ptr:ptr + n, :] = embeddings.to(self.queue.dtype)
        self.queue_ptr[0] = (ptr + n) % self.k


def host_scores(outputs, fp16=False):
    """The reference's two [B, 2B + 2] score matrices on the CPU, by its own sequence of torch calls (mm, bmm, the masked_fill round
    trip, cat). fp16: the operands are cast to fp16 as apex O1's patched mm / bmm do, the products accumulate in fp32 and the result is
    rounded to fp16 (torch's CPU half matmul accumulates in fp32 as well, but in blocks that are rounded in between on some builds:
    the fp32 matmul of the widened operands followed by one rounding is the O1 contract stated literally)."""
    o = {k: v.detach().cpu().float() for k, v in outputs.items()}

    def mm(a, b):
        return torch.mm(a.half().float(), b.half().float()).half() if fp16 else torch.mm(a, b)

    def bmm(a, b):
        return torch.bmm(a.half().float(), b.half().float()).half() if fp16 else torch.bmm(a, b)

    all_ctx = torch.cat([o["c1"], o["c2"]], dim=0)
    neg_ctx = torch.cat([o["neg_1"].unsqueeze(1), o["neg_2"].unsqueeze(1)], dim=1)
    s1 = mm(o["q"], all_ctx.t())
    n1 = bmm(o["q"].unsqueeze(1), neg_ctx.transpose(1, 2)).squeeze(1)
    s2 = mm(o["q_sp1"], all_ctx.t())
    n2 = bmm(o["q_sp1"].unsqueeze(1), neg_ctx.transpose(1, 2)).squeeze(1)
    B = o["q"].size(0)
    mask = torch.cat([torch.zeros(B, B), torch.eye(B)], dim=1)
    s1 = s1.float().masked_fill(mask.bool(), float("-inf")).type_as(s1)
    return torch.cat([s1, n1], dim=1), torch.cat([s2, n2], dim=1)


def stable_ranks(scores, targets):
    """rank = 1 + #{j : s_j > s_t} + #{j < t : s_j == s_t} per row (1-based); a NaN target ranks last (NaN compares false)."""
    s = np.asarray(scores, dtype=np.float64)
    t = np.asarray(targets, dtype=np.int64)
    st = s[np.arange(s.shape[0]), t][:, None]
    before = np.arange(s.shape[1])[None, :] < t[:, None]
    rank = 1 + (s > st).sum(1) + ((s == st) & before).sum(1)
    return np.where(np.isnan(st[:, 0]), s.shape[1], rank)


def mhop_eval_host(outputs, fp16=False):
    """The reference formula with the stable tie rule, on the CPU (numpy / torch): what the tests hold mhop_eval against."""
    s1, s2 = host_scores(outputs, fp16)
    B = s1.shape[0]
    r1 = stable_ranks(s1.float().numpy(), np.arange(B))
    r2 = stable_ranks(s2.float().numpy(), np.arange(B) + B)
    return {"rrs_1": [1 / int(k) for k in r1], "rrs_2": [1 / int(k) for k in r2]}


def predict_summary(rrs_1, rrs_2):
    """predict() of scripts/train_mhop.py:244-250: the three log lines and the dict main() logs as `test performance`."""
    mrr_1 = np.mean(rrs_1)
    mrr_2 = np.mean(rrs_2)
    lines = [f"evaluated {len(rrs_1)} examples...", f"MRR-1: {mrr_1}", f"MRR-2: {mrr_2}"]
    return lines, {"mrr_1": mrr_1, "mrr_2": mrr_2, "mrr_avg": (mrr_1 + mrr_2) / 2}
