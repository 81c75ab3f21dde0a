"""The answer reader's training loss and its three heads as differentiable torch functions (include/mdr_reader_loss.h):

    qa_loss(start_logits, end_logits, rank_score, sp_score, batch, sp_weight)   the training branch of the reference's QAModel.forward
                                         (mdr/qa/qa_model.py:73-102) as a [1] fp32 device tensor, differentiable in the four score tensors
    reader_heads(h16, dense16, cu, batch, params, weight16=None)                qa_outputs, rank (behind the pooler's tanh) and sp on the
                                         trunk's packed final hidden states: the four score tensors, differentiable in h16, dense16 and the
                                         head parameters
    host_loss(...)                       the loss formula on the CPU by the reference's own sequence of torch calls (tests; not a fallback:
                                         the device functions raise on CPU tensors)

The loss (quirks of the reference kept). start / end logits are fp16 [B, L] with -inf outside the paragraph mask; per row and
candidate span log_prob = -(ce(start, s_a) + ce(end, e_a)) with ignore_index -1, in fp32 (CrossEntropyLoss runs in fp32 under apex O1). A
candidate is dropped iff log_prob == 0 EXACTLY (:89): the both-ignored padding, but also a real span whose fp32 loss is exactly 0; a
one-sided candidate counts with its valid side. span_loss = -sum over the rows with a non-zero marginal of log sum_a exp(log_prob).
rank_loss is a summed BCE of rank_score against label; sp_loss multiplies each BCE by the VALUE of sent_offsets (:78), not by a 0 / 1 mask.

Numerics (apex O1 as remembered, not captured: apex cannot be installed offline; criterions.py says the same of the in-batch loss). The
scores are fp16 and the loss is fp32; each score gradient is computed in fp32 and rounded to fp16 once, the backward of O1's cast in front
of the loss; the loss scale enters through the upstream gradient, which is read from device memory (no synchronisation). An overflow
becomes an infinity of the right sign, which optim.FusedAdam's overflow check sees. csrc/mdr_reader_loss.inl lists the
rounding points, tests/reader_loss_ref.py states them in fp64.

The heads. `params` holds the fp32 masters "qa_outputs.weight" [2, H], "qa_outputs.bias" [2], "rank.weight" [1, H], "rank.bias" [1] and, for
--sp-pred, "sp.weight" [1, H], "sp.bias" [1]; they are rounded to fp16 inside (weight AND bias, as apex O1 casts them and as
linear.packed_linear does), or weight16, the caller's fp16 [4, H] copy of the rows start, end, rank, sp, is used. The forward launches the
kernels of mdr_reader_forward: given the same h16 and dense16 the bits are the inference reader's. The pooler dense stays outside: the caller
composes dense16 = packed_linear(h16[cu[:-1]], pooler.dense.weight, pooler.dense.bias).
"""
import ctypes

import torch

from . import _lib
from ._lib import describe, is_like, ptr

_c = ctypes
_P = _c.c_void_p
# include/mdr_reader_loss.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_reader_loss_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "mdr_reader_loss_forward": (_c.c_int, [_P] * 9 + [_c.c_int] * 4 + [_c.c_float, _P, _P, _c.c_size_t, _c.c_int, _P]),
    "mdr_reader_loss_backward": (_c.c_int, [_P] * 9 + [_c.c_int] * 4 + [_c.c_float] + [_P] * 5 + [_c.c_int, _P]),
    "mdr_reader_heads_forward": (_c.c_int, [_P] * 5 + [_c.c_int] * 4 + [_P] * 6 + [_c.c_int, _P]),
    "mdr_reader_heads_backward_workspace_bytes": (_c.c_size_t, [_c.c_int] * 3),
    "mdr_reader_heads_backward": (_c.c_int, [_P] * 5 + [_c.c_int] * 5 + [_P] * 13 + [_c.c_int, _P, _c.c_size_t, _c.c_int, _P]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
MAX_L = 512
lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_reader_loss.h bound

HEAD_KEYS = ("qa_outputs.weight", "qa_outputs.bias", "rank.weight", "rank.bias", "sp.weight", "sp.bias")


def _i64(t, shape, dev, name):
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a tensor")
    t = t.to(device=dev, dtype=torch.int64).contiguous()
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be an int64 {list(shape)} tensor, got {describe(t)}")
    return t


def _loss_operands(start_logits, end_logits, rank_score, sp_score, batch):
    if not (torch.is_tensor(start_logits) and start_logits.is_cuda):
        raise RuntimeError("the reader's loss runs on a HIP device only (there is no CPU fallback)")
    dev = start_logits.device
    if start_logits.dtype != torch.float16 or start_logits.dim() != 2:
        raise ValueError(f"start_logits must be an fp16 [B, L] tensor, got {describe(start_logits)}")
    B, L = (int(n) for n in start_logits.shape)
    if B < 1 or not 1 <= L <= MAX_L:
        raise ValueError(f"[B, L] = [{B}, {L}]: B >= 1 and 1 <= L <= {MAX_L}")
    if not (torch.is_tensor(end_logits) and end_logits.dtype == torch.float16 and end_logits.device == dev and tuple(end_logits.shape) == (B, L)):
        raise ValueError(f"end_logits must be an fp16 [{B}, {L}] tensor on start_logits' device, got {describe(end_logits)}")
    if not (torch.is_tensor(rank_score) and rank_score.dtype == torch.float16 and rank_score.device == dev and rank_score.numel() == B):
        raise ValueError(f"rank_score must be an fp16 tensor of {B} elements on start_logits' device, got {describe(rank_score)}")
    starts = batch["starts"]
    A = int(starts.shape[1]) if torch.is_tensor(starts) and starts.dim() == 2 else 0
    if A < 1:
        raise ValueError(f"batch['starts'] must be an int64 [B, A >= 1] tensor, got {describe(starts)}")
    ints = {"starts": _i64(starts, (B, A), dev, "starts"), "ends": _i64(batch["ends"], (B, A), dev, "ends"),
            "label": _i64(batch["label"].reshape(-1), (B,), dev, "label"), "sent_offsets": None, "sent_labels": None}
    NS = 0
    if sp_score is not None:
        if not (torch.is_tensor(sp_score) and sp_score.dtype == torch.float16 and sp_score.device == dev and sp_score.dim() == 2 and sp_score.shape[0] == B):
            raise ValueError(f"sp_score must be an fp16 [{B}, NS] tensor on start_logits' device or None, got {describe(sp_score)}")
        NS = int(sp_score.shape[1])
        ints["sent_offsets"] = _i64(batch["sent_offsets"], (B, NS), dev, "sent_offsets")
        ints["sent_labels"] = _i64(batch["sent_labels"], (B, NS), dev, "sent_labels")
    return dev, B, L, A, NS, ints


class _QALoss(torch.autograd.Function):
    """forward: mdr_reader_loss_forward; backward: mdr_reader_loss_backward with the upstream gradient as a device scalar."""

    @staticmethod
    def forward(ctx, start_logits, end_logits, rank_score, sp_score, ints, shape, sp_weight):
        dev, (B, L, A, NS) = start_logits.device, shape
        s, e, r = (t.detach().contiguous() for t in (start_logits, end_logits, rank_score))
        sp = sp_score.detach().contiguous() if sp_score is not None else None
        L_ = lib()
        need = int(L_.mdr_reader_loss_workspace_bytes(B, L, A, NS))
        ws = _lib.workspace(need, dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        head = (ptr(s), ptr(e), ptr(r), ptr(sp), ptr(ints["starts"]), ptr(ints["ends"]), ptr(ints["label"]), ptr(ints["sent_offsets"]),
                ptr(ints["sent_labels"]), B, L, A, NS, float(sp_weight))
        _lib.call(L_.mdr_reader_loss_forward, *head, ptr(loss), ptr(ws), need, dev=dev)
        ctx.save_for_backward(s, e, r, *(() if sp is None else (sp,)))
        ctx.ints, ctx.shape, ctx.sp_weight, ctx.rank_shape = ints, shape, float(sp_weight), rank_score.shape
        return loss

    @staticmethod
    def backward(ctx, grad):
        s, e, r, *rest = ctx.saved_tensors
        sp = rest[0] if rest else None
        dev, (B, L, A, NS), ints = s.device, ctx.shape, ctx.ints
        g0 = grad.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        ds, de, dr = torch.empty_like(s), torch.empty_like(e), torch.empty_like(r)
        dsp = torch.empty_like(sp) if sp is not None else None
        _lib.call(lib().mdr_reader_loss_backward, ptr(s), ptr(e), ptr(r), ptr(sp), ptr(ints["starts"]), ptr(ints["ends"]), ptr(ints["label"]),
                  ptr(ints["sent_offsets"]), ptr(ints["sent_labels"]), B, L, A, NS, ctx.sp_weight, ptr(g0), ptr(ds), ptr(de), ptr(dr), ptr(dsp), dev=dev)
        return ds, de, dr.reshape(ctx.rank_shape), dsp, None, None, None


def qa_loss(start_logits, end_logits, rank_score, sp_score, batch, sp_weight):
    """qa_model.py:73-102 on the device: a [1] fp32 tensor (the shape the reference returns) that differentiates with respect to start_logits,
    end_logits, rank_score ([B] or [B, 1]) and sp_score (None without --sp-pred). `batch` holds starts / ends int64 [B, A], label [B] or [B, 1]
    and, with sp_score, sent_offsets / sent_labels [B, NS], as qa_collate pads them. Enqueued on the current stream."""
    dev, B, L, A, NS, ints = _loss_operands(start_logits, end_logits, rank_score, sp_score, batch)
    return _QALoss.apply(start_logits, end_logits, rank_score, sp_score, ints, (B, L, A, NS), float(sp_weight))


def heads_forward(h16, dense16, cu, pmask, offs, w16, b32, has_sp):
    """mdr_reader_heads_forward on prepared device tensors: (start, end fp16 [B, L], rank fp16 [B, 1], sp fp16 [B, NS] or None)."""
    dev, (B, L), H = h16.device, pmask.shape, int(h16.shape[1])
    NS = int(offs.shape[1]) if has_sp else 0
    start, end = (torch.empty((B, L), dtype=torch.float16, device=dev) for _ in range(2))
    rank = torch.empty((B, 1), dtype=torch.float16, device=dev)
    sp = torch.empty((B, NS), dtype=torch.float16, device=dev) if has_sp else None
    _lib.call(lib().mdr_reader_heads_forward, ptr(h16), ptr(cu), ptr(dense16), ptr(pmask), ptr(offs) if has_sp else None, B, L, NS, H, ptr(w16), ptr(b32),
              ptr(start), ptr(end), ptr(rank), ptr(sp) if NS else None, dev=dev)
    return start, end, rank, sp


def heads_backward(h16, dense16, cu, pmask, offs, w16, g_start, g_end, g_rank, g_sp, out=None, accumulate=False):
    """mdr_reader_heads_backward on prepared device tensors. `out`: None, or the dict of buffers to write (or add to): "d_h" fp16 [T, H], "d_dense"
    fp16 [B, H], "dw_qa" fp32 [2, H], "db_qa" [2], "dw_rank" [H], "db_rank" [1] and with g_sp "dw_sp" [H], "db_sp" [1]. Returns the dict."""
    dev, (B, L), (T, H) = h16.device, pmask.shape, h16.shape
    has_sp = g_sp is not None and g_sp.shape[1] > 0
    NS = int(g_sp.shape[1]) if has_sp else 0
    if out is None:
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        out = {"d_h": torch.empty_like(h16), "d_dense": torch.empty_like(dense16), "dw_qa": f32(2, H), "db_qa": f32(2), "dw_rank": f32(H), "db_rank": f32(1)}
        if has_sp:
            out.update({"dw_sp": f32(H), "db_sp": f32(1)})
    L_ = lib()
    need = int(L_.mdr_reader_heads_backward_workspace_bytes(B, L, H))
    ws = _lib.workspace(need, dev)
    _lib.call(L_.mdr_reader_heads_backward, ptr(h16), ptr(cu), ptr(dense16), ptr(pmask), ptr(offs) if has_sp else None, B, L, NS, H, int(T), ptr(w16),
              ptr(g_start), ptr(g_end), ptr(g_rank), ptr(g_sp) if has_sp else None, ptr(out["d_h"]), ptr(out["d_dense"]), ptr(out["dw_qa"]), ptr(out["db_qa"]),
              ptr(out.get("dw_sp")), ptr(out.get("db_sp")), ptr(out["dw_rank"]), ptr(out["db_rank"]), 1 if accumulate else 0, ptr(ws), need, dev=dev)
    return out


def head_rows16(params, has_sp, dev):
    """(fp16 [4, H] rows start, end, rank, sp -- the sp row 0 without an sp head -- and fp32 [4] biases rounded to fp16 values) of the masters."""
    rows = [params["qa_outputs.weight"].detach().reshape(2, -1), params["rank.weight"].detach().reshape(1, -1)]
    bias = [params["qa_outputs.bias"].detach().reshape(2), params["rank.bias"].detach().reshape(1)]
    if has_sp:
        rows.append(params["sp.weight"].detach().reshape(1, -1))
        bias.append(params["sp.bias"].detach().reshape(1))
    else:
        rows.append(torch.zeros_like(rows[1]))
        bias.append(torch.zeros_like(bias[1]))
    return torch.cat(rows).to(device=dev, dtype=torch.float16).contiguous(), torch.cat(bias).to(device=dev, dtype=torch.float16).float().contiguous()


class _ReaderHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h16, dense16, cu, pmask, offs, weight16, has_sp, w_qa, b_qa, w_rank, b_rank, w_sp, b_sp):
        dev = h16.device
        params = {"qa_outputs.weight": w_qa, "qa_outputs.bias": b_qa, "rank.weight": w_rank, "rank.bias": b_rank, "sp.weight": w_sp, "sp.bias": b_sp}
        w16, b32 = head_rows16(params, has_sp, dev)
        if weight16 is not None:
            w16 = weight16.detach()
        hd, dd = h16.detach(), dense16.detach()
        start, end, rank, sp = heads_forward(hd, dd, cu, pmask, offs, w16, b32, has_sp)
        ctx.save_for_backward(hd, dd, cu, pmask, w16, *((offs,) if has_sp else ()))
        ctx.has_sp = has_sp
        return (start, end, rank, sp) if has_sp else (start, end, rank)

    @staticmethod
    def backward(ctx, g_start, g_end, g_rank, g_sp=None):
        hd, dd, cu, pmask, w16, *rest = ctx.saved_tensors
        offs = rest[0] if rest else None
        h16g = lambda g, like: (torch.zeros(like, dtype=torch.float16, device=hd.device) if g is None  # noqa: E731
                                else g.detach().to(dtype=torch.float16).contiguous())
        B, L = pmask.shape
        g_start, g_end, g_rank = h16g(g_start, (B, L)), h16g(g_end, (B, L)), h16g(g_rank, (B, 1))
        if ctx.has_sp:
            g_sp = h16g(g_sp, tuple(offs.shape))
        o = heads_backward(hd, dd, cu, pmask, offs, w16, g_start, g_end, g_rank, g_sp if ctx.has_sp else None)
        need = ctx.needs_input_grad
        pick = lambda i, t: t if need[i] else None  # noqa: E731
        return (pick(0, o["d_h"]), pick(1, o["d_dense"]), None, None, None, None, None, pick(7, o["dw_qa"]), pick(8, o["db_qa"]),
                pick(9, o["dw_rank"].reshape(1, -1)), pick(10, o["db_rank"]), pick(11, o["dw_sp"].reshape(1, -1)) if ctx.has_sp else None,
                pick(12, o["db_sp"]) if ctx.has_sp else None)


def reader_heads(h16, dense16, cu, batch, params, weight16=None):
    """The reader's heads on packed rows: h16 fp16 [T, H] (the trunk's final hidden states), dense16 fp16 [B, H] (the pooler dense output),
    cu int32 [B + 1]; batch["paragraph_mask"] [B, L] and, when `params` has "sp.weight", batch["sent_offsets"] [B, NS]. Returns
    {"start_logits", "end_logits" fp16 [B, L], "rank_score" fp16 [B, 1], "sp_score" fp16 [B, NS] or None}, differentiable with respect to h16,
    dense16 and the head parameters (module docstring). An sp offset at or behind its row's length scores -inf and gets no gradient."""
    if not (torch.is_tensor(h16) and h16.is_cuda):
        raise RuntimeError("the reader's heads run on a HIP device only (there is no CPU fallback)")
    dev = h16.device
    if h16.dtype != torch.float16 or h16.dim() != 2 or not h16.is_contiguous():
        raise ValueError(f"h16 must be a contiguous fp16 [T, H] tensor, got {describe(h16)}")
    T, H = (int(n) for n in h16.shape)
    if H < 128 or H > 1024 or H % 128:
        raise ValueError(f"H = {H}: must be a multiple of 128, 128 .. 1024")
    pmask = batch["paragraph_mask"]
    if not (torch.is_tensor(pmask) and pmask.dim() == 2):
        raise ValueError("batch['paragraph_mask'] must be a [B, L] tensor")
    B, L = (int(n) for n in pmask.shape)
    pmask = _i64(pmask, (B, L), dev, "paragraph_mask")
    if not is_like(dense16, (torch.float16,), (B, H), dev):
        raise ValueError(f"dense16 must be a contiguous fp16 [{B}, {H}] tensor on h16's device, got {describe(dense16)}")
    if not is_like(cu, (torch.int32,), (B + 1,), dev):
        raise ValueError(f"cu must be an int32 [{B + 1}] tensor on h16's device, got {describe(cu)}")
    has_sp = "sp.weight" in params and params["sp.weight"] is not None
    offs = None
    if has_sp:
        offs = batch["sent_offsets"]
        offs = _i64(offs, (B, int(offs.shape[1])), dev, "sent_offsets")
        has_sp = offs.shape[1] > 0
    for k in HEAD_KEYS[:4] + (HEAD_KEYS[4:] if has_sp else ()):
        t = params[k]
        want = {"qa_outputs.weight": (2, H), "qa_outputs.bias": (2,)}.get(k, (1, H) if k.endswith("weight") else (1,))
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == dev and tuple(t.shape) == want):
            raise ValueError(f"{k} must be the fp32 master {list(want)} on h16's device, got {describe(t)}")
    if weight16 is not None and not is_like(weight16, (torch.float16,), (4, H), dev):
        raise ValueError(f"weight16 must be a contiguous fp16 [4, {H}] tensor on h16's device, got {describe(weight16)}")
    out = _ReaderHeads.apply(h16, dense16, cu, pmask, offs, weight16, has_sp, params["qa_outputs.weight"], params["qa_outputs.bias"], params["rank.weight"],
                             params["rank.bias"], params.get("sp.weight") if has_sp else None, params.get("sp.bias") if has_sp else None)
    return {"start_logits": out[0], "end_logits": out[1], "rank_score": out[2], "sp_score": out[3] if has_sp else None}


def host_loss(start_logits, end_logits, rank_score, sp_score, batch, sp_weight):
    """The training branch of qa_model.py:73-102 on the CPU in fp32 on the widened scores (what CrossEntropyLoss and the BCEs see under apex O1),
    stated with the same torch calls in the same order: a [1] fp32 tensor that differentiates through torch autograd. For tests."""
    F = torch.nn.functional
    s, e = start_logits.float().cpu(), end_logits.float().cpu()
    r = rank_score.float().cpu().reshape(-1, 1)
    label = batch["label"].cpu().reshape(-1, 1)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, reduction="none")
    rank_loss = F.binary_cross_entropy_with_logits(r, label.float(), reduction="sum")
    starts, ends = batch["starts"].cpu(), batch["ends"].cpu()
    loss_tensor = torch.stack([ce(s, a) for a in torch.unbind(starts, dim=1)], dim=1) + torch.stack([ce(e, a) for a in torch.unbind(ends, dim=1)], dim=1)
    log_prob = -loss_tensor
    log_prob = log_prob.masked_fill(log_prob == 0, float("-inf"))
    marginal = torch.sum(torch.exp(log_prob), dim=1)
    counted = marginal[marginal != 0]
    span_loss = -torch.log(counted).sum() if counted.numel() else s.sum() * 0.0
    loss = rank_loss + span_loss
    if sp_score is not None:
        sp = F.binary_cross_entropy_with_logits(sp_score.float().cpu(), batch["sent_labels"].cpu().float(), reduction="none")
        loss = loss + ((sp * batch["sent_offsets"].cpu()) * label).sum() * sp_weight
    return loss.unsqueeze(0)
