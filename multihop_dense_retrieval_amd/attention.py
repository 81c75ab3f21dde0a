"""Self-attention on the trunk's packed, ragged rows as a differentiable torch function:

    packed_self_attention(qkv, cu, heads, max_len, cls_only=False, dropout=None) -> ctx

qkv is a CUDA fp16 tensor [T, 3 * hidden] (a token's row is Q | K | V, head h in columns 64 h .. 64 h + 63 of each part), cu an int32
tensor [B + 1] on the same device; sequence b owns rows cu[b] .. cu[b + 1] - 1 and none is longer than max_len. The forward is the kernel
the encoder launches for max_len (mdr_test_attention of include/mdr_hip.h with kernel = 0; with cls_only the last layer's kernel 3, whose
context is [B, hidden], the first query of each sequence): the context bits are the encoder's. The backward is mdr_attention_backward
(include/mdr_attention_grad.h; csrc/mdr_attention_grad.hip lists its rounding points): no atomics, two runs give the same bits. The
gradient is returned for qkv only. Both directions are enqueued on the current stream and never synchronise.

dropout = (p, seed, site) drops attention probabilities as the reference's training does (attention_probs_dropout_prob = 0.1): the forward is
then mdr_attention_dropout_forward and the backward mdr_attention_dropout_backward (include/mdr_dropout.h), which replays the forward's mask
from (seed, site) -- nothing but qkv and cu is saved. The mask function, the rate actually drawn (dropout.effective_p) and the caller's duty to
give every use its own site or seed are those of dropout.py. With dropout=None, or a p whose threshold is 0, the call and its bits are the
ones above.
"""
import ctypes

import torch

from . import _lib
from . import dropout as _dropout
from ._lib import ptr

_c = ctypes
# include/mdr_attention_grad.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_attention_backward_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "mdr_attention_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                          _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
MODE_ALL, MODE_CLS = 0, 3
lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_attention_grad.h bound


def attention_backward(qkv, dctx, cu, heads, max_len, mode=MODE_ALL, out=None):
    """mdr_attention_backward on device tensors: dqkv, fp16 [T, 3 * hidden] (`out` if given: the call writes every row of the batch's
    sequences and nothing else). dctx is fp16 [T, hidden], or [B, hidden] in mode 3. Enqueued on the current stream."""
    dev = qkv.device
    B, hidden = cu.numel() - 1, qkv.shape[1] // 3
    dqkv = torch.empty_like(qkv) if out is None else out
    L = lib()
    need = int(L.mdr_attention_backward_workspace_bytes(B, int(max_len), int(heads), int(mode)))
    ws = _lib.workspace(need, dev)
    _lib.call(L.mdr_attention_backward, ptr(qkv), ptr(dctx), ptr(cu), B, int(max_len), hidden, int(heads), int(mode), ptr(dqkv), ptr(ws), need, dev=dev)
    return dqkv


def attention_dropout_forward(qkv, cu, heads, max_len, mode, T, seed, site, out=None):
    """mdr_attention_dropout_forward on device tensors: ctx, fp16 [T, hidden] (mode 3: [B, hidden]; `out` if given: the call writes the rows of the
    batch's non-empty sequences and nothing else). 1 <= T <= 255. Enqueued on the current stream."""
    dev = qkv.device
    B, hidden = cu.numel() - 1, qkv.shape[1] // 3
    ctx = torch.zeros((B if mode == MODE_CLS else qkv.shape[0], hidden), dtype=torch.float16, device=dev) if out is None else out
    _lib.call(_dropout.lib().mdr_attention_dropout_forward, ptr(qkv), ptr(cu), B, int(max_len), hidden, int(heads), int(mode), int(T), int(seed), int(site),
              ptr(ctx), dev=dev)
    return ctx


def attention_dropout_backward(qkv, dctx, cu, heads, max_len, mode, T, seed, site, out=None):
    """mdr_attention_dropout_backward on device tensors: attention_backward with the mask of (T, seed, site) replayed."""
    dev = qkv.device
    B, hidden = cu.numel() - 1, qkv.shape[1] // 3
    dqkv = torch.empty_like(qkv) if out is None else out
    need = int(lib().mdr_attention_backward_workspace_bytes(B, int(max_len), int(heads), int(mode)))
    ws = _lib.workspace(need, dev)
    _lib.call(_dropout.lib().mdr_attention_dropout_backward, ptr(qkv), ptr(dctx), ptr(cu), B, int(max_len), hidden, int(heads), int(mode), int(T), int(seed),
              int(site), ptr(dqkv), ptr(ws), need, dev=dev)
    return dqkv


class _PackedSelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cu, heads, max_len, cls_only, drop):
        dev = qkv.device
        B, hidden = cu.numel() - 1, qkv.shape[1] // 3
        q = qkv.detach()
        ctx.heads, ctx.max_len, ctx.mode, ctx.drop = int(heads), int(max_len), MODE_CLS if cls_only else MODE_ALL, drop
        if drop is None:
            out = torch.empty((B if cls_only else q.shape[0], hidden), dtype=torch.float16, device=dev)
            _lib.call(_lib.lib().mdr_test_attention, ptr(q), ptr(cu), None, B, int(max_len), hidden, int(heads), 3 if cls_only else 0, ptr(out), dev=dev)
        else:
            out = attention_dropout_forward(q, cu, ctx.heads, ctx.max_len, ctx.mode, *drop)
        ctx.save_for_backward(q, cu)
        return out

    @staticmethod
    def backward(ctx, grad):
        q, cu = ctx.saved_tensors
        g = grad.detach().to(dtype=torch.float16).contiguous()
        if ctx.drop is None:
            return attention_backward(q, g, cu, ctx.heads, ctx.max_len, ctx.mode), None, None, None, None, None
        return attention_dropout_backward(q, g, cu, ctx.heads, ctx.max_len, ctx.mode, *ctx.drop), None, None, None, None, None


def packed_self_attention(qkv, cu, heads, max_len, cls_only=False, dropout=None):
    """softmax(Q K^T / 8) V per (sequence, head) on packed rows, differentiable with respect to qkv; dropout = (p, seed, site) drops
    probabilities (module docstring)."""
    if not (torch.is_tensor(qkv) and qkv.is_cuda):
        raise RuntimeError("packed self-attention runs on a HIP device only (there is no CPU fallback)")
    if qkv.dtype != torch.float16 or qkv.dim() != 2 or not qkv.is_contiguous() or qkv.shape[1] != 3 * 64 * int(heads):
        raise ValueError(f"qkv must be a contiguous fp16 [T, {3 * 64 * int(heads)}] tensor, got {qkv.dtype} {tuple(qkv.shape)}")
    if not (torch.is_tensor(cu) and cu.device == qkv.device and cu.dtype == torch.int32 and cu.dim() == 1 and cu.numel() >= 2 and cu.is_contiguous()):
        raise ValueError("cu must be a contiguous int32 [B + 1] tensor on qkv's device")
    if not 1 <= int(max_len) <= 512:
        raise ValueError(f"max_len = {max_len} outside 1..512")
    drop = None
    if dropout is not None:
        p, seed, site = dropout
        T = _dropout.threshold(p)
        if T:
            drop = (T,) + _dropout.check_seed_site(seed, site)
    return _PackedSelfAttention.apply(qkv, cu, int(heads), int(max_len), bool(cls_only), drop)
