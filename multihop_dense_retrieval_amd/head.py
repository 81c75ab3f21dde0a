"""The retriever's head Linear (project.0) as a differentiable torch function whose output stays in fp32:

    packed_head_linear(x, weight, bias, weight16=None) -> y32 = x weight^T + bias

x is a CUDA fp16 tensor [M, K], weight the fp32 master [N, K] (rounded to fp16 inside, as apex O1's cast does), bias fp32 [N]; N and K are
multiples of 64 and M >= 1. There is no rows argument: the head runs on the B CLS rows of a batch, all valid. The forward is the encoder's
own GEMM with its fp32 epilogue (mdr_test_gemm_f16 of include/mdr_hip.h with kernel = 0 and epilogue 3): the output bits are the ones
encode_q hands to the last LayerNorm, where linear.packed_linear rounds them to fp16 once more. The backward is mdr_head_backward
(include/mdr_head_grad.h; csrc/mdr_head_grad.hip lists its rounding points): the fp32 gradient of y32 is taken as it is, never rounded to
fp16; dx fp16, dweight and dbias fp32, no atomics, two runs give the same bits, and a non-finite gradient element arrives non-finite in all
three. Both directions are enqueued on the current stream and never synchronise. There is no CPU fallback. weight16, when given, is the
caller's fp16 copy of weight (optim.FusedAdam keeps one current): the forward and the saved tensor use it in place of the cast inside, and
the gradient still goes to weight.
"""
import ctypes

import torch

from . import _lib
from ._lib import describe, is_like, ptr

_c = ctypes
# include/mdr_head_grad.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_head_backward_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "mdr_head_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                     _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
WANT_DX, WANT_DW, WANT_DB = 1, 2, 4
CHUNK = 128  # token rows per chunk of the dW / db sums: S = ceil(M / 128)
lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_head_grad.h bound


def _check_operands(x, w16, N, K):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("the head Linear runs on a HIP device only (there is no CPU fallback)")
    if x.dtype != torch.float16 or x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] != K:
        raise ValueError(f"x must be a contiguous fp16 [M >= 1, {K}] tensor, got {describe(x)}")
    if N < 64 or K < 64 or N % 64 or K % 64:
        raise ValueError(f"weight [N, K] = [{N}, {K}]: N and K must be positive multiples of 64")
    if w16 is not None and not is_like(w16, (torch.float16,), (N, K), x.device):
        raise ValueError(f"w must be a contiguous fp16 [{N}, {K}] tensor on x's device, got {describe(w16)}")


def head_backward(x, w, dy, need_dx=True, dw=None, db=None, accumulate=False):
    """mdr_head_backward on device tensors. x fp16 [M, K], w fp16 [N, K], dy fp32 [M, N]. Returns (dx, dw, db): dx fp16 [M, K] (None unless
    need_dx), dw fp32 [N, K] and db fp32 [N] (the tensors given, written or with accumulate added to; None where None was given). Enqueued on
    the current stream."""
    if not torch.is_tensor(w) or w.dim() != 2:
        raise ValueError("w must be a 2-d tensor")
    N, K = int(w.shape[0]), int(w.shape[1])
    _check_operands(x, w, N, K)
    M, dev = int(x.shape[0]), x.device
    if not is_like(dy, (torch.float32,), (M, N), dev):
        raise ValueError(f"dy must be a contiguous fp32 [{M}, {N}] tensor on x's device, got {describe(dy)}")
    for name, t, shape in (("dw", dw, (N, K)), ("db", db, (N,))):
        if t is not None and not is_like(t, (torch.float32,), shape, dev):
            raise ValueError(f"{name} must be a contiguous fp32 {list(shape)} tensor on x's device, got {describe(t)}")
    if not need_dx and dw is None and db is None:
        raise ValueError("nothing to compute: need_dx is False and dw and db are None")
    dx = torch.empty((M, K), dtype=torch.float16, device=dev) if need_dx else None
    want = (WANT_DX if need_dx else 0) | (WANT_DW if dw is not None else 0) | (WANT_DB if db is not None else 0)
    L = lib()
    need = int(L.mdr_head_backward_workspace_bytes(M, N, K, want))
    ws = _lib.workspace(need, dev)
    _lib.call(L.mdr_head_backward, ptr(x), ptr(w), ptr(dy), M, N, K, ptr(dx), ptr(dw), ptr(db), 1 if accumulate else 0, ptr(ws), need, dev=dev)
    return dx, dw, db


def head_forward(x, w16, bias):
    """mdr_test_gemm_f16 with kernel = 0 and epilogue 3: fp32 [M, N], the sums the encoder's head hands to its LayerNorm."""
    M, (N, K), dev = x.shape[0], w16.shape, x.device
    out = torch.empty((M, N), dtype=torch.float32, device=dev)
    _lib.call(_lib.lib().mdr_test_gemm_f16, ptr(x), ptr(w16), ptr(bias), M, None, N, K, ptr(out), 3, 0, dev=dev)
    return out


class _PackedHeadLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, weight16=None):
        xd = x.detach()
        w16 = weight.detach().to(dtype=torch.float16).contiguous() if weight16 is None else weight16.detach()
        ctx.save_for_backward(xd, w16)
        return head_forward(xd, w16, bias.detach().contiguous())

    @staticmethod
    def backward(ctx, grad):
        x, w16 = ctx.saved_tensors
        need_dx, need_dw, need_db = ctx.needs_input_grad[:3]
        if not (need_dx or need_dw or need_db):
            return None, None, None, None
        g = grad.detach().to(dtype=torch.float32).contiguous()
        dw = torch.empty(w16.shape, dtype=torch.float32, device=x.device) if need_dw else None
        db = torch.empty(w16.shape[0], dtype=torch.float32, device=x.device) if need_db else None
        dx, dw, db = head_backward(x, w16, g, need_dx, dw, db, False)
        return dx, dw, db, None


def packed_head_linear(x, weight, bias, weight16=None):
    """x weight^T + bias in fp32 through the encoder's GEMM, differentiable with respect to x, weight and bias (module docstring)."""
    if not (torch.is_tensor(weight) and weight.dim() == 2):
        raise ValueError("weight must be a 2-d tensor")
    N, K = int(weight.shape[0]), int(weight.shape[1])
    _check_operands(x, weight16, N, K)
    if weight.dtype != torch.float32 or weight.device != x.device:
        raise ValueError(f"weight must be the fp32 master [{N}, {K}] on x's device, got {weight.dtype} {tuple(weight.shape)} on {weight.device}")
    if not (torch.is_tensor(bias) and bias.dtype == torch.float32 and bias.device == x.device and tuple(bias.shape) == (N,)):
        raise ValueError(f"bias must be an fp32 [{N}] tensor on x's device, got {getattr(bias, 'dtype', None)} {tuple(getattr(bias, 'shape', ()))}")
    return _PackedHeadLinear.apply(x, weight, bias, weight16)
