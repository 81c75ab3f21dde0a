"""A Linear of the trunk on packed rows as a differentiable torch function:

    packed_linear(x, weight, bias, gelu=False, rows=None, weight16=None) -> y = act(x weight^T + bias)

x is a CUDA fp16 tensor [M, K], weight the fp32 master [N, K] (rounded to fp16 inside, as apex O1's cast does), bias fp32 [N]; N and K are
multiples of 64. rows is an optional int32 device scalar tensor, the forward's m_dev: only the first rows[0] rows are valid, the others are
neither read as values nor written. The forward is the encoder's own GEMM (mdr_test_gemm_f16 of include/mdr_hip.h with kernel = 0 and
epilogue 0, or 1 with gelu): the output bits are the encoder's. The backward is mdr_linear_backward (include/mdr_linear_grad.h;
csrc/mdr_linear_grad.inl lists its rounding points): dx fp16, dweight and dbias fp32, no atomics, two runs give the same bits. With gelu the
backward first recomputes the pre-activation u = fp16(x weight^T + bias) with epilogue 0 into a temporary -- one more forward GEMM instead of
M x N fp16 kept alive per layer. Both directions are enqueued on the current stream and never synchronise. There is no
dropout and no CPU fallback. weight16, when given, is the caller's fp16 copy of weight (same shape and device; optim.FusedAdam keeps one
current): the forward and the saved tensor use it in place of the cast inside, and the gradient still goes to weight.
"""
import ctypes

import torch

from . import _lib
from ._lib import check_rows, describe, is_like, ptr

_c = ctypes
# include/mdr_linear_grad.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_linear_backward_chunks": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "mdr_linear_backward_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "mdr_linear_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
WANT_DX, WANT_DW, WANT_DB, WANT_PRE = 1, 2, 4, 8
lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_linear_grad.h bound


def backward_chunks(M, N, K):
    """(S, rows_per_chunk): the split of the token rows the weight-gradient kernel uses, a function of (M, N, K) alone."""
    rpc = ctypes.c_int(0)
    S = int(lib().mdr_linear_backward_chunks(int(M), int(N), int(K), ctypes.byref(rpc)))
    return S, int(rpc.value)


def _check_operands(x, w16, N, K):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("the packed Linear runs on a HIP device only (there is no CPU fallback)")
    if x.dtype != torch.float16 or x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] != K:
        raise ValueError(f"x must be a contiguous fp16 [M >= 1, {K}] tensor, got {describe(x)}")
    if N < 64 or K < 64 or N % 64 or K % 64:
        raise ValueError(f"weight [N, K] = [{N}, {K}]: N and K must be positive multiples of 64")
    if w16 is not None and not is_like(w16, (torch.float16,), (N, K), x.device):
        raise ValueError(f"w must be a contiguous fp16 [{N}, {K}] tensor on x's device, got {describe(w16)}")


def linear_backward(x, w, dy, pre=None, rows=None, need_dx=True, dw=None, db=None, accumulate=False):
    """mdr_linear_backward on device tensors. x fp16 [M, K], w fp16 [N, K], dy fp16 [M, N], pre None or the fp16 pre-activation [M, N],
    rows None or the int32 device scalar of valid rows. Returns (dx, dw, db): dx fp16 [M, K] (None unless need_dx; rows at or behind the
    valid count are NOT written -- they are zero here because the buffer starts zeroed), dw fp32 [N, K] and db fp32 [N] (the tensors given,
    written or with accumulate added to; None where None was given). Enqueued on the current stream."""
    if not torch.is_tensor(w) or w.dim() != 2:
        raise ValueError("w must be a 2-d tensor")
    N, K = int(w.shape[0]), int(w.shape[1])
    _check_operands(x, w, N, K)
    M, dev = int(x.shape[0]), x.device
    for name, t in (("dy", dy), ("pre", pre)):
        if t is not None and not is_like(t, (torch.float16,), (M, N), dev):
            raise ValueError(f"{name} must be a contiguous fp16 [{M}, {N}] tensor on x's device, got {describe(t)}")
    if dy is None:
        raise ValueError("dy is required")
    if rows is not None:
        check_rows(rows, x.device)
    for name, t, shape in (("dw", dw, (N, K)), ("db", db, (N,))):
        if t is not None and not is_like(t, (torch.float32,), shape, dev):
            raise ValueError(f"{name} must be a contiguous fp32 {list(shape)} tensor on x's device, got {describe(t)}")
    if not need_dx and dw is None and db is None:
        raise ValueError("nothing to compute: need_dx is False and dw and db are None")
    dx = torch.zeros((M, K), dtype=torch.float16, device=dev) if need_dx else None
    want = (WANT_DX if need_dx else 0) | (WANT_DW if dw is not None else 0) | (WANT_DB if db is not None else 0) | (WANT_PRE if pre is not None else 0)
    L = lib()
    need = int(L.mdr_linear_backward_workspace_bytes(M, N, K, want))
    ws = _lib.workspace(need, dev)
    _lib.call(L.mdr_linear_backward, ptr(x), ptr(w), ptr(dy), ptr(pre), M, ptr(rows), N, K, ptr(dx), ptr(dw), ptr(db), 1 if accumulate else 0, ptr(ws), need,
              dev=dev)
    return dx, dw, db


def _forward_gemm(x, w16, bias, rows, epilogue):
    """mdr_test_gemm_f16 with kernel = 0: the kernel the encoder picks for this shape. Rows at or behind the valid count stay zero."""
    M, (N, K), dev = x.shape[0], w16.shape, x.device
    out = torch.zeros((M, N), dtype=torch.float16, device=dev)
    _lib.call(_lib.lib().mdr_test_gemm_f16, ptr(x), ptr(w16), ptr(bias), M, ptr(rows), N, K, ptr(out), epilogue, 0, dev=dev)
    return out


class _PackedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gelu, rows, weight16=None):
        xd = x.detach()
        w16 = weight.detach().to(dtype=torch.float16).contiguous() if weight16 is None else weight16.detach()
        b32 = bias.detach().contiguous()
        ctx.save_for_backward(xd, w16, b32, rows)
        ctx.gelu = bool(gelu)
        return _forward_gemm(xd, w16, b32, rows, 1 if gelu else 0)

    @staticmethod
    def backward(ctx, grad):
        x, w16, b32, rows = ctx.saved_tensors
        g = grad.detach().to(dtype=torch.float16).contiguous()
        pre = _forward_gemm(x, w16, b32, rows, 0) if ctx.gelu else None
        need_dx, need_dw, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_dx or need_dw or need_db):
            return None, None, None, None, None, None
        dw = torch.empty(w16.shape, dtype=torch.float32, device=x.device) if need_dw else None
        db = torch.empty(w16.shape[0], dtype=torch.float32, device=x.device) if need_db else None
        dx, dw, db = linear_backward(x, w16, g, pre, rows, need_dx, dw, db, False)
        return dx, dw, db, None, None, None


def packed_linear(x, weight, bias, gelu=False, rows=None, weight16=None):
    """act(x weight^T + bias) on packed rows through the encoder's GEMM, differentiable with respect to x, weight and bias (module docstring)."""
    if not (torch.is_tensor(weight) and weight.dim() == 2):
        raise ValueError("weight must be a 2-d tensor")
    N, K = int(weight.shape[0]), int(weight.shape[1])
    _check_operands(x, weight16, N, K)
    if weight.dtype != torch.float32 or weight.device != x.device:
        raise ValueError(f"weight must be the fp32 master [{N}, {K}] on x's device, got {weight.dtype} {tuple(weight.shape)} on {weight.device}")
    if not (torch.is_tensor(bias) and bias.dtype == torch.float32 and bias.device == x.device and tuple(bias.shape) == (N,)):
        raise ValueError(f"bias must be an fp32 [{N}] tensor on x's device, got {getattr(bias, 'dtype', None)} {tuple(getattr(bias, 'shape', ()))}")
    if rows is not None:
        check_rows(rows, x.device)
    return _PackedLinear.apply(x, weight, bias, bool(gelu), rows, weight16)
