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
_bound = False


def lib():
    """libmdrhip.so with the signatures of include/mdr_linear_grad.h bound (AttributeError if the library lacks one: no fallback)."""
    global _bound
    L = _lib.lib()
    if not _bound:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _bound = True
    return L


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _dev_index(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


def backward_chunks(M, N, K):
    """(S, rows_per_chunk): the split of the token rows the weight-gradient kernel uses, a function of (M, N, K) alone."""
    rpc = ctypes.c_int(0)
    S = int(lib().mdr_linear_backward_chunks(int(M), int(N), int(K), ctypes.byref(rpc)))
    return S, int(rpc.value)


def _check_operands(x, w16, N, K):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("the packed Linear runs on a HIP device only (there is no CPU fallback)")
    if x.dtype != torch.float16 or x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] != K:
        raise ValueError(f"x must be a contiguous fp16 [M >= 1, {K}] tensor, got {x.dtype} {tuple(x.shape)}")
    if N < 64 or K < 64 or N % 64 or K % 64:
        raise ValueError(f"weight [N, K] = [{N}, {K}]: N and K must be positive multiples of 64")
    if w16 is not None and not (w16.dtype == torch.float16 and w16.is_contiguous() and w16.device == x.device and tuple(w16.shape) == (N, K)):
        raise ValueError(f"w must be a contiguous fp16 [{N}, {K}] tensor on x's device, got {w16.dtype} {tuple(w16.shape)}")


def _check_rows(rows, x):
    if rows is not None and not (torch.is_tensor(rows) and rows.device == x.device and rows.dtype == torch.int32 and rows.numel() == 1):
        raise ValueError("rows must be an int32 tensor of one element on x's device")


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
        if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float16 and t.is_contiguous() and t.device == dev and tuple(t.shape) == (M, N)):
            raise ValueError(f"{name} must be a contiguous fp16 [{M}, {N}] tensor on x's device, got {getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))}")
    if dy is None:
        raise ValueError("dy is required")
    _check_rows(rows, x)
    if dw is not None and not (dw.dtype == torch.float32 and dw.is_contiguous() and dw.device == dev and tuple(dw.shape) == (N, K)):
        raise ValueError(f"dw must be a contiguous fp32 [{N}, {K}] tensor on x's device, got {dw.dtype} {tuple(dw.shape)}")
    if db is not None and not (db.dtype == torch.float32 and db.is_contiguous() and db.device == dev and tuple(db.shape) == (N,)):
        raise ValueError(f"db must be a contiguous fp32 [{N}] tensor on x's device, got {db.dtype} {tuple(db.shape)}")
    if not need_dx and dw is None and db is None:
        raise ValueError("nothing to compute: need_dx is False and dw and db are None")
    dx = torch.zeros((M, K), dtype=torch.float16, device=dev) if need_dx else None
    want = (WANT_DX if need_dx else 0) | (WANT_DW if dw is not None else 0) | (WANT_DB if db is not None else 0) | (WANT_PRE if pre is not None else 0)
    L = lib()
    with torch.cuda.device(dev):
        need = int(L.mdr_linear_backward_workspace_bytes(M, N, K, want))
        ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
        _lib.check(L.mdr_linear_backward(_ptr(x), _ptr(w), _ptr(dy), _ptr(pre), M, _ptr(rows), N, K, _ptr(dx), _ptr(dw), _ptr(db),
                                         1 if accumulate else 0, _ptr(ws), need, _dev_index(dev), _lib.current_stream_ptr(dev)))
    return dx, dw, db


def _forward_gemm(x, w16, bias, rows, epilogue):
    """mdr_test_gemm_f16 with kernel = 0: the kernel the encoder picks for this shape. Rows at or behind the valid count stay zero."""
    M, (N, K), dev = x.shape[0], w16.shape, x.device
    out = torch.zeros((M, N), dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mdr_test_gemm_f16(_ptr(x), _ptr(w16), _ptr(bias), M, _ptr(rows), N, K, _ptr(out), epilogue, 0, _dev_index(dev),
                                                _lib.current_stream_ptr(dev)))
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
    _check_rows(rows, x)
    return _PackedLinear.apply(x, weight, bias, bool(gelu), rows, weight16)
