"""A LayerNorm of the trunk on packed rows as a differentiable torch function, and the backward of the CLS gather:

    packed_layer_norm(x, residual, weight, bias, eps=1e-5, rows=None, keep32=False) -> y16, or (y16, y32) with keep32

x is a CUDA fp32 or fp16 tensor [M, H], residual None or an fp16 / fp32 tensor [M, H], weight and bias fp32 [H]; H is a multiple of 64, at most
1024. rows is an optional int32 device scalar tensor, the forward's rows_dev: only the first rows[0] rows are valid, the others are neither
read as values nor written. The forward is the encoder's own kernel (mdr_test_layernorm of include/mdr_hip.h): the output bits are the
encoder's. y16 is the fp16 operand of the next Linear, y32 the same value unrounded (the fp32 residual stream). The backward is
mdr_layernorm_backward (include/mdr_layernorm_grad.h; csrc/mdr_layernorm_grad.hip lists its rounding points): the gradient of y16 goes in as
dy16 and that of y32 as the fp32 dy2, x and residual each get dx in their own dtype, weight and bias get dg and db in fp32; no atomics, two
runs give the same bits. Nothing is saved but the inputs: the backward recomputes the statistics. Both directions are enqueued on the
current stream and never synchronise. The hidden dropout in front of a residual LayerNorm is a call of its own (dropout.packed_dropout on the
Linear's output). There is no CPU fallback.
"""
import ctypes

import torch

from . import _lib
from ._lib import check_hidden, check_rows, describe, is_like, ptr

_c = ctypes
# include/mdr_layernorm_grad.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_layernorm_backward_chunks": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "mdr_layernorm_backward_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "mdr_layernorm_backward": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p,
                                          _c.c_int, _c.c_void_p, _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                          _c.c_size_t, _c.c_int, _c.c_void_p]),
    "mdr_gather_cls_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
WANT_DG, WANT_DB = 1, 2
lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_layernorm_grad.h bound


def backward_chunks(M, H):
    """(S, rows_per_chunk): the split of the rows the dg / db sums use, a function of (M, H) alone."""
    rpc = ctypes.c_int(0)
    S = int(lib().mdr_layernorm_backward_chunks(int(M), int(H), ctypes.byref(rpc)))
    return S, int(rpc.value)


def _check_operands(x, residual, weight, rows):
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("the packed LayerNorm runs on a HIP device only (there is no CPU fallback)")
    if x.dtype not in (torch.float32, torch.float16) or x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 1:
        raise ValueError(f"x must be a contiguous fp32 or fp16 [M >= 1, H] tensor, got {describe(x)}")
    M, H = int(x.shape[0]), int(x.shape[1])
    check_hidden(H)
    if residual is not None and not is_like(residual, (torch.float16, torch.float32), (M, H), x.device):
        raise ValueError(f"residual must be None or a contiguous fp16 or fp32 [{M}, {H}] tensor on x's device, got {describe(residual)}")
    if not is_like(weight, (torch.float32,), (H,), x.device):
        raise ValueError(f"weight must be a contiguous fp32 [{H}] tensor on x's device, got {describe(weight)}")
    if rows is not None:
        check_rows(rows, x.device)
    return M, H


def _residuals(residual):
    res16 = residual if residual is not None and residual.dtype == torch.float16 else None
    res32 = residual if residual is not None and residual.dtype == torch.float32 else None
    return res16, res32


def layer_norm_backward(x, residual, dy16, dy2, weight, eps=1e-5, rows=None, need_dx16=True, need_dx32=False, dg=None, db=None, accumulate=False):
    """mdr_layernorm_backward on device tensors. x fp32 or fp16 [M, H] and residual None / fp16 / fp32 [M, H]: the forward's inputs; dy16 None or
    fp16 [M, H]; dy2 None or fp16 / fp32 [M, H] (not both None); weight fp32 [H]; rows None or the int32 device scalar of valid rows. Returns
    (dx16, dx32, dg, db): dx16 fp16 and dx32 fp32 [M, H] (None unless needed; rows at or behind the valid count are NOT written -- they are
    zero here because the buffers start zeroed), dg and db fp32 [H] (the tensors given, written or with accumulate added to; None where None
    was given). Enqueued on the current stream."""
    M, H = _check_operands(x, residual, weight, rows)
    dev = x.device
    if dy16 is not None and not is_like(dy16, (torch.float16,), (M, H), dev):
        raise ValueError(f"dy16 must be None or a contiguous fp16 [{M}, {H}] tensor on x's device, got {describe(dy16)}")
    if dy2 is not None and not is_like(dy2, (torch.float16, torch.float32), (M, H), dev):
        raise ValueError(f"dy2 must be None or a contiguous fp16 or fp32 [{M}, {H}] tensor on x's device, got {describe(dy2)}")
    if dy16 is None and dy2 is None:
        raise ValueError("dy16 and dy2 are both None: one output gradient is required")
    for name, t in (("dg", dg), ("db", db)):
        if t is not None and not is_like(t, (torch.float32,), (H,), dev):
            raise ValueError(f"{name} must be None or a contiguous fp32 [{H}] tensor on x's device, got {describe(t)}")
    if not (need_dx16 or need_dx32 or dg is not None or db is not None):
        raise ValueError("nothing to compute: neither dx16 nor dx32 is needed and dg and db are None")
    dx16 = torch.zeros((M, H), dtype=torch.float16, device=dev) if need_dx16 else None
    dx32 = torch.zeros((M, H), dtype=torch.float32, device=dev) if need_dx32 else None
    res16, res32 = _residuals(residual)
    want = (WANT_DG if dg is not None else 0) | (WANT_DB if db is not None else 0)
    L = lib()
    need = int(L.mdr_layernorm_backward_workspace_bytes(M, H, want))
    ws = _lib.workspace(need, dev)
    _lib.call(L.mdr_layernorm_backward, ptr(x), 1 if x.dtype == torch.float16 else 0, ptr(res16), ptr(res32), ptr(dy16), ptr(dy2),
              1 if dy2 is not None and dy2.dtype == torch.float32 else 0, M, ptr(rows), H, ptr(weight), float(eps), ptr(dx16), ptr(dx32), ptr(dg), ptr(db),
              1 if accumulate else 0, ptr(ws), need, dev=dev)
    return dx16, dx32, dg, db


def gather_cls_backward(d, cu, acc):
    """mdr_gather_cls_backward: d fp16 [B, H], the gradient of the gathered CLS rows; cu int32 [B + 1], the packed batch's sequence starts; acc
    fp16 [T, H], T >= cu[B]: row cu[b] of acc becomes fp16(fp32(acc) + fp32(d[b])) for every non-empty sequence b, in place. Returns acc."""
    if not (torch.is_tensor(d) and d.is_cuda):
        raise RuntimeError("the CLS gather's backward runs on a HIP device only (there is no CPU fallback)")
    if d.dtype != torch.float16 or d.dim() != 2 or not d.is_contiguous() or d.shape[0] < 1:
        raise ValueError(f"d must be a contiguous fp16 [B >= 1, H] tensor, got {describe(d)}")
    B, H = int(d.shape[0]), int(d.shape[1])
    check_hidden(H)
    if not is_like(cu, (torch.int32,), (B + 1,), d.device):
        raise ValueError(f"cu must be a contiguous int32 [{B + 1}] tensor on d's device, got {describe(cu)}")
    if not (torch.is_tensor(acc) and acc.dtype == torch.float16 and acc.dim() == 2 and acc.is_contiguous() and acc.device == d.device
            and acc.shape[1] == H):
        raise ValueError(f"acc must be a contiguous fp16 [T, {H}] tensor on d's device, got {describe(acc)}")
    _lib.call(lib().mdr_gather_cls_backward, ptr(d), ptr(cu), B, H, ptr(acc), dev=d.device)
    return acc


def _forward(x, residual, weight, bias, eps, rows, keep32):
    """mdr_test_layernorm: the encoder's kernel. Rows at or behind the valid count stay zero."""
    (M, H), dev = x.shape, x.device
    y16 = torch.zeros((M, H), dtype=torch.float16, device=dev)
    y32 = torch.zeros((M, H), dtype=torch.float32, device=dev) if keep32 else None
    res16, res32 = _residuals(residual)
    _lib.call(_lib.lib().mdr_test_layernorm, ptr(x), 1 if x.dtype == torch.float16 else 0, ptr(res16), ptr(res32), M, ptr(rows), H, ptr(weight), ptr(bias),
              float(eps), ptr(y16), ptr(y32), dev=dev)
    return y16, y32


class _PackedLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, eps, rows, keep32):
        xd, rd = x.detach(), None if residual is None else residual.detach()
        wd, bd = weight.detach().contiguous(), bias.detach().contiguous()
        ctx.save_for_backward(xd, rd, wd, rows)
        ctx.eps = float(eps)
        ctx.set_materialize_grads(False)
        y16, y32 = _forward(xd, rd, wd, bd, eps, rows, keep32)
        return (y16, y32) if keep32 else y16

    @staticmethod
    def backward(ctx, g16, g32=None):
        x, residual, weight, rows = ctx.saved_tensors
        need_x, need_r, need_w, need_b = ctx.needs_input_grad[:4]
        need_r = need_r and residual is not None
        if (g16 is None and g32 is None) or not (need_x or need_r or need_w or need_b):
            return (None,) * 7
        dy16 = None if g16 is None else g16.detach().to(dtype=torch.float16).contiguous()
        dy2 = None if g32 is None else g32.detach().to(dtype=torch.float32).contiguous()
        dts = {t.dtype for t, need in ((x, need_x), (residual, need_r)) if need}
        dg = torch.empty(weight.shape, dtype=torch.float32, device=x.device) if need_w else None
        db = torch.empty(weight.shape, dtype=torch.float32, device=x.device) if need_b else None
        dx16, dx32, dg, db = layer_norm_backward(x, residual, dy16, dy2, weight, ctx.eps, rows, torch.float16 in dts, torch.float32 in dts, dg, db)
        pick = lambda t: dx16 if t.dtype == torch.float16 else dx32  # noqa: E731
        return pick(x) if need_x else None, pick(residual) if need_r else None, dg, db, None, None, None


def packed_layer_norm(x, residual, weight, bias, eps=1e-5, rows=None, keep32=False):
    """LayerNorm(x + residual) * weight + bias on packed rows through the encoder's kernel, differentiable with respect to x, residual, weight
    and bias (module docstring)."""
    M, H = _check_operands(x, residual, weight, rows)
    if not is_like(bias, (torch.float32,), (H,), x.device):
        raise ValueError(f"bias must be a contiguous fp32 [{H}] tensor on x's device, got {describe(bias)}")
    return _PackedLayerNorm.apply(x, residual, weight, bias, float(eps), rows, bool(keep32))
