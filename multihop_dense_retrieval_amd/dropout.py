"""Dropout for the training bricks: a replayable Philox4x32-10 mask (include/mdr_dropout.h; csrc/mdr_dropout.h is the mask function).

    packed_dropout(x, p, seed, site, rows=None, also16=False) -> y, or (y32, y16) with also16

x is a CUDA fp16 or fp32 tensor [M, N], N a multiple of 16. Element (row, col) is multiplied by m in {0, scale}: it is kept iff byte col & 15 of
the generator call with counter (col >> 4, row, 0, site) under the key of `seed` is >= T = threshold(p). rows is an optional int32 device
scalar tensor: only the first rows[0] rows are valid, the others are neither read as values nor written (they are zero in the outputs). With
also16 (fp32 x only) the call also returns y16 = fp16(y32): the embedding's h16 / h32 pair under one mask and one rounding.

The rate actually drawn is effective_p(p) = T / 256, not the nominal p: p = 0.1 draws 26 / 256 = 0.1016. The scale is fp32(256 / (256 - T)),
exact in expectation for the rate drawn. The factor is applied as a multiplication: a non-finite x at a dropped position gives NaN, as
torch's x * mask does.

Nothing is saved for the backward but (T, seed, site) and rows: the backward is the same call on the gradient and draws the same mask. With
also16 the input's gradient is the mask times (g32 + fp32(g16)). A p with T = 0 returns x itself without a launch (also16: one launch, for y16). That
y16 is fp16(y32), a second rounding: embedding.packed_embedding_layer_norm's own fp16 copy is one rounding of the unrounded value and differs from it
by an fp16 ulp where y32 sits exactly between two fp16 values, so a caller whose T is 0 keeps the embedding's pair and makes no call.

Uniqueness is the CALLER's duty: every use -- every step, encode, layer and place -- needs its own site or seed; two uses that share
(seed, site) share their mask. The attention probabilities' dropout is attention.packed_self_attention(..., dropout=(p, seed, site)).
Everything is enqueued on the current stream and never synchronises. There is no CPU fallback.
"""
import ctypes

import torch

from . import _lib
from ._lib import check_rows, describe, is_like, ptr

_c = ctypes
# include/mdr_dropout.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_dropout_threshold": (_c.c_int, [_c.c_float]),
    "mdr_test_dropout_bytes": (_c.c_int, [_c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "mdr_dropout_rows": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_uint64, _c.c_uint32, _c.c_void_p,
                                    _c.c_void_p, _c.c_int, _c.c_void_p]),
    "mdr_attention_dropout_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_uint64,
                                                 _c.c_uint32, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "mdr_attention_dropout_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                                  _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_dropout.h bound


ENCODES, MAX_LAYERS = 6, 64  # the six encodes of one in-batch loss; more layers than any geometry has
PLACES = ("emb", "attn", "ao", "ff2")


def site_of(encode, layer, place):
    """The uint32 site of one dropout call of a training step (train.TrainableRetriever): encode 0 .. 5 (the index of the batch key in q,
    q_sp1, c1, c2, neg_1, neg_2; a lone encode is 0), layer 0 .. 63, place one of PLACES ("emb" belongs to layer 0). Injective, and never 0.
    The step itself is told apart by the seed."""
    if not (0 <= encode < ENCODES and 0 <= layer < MAX_LAYERS and place in PLACES and (place != "emb" or layer == 0)):
        raise ValueError(f"no dropout site for encode {encode}, layer {layer}, place {place!r}")
    return 1 + (encode * MAX_LAYERS + layer) * len(PLACES) + PLACES.index(place)


def threshold(p):
    """T = floor(256 p + 0.5) of mdr_dropout_threshold; ValueError for a p outside [0, 1) or one that rounds to 256."""
    T = int(lib().mdr_dropout_threshold(float(p)))
    if T < 0:
        raise ValueError(f"dropout p = {p!r}: must lie in [0, 1) and round to fewer than 256 / 256")
    return T


def effective_p(p):
    """The rate actually drawn, threshold(p) / 256 (0.1 -> 0.1015625): eight bits per element decide."""
    return threshold(p) / 256.0


def check_seed_site(seed, site):
    seed, site = int(seed), int(site)
    if not (0 <= seed < 2 ** 64 and 0 <= site < 2 ** 32):
        raise ValueError(f"seed = {seed} must fit a uint64 and site = {site} a uint32")
    return seed, site


def dropout_rows(x, T, seed, site, rows=None, add16=None, also16=False):
    """mdr_dropout_rows on device tensors: y = (x + add16) * m, and with also16 (y, fp16(y)). Rows at or behind the valid count are NOT written:
    they are zero here because the buffers start zeroed. Enqueued on the current stream."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise RuntimeError("dropout runs on a HIP device only (there is no CPU fallback)")
    if x.dtype not in (torch.float32, torch.float16) or x.dim() != 2 or not x.is_contiguous() or x.shape[0] < 1 or x.shape[1] < 16 or x.shape[1] % 16:
        raise ValueError(f"x must be a contiguous fp32 or fp16 [M >= 1, N] tensor, N a multiple of 16, got {describe(x)}")
    M, N = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    if (also16 or add16 is not None) and x.dtype != torch.float32:
        raise ValueError("also16 and add16 go with an fp32 x only")
    if add16 is not None and not is_like(add16, (torch.float16,), (M, N), dev):
        raise ValueError(f"add16 must be None or a contiguous fp16 [{M}, {N}] tensor on x's device, got {describe(add16)}")
    if rows is not None:
        check_rows(rows, dev)
    seed, site = check_seed_site(seed, site)
    y = torch.zeros_like(x)
    y16 = torch.zeros((M, N), dtype=torch.float16, device=dev) if also16 else None
    _lib.call(lib().mdr_dropout_rows, ptr(x), 1 if x.dtype == torch.float16 else 0, ptr(add16), M, ptr(rows), N, int(T), seed, site, ptr(y), ptr(y16), dev=dev)
    return (y, y16) if also16 else y


class _PackedDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, T, seed, site, rows, also16):
        ctx.T, ctx.seed, ctx.site, ctx.rows = T, seed, site, rows  # no tensor is saved: the backward draws the mask again
        ctx.set_materialize_grads(False)
        return dropout_rows(x.detach(), T, seed, site, rows, None, also16)

    @staticmethod
    def backward(ctx, g, g16=None):
        if (g is None and g16 is None) or not ctx.needs_input_grad[0]:
            return (None,) * 6
        if g is None:  # only y16 was used: an fp32 zero carries its gradient into the input's dtype
            g = torch.zeros(g16.shape, dtype=torch.float32, device=g16.device)
        g = g.detach().contiguous()
        add16 = None if g16 is None else g16.detach().to(dtype=torch.float16).contiguous()
        return dropout_rows(g, ctx.T, ctx.seed, ctx.site, ctx.rows, add16, False), None, None, None, None, None


def packed_dropout(x, p, seed, site, rows=None, also16=False):
    """x * m on packed rows, differentiable with respect to x (module docstring)."""
    T = threshold(p)
    seed, site = check_seed_site(seed, site)
    if T == 0 and not also16:
        if not (torch.is_tensor(x) and x.is_cuda):
            raise RuntimeError("dropout runs on a HIP device only (there is no CPU fallback)")
        return x
    return _PackedDropout.apply(x, T, seed, site, rows, bool(also16))
