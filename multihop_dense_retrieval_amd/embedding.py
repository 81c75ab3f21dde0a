"""The retriever's embedding layer on packed rows as a differentiable torch function, and its backward's three calls:

    packed_embedding_layer_norm(ids, tok_src, tok_pid, total, word, pos, type0, weight, bias, eps, cap, pad_row, keep32=False)
        -> y16 [cap, H], or (y16, y32) with keep32

ids is a CUDA int64 tensor (any shape; tok_src indexes it flat), tok_src and tok_pid int32 [cap] and total an int32 device scalar: what the
packing prologue of a forward leaves (mdr_test_pack). word fp32 [vocab, H], pos fp32 [max_pos, H], type0 fp32 [H], weight and bias fp32 [H];
H a multiple of 64, at most 1024. The forward is the encoder's own kernel (flavour 0 of mdr_test_embed_ln, include/mdr_hip.h): the output bits
are the encoder's; rows at or behind total stay zero. The backward is mdr_embedding_backward (include/mdr_embedding_grad.h;
csrc/mdr_embedding_grad.hip lists its rounding points) on a plan built at forward time (mdr_embedding_plan): dense fp32 gradients for word,
pos, type0, weight and bias, no floating-point atomics, two runs give the same bits. pad_row is Hugging Face's padding_idx: that row of both
tables gets no gradient (-1: no such row). Everything is enqueued on the current stream and never synchronises. The hidden dropout behind
this LayerNorm is a call of its own, dropout.packed_dropout(y32, p, seed, site, rows=total, also16=True). There is no CPU fallback.
"""
import ctypes

import torch

from . import _lib
from ._lib import check_hidden, check_rows, describe, is_like, ptr

_c = ctypes
# include/mdr_embedding_grad.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_embedding_plan_bytes": (_c.c_size_t, [_c.c_int]),
    "mdr_embedding_plan": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                      _c.c_int, _c.c_void_p]),
    "mdr_embedding_backward_chunks": (_c.c_int, [_c.c_int, _c.c_int, _c.POINTER(_c.c_int)]),
    "mdr_embedding_scatter_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "mdr_embedding_scatter": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                         _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "mdr_embedding_backward_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "mdr_embedding_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                          _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                          _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
# include/mdr_reader_embedding_grad.h: the reader's (ELECTRA) flavour
READER_SIGNATURES = {
    "mdr_reader_embedding_plan": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                             _c.c_size_t, _c.c_int, _c.c_void_p]),
    "mdr_reader_embedding_backward_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "mdr_reader_embedding_backward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                 _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                                 _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t,
                                                 _c.c_int, _c.c_void_p]),
}
READER_EXPORTED_SYMBOLS = tuple(READER_SIGNATURES)
READER_PLAN_MAGIC = 0x4D455032  # MDR_READER_EMBEDDING_PLAN_MAGIC
READER_MAX_TYPES = 4            # MDR_READER_EMBEDDING_MAX_TYPES
PIECE = 16                 # MDR_EMBEDDING_PIECE
PLAN_HEADER = 16           # MDR_EMBEDDING_PLAN_HEADER
PLAN_MAGIC = 0x4D455031    # MDR_EMBEDDING_PLAN_MAGIC
MAX_CAP, MAX_VOCAB, MAX_POS = 1 << 20, 1 << 20, 1 << 16
lib = _lib.binder(SIGNATURES, READER_SIGNATURES)  # libmdrhip.so with the signatures of both headers bound


def plan_layout(cap):
    """Offsets, in int32 words, of the sections of a plan for `cap` tokens (the layout include/mdr_embedding_grad.h documents):
    {"word" | "pos": {"order", "seg_start", "seg_row", "key"}, "words"}."""
    stride = (3 * cap + 1 + 3) // 4 * 4
    out = {"words": PLAN_HEADER + 2 * stride + 2 * cap}
    for i, name in enumerate(("word", "pos")):
        base = PLAN_HEADER + i * stride
        out[name] = {"order": base, "seg_start": base + cap, "seg_row": base + 2 * cap + 1, "key": PLAN_HEADER + 2 * stride + i * cap}
    return out


def backward_chunks(cap, H):
    """(S, rows_per_chunk): the split of the rows the dtype0 / dg / db sums use, a function of (cap, H) alone."""
    rpc = ctypes.c_int(0)
    S = int(lib().mdr_embedding_backward_chunks(int(cap), int(H), ctypes.byref(rpc)))
    return S, int(rpc.value)


def _check_pack(ids, tok_src, tok_pid, total, cap):
    if not (torch.is_tensor(ids) and ids.is_cuda):
        raise RuntimeError("the embedding backward runs on a HIP device only (there is no CPU fallback)")
    dev = ids.device
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.numel() < 1:
        raise ValueError(f"ids must be a contiguous int64 tensor, got {describe(ids)}")
    if not (isinstance(cap, int) and 1 <= cap <= MAX_CAP):
        raise ValueError(f"cap = {cap!r}: must be an int, 1 .. 2^20")
    for name, t in (("tok_src", tok_src), ("tok_pid", tok_pid)):
        if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.device == dev and t.shape[0] >= cap):
            raise ValueError(f"{name} must be a contiguous int32 [>= {cap}] tensor on ids' device, got {describe(t)}")
    check_rows(total, dev, "total", "ids")
    return dev


def _check_sizes(vocab, max_pos, pad_row):
    if not 1 <= vocab <= MAX_VOCAB:
        raise ValueError(f"vocab = {vocab}: must be 1 .. 2^20")
    if not 1 <= max_pos <= MAX_POS:
        raise ValueError(f"max_pos = {max_pos}: must be 1 .. 2^16")
    if not (isinstance(pad_row, int) and -1 <= pad_row < MAX_VOCAB):
        raise ValueError(f"pad_row = {pad_row!r}: must be an int, -1 .. 2^20 - 1")


def _check_plan(plan, cap, dev):
    if not (torch.is_tensor(plan) and plan.dtype == torch.int32 and plan.dim() == 1 and plan.is_contiguous() and plan.device == dev
            and plan.shape[0] >= plan_layout(cap)["words"]):
        raise ValueError(f"plan must be the int32 tensor embedding_plan returned for cap = {cap} on the same device, got {describe(plan)}")


def _check_outputs(outs, H, dev):
    for name, t, rows in outs:
        shape = (H,) if rows is None else (rows, H)
        if t is not None and not is_like(t, (torch.float32,), shape, dev):
            raise ValueError(f"{name} must be None or a contiguous fp32 {list(shape)} tensor on the inputs' device, got {describe(t)}")


def embedding_plan(ids, tok_src, tok_pid, total, cap, vocab, max_pos, pad_row=-1):
    """mdr_embedding_plan -> the plan, an int32 device tensor (plan_layout(cap) gives its sections). Enqueued on the current stream."""
    dev = _check_pack(ids, tok_src, tok_pid, total, cap)
    _check_sizes(vocab, max_pos, pad_row)
    L = lib()
    nbytes = int(L.mdr_embedding_plan_bytes(cap))
    plan = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    _lib.call(L.mdr_embedding_plan, ptr(ids), ptr(tok_src), ptr(tok_pid), ptr(total), cap, vocab, max_pos, pad_row, ptr(plan), nbytes, dev=dev)
    return plan


def embedding_scatter(d32, plan, vocab, max_pos, dword=None, dpos=None, dtype0=None, accumulate=False):
    """mdr_embedding_scatter: d32 fp32 [cap, H], the gradient of x; the plan of the same cap, vocab and max_pos. dword fp32 [vocab, H], dpos
    fp32 [max_pos, H], dtype0 fp32 [H]: the tensors given are written (every row) or, with accumulate, added to (only the rows that own
    tokens). Returns (dword, dpos, dtype0)."""
    if not (torch.is_tensor(d32) and d32.is_cuda):
        raise RuntimeError("the embedding scatter runs on a HIP device only (there is no CPU fallback)")
    if d32.dtype != torch.float32 or d32.dim() != 2 or not d32.is_contiguous() or not 1 <= d32.shape[0] <= MAX_CAP:
        raise ValueError(f"d32 must be a contiguous fp32 [1 <= cap <= 2^20, H] tensor, got {describe(d32)}")
    cap, H = int(d32.shape[0]), int(d32.shape[1])
    dev = d32.device
    check_hidden(H)
    _check_sizes(vocab, max_pos, -1)
    _check_plan(plan, cap, dev)
    _check_outputs((("dword", dword, vocab), ("dpos", dpos, max_pos), ("dtype0", dtype0, None)), H, dev)
    if dword is None and dpos is None and dtype0 is None:
        raise ValueError("nothing to compute: dword, dpos and dtype0 are all None")
    L = lib()
    need = int(L.mdr_embedding_scatter_workspace_bytes(cap, H))
    ws = _lib.workspace(need, dev)
    _lib.call(L.mdr_embedding_scatter, ptr(d32), ptr(plan), cap, H, vocab, max_pos, ptr(dword), ptr(dpos), ptr(dtype0), 1 if accumulate else 0, ptr(ws), need,
              dev=dev)
    return dword, dpos, dtype0


def _check_params(word, pos, type0, weight, dev):
    if not (torch.is_tensor(word) and word.dtype == torch.float32 and word.dim() == 2 and word.is_contiguous() and word.device == dev and word.shape[0] >= 1):
        raise ValueError(f"word must be a contiguous fp32 [vocab, H] tensor on ids' device, got {describe(word)}")
    vocab, H = int(word.shape[0]), int(word.shape[1])
    check_hidden(H)
    if not (torch.is_tensor(pos) and pos.dtype == torch.float32 and pos.dim() == 2 and pos.is_contiguous() and pos.device == dev and pos.shape[0] >= 1
            and pos.shape[1] == H):
        raise ValueError(f"pos must be a contiguous fp32 [max_pos, {H}] tensor on ids' device, got {describe(pos)}")
    for name, t in (("type0", type0), ("weight", weight)):
        if not is_like(t, (torch.float32,), (H,), dev):
            raise ValueError(f"{name} must be a contiguous fp32 [{H}] tensor on ids' device, got {describe(t)}")
    return vocab, int(pos.shape[0]), H


def embedding_backward(ids, tok_src, tok_pid, total, cap, word, pos, type0, weight, eps, dy16, dy2, plan, dword=None, dpos=None, dtype0=None, dg=None,
                       db=None, d32=None, accumulate=False):
    """mdr_embedding_backward on device tensors: the forward's inputs, dy16 None or fp16 [cap, H], dy2 None or fp16 / fp32 [cap, H] (not both
    None), the plan (None when neither dword nor dpos is wanted). The output tensors given are written or, with accumulate, added to; d32
    fp32 [cap, H] receives d (rows at or behind total are not written). Returns (dword, dpos, dtype0, dg, db, d32)."""
    dev = _check_pack(ids, tok_src, tok_pid, total, cap)
    vocab, max_pos, H = _check_params(word, pos, type0, weight, dev)
    _check_sizes(vocab, max_pos, -1)
    if dy16 is not None and not is_like(dy16, (torch.float16,), (cap, H), dev):
        raise ValueError(f"dy16 must be None or a contiguous fp16 [{cap}, {H}] tensor on ids' device, got {describe(dy16)}")
    if dy2 is not None and not is_like(dy2, (torch.float16, torch.float32), (cap, H), dev):
        raise ValueError(f"dy2 must be None or a contiguous fp16 or fp32 [{cap}, {H}] tensor on ids' device, got {describe(dy2)}")
    if dy16 is None and dy2 is None:
        raise ValueError("dy16 and dy2 are both None: one output gradient is required")
    _check_outputs((("dword", dword, vocab), ("dpos", dpos, max_pos), ("dtype0", dtype0, None), ("dg", dg, None), ("db", db, None), ("d32", d32, cap)), H, dev)
    if all(t is None for t in (dword, dpos, dtype0, dg, db, d32)):
        raise ValueError("nothing to compute: every output is None")
    if dword is not None or dpos is not None:
        _check_plan(plan, cap, dev)
    L = lib()
    need = int(L.mdr_embedding_backward_workspace_bytes(cap, H))
    ws = _lib.workspace(need, dev)
    _lib.call(L.mdr_embedding_backward, ptr(ids), ptr(tok_src), ptr(tok_pid), ptr(total), cap, ptr(word), ptr(pos), ptr(type0), ptr(weight), H, vocab, max_pos,
              float(eps), ptr(dy16), ptr(dy2), 1 if dy2 is not None and dy2.dtype == torch.float32 else 0, ptr(plan), ptr(dword), ptr(dpos), ptr(dtype0), ptr(dg),
              ptr(db), ptr(d32), 1 if accumulate else 0, ptr(ws), need, dev=dev)
    return dword, dpos, dtype0, dg, db, d32


def _forward(ids, tok_src, tok_pid, total, cap, word, pos, type0, weight, bias, eps, keep32):
    """flavour 0 of mdr_test_embed_ln: the encoder's kernel. Rows at or behind total stay zero."""
    dev, (vocab, H), max_pos = ids.device, word.shape, pos.shape[0]
    y16 = torch.zeros((cap, H), dtype=torch.float16, device=dev)
    y32 = torch.zeros((cap, H), dtype=torch.float32, device=dev) if keep32 else None
    _lib.call(_lib.lib().mdr_test_embed_ln, 0, ptr(ids), None, ptr(tok_src), ptr(tok_pid), ptr(total), cap, 0, ptr(word), ptr(pos), ptr(type0), 1, ptr(weight),
              ptr(bias), H, vocab, max_pos, float(eps), ptr(y16), ptr(y32), dev=dev)
    return y16, y32


class _PackedEmbeddingLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, tok_src, tok_pid, total, word, pos, type0, weight, bias, eps, cap, pad_row, keep32):
        wd, pd, td, gd, bd = (t.detach().contiguous() for t in (word, pos, type0, weight, bias))
        y16, y32 = _forward(ids, tok_src, tok_pid, total, cap, wd, pd, td, gd, bd, eps, keep32)
        # the sort is enqueued here, at forward time: the backward finds it done
        plan = embedding_plan(ids, tok_src, tok_pid, total, cap, int(wd.shape[0]), int(pd.shape[0]), pad_row)
        ctx.save_for_backward(ids, tok_src, tok_pid, total, wd, pd, td, gd, plan)
        ctx.eps, ctx.cap = float(eps), cap
        ctx.set_materialize_grads(False)
        return (y16, y32) if keep32 else y16

    @staticmethod
    def backward(ctx, g16, g32=None):
        ids, tok_src, tok_pid, total, word, pos, type0, weight, plan = ctx.saved_tensors
        need = ctx.needs_input_grad[4:9]
        if (g16 is None and g32 is None) or not any(need):
            return (None,) * 13
        dy16 = None if g16 is None else g16.detach().to(dtype=torch.float16).contiguous()
        dy2 = None if g32 is None else g32.detach().to(dtype=torch.float32).contiguous()
        outs = [torch.empty(t.shape, dtype=torch.float32, device=ids.device) if n else None for t, n in zip((word, pos, type0, weight, weight), need)]
        embedding_backward(ids, tok_src, tok_pid, total, ctx.cap, word, pos, type0, weight, ctx.eps, dy16, dy2, plan, *outs)
        return (None, None, None, None, *outs, None, None, None, None)


def packed_embedding_layer_norm(ids, tok_src, tok_pid, total, word, pos, type0, weight, bias, eps, cap, pad_row, keep32=False):
    """LayerNorm((word[ids] + pos[position ids]) + type0) * weight + bias over the packed tokens through the encoder's kernel, differentiable
    with respect to word, pos, type0, weight and bias (module docstring)."""
    dev = _check_pack(ids, tok_src, tok_pid, total, cap)
    vocab, max_pos, H = _check_params(word, pos, type0, weight, dev)
    _check_sizes(vocab, max_pos, pad_row)
    if not is_like(bias, (torch.float32,), (H,), dev):
        raise ValueError(f"bias must be a contiguous fp32 [{H}] tensor on ids' device, got {describe(bias)}")
    return _PackedEmbeddingLayerNorm.apply(ids, tok_src, tok_pid, total, word, pos, type0, weight, bias, float(eps), cap, pad_row, bool(keep32))


# ---- the reader's flavour (include/mdr_reader_embedding_grad.h) ----------------------------------------------------------------------------
def _check_reader_pack(ids, types, tok_src, total, cap, L):
    if not (torch.is_tensor(ids) and ids.is_cuda):
        raise RuntimeError("the embedding backward runs on a HIP device only (there is no CPU fallback)")
    dev = ids.device
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.numel() < 1:
        raise ValueError(f"ids must be a contiguous int64 tensor, got {describe(ids)}")
    if types is not None and not (torch.is_tensor(types) and types.dtype == torch.int64 and types.is_contiguous() and types.device == dev
                                  and types.numel() == ids.numel()):
        raise ValueError(f"types must be None or a contiguous int64 tensor of ids' size on ids' device, got {describe(types)}")
    if not (isinstance(cap, int) and 1 <= cap <= MAX_CAP):
        raise ValueError(f"cap = {cap!r}: must be an int, 1 .. 2^20")
    if not (isinstance(L, int) and L >= 1):
        raise ValueError(f"L = {L!r}: must be an int, at least 1")
    if not (torch.is_tensor(tok_src) and tok_src.dtype == torch.int32 and tok_src.dim() == 1 and tok_src.is_contiguous() and tok_src.device == dev
            and tok_src.shape[0] >= cap):
        raise ValueError(f"tok_src must be a contiguous int32 [>= {cap}] tensor on ids' device, got {describe(tok_src)}")
    check_rows(total, dev, "total", "ids")
    return dev


def _check_reader_sizes(vocab, max_pos, L, type_vocab, pad_row):
    _check_sizes(vocab, max_pos, pad_row)
    if L > max_pos:
        raise ValueError(f"L = {L} exceeds max_pos = {max_pos}: the position of a token is its place in the row")
    if not 1 <= type_vocab <= READER_MAX_TYPES:
        raise ValueError(f"type_vocab = {type_vocab}: must be 1 .. {READER_MAX_TYPES}")


def _check_reader_plan(plan, cap, dev):
    _check_plan(plan, cap, dev)
    if getattr(plan, "mdr_plan_kind", None) != "reader":
        raise ValueError("plan must be one reader_embedding_plan returned: a retriever plan (embedding_plan) holds other position rows and pad rows")


def reader_embedding_plan(ids, tok_src, total, cap, L, vocab, max_pos, pad_row=-1):
    """mdr_reader_embedding_plan -> the plan (plan_layout(cap) gives its sections; header words 7, 8, 9 hold pad_row, -1 and L). pad_row is the
    WORD table's; the position table has none. Enqueued on the current stream."""
    dev = _check_reader_pack(ids, None, tok_src, total, cap, L)
    _check_reader_sizes(vocab, max_pos, L, 1, pad_row)
    Lb = lib()
    nbytes = int(Lb.mdr_embedding_plan_bytes(cap))
    plan = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    _lib.call(Lb.mdr_reader_embedding_plan, ptr(ids), ptr(tok_src), ptr(total), cap, L, vocab, max_pos, pad_row, -1, ptr(plan), nbytes, dev=dev)
    plan.mdr_plan_kind = "reader"
    return plan


def _check_reader_params(word, pos, type_table, weight, dev):
    if not (torch.is_tensor(type_table) and type_table.dim() == 2):
        raise ValueError(f"type_table must be a contiguous fp32 [type_vocab, H] tensor on ids' device, got {describe(type_table)}")
    vocab, max_pos, H = _check_params(word, pos, weight, weight, dev)
    if not is_like(type_table, (torch.float32,), (int(type_table.shape[0]), H), dev) or type_table.shape[0] < 1:
        raise ValueError(f"type_table must be a contiguous fp32 [type_vocab, {H}] tensor on ids' device, got {describe(type_table)}")
    return vocab, max_pos, H, int(type_table.shape[0])


def reader_embedding_backward(ids, types, tok_src, total, cap, L, word, pos, type_table, weight, eps, dy16, dy2, plan, dword=None, dpos=None, dtype=None,
                              dg=None, db=None, d32=None, accumulate=False):
    """mdr_reader_embedding_backward on device tensors: embedding_backward for flavour 1 of the forward. types None or int64 of ids' size;
    type_table fp32 [type_vocab <= 4, H]; dtype fp32 [type_vocab, H]; plan from reader_embedding_plan with the same L. Returns (dword, dpos,
    dtype, dg, db, d32)."""
    dev = _check_reader_pack(ids, types, tok_src, total, cap, L)
    vocab, max_pos, H, tv = _check_reader_params(word, pos, type_table, weight, dev)
    _check_reader_sizes(vocab, max_pos, L, tv, -1)
    if dy16 is not None and not is_like(dy16, (torch.float16,), (cap, H), dev):
        raise ValueError(f"dy16 must be None or a contiguous fp16 [{cap}, {H}] tensor on ids' device, got {describe(dy16)}")
    if dy2 is not None and not is_like(dy2, (torch.float16, torch.float32), (cap, H), dev):
        raise ValueError(f"dy2 must be None or a contiguous fp16 or fp32 [{cap}, {H}] tensor on ids' device, got {describe(dy2)}")
    if dy16 is None and dy2 is None:
        raise ValueError("dy16 and dy2 are both None: one output gradient is required")
    _check_outputs((("dword", dword, vocab), ("dpos", dpos, max_pos), ("dtype", dtype, tv), ("dg", dg, None), ("db", db, None), ("d32", d32, cap)), H, dev)
    if all(t is None for t in (dword, dpos, dtype, dg, db, d32)):
        raise ValueError("nothing to compute: every output is None")
    if dword is not None or dpos is not None:
        _check_reader_plan(plan, cap, dev)
    Lb = lib()
    need = int(Lb.mdr_reader_embedding_backward_workspace_bytes(cap, H, tv))
    ws = _lib.workspace(need, dev)
    _lib.call(Lb.mdr_reader_embedding_backward, ptr(ids), ptr(types), ptr(tok_src), ptr(total), cap, L, ptr(word), ptr(pos), ptr(type_table), tv, ptr(weight), H,
              vocab, max_pos, float(eps), ptr(dy16), ptr(dy2), 1 if dy2 is not None and dy2.dtype == torch.float32 else 0, ptr(plan), ptr(dword), ptr(dpos),
              ptr(dtype), ptr(dg), ptr(db), ptr(d32), 1 if accumulate else 0, ptr(ws), need, dev=dev)
    return dword, dpos, dtype, dg, db, d32


def _reader_forward(ids, types, tok_src, total, cap, L, word, pos, type_table, weight, bias, eps, keep32):
    """flavour 1 of mdr_test_embed_ln: the reader's kernel. Rows at or behind total stay zero."""
    dev, (vocab, H), max_pos = ids.device, word.shape, pos.shape[0]
    y16 = torch.zeros((cap, H), dtype=torch.float16, device=dev)
    y32 = torch.zeros((cap, H), dtype=torch.float32, device=dev) if keep32 else None
    _lib.call(_lib.lib().mdr_test_embed_ln, 1, ptr(ids), ptr(types), ptr(tok_src), None, ptr(total), cap, L, ptr(word), ptr(pos), ptr(type_table),
              int(type_table.shape[0]), ptr(weight), ptr(bias), H, vocab, max_pos, float(eps), ptr(y16), ptr(y32), dev=dev)
    return y16, y32


class _PackedReaderEmbeddingLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, types, tok_src, total, L, word, pos, type_table, weight, bias, eps, cap, pad_row, keep32):
        wd, pd, td, gd, bd = (t.detach().contiguous() for t in (word, pos, type_table, weight, bias))
        y16, y32 = _reader_forward(ids, types, tok_src, total, cap, L, wd, pd, td, gd, bd, eps, keep32)
        # the sort is enqueued here, at forward time: the backward finds it done
        plan = reader_embedding_plan(ids, tok_src, total, cap, L, int(wd.shape[0]), int(pd.shape[0]), pad_row)
        ctx.save_for_backward(ids, tok_src, total, wd, pd, td, gd, plan)
        ctx.types = types  # (None or an int64 tensor that needs no gradient)
        ctx.eps, ctx.cap, ctx.L = float(eps), cap, L
        ctx.set_materialize_grads(False)
        return (y16, y32) if keep32 else y16

    @staticmethod
    def backward(ctx, g16, g32=None):
        ids, tok_src, total, word, pos, type_table, weight, plan = ctx.saved_tensors
        plan.mdr_plan_kind = "reader"  # (saved_tensors hands back a tensor without the attribute)
        need = ctx.needs_input_grad[5:10]
        if (g16 is None and g32 is None) or not any(need):
            return (None,) * 14
        dy16 = None if g16 is None else g16.detach().to(dtype=torch.float16).contiguous()
        dy2 = None if g32 is None else g32.detach().to(dtype=torch.float32).contiguous()
        outs = [torch.empty(t.shape, dtype=torch.float32, device=ids.device) if n else None for t, n in zip((word, pos, type_table, weight, weight), need)]
        reader_embedding_backward(ids, ctx.types, tok_src, total, ctx.cap, ctx.L, word, pos, type_table, weight, ctx.eps, dy16, dy2, plan, *outs)
        return (None, None, None, None, None, *outs, None, None, None, None)


def packed_reader_embedding_layer_norm(ids, types, tok_src, total, L, word, pos, type_table, weight, bias, eps, cap, pad_row, keep32=False):
    """LayerNorm((word[ids] + pos[place in the row]) + type_table[types]) * weight + bias over the packed tokens through the reader's kernel
    (flavour 1 of mdr_test_embed_ln: the output bits are reader.QAModel's), differentiable with respect to word, pos, type_table, weight and
    bias. ids and types (or None: every token is type 0) int64 [B, L], L the row length, at most pos.shape[0]; type_table fp32 [1 .. 4, H].
    pad_row is ELECTRA's word_embeddings.padding_idx: that row of the WORD table gets no gradient (-1: none); the position table has no such
    row, position 0 is every sequence's [CLS]. The backward is mdr_reader_embedding_backward on a plan built at forward time."""
    dev = _check_reader_pack(ids, types, tok_src, total, cap, L)
    vocab, max_pos, H, tv = _check_reader_params(word, pos, type_table, weight, dev)
    _check_reader_sizes(vocab, max_pos, L, tv, pad_row)
    if not is_like(bias, (torch.float32,), (H,), dev):
        raise ValueError(f"bias must be a contiguous fp32 [{H}] tensor on ids' device, got {describe(bias)}")
    return _PackedReaderEmbeddingLayerNorm.apply(ids, types, tok_src, total, L, word, pos, type_table, weight, bias, float(eps), cap, pad_row, bool(keep32))
