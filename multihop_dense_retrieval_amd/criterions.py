"""In-batch-negative evaluation of a retriever checkpoint (mdr/retrieval/criterions.py of the reference):

    mhop_eval(outputs, args)         :153-182  -> {"rrs_1": [...], "rrs_2": [...]}, on the device (include/mdr_inbatch.h)
    mhop_loss_value(outputs, fp16)   :114-151  the forward value of mhop_loss from the same kernel's log-sum-exp outputs
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
construction and by the exact-grid tests (tests/test_inbatch_rank_gpu.py), as reader.py does for its heads.
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
_bound = False


def lib():
    """libmdrhip.so with the signatures of include/mdr_inbatch.h bound (AttributeError if the library lacks one: no fallback)."""
    global _bound
    L = _lib.lib()
    if not _bound:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _bound = True
    return L


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
    L = lib()
    with torch.cuda.device(dev):
        need = int(L.mdr_inbatch_workspace_bytes(B, d, mode))
        ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(L.mdr_inbatch_rank(p(q), p(q_sp), p(ctx), p(neg), B, d, int(mode), p(out["rank1"]), p(out["rank2"]), p(out["tscore1"]),
                                      p(out["tscore2"]), p(out["lse1"]), p(out["lse2"]), p(ws) if ws is not None else None, need,
                                      _lib.current_stream_ptr(dev)))
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
