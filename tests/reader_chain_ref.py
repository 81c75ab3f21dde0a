"""Host statements of the WHOLE answer reader's training chain (multihop_dense_retrieval_amd/reader_train.py: TrainableReader.scores and
reader_loss.qa_loss), for the tests that run it as one chain at three layers (tests/test_reader_chain_host.py, tests/test_reader_chain_gpu.py).
CPU only, torch and numpy; nothing here imports anything compiled and nothing here was measured on a kernel. What the retriever's chain has in
tests/encoder_chain_ref.py: the rounding functions R, Rv, Rg and _GeluAt, the error ratios and the dropout replica's masks are THAT file's.

READER3    ELECTRA, 3 layers (a first, a middle and a last full layer), hidden 256, 4 heads of 64, FFN 384, vocab 512, 512 positions, 2 types,
           eps 1e-12, pad id 0. READER1 is the same at one layer: the depth every earlier value test of the reader's chain ran at.
BATCHES    two batches shaped as qa_collate builds them ([CLS] q [SEP] paragraph [SEP], right padding, types 1 behind the first [SEP],
           paragraph_mask over the paragraph without its last [SEP]): R160 (the ring attention kernel, rows on both sides of the 64-row chunks)
           and R48 (the one-shot kernel). Per row one to three answer candidates inside the paragraph (padded with -1), up to five sentence
           offsets in NS = 6 slots (the rest 0; a paragraph of fewer than five tokens has one per token), sent_labels, and label = row & 1.
           The question is short and the offsets sit in the paragraph's first tokens: the reference's loss weights a sentence's BCE by the
           VALUE of its offset, so large offsets would let the sp term own every gradient.
model64    the whole forward and the loss formula of reader_loss.host_loss in fp64, nothing rounded. Its gradients are the reference g64.
regime     the device chain's numerics restated in torch autograd: fp64 arithmetic, the VALUE and the INCOMING GRADIENT rounded to fp16 at
           every tensor the chain holds in fp16. The trunk: the points of tests/encoder_chain_ref.py in the trunk's default mode
           (residual_fp32 = 2), EVERY layer on all rows. The embedding: one fp16 copy next to the unrounded stream. The heads, the pooler and the
           loss (csrc/mdr_reader.inl, csrc/mdr_reader_loss.inl, tests/reader_loss_ref.py with o1 = True): the head weights AND biases are fp16
           values, the logits / rank / sp scores are fp16 and their gradients are rounded to fp16 once; the pooler dense is a packed Linear
           (fp16 input, weight and output, fp32 bias); pooled = fp16(tanh(dense)), differentiated AT that rounded value, its gradient
           fp16(g_rank w_rank) and the dense's fp16 again; the three heads' terms of d_h are added unrounded and rounded once; the final hidden
           state's fp16 copy has two consumers -- the heads and the CLS gather in front of the pooler -- whose fp16 gradients meet in an fp16 add.
           These points round ONCE from fp64 (_h1), as the numpy statement does that tests/test_reader_chain_host.py holds them equal to.
regime_b   a second correct implementation: the same in fp32 arithmetic with the batch reversed.
MUTATIONS  wiring defects of `regime`, one at a time, each a wrong composition of correct functions. ONE_LAYER_BLIND are those that change no
           element of any gradient at one layer.

Dropout (drop = (p, seed); None: none): explicit mask factors from the replica of tests/dropout_ref.py at site_of(0, layer, place), at the sites
reader_train.py uses -- behind the embedding LayerNorm as the also16 pair, on the probabilities, behind attention.output.dense and output.dense
in front of the residual -- every site over all rows: the reader has no CLS tail.

Criterion E is tests/encoder_chain_ref.py's (rel_errors, the factor 2, the floor e_pool) over the reader's parameters. Two kinds of parameter
have a gradient that is zero by symmetry (every attention.self.key.bias: softmax does not see a shift of a row of scores; qa_outputs.bias: nor
does the cross-entropy): what a computation returns there is rounding noise, two draws of which need not lie within a factor of each other.
Their row holds |g| over the fp64 norm of a sibling (the layer's query.bias, rank.bias) in place of the ratio, and its bar is the one
tests/reader_train_ref.py holds that same measure to (THRESHOLD, 2^-6). Rows that are exactly zero on both sides (zero_rows): word rows that
own no token, the pad row, position rows at or behind L, type rows no token has. The forward's score tensors are held by the same 2-norm
criterion over their finite entries (criterion_fwd); their -inf positions must be the same.
"""
import math
import types

import numpy as np
import torch

import dropout_ref
import encoder_chain_ref as ch
from encoder_chain_ref import R, Rg, Rv, _GeluAt
from oracle import roberta_torch, seeded
from reader_train_ref import THRESHOLD as ZERO_BAR

READER3 = dict(vocab=512, hidden=256, layers=3, heads=4, ffn=384, max_pos=512, type_vocab=2, ln_eps=1e-12, pad_id=0)
READER1 = dict(READER3, layers=1)
WEIGHT_SEED, BATCH_SEED = 29, 43
SP_WEIGHT = 0.25
NS, A = 6, 3
CLS, SEP = 2, 3
BATCHES = {"R160": (160, (160, 129, 65, 64, 33, 17)), "R48": (48, (48, 33, 17, 16, 9, 7))}
SCORES = ("start_logits", "end_logits", "rank_score", "sp_score")
INT_KEYS = ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "label", "sent_offsets", "starts", "ends", "sent_labels")
E_ = "encoder.embeddings."
WORD, POS, TYPE = E_ + "word_embeddings.weight", E_ + "position_embeddings.weight", E_ + "token_type_embeddings.weight"
MUTATIONS = ("res_from_embedding", "h16_from_embedding_qkv", "mid_dy16_dropped", "res_dropped_ln1_mid", "res_dropped_ln2_mid", "last_layer_cls_only",
             "cls_grad_not_added", "sp_grad_not_added", "site_layer_0", "attn_site_as_ao", "pos_roberta", "type_all_to_row0")
# a loop that runs once cannot show these: every gradient equals the unmutated regime's, element for element, on READER1
ONE_LAYER_BLIND = ("res_from_embedding", "h16_from_embedding_qkv", "mid_dy16_dropped", "res_dropped_ln1_mid", "res_dropped_ln2_mid", "site_layer_0")
DROP_ONLY = ("site_layer_0", "attn_site_as_ao")  # defects of which mask a site is handed: nothing without dropout
SP_ONLY = ("sp_grad_not_added",)
DROP = (ch.DROP_P, ch.DROP_SEED)


# ---- geometry, weights, batches --------------------------------------------------------------------------------------------------------------
def config(geom=READER3, p_hidden=0.0, p_attn=0.0):
    return types.SimpleNamespace(vocab_size=geom["vocab"], hidden_size=geom["hidden"], embedding_size=geom["hidden"], num_hidden_layers=geom["layers"],
                                 num_attention_heads=geom["heads"], intermediate_size=geom["ffn"], max_position_embeddings=geom["max_pos"],
                                 type_vocab_size=geom["type_vocab"], layer_norm_eps=geom["ln_eps"], hidden_act="gelu", pad_token_id=geom["pad_id"],
                                 hidden_dropout_prob=p_hidden, attention_probs_dropout_prob=p_attn)


def make_args(sp_pred, **kw):
    base = dict(model_name="electra-reader3", sp_pred=sp_pred, sp_weight=SP_WEIGHT, learning_rate=1e-4, adam_epsilon=1e-8, max_grad_norm=2.0, weight_decay=0.01,
                gradient_accumulation_steps=1, use_adam=False, fp16=True)
    base.update(kw)
    return types.SimpleNamespace(**base)


def state_dict_shapes(geom, sp_pred):
    """the keys and the order of reader.expected_state_dict_shapes(config(geom), "electra", sp_pred) (the host test holds the two equal)"""
    H = geom["hidden"]
    sd = {k: v for k, v in seeded.state_dict_shapes(dict(geom), with_pooler=False).items() if k.startswith("encoder.")}
    sd[TYPE] = (geom["type_vocab"], H)
    sd.update({"pooler.dense.weight": (H, H), "pooler.dense.bias": (H,), "qa_outputs.weight": (2, H), "qa_outputs.bias": (2,), "rank.weight": (1, H),
               "rank.bias": (1,)})
    if sp_pred:
        sd.update({"sp.weight": (1, H), "sp.bias": (1,)})
    return sd


def state_dict(geom=READER3, sp_pred=True, seed=WEIGHT_SEED):
    """name -> float32 ndarray in the manner of seeded.make_state_dict: LayerNorm weights 1 + 0.1 n, biases 0.1 n, tables 0.5 n, Linear weights
    (the heads' rows too) 1.5 n / sqrt(fan_in) so that every sub-layer's output is O(1). A tensor's values depend on its name and shape alone:
    the model without the sp head is the other one without sp.*, and READER1 is READER3's first layer."""
    out = {}
    for name, shape in state_dict_shapes(geom, sp_pred).items():
        if name.endswith("LayerNorm.weight"):
            out[name] = seeded.normal(seed, name, shape, 0.1, 1.0)
        elif name.endswith("bias"):
            out[name] = seeded.normal(seed, name, shape, 0.1, 0.0)
        elif "embeddings" in name:
            out[name] = seeded.normal(seed, name, shape, 0.5, 0.0)
        else:
            out[name] = seeded.normal(seed, name, shape, 1.5 / np.sqrt(shape[1]), 0.0)
    return out


def make_batch(name, geom=READER3, seed=BATCH_SEED):
    """{key: int64 ndarray} of INT_KEYS (module docstring). Row b of n tokens: [CLS] q tokens [SEP] at q + 1, the paragraph from p0 = q + 2 to
    n - 2, [SEP] at n - 1; q = n // 8 clipped to 1 .. 6."""
    L, lens = BATCHES[name]
    B = len(lens)
    body = seeded.integers(seed, f"reader.tok.{name}", (B, L), 5, geom["vocab"])
    pick = seeded.integers(seed, f"reader.pick.{name}", (B, 16), 0, 1 << 20)
    z = lambda *s: np.zeros(s, np.int64)  # noqa: E731
    ids, mask, tt, pm, so, sl = z(B, L), z(B, L), z(B, L), z(B, L), z(B, NS), z(B, NS)
    starts, ends = np.full((B, A), -1, np.int64), np.full((B, A), -1, np.int64)
    for b, n in enumerate(lens):
        q = max(1, min(n // 8, 6))
        p0, hi = q + 2, n - 1  # the paragraph is [p0, hi)
        assert hi - p0 >= 3
        ids[b, :n] = body[b, :n]
        ids[b, 0], ids[b, q + 1], ids[b, n - 1] = CLS, SEP, SEP
        mask[b, :n] = 1
        tt[b, p0:n] = 1
        pm[b, p0:hi] = 1
        step = max(1, min((hi - p0) // 5, 7))
        offs = [p0 + j * step for j in range(5) if p0 + j * step < hi]
        so[b, :len(offs)] = offs
        sl[b, :len(offs)] = pick[b, 8:8 + len(offs)] & 1
        for a in range(1 + b % A):
            s = p0 + int(pick[b, 2 * a]) % (hi - p0)
            starts[b, a], ends[b, a] = s, s + int(pick[b, 2 * a + 1]) % min(8, hi - s)
    label = (np.arange(B) & 1).astype(np.int64)
    assert set(label) == {0, 1}
    return {"input_ids": ids, "attention_mask": mask, "token_type_ids": tt, "paragraph_mask": pm, "label": label, "sent_offsets": so, "starts": starts,
            "ends": ends, "sent_labels": sl}


def torch_batch(batch, device="cpu"):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in batch.items()}


def zero_rows(batch, geom=READER3):
    """{table: bool [rows]}: the rows whose gradient is exactly zero -- word rows no masked-in token reads and the pad row, position rows no token
    stands at (all rows at or behind L among them), type rows no token has"""
    ids, mask, tt = (np.asarray(batch[k]) for k in ("input_ids", "attention_mask", "token_type_ids"))
    live = mask != 0
    word, pos, typ = np.ones(geom["vocab"], bool), np.ones(geom["max_pos"], bool), np.ones(geom["type_vocab"], bool)
    word[ids[live]] = False
    word[geom["pad_id"]] = True
    pos[np.nonzero(live)[1]] = False
    typ[tt[live]] = False
    return {WORD: word, POS: pos, TYPE: typ}


# ---- dropout masks ---------------------------------------------------------------------------------------------------------------------------
def dropout_masks(geom, batch, p, seed, mutation=None):
    """encoder_chain_ref.dropout_masks' layout for the reader: "emb" / "emb16" [B, L, hidden], ("attn", i) [B, heads, L, L], ("ao", i) and
    ("ff2", i) [B, L, hidden] for EVERY layer i (no CLS tail: that function lays a full layer out this way, so it is asked for one layer more
    and its CLS-only last one is left out). mutation: the mask-side defects of MUTATIONS."""
    ids, mask = np.asarray(batch["input_ids"]), np.asarray(batch["attention_mask"])
    nl = geom["layers"]
    full = ch.dropout_masks(dict(geom, layers=nl + 1), ids, mask, p, seed, 0)
    m = {k: v for k, v in full.items() if not (isinstance(k, tuple) and k[1] == nl)}
    assert len(m) == 3 * nl + 2
    if mutation == "site_layer_0":
        m = {k: (m[k[0], 0] if isinstance(k, tuple) else v) for k, v in m.items()}
    if mutation == "attn_site_as_ao":
        T = dropout_ref.threshold(p)
        lens = mask.sum(1).astype(np.int64)
        cu = np.concatenate([[0], np.cumsum(lens)])
        for i in range(nl):
            out = np.ones_like(m["attn", i])
            for b, per in enumerate(dropout_ref.attn_masks(cu, geom["heads"], 0, T, seed, ch.site_of(0, i, "ao"))):
                out[b, :, :lens[b], :lens[b]] = per
            m["attn", i] = out
    return m


# ---- the models ------------------------------------------------------------------------------------------------------------------------------
def _h1(t):
    """t rounded to fp16 ONCE, by numpy's conversion (reader_loss_ref.h16's). torch converts an fp64 tensor through fp32, and a product of
    an fp16 and a 22-bit value (d_pooled * (1 - pooled^2)) that lands within an fp32 ulp of an fp16 tie then goes the other way: one element
    of a batch, enough to part this statement from the numpy one it is held equal to. From fp32 the two conversions are the same."""
    with np.errstate(over="ignore"):
        return torch.from_numpy(t.detach().numpy().astype(np.float16)).to(t.dtype)


class _Round1(torch.autograd.Function):
    """encoder_chain_ref._Round with _h1: the rounding points of the heads, the pooler and the loss"""
    @staticmethod
    def forward(ctx, x, grad):
        ctx.grad = grad
        return _h1(x)

    @staticmethod
    def backward(ctx, g):
        return (_h1(g) if ctx.grad else g), None


def R1(x, label="?"):
    """R's signature; the label only names the rounding point at the call site (nothing records the heads' gradient peaks)"""
    return _Round1.apply(x, True)


def R1v(x):
    return _Round1.apply(x, False)


class _TanhAt(torch.autograd.Function):
    """fp16(tanh(x)), differentiated at that ROUNDED value as the device does (csrc/mdr_reader_loss.inl, point 10)"""
    @staticmethod
    def forward(ctx, x):
        y = _h1(torch.tanh(x))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * (1.0 - y * y)


def _ident(x, label=None):
    return x


def leaves(sd, dtype=torch.float64):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}


def loss_of(start, end, rank, sp, batch, sp_weight):
    """the formula and the torch calls of reader_loss.host_loss in the dtype of the scores (that function widens to fp32 and no further)"""
    F = torch.nn.functional
    label = batch["label"].reshape(-1, 1)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, reduction="none")
    rank_loss = F.binary_cross_entropy_with_logits(rank.reshape(-1, 1), label.to(rank.dtype), reduction="sum")
    loss_tensor = torch.stack([ce(start, a) for a in torch.unbind(batch["starts"], dim=1)], dim=1) + \
        torch.stack([ce(end, a) for a in torch.unbind(batch["ends"], dim=1)], dim=1)
    log_prob = -loss_tensor
    log_prob = log_prob.masked_fill(log_prob == 0, float("-inf"))
    marginal = torch.sum(torch.exp(log_prob), dim=1)
    counted = marginal[marginal != 0]
    loss = rank_loss + (-torch.log(counted).sum() if counted.numel() else start.sum() * 0.0)
    if sp is not None:
        bce = F.binary_cross_entropy_with_logits(sp, batch["sent_labels"].to(sp.dtype), reduction="none")
        loss = loss + ((bce * batch["sent_offsets"]) * label).sum() * sp_weight
    return loss


def heads_and_loss(W, h16, batch, sp_weight, exact=False, mutation=None):
    """(loss, scores) from the final hidden state's fp16 copy h16 [B, L, hidden] (in `regime` the tensor whose gradient rounding is the fp16 add
    of its consumers' gradients): the CLS gather, the pooler dense, the three heads, the loss. exact: nothing rounded. sp: iff W has sp.weight."""
    r, rv = (_ident, _ident) if exact else (R1, R1v)
    B, L, H = h16.shape
    hs = r(h16, "heads:d_h")  # the three heads' terms of d_h, added unrounded and rounded once
    cls = h16[:, 0]
    if mutation == "cls_grad_not_added":
        cls = cls.detach()
    dense = r(r(cls, "pooler.dense:x") @ rv(W["pooler.dense.weight"]).T + W["pooler.dense.bias"], "pooler.dense:y")
    pooled = torch.tanh(dense) if exact else R1(_TanhAt.apply(dense), "pooled:d")
    logits = r(hs @ rv(W["qa_outputs.weight"]).T + rv(W["qa_outputs.bias"]), "qa_outputs:y")
    outside = batch["paragraph_mask"].ne(1)
    start, end = (logits[..., j].masked_fill(outside, float("-inf")) for j in (0, 1))
    rank = r(pooled @ rv(W["rank.weight"]).T + rv(W["rank.bias"]), "rank:y")
    sp = None
    if "sp.weight" in W:
        src = hs.detach() if mutation == "sp_grad_not_added" else hs
        rows = torch.gather(src, 1, batch["sent_offsets"].unsqueeze(2).expand(-1, -1, H))
        sp = r(rows @ rv(W["sp.weight"]).T + rv(W["sp.bias"]), "sp:y").squeeze(2)
    scores = {"start_logits": start, "end_logits": end, "rank_score": rank, "sp_score": sp}
    return loss_of(start, end, rank, sp, batch, sp_weight), scores


def forward(W, geom, batch, sp_weight=SP_WEIGHT, exact=False, mutation=None, masks=None, tap=None):
    """(loss, scores) of one torch batch in the dtype of the leaves W. exact: model64 (nothing rounded); else the regime (module docstring).
    masks: torch constants in dropout_masks' layout, None for no dropout. tap: None, or a dict that receives the final hidden state "h16"."""
    dtype = W["rank.bias"].dtype
    r, rv, rg = (_ident, _ident, _ident) if exact else (R, Rv, Rg)
    H, nh, eps, pad, nl = geom["hidden"], geom["heads"], geom["ln_eps"], geom["pad_id"], geom["layers"]
    hd = H // nh
    ids, mask, tt = batch["input_ids"], batch["attention_mask"], batch["token_type_ids"]
    B, L = ids.shape
    pos = torch.arange(L).expand(B, L)
    if mutation == "pos_roberta":
        pos = torch.cumsum(mask, 1) * mask + pad
    ln = roberta_torch.layer_norm
    M = masks if masks is not None else {}
    x = (W[WORD][ids] + W[POS][pos]) + W[TYPE][tt]
    emb32 = ln(x, W[E_ + "LayerNorm.weight"], W[E_ + "LayerNorm.bias"], eps)
    emb16 = r(emb32 if masks is None else emb32 * M["emb16"], "emb.y16")  # the also16 pair: one mask, one rounding of the masked value
    if masks is not None:
        emb32 = emb32 * M["emb"]
    hidden = mask.eq(0)[:, None, None, :]

    def linear(t, name, gelu=False):
        z = r(t, name + ":x") @ rv(W[name + ".weight"]).T + W[name + ".bias"]
        if not gelu:
            return r(z, name + ":y")
        return ch._gelu(z) if exact else R(_GeluAt.apply(Rg(z, name + ":dZ"), False), name + ":y")

    def heads(t):
        return t.reshape(B, L, nh, hd).permute(0, 2, 1, 3)

    def dropped(y, key, name):
        """a Linear's fp16 output through the hidden dropout: fp16(fp32(y) * m), and fp16(dy * m) on the way back"""
        return y if masks is None else r(y * M[key], name + ":drop")

    def cls_only(t, dim):
        return torch.cat([t.narrow(dim, 0, 1), t.narrow(dim, 1, t.shape[dim] - 1).detach()], dim)

    h16, h32 = emb16, emb32
    for i in range(nl):
        p = f"encoder.encoder.layer.{i}."
        mid, tail = i == 1, mutation == "last_layer_cls_only" and i == nl - 1
        x16 = emb16 if mutation == "h16_from_embedding_qkv" else h16
        if mutation == "mid_dy16_dropped" and mid:
            x16 = x16.detach()
        q, k, v = (heads(linear(x16, p + "attention.self." + n)) for n in ("query", "key", "value"))
        if tail:  # the retriever's last layer: the query, the attention and the tail of the CLS rows alone
            q = cls_only(q, 2)
        s = rg((q @ k.transpose(-1, -2) / math.sqrt(hd)).masked_fill(hidden, float("-inf")), p + "attention:dS")
        pr = torch.softmax(s, -1)
        if masks is not None:  # Pd = p o m, rounded as the operand of Pd V only; dP = (dO V^T) o m in front of the rounding of dS
            pr = pr * M["attn", i]
        ctx = r(rv(pr) @ v, p + "attention:ctx").permute(0, 2, 1, 3).reshape(B, L, H)
        res = emb32 if mutation == "res_from_embedding" else h32
        if mutation == "res_dropped_ln1_mid" and mid:
            res = res.detach()
        if tail:
            res = cls_only(res, 1)
        ao = dropped(linear(ctx, p + "attention.output.dense"), ("ao", i), p + "attention.output.dense")
        a32 = ln(ao + res, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        f = linear(linear(r(a32, p + "attention.output.LayerNorm:y16"), p + "intermediate.dense", True), p + "output.dense")
        f = dropped(f, ("ff2", i), p + "output.dense")
        res = a32.detach() if mutation == "res_dropped_ln2_mid" and mid else a32
        h32 = ln(f + res, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
        h16 = r(h32, p + "output.LayerNorm:y16")
    if tap is not None:
        tap["h16"] = h16.detach().clone()
    return heads_and_loss(W, h16, batch, sp_weight, exact, mutation)


# ---- runs ------------------------------------------------------------------------------------------------------------------------------------
def run(kind, sd, geom, batch, scale=1.0, mutation=None, drop=None, sp_weight=SP_WEIGHT):
    """{"loss": float, "grads": {parameter: float64 ndarray}, "scores": {name: float64 ndarray or None}} of kind "model64", "regime" or
    "regime_b" on the numpy batch. The backward runs on scale * loss (the loss scale riding in the gradient) and the result is divided by
    it. drop: None, (p, seed), or ready-made masks in dropout_masks' layout (of the ORIGINAL row order). The sp head: iff sd has sp.weight."""
    dtype, flip, exact = {"model64": (torch.float64, False, True), "regime": (torch.float64, False, False), "regime_b": (torch.float32, True, False)}[kind]
    assert mutation is None or (mutation in MUTATIONS and not exact), mutation
    masks = drop if drop is None or isinstance(drop, dict) else dropout_masks(geom, batch, *drop, mutation=mutation)
    masks = ch._torch_masks(masks, dtype, flip)
    tb = torch_batch({k: (np.asarray(v)[::-1].copy() if flip else np.asarray(v)) for k, v in batch.items()})
    W = leaves(sd, dtype)
    loss, scores = forward(W, geom, tb, sp_weight, exact, mutation, masks)
    (loss * scale).backward()
    g = {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.detach().to(torch.float64).numpy() / scale) for k, v in W.items()}
    if mutation == "type_all_to_row0":
        g[TYPE] = np.concatenate([g[TYPE].sum(0, keepdims=True), np.zeros_like(g[TYPE][1:])])
    out = {k: None if v is None else v.detach().to(torch.float64).numpy().reshape(len(tb["label"]), -1) for k, v in scores.items()}
    return {"loss": float(loss.detach()), "grads": g, "scores": {k: (v if v is None or not flip else v[::-1].copy()) for k, v in out.items()}}


# ---- criterion E -----------------------------------------------------------------------------------------------------------------------------
def zero_by_symmetry(name):
    """None, or the sibling whose fp64 norm gives the scale (tests/reader_train_ref.py)"""
    if name.endswith("attention.self.key.bias"):
        return name.replace("key.bias", "query.bias")
    return "rank.bias" if name == "qa_outputs.bias" else None


def criterion_e(g_cand, g_reg, g64):
    """encoder_chain_ref.criterion_e over the reader's parameters: [(p, e_cand, e_reg, bar, e_cand / bar)] and e_pool of the regime; passing:
    every share <= 1. A parameter that is zero by symmetry is not part of e_pool, has |g| / |g64(sibling)| as its e and ZERO_BAR as its bar."""
    names = [k for k in g64 if not zero_by_symmetry(k)]
    e_reg, e_pool = ch.rel_errors(g_reg, g64, names)
    e_cand, _ = ch.rel_errors(g_cand, g64, names)
    for k in g64:
        if zero_by_symmetry(k):
            n = ch._norm(g64[zero_by_symmetry(k)])
            e_reg[k], e_cand[k] = ch._norm(g_reg[k]) / n, ch._norm(g_cand[k]) / n
    rows = []
    for k in g64:
        bar = ZERO_BAR if zero_by_symmetry(k) else 2.0 * max(e_reg[k], e_pool)
        rows.append((k, e_cand[k], e_reg[k], bar, e_cand[k] / bar))
    return rows, e_pool


def criterion_fwd(s_cand, s_reg, s64):
    """the same over the forward's score tensors, each on its finite entries: rows as criterion_e's, e_pool, and whether the -inf positions of
    the candidate are the fp64 model's"""
    names = [k for k in SCORES if s64[k] is not None]
    fin = {k: np.isfinite(s64[k]) for k in names}
    same_inf = all(np.array_equal(np.asarray(s_cand[k], np.float64) == -np.inf, ~fin[k]) and not np.isnan(np.asarray(s_cand[k], np.float64)).any() for k in names)
    pick = lambda s: {k: np.asarray(s[k], np.float64)[fin[k]] for k in names}  # noqa: E731
    e_reg, e_pool = ch.rel_errors(pick(s_reg), pick(s64), names)
    e_cand, _ = ch.rel_errors(pick(s_cand), pick(s64), names) if same_inf else ({k: float("inf") for k in names}, None)
    rows = [(k, e_cand[k], e_reg[k], 2.0 * max(e_reg[k], e_pool), e_cand[k] / (2.0 * max(e_reg[k], e_pool))) for k in names]
    return rows, e_pool, same_inf


def exact_zeros_hold(g, batch, geom=READER3):
    """the rows of zero_rows are exactly zero in g, and the tables have other rows that are not"""
    zr = zero_rows(batch, geom)
    return all(not np.asarray(g[k])[zr[k]].any() for k in zr) and all(np.asarray(g[k])[~zr[k]].any() for k in zr) and zr[WORD].any() and zr[POS].any()


failures, table = ch.failures, ch.table
