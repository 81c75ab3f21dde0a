"""What the tests of multihop_dense_retrieval_amd/reader_train.py share: the golden of scripts/gen_reader_train_golden.py
(tests/golden/reader_train_ref.npz: the reference's QAModel in training mode on the CPU in fp32), the committed tiny ELECTRA it ran on, a CPU
fp32 torch restatement of its computation with three switchable defects, and the error measure of the GPU test with its threshold.

The measure. Per parameter, over the entries the golden stores (every 1-D gradient and the type table's in full, position rows 0 .. L - 1,
the word rows of the ids that occur, rows 0, 32, 64, ... of every other matrix):  e = ||g / scale - g_gold|| / ||g_gold||.
Two parameters are left out of e because their gradient is identically zero, so that the golden holds rounding noise (norm ~1e-7) and a
ratio of noise to noise says nothing: encoder.encoder.layer.*.attention.self.key.bias (a constant added to every key of a row shifts every
score of a query by the same q . b, and the softmax does not see it) and qa_outputs.bias (a constant added to every start or end logit of
a row: the cross-entropy does not see it either). Each is held instead to ||g / scale|| <= THRESHOLD * ||g_gold(sibling)||, the sibling
being the layer's query.bias and rank.bias.

THRESHOLD. Measured on an MI355X (profiles/reader_train_step.md lists e per parameter): the largest e over both sets is written there; the
assertion is at four times that, rounded up to a power of two. The margin is for other seeds' fp16 rounding; every mutant below misses the
golden by more than ten times THRESHOLD (tests/test_reader_train_host.py asserts it), so the threshold cannot hide those defects.
"""
import json
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "reader_electra_tiny")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reader_train_ref.npz")
SETS = (("sp.b0", True), ("nosp.b1", False))
WORD = "encoder.embeddings.word_embeddings.weight"
POS = "encoder.embeddings.position_embeddings.weight"
TYPE = "encoder.embeddings.token_type_embeddings.weight"
MUTANTS = ("pos_row0_dropped", "type_all_to_row0", "pos_roberta")
THRESHOLD = 2.0 ** -6  # 4 x the largest measured e (profiles/reader_train_step.md), rounded up to a power of two
INT_KEYS = ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "label", "sent_offsets", "starts", "ends", "sent_labels")


def golden():
    return np.load(GOLDEN)


def tiny_config(p_hidden=0.0, p_attn=0.0):
    c = json.load(open(os.path.join(ASSETS, "config.json")))
    return types.SimpleNamespace(vocab_size=c["vocab_size"], hidden_size=c["hidden_size"], embedding_size=c["embedding_size"],
                                 num_hidden_layers=c["num_hidden_layers"], num_attention_heads=c["num_attention_heads"], intermediate_size=c["intermediate_size"],
                                 max_position_embeddings=c["max_position_embeddings"], type_vocab_size=c["type_vocab_size"], layer_norm_eps=c["layer_norm_eps"],
                                 hidden_act=c["hidden_act"], pad_token_id=c["pad_token_id"], hidden_dropout_prob=p_hidden, attention_probs_dropout_prob=p_attn)


def make_args(sp_pred, **kw):
    z = golden()
    base = dict(model_name="electra-tiny", sp_pred=sp_pred, sp_weight=float(z["meta.sp_weight"]), learning_rate=1e-4, adam_epsilon=1e-8, max_grad_norm=2.0,
                weight_decay=0.01, gradient_accumulation_steps=1, use_adam=False, fp16=True)
    base.update(kw)
    return types.SimpleNamespace(**base)


def checkpoint(sp_pred):
    """the committed fp32 weights, the parameters alone (no buffers), without sp.* for a model without the sp head"""
    from multihop_dense_retrieval_amd import reader
    sd = torch.load(os.path.join(ASSETS, "ckpt.pt"), map_location="cpu")
    return {k: sd[k].float().contiguous() for k in reader.expected_state_dict_shapes(tiny_config(), "electra", sp_pred)}


def batch_of(z, tag, device="cpu"):
    return {k: torch.from_numpy(z[f"{tag}.in.{k}"].astype(np.int64)).to(device) for k in INT_KEYS if f"{tag}.in.{k}" in z.files}


def stored(grads, z, tag):
    """{name: the entries of gradient `name` that the golden stores} from {name: whole gradient (numpy)}"""
    stride = int(z["meta.row_stride"])
    L = z[f"{tag}.in.input_ids"].shape[1]
    out = {}
    for name, g in grads.items():
        g = np.asarray(g)
        if g.ndim == 1 or name == TYPE:
            out[name] = g
        elif name == POS:
            out[name] = g[:L]
        elif name == WORD:
            out[name] = g[z[f"{tag}.rows.{WORD}"]]
        else:
            out[name] = g[::stride]
    return out


def zero_by_symmetry(name):
    """None, or the sibling whose golden norm gives the scale (module docstring)"""
    if name.endswith("attention.self.key.bias"):
        return name.replace("key.bias", "query.bias")
    return "rank.bias" if name == "qa_outputs.bias" else None


def errors(grads, z, tag):
    """{name: e} over the stored entries (module docstring); a gradient that is zero by symmetry maps to ||g|| / ||g_gold(sibling)||"""
    out = {}
    for name, g in stored(grads, z, tag).items():
        gold = z[f"{tag}.g.{name}"].astype(np.float64)
        assert gold.shape == g.shape, (name, gold.shape, g.shape)
        if zero_by_symmetry(name):
            out[name] = float(np.linalg.norm(g.astype(np.float64)) / np.linalg.norm(z[f"{tag}.g.{zero_by_symmetry(name)}"].astype(np.float64)))
        else:
            out[name] = float(np.linalg.norm(g.astype(np.float64) - gold) / np.linalg.norm(gold))
    return out


def restate(sd, batch, sp_pred, sp_weight, mutant=None):
    """Hugging Face's ElectraModel (post-LN BERT layers, erf GELU, absolute positions, token types, no dropout), QAModel's pooler and heads
    and reader_loss.host_loss, in torch fp32 on the CPU: (loss, {name: gradient as numpy}, scores). mutant: None, or one of MUTANTS --
    pos_row0_dropped: the position table's row 0 gets no gradient (the retriever's pad-row rule applied to it); type_all_to_row0: the whole
    type gradient lands in row 0; pos_roberta: position ids counted RoBERTa's way (1-based counts of the mask, offset by the pad id)."""
    from multihop_dense_retrieval_amd import reader_loss
    F = torch.nn.functional
    P = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    cfg = tiny_config()
    H, NH, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    ids, mask, tt = batch["input_ids"], batch["attention_mask"], batch["token_type_ids"]
    B, L = ids.shape
    pos_ids = torch.arange(L)[None].expand(B, L)
    if mutant == "pos_roberta":
        pos_ids = torch.cumsum(mask, 1) * mask + cfg.pad_token_id
    E = "encoder.embeddings."
    x = F.embedding(ids, P[E + "word_embeddings.weight"], padding_idx=cfg.pad_token_id) + F.embedding(pos_ids, P[E + "position_embeddings.weight"]) + \
        F.embedding(tt, P[E + "token_type_embeddings.weight"])
    h = F.layer_norm(x, (H,), P[E + "LayerNorm.weight"], P[E + "LayerNorm.bias"], eps)
    bias = (1.0 - mask[:, None, None, :].float()) * torch.finfo(torch.float32).min
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.encoder.layer.{i}."
        lin = lambda t, n: F.linear(t, P[p + n + ".weight"], P[p + n + ".bias"])  # noqa: E731
        split = lambda t: t.view(B, L, NH, H // NH).transpose(1, 2)  # noqa: E731
        q, k, v = (split(lin(h, "attention.self." + n)) for n in ("query", "key", "value"))
        a = torch.softmax(q @ k.transpose(-1, -2) / (H // NH) ** 0.5 + bias, -1) @ v
        a = a.transpose(1, 2).reshape(B, L, H)
        h1 = F.layer_norm(lin(a, "attention.output.dense") + h, (H,), P[p + "attention.output.LayerNorm.weight"], P[p + "attention.output.LayerNorm.bias"], eps)
        f = lin(F.gelu(lin(h1, "intermediate.dense")), "output.dense")
        h = F.layer_norm(f + h1, (H,), P[p + "output.LayerNorm.weight"], P[p + "output.LayerNorm.bias"], eps)
    pooled = torch.tanh(F.linear(h[:, 0], P["pooler.dense.weight"], P["pooler.dense.bias"]))
    logits = F.linear(h, P["qa_outputs.weight"], P["qa_outputs.bias"])
    outside = batch["paragraph_mask"].ne(1)
    start, end = (logits[..., j].masked_fill(outside, float("-inf")) for j in (0, 1))
    rank = F.linear(pooled, P["rank.weight"], P["rank.bias"])
    sp = None
    if sp_pred:
        idx = batch["sent_offsets"].unsqueeze(2).expand(-1, -1, H)
        sp = F.linear(torch.gather(h, 1, idx), P["sp.weight"], P["sp.bias"]).squeeze(2)
    loss = reader_loss.host_loss(start, end, rank, sp, batch, sp_weight)
    loss.backward()
    grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().copy() for k, v in P.items()}
    if mutant == "pos_row0_dropped":
        grads[POS][0] = 0
    if mutant == "type_all_to_row0":
        grads[TYPE][0] = grads[TYPE].sum(0)
        grads[TYPE][1:] = 0
    scores = {"start_logits": start.detach(), "end_logits": end.detach(), "rank_score": rank.detach(), "sp_score": None if sp is None else sp.detach()}
    return loss.detach(), grads, scores
