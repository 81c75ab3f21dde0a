"""Host statements of the WHOLE retriever encoder's backward, for the tests that chain the differentiable functions of the package
(tests/test_encoder_chain_host.py, tests/test_encoder_chain_gpu.py). CPU only, torch and numpy; nothing here imports the product and nothing
here was measured on a kernel.

model64    the fp64 model with no rounding anywhere: oracle/roberta_torch.encode (o1 = None) on fp64 leaf tensors; its loss is loss64, the
           formula of tests/mhop_loss_ref.py written with differentiable torch ops. Its gradients are the reference g64.
regime     an independent restatement of the device chain's numerics in plain torch autograd: fp64 arithmetic, and an fp16 rounding of the
           VALUE (forward) and of the INCOMING GRADIENT (backward) at every tensor the device chain holds in fp16:
             each Linear's input, its fp16 weight (value only: dW is fp32) and its fp16 output; the scores' gradient dS (the operand of the
             dQ / dK contractions); P as operand of P V (value only) and ctx; the GELU output, with GELU' taken at the fp16 pre-activation and
             dZ rounded; the fp16 copy of each LayerNorm output next to the unrounded one (the fp32 residual stream); the head's fp16
             pre-activation (project.0 through the fp16 Linear). The in-batch loss rounds as `o1` of tests/mhop_loss_ref.py does.
           The dataflow is the default mode of the product's trunk (residual_fp32 = 2): a Linear's fp16 output meets the fp32 stream in the
           LayerNorm; the last layer runs its query, its attention and its tail on the CLS rows alone.
regime_b   a second correct implementation: the same in fp32 arithmetic with the batch reversed.
MUTATIONS  wiring defects of `regime`, one at a time (what a wrong composition of correct functions looks like). MID_MUTATIONS are the ones
           that touch only a full layer that has a full layer behind it (0 < i < layers - 1): they change nothing on a two-layer geometry.

Every function takes the geometry (oracle.seeded.TINY or DEEP); the default is TINY.

Dropout (drop = (p, seed, encode); None: none, and then every function computes what it computed before dropout came). dropout_masks builds the
explicit mask FACTORS (0 or dropout_ref.scale(T)) of every site of one encode from the replica of tests/dropout_ref.py; site_of is the one
site function the host and the device chain share. The factors are constants of the differentiated function: model64 and regime multiply by
them where Hugging Face RoBERTa has its dropout modules -- behind the embedding LayerNorm, on the softmax probabilities, behind
attention.output.dense and output.dense in front of the residual add; none in the project head. The rounding points dropout adds to the
regime, read off csrc/mdr_dropout.hip and DESIGN.md 23: h32 * m unrounded with ONE fp16 copy (the also16 pair: the gradient is
m (g32 + fp32(g16))); a Linear's fp16 output y becomes R(R(z) * m), so the gradient the LayerNorm hands back (fp16) is rounded again behind
the mask; Pd = p o m is rounded only as the operand of Pd V; dP is multiplied by m in front of the rounding of dS. regime_b takes the masks of
the ORIGINAL sequence order and reverses them with the batch. DROP_MUTATIONS are the wiring defects of the dropout recipe.

Criterion E (criterion_e). For every parameter tensor p, e(p) = |g(p) - g64(p)|_2 / |g64(p)|_2, and e_pool the same ratio over all compared
tensors at once. A candidate passes when e_cand(p) <= 2 max(e_reg(p), e_pool) for every p: the yardstick is the reference regime's own error.
The factor 2: the candidate and `regime` share the rounding points but not the summation orders, so their errors against fp64 are two draws of
one size. The floor e_pool: a few tensors have e_reg = 0 (project.1.bias is a plain sum of the cotangent).

Not compared by a ratio (ZERO_GRAD): attention.self.key.bias of every layer. Softmax is invariant under a shift of a row of scores, and the key
bias adds q_i . b_k to every score of query i: its gradient is mathematically zero, what a computation returns is rounding noise, and no
relative criterion over it can hold. Rows of word_embeddings that own no token, and padding_idx's row, are exactly zero on both sides
(zero_rows): equality is asserted there.
"""
import math

import numpy as np
import torch

import dropout_ref
from oracle import roberta_torch, seeded

GEOM = seeded.TINY
WEIGHT_SEED = 23
KEYS = ("q", "q_sp1", "c1", "c2", "neg_1", "neg_2")
# (L, lengths): 501 tokens in 1280 slots, the ring attention kernel, row counts on both sides of the 64-row chunks; and the one-shot kernel
BATCHES = {"L160": (160, (1, 2, 17, 63, 64, 65, 129, 160)), "L48": (48, (1, 5, 16, 17, 33, 48))}
# the six encodes of the in-batch loss: 4 sequences each, two padded lengths
LOSS_L = {"q": 48, "q_sp1": 48, "c1": 160, "c2": 160, "neg_1": 48, "neg_2": 160}
MUTATIONS = ("res_dropped_ln1", "res_dropped_ln2", "cls_rows_not_added", "dy2_dropped", "dw_qk_swapped", "last_call_only", "gelu_grad_at_output",
             "pos_from_padded_index", "mid_stream_cls_only", "mid_dy16_dropped", "res_dropped_ln1_mid", "res_dropped_ln2_mid")
# the defects that only a full layer BEHIND a full layer can show (0 < i < layers - 1): invisible on a two-layer geometry
MID_MUTATIONS = MUTATIONS[-4:]
# dropout: the reference's rate, a seed whose high word is set, and the wiring defects of the recipe with dropout (each a wrong composition of
# correct functions): the first two are defects of the dataflow, the others of which mask a site is handed
DROP_P, DROP_SEED = 0.1, 0x5EED0123456789AB
PLACES = ("emb", "attn", "ao", "ff2")
MAX_LAYERS = 64
DROP_MUTATIONS = ("drop_after_residual", "cls_tail_not_dropped", "cls_mask_from_packed_row", "hidden_mask_from_padded_index", "attn_mask_of_reversed_batch",
                  "keep_without_scale", "ao_ff2_share_site", "emb_h16_h32_masks_differ")


def site_of(encode, layer, place):
    """the uint32 site of one dropout call: encode 0 .. 5 (the index in KEYS; a dense run is encode 0), layer 0 .. layers - 1, place one of
    PLACES ("emb" belongs to layer 0). Injective, and never 0. Used by the host models and by the device chain (tests/encoder_chain_dev.py)."""
    assert 0 <= encode < len(KEYS) and 0 <= layer < MAX_LAYERS and (place != "emb" or layer == 0)
    return 1 + (encode * MAX_LAYERS + layer) * len(PLACES) + PLACES.index(place)


def param_names(geom=GEOM):
    return [k for k in seeded.state_dict_shapes(geom, with_pooler=False)]


def zero_grad_names(geom=GEOM):
    return [k for k in param_names(geom) if k.endswith("attention.self.key.bias")]


def state_dict(geom=GEOM, seed=WEIGHT_SEED):
    return seeded.make_state_dict(seed, geom, with_pooler=False)


def make_batch(L, lens, seed, geom=GEOM):
    """ids, mask int64 [B, L]: <s> tokens </s> then pad (a sequence of one token is <s> alone)"""
    B = len(lens)
    body = seeded.integers(seed, f"chain.tok.{L}", (B, L), 3, geom["vocab"])
    ids, mask = np.full((B, L), geom["pad_id"], np.int64), np.zeros((B, L), np.int64)
    for b, n in enumerate(lens):
        ids[b, :n] = body[b, :n]
        ids[b, 0] = 0
        if n >= 2:
            ids[b, n - 1] = 2
        mask[b, :n] = 1
    return ids, mask


def batch(name, geom=GEOM):
    L, lens = BATCHES[name]
    return make_batch(L, lens, 31, geom)


def loss_batches(geom=GEOM):
    return {k: seeded.make_token_batch(37 + i, "chain." + k, 4, LOSS_L[k], geom["vocab"], pad_fill=geom["pad_id"])
            for i, k in enumerate(KEYS)}


def cotangent(B, geom=GEOM):
    return seeded.normal(41, f"chain.G.{B}", (B, geom["hidden"])).astype(np.float32)


def zero_rows(batches, geom=GEOM):
    """bool [vocab]: the rows of word_embeddings whose gradient is exactly zero -- no masked-in token of any batch reads them, or padding_idx"""
    used = np.zeros(geom["vocab"], bool)
    for ids, mask in batches:
        used[np.asarray(ids)[np.asarray(mask) != 0]] = True
    used[geom["pad_id"]] = False
    return ~used


# ---- rounding points -----------------------------------------------------------------------------------------------------------------------
def _h(t):
    return t.to(torch.float16).to(t.dtype)


GRAD_PEAKS = None  # a dict while record_grad_peaks() is open: {label of a gradient-rounding point: the largest |g| it was handed, before rounding}


class record_grad_peaks:
    """with record_grad_peaks() as peaks: ... -- every gradient-rounding point of the regime notes the largest magnitude it is handed BEFORE it
    rounds it to fp16 (tests/overflow_ref.py predicts from it which loss scales overflow). Nothing is recorded outside the block."""

    def __enter__(self):
        global GRAD_PEAKS
        GRAD_PEAKS = {}
        return GRAD_PEAKS

    def __exit__(self, *exc):
        global GRAD_PEAKS
        GRAD_PEAKS = None


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, value, grad, label):
        ctx.grad, ctx.label = grad, label
        return _h(x) if value else x.clone()

    @staticmethod
    def backward(ctx, g):
        if ctx.grad and GRAD_PEAKS is not None and g.numel():
            GRAD_PEAKS[ctx.label] = max(GRAD_PEAKS.get(ctx.label, 0.0), float(g.detach().abs().max()))
        return (_h(g) if ctx.grad else g), None, None, None


def R(x, label="?"):
    """a tensor the device holds in fp16: its value and its gradient are rounded"""
    return _Round.apply(x, True, True, label)


def Rv(x):
    """an fp16 operand made from an fp32 tensor whose gradient stays fp32 (a weight, P)"""
    return _Round.apply(x, True, False, None)


def Rg(x, label="?"):
    """an fp32 value whose gradient the device rounds to fp16 (the scores, the GELU's pre-activation)"""
    return _Round.apply(x, False, True, label)


def _gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def _gelu_grad(u):
    return 0.5 * torch.erfc(-u / math.sqrt(2.0)) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


class _GeluAt(torch.autograd.Function):
    """gelu(z), differentiated at the fp16 pre-activation as the device does (at_output: at the rounded OUTPUT, a defect)"""
    @staticmethod
    def forward(ctx, z, at_output):
        y = _gelu(z)
        ctx.save_for_backward(_h(y) if at_output else _h(z))
        return y

    @staticmethod
    def backward(ctx, g):
        (at,) = ctx.saved_tensors
        return g * _gelu_grad(at), None


# ---- the encoders --------------------------------------------------------------------------------------------------------------------------
def leaves(sd, dtype=torch.float64):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items() if "pooler" not in k}


_MASKS = {}


def dropout_masks(geom, ids, mask, p, seed, encode, mutation=None):
    """the mask factors (float64: 0 or dropout_ref.scale(T)) of every dropout site of ONE encode, on the padded tensors the host models use:
         "emb"       [B, L, hidden]                 ("emb16": the fp16 copy's, the same array but under emb_h16_h32_masks_differ)
         ("attn", i) [B, heads, L, L] for a full layer (mode 0), [B, heads, 1, L] for the last one (mode 3: query 0 alone)
         ("ao", i), ("ff2", i)  [B, L, hidden] for a full layer, [B, hidden] for the last one
    THE MAPPING, stated here once. The device packs the masked-in tokens sequence after sequence: cu[b] = the number of tokens of the sequences
    in front of b, and token t of sequence b is packed row cu[b] + t. A hidden site's mask of that token is row cu[b] + t of
    dropout_ref.hidden_keep(total, hidden, ...); on the B CLS rows of the last layer (rows = None) the row index is the sequence index b.
    An attention site's mask of (b, h, i, j) is dropout_ref.attn_masks(cu, ...)[b][h, i, j]: its counter holds b * heads + h, b the index in
    THIS call's cu. Padded positions own no mask element: their factor is 1 (no valid token reads them).
    mutation: the mask-side defects of DROP_MUTATIONS; any other value builds the correct masks."""
    ids, mask = np.asarray(ids), np.asarray(mask)
    key = (tuple(sorted(geom.items())), ids.tobytes(), mask.tobytes(), ids.shape, float(p), int(seed), int(encode), mutation if mutation in DROP_MUTATIONS else None)
    if key in _MASKS:
        return _MASKS[key]
    T = dropout_ref.threshold(p)
    assert T > 0, "no dropout is drop = None"
    H, nh, nl = geom["hidden"], geom["heads"], geom["layers"]
    B, L = ids.shape
    lens = mask.sum(1).astype(np.int64)
    assert all((mask[b, :n] == 1).all() for b, n in enumerate(lens)), "a sequence's tokens are its first ones"
    cu = np.concatenate([[0], np.cumsum(lens)])
    total = int(cu[-1])
    factor = float(dropout_ref.scale(T)) if mutation != "keep_without_scale" else 1.0

    def hidden_rows(site):
        """[B, L, hidden]: row cu[b] + t of the packed mask at (b, t)"""
        out = np.ones((B, L, H))
        if mutation == "hidden_mask_from_padded_index":
            keep = dropout_ref.hidden_keep(B * L, H, T, seed, site).reshape(B, L, H)
            for b, n in enumerate(lens):
                out[b, :n] = keep[b, :n] * factor
            return out
        keep = dropout_ref.hidden_keep(total, H, T, seed, site)
        for b, n in enumerate(lens):
            out[b, :n] = keep[cu[b]:cu[b] + n] * factor
        return out

    def hidden_cls(site):
        """[B, hidden]: row b"""
        if mutation == "cls_tail_not_dropped":
            return np.ones((B, H))
        if mutation == "cls_mask_from_packed_row":
            return dropout_ref.hidden_keep(total, H, T, seed, site)[cu[:-1]] * factor
        return dropout_ref.hidden_keep(B, H, T, seed, site) * factor

    def attn(site, mode):
        out = np.ones((B, nh, 1 if mode == 3 else L, L))
        if mutation == "attn_mask_of_reversed_batch":  # every sequence at full length: the mask of (b, h, i, j) does not depend on the lengths
            full = dropout_ref.attn_masks(np.arange(B + 1) * L, nh, mode, T, seed, site)
            per = [full[B - 1 - b][:, :(1 if mode == 3 else n), :n] for b, n in enumerate(lens)]
        else:
            per = dropout_ref.attn_masks(cu, nh, mode, T, seed, site)
        for b, n in enumerate(lens):
            out[b, :, :(1 if mode == 3 else n), :n] = (per[b] != 0) * factor
        return out

    m = {"emb": hidden_rows(site_of(encode, 0, "emb"))}
    m["emb16"] = m["emb"]
    if mutation == "emb_h16_h32_masks_differ":
        m["emb16"] = hidden_rows(site_of(encode, 0, "emb") ^ 0x80000000)
    for i in range(nl):
        last = i == nl - 1
        ao, ff2 = site_of(encode, i, "ao"), site_of(encode, i, "ff2")
        if mutation == "ao_ff2_share_site":
            ff2 = ao
        m["attn", i] = attn(site_of(encode, i, "attn"), 3 if last else 0)
        m["ao", i], m["ff2", i] = (hidden_cls(ao), hidden_cls(ff2)) if last else (hidden_rows(ao), hidden_rows(ff2))
    _MASKS[key] = m
    return m


def ones_masks(masks):
    return {k: np.ones_like(v) for k, v in masks.items()}


def _torch_masks(masks, dtype, flip):
    """the masks as torch constants; flip: the batch reversed (regime_b takes the masks of the original order)"""
    return None if masks is None else {k: torch.tensor(v[::-1].copy() if flip else v, dtype=dtype) for k, v in masks.items()}


def model64(W, geom, ids, mask, masks=None):
    """[B, hidden] fp64, differentiable with respect to the fp64 leaves W: nothing is rounded. masks (torch constants, dropout_masks' layout):
    the same model with the factors where Hugging Face RoBERTa has dropout; the last layer then runs its query and its tail on the CLS rows
    alone, which changes nothing mathematically (nothing else of it is read) and is what the last layer's masks are laid out for"""
    if masks is None:
        return roberta_torch.encode(W, geom, ids, mask, torch.float64, o1=None)
    H, nh, eps, pad, nl = geom["hidden"], geom["heads"], geom["ln_eps"], geom["pad_id"], geom["layers"]
    hd = H // nh
    ids, mask = torch.as_tensor(ids), torch.as_tensor(mask)
    B, L = ids.shape
    tok = (ids != pad).long()
    pos = torch.cumsum(tok, 1) * tok + pad
    ln = roberta_torch.layer_norm
    e = "encoder.embeddings."
    x = W[e + "word_embeddings.weight"][ids] + W[e + "position_embeddings.weight"][pos] + W[e + "token_type_embeddings.weight"][0]
    x = ln(x, W[e + "LayerNorm.weight"], W[e + "LayerNorm.bias"], eps) * masks["emb"]
    add_mask = ((1.0 - mask.to(torch.float64)) * -10000.0)[:, None, None, :]
    for i in range(nl):
        p = f"encoder.encoder.layer.{i}."
        lin = lambda t, n: t @ W[p + n + ".weight"].T + W[p + n + ".bias"]  # noqa: E731
        q, k, v = (lin(x, "attention.self." + n).reshape(B, L, nh, hd).permute(0, 2, 1, 3) for n in ("query", "key", "value"))
        if i == nl - 1:
            q, x = q[:, :, :1], x[:, 0]
        pr = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd) + add_mask, -1) * masks["attn", i]
        ctx = (pr @ v).permute(0, 2, 1, 3).reshape(B, -1, H)
        if i == nl - 1:
            ctx = ctx[:, 0]
        x = ln(lin(ctx, "attention.output.dense") * masks["ao", i] + x, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        x = ln(lin(_gelu(lin(x, "intermediate.dense")), "output.dense") * masks["ff2", i] + x, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
    return ln(x @ W["project.0.weight"].T + W["project.0.bias"], W["project.1.weight"], W["project.1.bias"], eps)


def regime_encode(W, geom, ids, mask, mutation=None, masks=None):
    """[B, hidden] in the dtype of the leaves W (module docstring). masks: torch constants in dropout_masks' layout, None for no dropout"""
    dtype = W["project.1.bias"].dtype
    H, nh, eps, pad, nl = geom["hidden"], geom["heads"], geom["ln_eps"], geom["pad_id"], geom["layers"]
    hd = H // nh
    ids, mask = torch.as_tensor(ids), torch.as_tensor(mask)
    B, L = ids.shape
    m = (ids != pad).long()
    pos = torch.cumsum(m, 1) * m + pad
    if mutation == "pos_from_padded_index":
        pos = torch.arange(L).expand(B, L)
    ln = roberta_torch.layer_norm
    e = "encoder.embeddings."
    x = (W[e + "word_embeddings.weight"][ids] + W[e + "position_embeddings.weight"][pos]) + W[e + "token_type_embeddings.weight"][0]
    h32 = ln(x, W[e + "LayerNorm.weight"], W[e + "LayerNorm.bias"], eps)
    M = masks if masks is not None else {}
    h16 = R(h32 if masks is None else h32 * M["emb16"], "emb.y16")  # the also16 pair: one mask (emb16 is emb), one rounding of the masked value
    if masks is not None:
        h32 = h32 * M["emb"]
    add_mask = ((1.0 - mask.to(dtype)) * -10000.0)[:, None, None, :]

    def linear(t, name, gelu=False):
        z = R(t, name + ":x") @ Rv(W[name + ".weight"]).T + W[name + ".bias"]
        return R(_GeluAt.apply(Rg(z, name + ":dZ"), mutation == "gelu_grad_at_output"), name + ":y") if gelu else R(z, name + ":y")

    def heads(t):
        return t.reshape(B, -1, nh, hd).permute(0, 2, 1, 3)

    def dropped(y, key, name):
        """a Linear's fp16 output through the hidden dropout: fp16(fp32(y) * m), and fp16(dy * m) on the way back"""
        return y if masks is None or mutation == "drop_after_residual" else R(y * M[key], name + ":drop")

    def after(s, key):
        """drop_after_residual: the mask on the sum (a defect)"""
        return s * M[key] if masks is not None and mutation == "drop_after_residual" else s

    def tail(p, ctx, h32, i, li):
        """i: the index of a full layer, None for the last layer's CLS rows; li: the layer's index"""
        first, mid = i == 0, i == 1
        res = h32.detach() if (mutation == "res_dropped_ln1" and first) or (mutation == "res_dropped_ln1_mid" and mid) else h32
        if mutation == "mid_stream_cls_only" and i is not None and i > 0:  # every layer taken for the one under the last
            res = torch.cat([res[:, :1], res[:, 1:].detach()], 1)
        ao = dropped(linear(ctx, p + "attention.output.dense"), ("ao", li), p + "attention.output.dense")
        a32 = ln(after(ao + res, ("ao", li)), W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps)
        f = linear(linear(R(a32, p + "attention.output.LayerNorm:y16"), p + "intermediate.dense", True), p + "output.dense")
        f = dropped(f, ("ff2", li), p + "output.dense")
        drop2 = (mutation == "res_dropped_ln2" and first) or (mutation == "res_dropped_ln2_mid" and mid) or (mutation == "dy2_dropped" and not first)
        res = a32.detach() if drop2 else a32
        o32 = ln(after(f + res, ("ff2", li)), W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps)
        return R(o32, p + "output.LayerNorm:y16"), o32

    for i in range(nl):
        p = f"encoder.encoder.layer.{i}."
        last = i == nl - 1
        x16 = h16.detach() if (mutation == "mid_dy16_dropped" and 0 < i < nl - 1) else h16
        q, k, v = (heads(linear(x16, p + "attention.self." + n)) for n in ("query", "key", "value"))
        if last:  # the query, the attention and the tail of the CLS rows alone
            q = q[:, :, :1]
        s = Rg(q @ k.transpose(-1, -2) / math.sqrt(hd) + add_mask, p + "attention:dS")
        pr = torch.softmax(s, -1)
        if masks is not None:  # Pd = p o m, rounded as the operand of Pd V only; on the way back dP = (dO V^T) o m in front of Rg's rounding of dS
            pr = pr * M["attn", i]
        ctx = R(Rv(pr) @ v, p + "attention:ctx").permute(0, 2, 1, 3).reshape(B, -1, H)
        if last:
            cls32 = h32[:, 0]
            h16, h32 = tail(p, ctx[:, 0], cls32.detach() if mutation == "cls_rows_not_added" else cls32, None, i)
        else:
            h16, h32 = tail(p, ctx, h32, i, i)
    y = linear(h16, "project.0")
    return ln(y, W["project.1.weight"], W["project.1.bias"], eps)


# ---- the loss ------------------------------------------------------------------------------------------------------------------------------
def _loss(o, mm, bmm):
    B = o["q"].shape[0]
    rows = torch.arange(B)
    total = 0.0
    for h, x in enumerate((o["q"], o["q_sp1"])):
        s = torch.cat([mm(x, torch.cat([o["c1"], o["c2"]])), bmm(x, torch.stack([o["neg_1"], o["neg_2"]], 1))], 1)
        if h == 0:
            hide = torch.zeros_like(s, dtype=torch.bool)
            hide[rows, B + rows] = True
            s = s.masked_fill(hide, float("-inf"))
        total = total + (torch.logsumexp(s, 1) - s[rows, rows + (B if h else 0)]).mean()
    return total


def loss64(o):
    """the formula of tests/mhop_loss_ref.py (no queue) on six [B, d] tensors, differentiable, nothing rounded"""
    return _loss(o, lambda x, c: x @ c.T, lambda x, n: torch.einsum("bd,bnd->bn", x, n))


def loss_regime(o):
    """mode O1 of tests/mhop_loss_ref.py: fp16 operands, fp16 scores, g rounded to fp16, every contraction's backward result rounded to fp16 per
    call, the terms of one leaf added unrounded"""
    return _loss(o, lambda x, c: R(R(x, "loss:operand") @ R(c, "loss:operand").T, "loss:g"),
                 lambda x, n: R(torch.einsum("bd,bnd->bn", R(x, "loss:operand"), R(n, "loss:operand")), "loss:g"))


# ---- gradients -----------------------------------------------------------------------------------------------------------------------------
def _encoder(kind):
    if kind == "model64":
        return torch.float64, False, model64
    if kind == "regime":
        return torch.float64, False, regime_encode
    if kind == "regime_b":
        return torch.float32, True, regime_encode
    raise ValueError(kind)


def _finish(W, mutation):
    g = {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.detach().to(torch.float64).numpy().copy()) for k, v in W.items()}
    if mutation == "dw_qk_swapped":
        for k in [k for k in g if k.endswith("attention.self.query.weight")]:
            k2 = k.replace("query", "key")
            g[k], g[k2] = g[k2], g[k]
    return g


def _masks_for(geom, ids, mask, drop, mutation, dtype, flip):
    """drop: None, (p, seed, encode), or ready-made masks in dropout_masks' layout (of the ORIGINAL sequence order)"""
    if drop is None or isinstance(drop, dict):
        return _torch_masks(drop, dtype, flip)
    return _torch_masks(dropout_masks(geom, ids, mask, *drop, mutation=mutation), dtype, flip)


def grads_cotangent(kind, sd, geom, ids, mask, G, scale=1.0, mutation=None, drop=None):
    """(embeddings float64 [B, hidden], {parameter: d <embeddings, G> / d parameter, float64}): the backward runs on scale * G (a loss scale
    riding in the gradient, a power of two) and the result is divided by it. drop: _masks_for's"""
    dtype, flip, enc = _encoder(kind)
    W = leaves(sd, dtype)
    ids, mask, G = np.asarray(ids), np.asarray(mask), np.asarray(G)
    masks = _masks_for(geom, ids, mask, drop, mutation if enc is regime_encode else None, dtype, flip)
    if flip:
        ids, mask, G = ids[::-1].copy(), mask[::-1].copy(), G[::-1].copy()
    out = enc(W, geom, ids, mask, mutation, masks) if enc is regime_encode else enc(W, geom, ids, mask, masks)
    out.backward(torch.tensor(G * scale, dtype=dtype))
    emb = out.detach().to(torch.float64).numpy()
    return (emb[::-1].copy() if flip else emb), {k: v / scale for k, v in _finish(W, mutation).items()}


def grads_loss(kind, sd, geom, batches, mutation=None, drop=None):
    """(loss, {parameter: gradient}, {name: embeddings}, {name: d loss / d embeddings}) of the in-batch loss over six encodes that share the
    weights. Each encode differentiates into leaves of its own; the parameter's gradient is their sum (last_call_only: the last one's alone).
    drop: None or (p, seed): encode number n of KEYS draws the masks of site_of(n, ., .)"""
    dtype, flip, enc = _encoder(kind)
    Ws, o = [], {}
    for n, k in enumerate(KEYS):
        ids, mask = batches[k]
        masks = _masks_for(geom, ids, mask, None if drop is None else (*drop, n), mutation if enc is regime_encode else None, dtype, flip)
        if flip:
            ids, mask = ids[::-1].copy(), mask[::-1].copy()
        W = leaves(sd, dtype)
        Ws.append(W)
        out = enc(W, geom, ids, mask, mutation, masks) if enc is regime_encode else enc(W, geom, ids, mask, masks)
        o[k] = (out.flip(0) if flip else out)
        o[k].retain_grad()
    loss = (loss64 if kind == "model64" else loss_regime)(o)
    loss.backward()
    per = [_finish(W, mutation) for W in Ws]
    keep = per[-1:] if mutation == "last_call_only" else per
    g = {k: sum(p[k] for p in keep) for k in per[0]}
    return (float(loss.detach()), g, {k: v.detach().to(torch.float64).numpy() for k, v in o.items()},
            {k: v.grad.detach().to(torch.float64).numpy() for k, v in o.items()})


# ---- criterion E ---------------------------------------------------------------------------------------------------------------------------
def _norm(a):
    return float(np.sqrt((np.asarray(a, np.float64) ** 2).sum()))


def rel_errors(g, g64, names):
    """({p: |g - g64| / |g64|}, the same ratio over all of `names` at once)"""
    per = {k: _norm(np.asarray(g[k], np.float64) - g64[k]) / _norm(g64[k]) for k in names}
    num = math.sqrt(sum(_norm(np.asarray(g[k], np.float64) - g64[k]) ** 2 for k in names))
    return per, num / math.sqrt(sum(_norm(g64[k]) ** 2 for k in names))


def criterion_e(g_cand, g_reg, g64, geom=GEOM):
    """[(p, e_cand, e_reg, bar, e_cand / bar)] over every parameter but ZERO_GRAD's, and e_pool of the regime. Passing: every ratio <= 1."""
    skip = set(zero_grad_names(geom))
    names = [k for k in param_names(geom) if k not in skip]
    e_reg, e_pool = rel_errors(g_reg, g64, names)
    e_cand, _ = rel_errors(g_cand, g64, names)
    rows = []
    for k in names:
        bar = 2.0 * max(e_reg[k], e_pool)
        rows.append((k, e_cand[k], e_reg[k], bar, e_cand[k] / bar))
    return rows, e_pool


def failures(rows):
    return [r for r in rows if not r[4] <= 1.0]


def table(rows, e_pool, title):
    short = lambda k: k.replace("encoder.encoder.layer.", "L").replace("encoder.embeddings.", "emb.").replace("attention.", "att.")  # noqa: E731
    out = [f"{title}: e_pool(regime) = {e_pool:.3e}", "| tensor | e_cand | e_reg | e_cand / e_reg | e_cand / bar |", "|---|---|---|---|---|"]
    for k, ec, er, bar, share in rows:
        out.append(f"| {short(k)} | {ec:.3e} | {er:.3e} | {(ec / er if er > 0 else float('inf')):.2f} | {share:.2f} |")
    return "\n".join(out)
