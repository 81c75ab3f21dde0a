"""The answer reader's training step on the HIP bricks (what train.py is for the retriever):

    model = TrainableReader(config, args).cuda();  model.load_state_dict(...)
    opt = optimizer_for(model, args)
    loss = train_step(model, batch["net_inputs"], args, opt, seed);  opt.step();  scheduler.step()

TrainableReader is a torch.nn.Module whose parameters are the reference QAModel's named_parameters() for ELECTRA (the keys and the order of
reader.expected_state_dict_shapes(config, "electra", sp_pred), query / key / value as separate leaves). forward() is one pass through the
differentiable functions of the package: mdr_test_pack, embedding.packed_reader_embedding_layer_norm (absolute positions, the token type
table), per layer linear.packed_linear (the three projections as one GEMM over the concatenated leaves), attention.packed_self_attention in
mode 0, layernorm.packed_layer_norm and dropout.packed_dropout -- EVERY layer on all rows: the heads need every token's final hidden state --
then the pooler dense on the CLS rows (gathered on the device by cu[:-1]), reader_loss.reader_heads and, in train() mode,
reader_loss.qa_loss. The kernels are the inference reader's: in eval() mode, or with dropout off, the four score tensors equal
reader.QAModel(batch) bit for bit on the same weights. The reference's QAModel adds no dropout of its own (mdr/qa/qa_model.py): the sites
are the encoder's. Only the default numerics mode of the trunk (residual_fp32 = 2) is built.

Everything runs on one HIP device and is enqueued on the current stream; there is no CPU fallback. `batch` is a qa_collate net_inputs dict
that already holds starts, ends, label and, with --sp-pred, sent_labels: the training dataset and MhopSampler are qa_train_data.py, the
batches come from qa_train_arena.py, and the loop is scripts/train_qa.py --do_train.
"""
import os

import torch

from . import _lib, dropout as _dropout, optim, reader, reader_loss
from ._lib import ptr
from .attention import packed_self_attention
from .embedding import packed_reader_embedding_layer_norm
from .layernorm import packed_layer_norm
from .linear import packed_linear
from .train import NO_DECAY

_E = "encoder.embeddings."


def decay_groups(names):
    """(decay, no_decay): scripts/train_qa.py:106-113 of the reference over every name, each group in the given order. A name belongs to
    no_decay when it CONTAINS "bias" or "LayerNorm.weight" (train.NO_DECAY: the retriever's rule; the reader's pooler, unlike the
    retriever's, trains and decays)."""
    names = list(names)
    return ([n for n in names if not any(nd in n for nd in NO_DECAY)], [n for n in names if any(nd in n for nd in NO_DECAY)])


def fp16_copy_names(names):
    """The Linear weights the chain reads as fp16 through linear.packed_linear, of which optim.FusedAdam keeps a current fp16 copy: the
    trunk's and the pooler's. (The three head rows are rounded inside reader_loss.reader_heads.)"""
    return [n for n in names if n.endswith(".weight") and ("dense" in n or "attention.self." in n)]


class TrainableReader(torch.nn.Module):
    def __init__(self, config, args):
        super().__init__()
        mode = int(os.environ.get("MDR_RESIDUAL_FP32", str(reader.QAModel.RESIDUAL_FP32_DEFAULT)))
        if mode != 2:
            raise NotImplementedError(f"training is built for the trunk's default numerics mode only (residual_fp32 = 2), not for MDR_RESIDUAL_FP32={mode}")
        family = reader.model_family(args.model_name, config)  # (refuses RoBERTa, SpanBERT, ELECTRA-small, a hidden_act other than gelu)
        if family != "electra":
            raise NotImplementedError(f"{args.model_name}: the trainable reader is built for ELECTRA only (QAModel's own pooler.dense)")
        if not 1 <= int(config.type_vocab_size) <= 4:
            raise NotImplementedError(f"type_vocab_size = {config.type_vocab_size}: the embedding backward keeps sums for 1 .. 4 type rows")
        self.config, self.args = config, args
        self.sp_pred = bool(getattr(args, "sp_pred", False))
        self.hidden_dropout_prob = float(getattr(config, "hidden_dropout_prob", 0.0))
        self.attention_probs_dropout_prob = float(getattr(config, "attention_probs_dropout_prob", 0.0))
        self.shapes = reader.expected_state_dict_shapes(config, "electra", self.sp_pred)
        for name, shape in self.shapes.items():
            if name.endswith("LayerNorm.weight"):
                t = torch.ones(shape)
            elif name.endswith("bias"):
                t = torch.zeros(shape)
            else:
                t = torch.empty(shape).normal_(0.0, 0.02)
            self._register(name, torch.nn.Parameter(t))

    def _register(self, dotted, param):
        mod = self
        *path, leaf = dotted.split(".")
        for part in path:
            if part not in mod._modules:
                mod.add_module(part, torch.nn.Module())
            mod = mod._modules[part]
        mod.register_parameter(leaf, param)

    def leaves(self):
        """{name: parameter} in state_dict order."""
        return dict(self.named_parameters())

    # -- the forward -----------------------------------------------------------------------------------------------------------------------
    def scores(self, batch, half=None, dropout=None):
        """{'start_logits', 'end_logits' fp16 [B, L], 'rank_score' fp16 [B, 1], 'sp_score' fp16 [B, NS] or None} of one qa_collate
        net_inputs dict, differentiable with respect to every parameter. half: None, or a function from a weight leaf to its current fp16
        copy (optim.FusedAdam.half). dropout: None for none, or the seed: the probabilities are this module's, every call at
        dropout.site_of(0, layer, place). A probability whose threshold is 0 makes no call."""
        P = self.leaves()
        cfg = self.config
        NH, EPS, PAD, nl = cfg.num_attention_heads, float(cfg.layer_norm_eps), int(getattr(cfg, "pad_token_id", 0) or 0), cfg.num_hidden_layers
        dev = P["rank.bias"].device
        if dev.type != "cuda":
            raise RuntimeError("the trainable reader runs on a HIP device only (there is no CPU fallback)")
        ids = batch["input_ids"].to(device=dev, dtype=torch.int64).contiguous()
        mask = batch["attention_mask"].to(device=dev, dtype=torch.int64).contiguous()
        if ids.dim() != 2 or ids.shape != mask.shape:
            raise ValueError(f"input_ids {tuple(ids.shape)} and attention_mask {tuple(mask.shape)} must both be [B, L]")
        B, L = ids.shape
        if L > reader.MAX_SEQ_LEN or L > cfg.max_position_embeddings:
            raise ValueError(f"sequence length {L} > min({reader.MAX_SEQ_LEN}, max_position_embeddings = {cfg.max_position_embeddings})")
        if B and L > 1 and bool((mask[:, 1:] > mask[:, :-1]).any()):  # the heads address position p of row b as packed token cu[b] + p
            raise ValueError("attention_mask must be right-padded (a prefix of ones in every row), as qa_collate builds it")
        tt = batch.get("token_type_ids", None)
        tt = None if tt is None else tt.to(device=dev, dtype=torch.int64).contiguous()
        cap = B * L
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
        lens, cu, total, order, src, pid = i32(B), i32(B + 1), i32(1), i32(B), i32(cap), i32(cap)
        _lib.call(_lib.lib().mdr_test_pack, ptr(ids), ptr(mask), B, L, PAD, ptr(lens), ptr(cu), ptr(total), ptr(order), ptr(src), ptr(pid), dev=dev)
        T_hid = T_att = 0
        seed = None
        if dropout is not None:
            seed = int(dropout)
            T_hid, T_att = _dropout.threshold(self.hidden_dropout_prob), _dropout.threshold(self.attention_probs_dropout_prob)

        def linear(x, names, gelu=False, rows=None):
            w = P[names[0] + ".weight"] if len(names) == 1 else torch.cat([P[n + ".weight"] for n in names])
            b = P[names[0] + ".bias"] if len(names) == 1 else torch.cat([P[n + ".bias"] for n in names])
            if half is None:
                return packed_linear(x, w, b, gelu, rows)
            w16 = half(P[names[0] + ".weight"]) if len(names) == 1 else torch.cat([half(P[n + ".weight"]) for n in names])
            return packed_linear(x, w, b, gelu, rows, w16)

        def ln(x, res, name):
            return packed_layer_norm(x, res, P[name + ".weight"], P[name + ".bias"], EPS, total, True)

        def drop(x, i, place):
            return _dropout.packed_dropout(x, self.hidden_dropout_prob, seed, _dropout.site_of(0, i, place), total) if T_hid else x

        h16, h32 = packed_reader_embedding_layer_norm(ids, tt, src, total, L, P[_E + "word_embeddings.weight"], P[_E + "position_embeddings.weight"],
                                                      P[_E + "token_type_embeddings.weight"], P[_E + "LayerNorm.weight"], P[_E + "LayerNorm.bias"], EPS, cap,
                                                      PAD, True)
        if T_hid:
            h32, h16 = _dropout.packed_dropout(h32, self.hidden_dropout_prob, seed, _dropout.site_of(0, 0, "emb"), total, True)
        for i in range(nl):
            p = f"encoder.encoder.layer.{i}."
            qkv = linear(h16, [p + "attention.self." + n for n in ("query", "key", "value")], False, total)
            att = (self.attention_probs_dropout_prob, seed, _dropout.site_of(0, i, "attn")) if T_att else None
            ctx = packed_self_attention(qkv, cu, NH, L, False, dropout=att)
            ao = drop(linear(ctx, [p + "attention.output.dense"], False, total), i, "ao")
            a16, a32 = ln(ao, h32, p + "attention.output.LayerNorm")
            f2 = linear(linear(a16, [p + "intermediate.dense"], True, total), [p + "output.dense"], False, total)
            h16, h32 = ln(drop(f2, i, "ff2"), a32, p + "output.LayerNorm")
        # the pooler dense on the CLS rows, gathered on the device: cu[b] is the packed row of sequence b's first token
        cls16 = h16[cu[:-1].to(torch.int64)].contiguous()
        dense16 = linear(cls16, ["pooler.dense"])
        heads = {k: P[k] for k in reader_loss.HEAD_KEYS if k in P}
        return reader_loss.reader_heads(h16, dense16, cu, batch, heads)

    def forward(self, batch, seed=None, half=None):
        """train() mode: the [1] fp32 loss of the reference's QAModel.forward (reader_loss.qa_loss with args.sp_weight), every dropout site
        live under the caller's `seed`. eval() mode: the dict of the four score tensors, no dropout call."""
        if not self.training:
            return self.scores(batch, half)
        live = _dropout.threshold(self.hidden_dropout_prob) or _dropout.threshold(self.attention_probs_dropout_prob)
        if live and seed is None:
            raise ValueError("a training forward with dropout needs the caller's seed")
        s = self.scores(batch, half, int(seed) if live else None)
        return reader_loss.qa_loss(s["start_logits"], s["end_logits"], s["rank_score"], s["sp_score"], batch, float(getattr(self.args, "sp_weight", 0.0)))

    def inference(self):
        """A reader.QAModel loaded from the current masters (device tensors; the library keeps its own fp16 copies), in eval mode."""
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        dev = sd["rank.bias"].device
        m = reader.QAModel(self.config, self.args)
        m.load_state_dict(sd)
        return m.to(dev).eval()


def optimizer_for(model, args, loss_scale="dynamic"):
    """The reference's two weight-decay groups (decay_groups) over model's parameters as an optim.FusedAdam with an fp16 copy of every
    Linear weight the chain reads in fp16: transformers.AdamW (decoupled decay) unless --use_adam, as scripts/train_qa.py:115-120 chooses.
    The product computes in fp16 whether or not --fp16 is given, so the loss scale is always on (dynamic unless a number is given)."""
    P = dict(model.named_parameters())
    decay, no_decay = decay_groups(list(P))
    groups = [{"params": [P[n] for n in decay], "weight_decay": float(args.weight_decay)}, {"params": [P[n] for n in no_decay], "weight_decay": 0.0}]
    return optim.FusedAdam(groups, lr=args.learning_rate, eps=args.adam_epsilon, max_grad_norm=args.max_grad_norm, loss_scale=loss_scale,
                           fp16_copies=[P[n] for n in fp16_copy_names(list(P))], decoupled_weight_decay=not getattr(args, "use_adam", False))


RANK_ROWS = "_rank_rows"  # a batch that holds one rank's rows alone says so here: (lo, hi, B), widths of the full batch (train.RANK_ROWS)


def rank_rows(batch, world):
    """(this rank's rows of `batch`, lo, hi): rows dist.slice_bounds(B, N)[rank] of the full batch's tensors, the widths untouched, so a
    row's input does not depend on the rank count. A batch that carries RANK_ROWS holds those rows already (scripts/train_qa.py's feed);
    its tensors may be missing altogether when the slice is empty."""
    from . import dist
    if RANK_ROWS in batch:
        lo, hi, B = batch[RANK_ROWS]
        local = {k: v for k, v in batch.items() if k != RANK_ROWS}
    else:
        B = int(batch["input_ids"].shape[0])
        lo, hi = dist.slice_bounds(B, world.size)[world.rank]
        local = {k: v[lo:hi] if torch.is_tensor(v) and v.dim() and v.shape[0] == B else v for k, v in batch.items()}
    if (lo, hi) != dist.slice_bounds(B, world.size)[world.rank]:
        raise ValueError(f"the batch holds rows {lo} .. {hi} of {B}, rank {world.rank} of {world.size} owns {dist.slice_bounds(B, world.size)[world.rank]}")
    return local, lo, hi


def train_step(model, batch, args, opt, seed, world=None, bucket=None):
    """One forward and backward of the reader's loss: model(batch, seed, opt.half), divided by gradient_accumulation_steps, scaled by the
    optimizer's loss scale for the backward. Returns the unscaled loss (a [1] device tensor). The caller owns opt.step() and
    scheduler.step(); FusedAdam zeroes the gradients in place, so zero_grad() is never called.

    world (a dist.TorchWorld or a rank of dist.LoopbackWorld) and bucket (the dist.GradBucket behind the parameters' gradients): the step of
    one rank of several. The reference's loss is a plain sum over the rows, so the full batch's loss is the sum of the
    ranks' partial losses and nothing is gathered before it: the rank forwards its rows (rank_rows) under dist.rank_seed(seed, rank) and
    backpropagates its partial loss; the caller runs bucket.reduce() at the accumulation boundary, immediately before opt.step(). A rank
    without rows makes no forward and no backward and contributes +0.0 and an all-zero bucket. Every rank returns the same bits: the
    partial losses (each already divided by gradient_accumulation_steps) added in rank order by dist.scalar_rank_sum. No division by the
    rank count: N ranks train what one rank trains."""
    if not model.training:
        raise RuntimeError("train_step needs the model in train() mode")
    if world is None:
        loss = model(batch, seed=seed, half=opt.half)
        if args.gradient_accumulation_steps > 1:
            loss = loss / args.gradient_accumulation_steps
        opt.scale_loss(loss).backward()
        return loss.detach()
    from . import dist
    if bucket is None or bucket.world is not world:
        raise ValueError("a step on several ranks needs the dist.GradBucket of this world behind the gradients")
    local, lo, hi = rank_rows(batch, world)
    if hi > lo:
        loss = model(local, seed=dist.rank_seed(seed, world.rank), half=opt.half)
        if args.gradient_accumulation_steps > 1:
            loss = loss / args.gradient_accumulation_steps
        opt.scale_loss(loss).backward()
        part = loss.detach()
    else:
        part = torch.zeros(1, dtype=torch.float32, device=bucket.flat.device)
    return dist.scalar_rank_sum(world, part)
