"""Training of the multi-hop retriever on the HIP bricks (the recipe of §18 as a module of the package):

    model = TrainableRetriever(config, args).cuda();  model.load_state_dict(...)
    opt = optimizer_for(model, args)
    loss = train_step(model, batch, args, opt, seed);  opt.step();  scheduler.step()

TrainableRetriever is a torch.nn.Module whose parameters are the reference's named_parameters() (the keys and the order of
retriever.expected_state_dict_shapes, query / key / value as separate leaves, the never-evaluated pooler carried along without a gradient).
encode() is one encoder pass through the differentiable functions of the package -- mdr_test_pack, embedding.packed_embedding_layer_norm,
per layer linear.packed_linear (the three projections as one GEMM over the concatenated leaves), attention.packed_self_attention,
layernorm.packed_layer_norm, dropout.packed_dropout, the last layer on the CLS rows alone (gathered on the device: the host never reads the
mask) -- and then the head: head.packed_head_linear, whose fp32 sums go to the last LayerNorm exactly as the inference encoder's do
(EPI_BIAS_F32). With dropout off the training forward therefore equals RobertaRetriever.encode_seq bit for bit. head_fp16=True is the head
the recipe was tested with before the fp32 brick existed (linear.packed_linear: one more rounding of the head's sums); it is kept as the
switch that ties this module to that recipe. Only the default numerics mode of the trunk (residual_fp32 = 2) is built.

Everything runs on one HIP device and is enqueued on the current stream; there is no CPU fallback. This module imports nothing outside the
package.
"""
import os

import torch

from . import _lib, criterions, dropout as _dropout, optim, retriever
from ._lib import ptr
from .attention import packed_self_attention
from .embedding import packed_embedding_layer_norm
from .head import packed_head_linear
from .layernorm import packed_layer_norm
from .linear import packed_linear

# the encode number of dropout.site_of for each output of one in-batch loss
ENCODE_INDEX = {"q": 0, "q_sp1": 1, "c1": 2, "c2": 3, "neg_1": 4, "neg_2": 5}
NO_DECAY = ("bias", "LayerNorm.weight")  # train_mhop.py:125 of the reference, matched by substring as it is there
_E = "encoder.embeddings."


def trainable_names(names):
    """The names an optimizer steps: all but the pooler's, whose gradient is None in the reference (Adam skips it there)."""
    return [n for n in names if "pooler" not in n]


def decay_groups(names):
    """(decay, no_decay): the reference's two groups over the trainable names, each in the given order. A name belongs to no_decay when it
    CONTAINS "bias" or "LayerNorm.weight"; project.1.weight (the head's LayerNorm, a Sequential member) contains neither and decays."""
    names = trainable_names(names)
    return ([n for n in names if not any(nd in n for nd in NO_DECAY)], [n for n in names if any(nd in n for nd in NO_DECAY)])


def fp16_copy_names(names):
    """The Linear weights: the leaves a Linear reads as fp16, of which optim.FusedAdam keeps a current fp16 copy."""
    return [n for n in trainable_names(names) if n.endswith(".weight") and ("dense" in n or "attention.self." in n or n == "project.0.weight")]


def accumulation_boundary(batch_step, gradient_accumulation_steps):
    """train_mhop.py:181 of the reference, quirk included: batch_step counts from 1 and the update comes when batch_step + 1 is a multiple,
    so with g > 1 the first update follows g - 1 batches."""
    return (batch_step + 1) % gradient_accumulation_steps == 0


def run_epoch(batches, step_fn, update_fn, gradient_accumulation_steps, batch_step=0):
    """One pass of the reference's inner loop over `batches`: step_fn(batch, batch_step) for every batch, update_fn(batch_step) at every
    accumulation boundary. Returns the new batch_step."""
    for batch in batches:
        batch_step += 1
        step_fn(batch, batch_step)
        if accumulation_boundary(batch_step, gradient_accumulation_steps):
            update_fn(batch_step)
    return batch_step


class TrainableRetriever(torch.nn.Module):
    def __init__(self, config, args=None, head_fp16=False):
        super().__init__()
        mode = int(os.environ.get("MDR_RESIDUAL_FP32", str(retriever.RobertaRetriever.RESIDUAL_FP32_DEFAULT)))
        if mode != 2:
            raise NotImplementedError(f"training is built for the trunk's default numerics mode only (residual_fp32 = 2), not for MDR_RESIDUAL_FP32={mode}")
        self.config, self.args, self.head_fp16 = config, args, bool(head_fp16)
        self.hidden_dropout_prob = float(getattr(config, "hidden_dropout_prob", 0.0))
        self.attention_probs_dropout_prob = float(getattr(config, "attention_probs_dropout_prob", 0.0))
        self.shapes = retriever.expected_state_dict_shapes(config)
        H = config.hidden_size
        head = torch.nn.Linear(H, H)  # torch's default initialisers for project.0, drawn from the global generator
        for name, shape in self.shapes.items():
            if name == "project.0.weight":
                t = head.weight.detach().clone()
            elif name == "project.0.bias":
                t = head.bias.detach().clone()
            elif name.endswith("LayerNorm.weight") or name == "project.1.weight":
                t = torch.ones(shape)
            elif name.endswith("bias"):
                t = torch.zeros(shape)
            else:
                t = torch.empty(shape).normal_(0.0, 0.02)
            self._register(name, torch.nn.Parameter(t, requires_grad="pooler" not in name))

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
    def encode(self, ids, mask, half=None, dropout=None):
        """[B, hidden] fp32 embeddings of one batch of token ids and masks (int64 [B, L] on the parameters' device), differentiable with
        respect to every parameter but the pooler. half: None, or a function from a weight leaf to its current fp16 copy
        (optim.FusedAdam.half). dropout: None for none, or (seed, encode): the probabilities are this module's hidden_dropout_prob and
        attention_probs_dropout_prob, every call at dropout.site_of(encode, layer, place). A probability whose threshold is 0 makes no call
        (the embedding then keeps its own fp16 copy)."""
        P = self.leaves()
        cfg = self.config
        NH, EPS, PAD, nl = cfg.num_attention_heads, float(cfg.layer_norm_eps), int(cfg.pad_token_id), cfg.num_hidden_layers
        dev = P["project.1.bias"].device
        if dev.type != "cuda":
            raise RuntimeError("the trainable retriever runs on a HIP device only (there is no CPU fallback)")
        ids = ids.to(device=dev, dtype=torch.int64).contiguous()
        mask = mask.to(device=dev, dtype=torch.int64).contiguous()
        if ids.dim() != 2 or ids.shape != mask.shape:
            raise ValueError(f"input_ids {tuple(ids.shape)} and mask {tuple(mask.shape)} must both be [B, L]")
        B, L = ids.shape
        cap = B * L
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
        lens, cu, total, order, src, pid = i32(B), i32(B + 1), i32(1), i32(B), i32(cap), i32(cap)
        _lib.call(_lib.lib().mdr_test_pack, ptr(ids), ptr(mask), B, L, PAD, ptr(lens), ptr(cu), ptr(total), ptr(order), ptr(src), ptr(pid), dev=dev)
        T_hid = T_att = 0
        if dropout is not None:
            seed, enc = dropout
            T_hid, T_att = _dropout.threshold(self.hidden_dropout_prob), _dropout.threshold(self.attention_probs_dropout_prob)

        def linear(x, names, gelu=False, rows=None):
            w = P[names[0] + ".weight"] if len(names) == 1 else torch.cat([P[n + ".weight"] for n in names])
            b = P[names[0] + ".bias"] if len(names) == 1 else torch.cat([P[n + ".bias"] for n in names])
            if half is None:
                return packed_linear(x, w, b, gelu, rows)
            w16 = half(P[names[0] + ".weight"]) if len(names) == 1 else torch.cat([half(P[n + ".weight"]) for n in names])
            return packed_linear(x, w, b, gelu, rows, w16)

        def ln(x, res, name, rows=None):
            return packed_layer_norm(x, res, P[name + ".weight"], P[name + ".bias"], EPS, rows, True)

        def attn(qkv, cls_only, i):
            drop = (self.attention_probs_dropout_prob, seed, _dropout.site_of(enc, i, "attn")) if T_att else None
            return packed_self_attention(qkv, cu, NH, L, cls_only, dropout=drop)

        def drop(x, i, place, rows):
            return _dropout.packed_dropout(x, self.hidden_dropout_prob, seed, _dropout.site_of(enc, i, place), rows) if T_hid else x

        def tail(p, ctx, res32, rows, i):
            ao = drop(linear(ctx, [p + "attention.output.dense"], False, rows), i, "ao", rows)
            a16, a32 = ln(ao, res32, p + "attention.output.LayerNorm", rows)
            f2 = linear(linear(a16, [p + "intermediate.dense"], True, rows), [p + "output.dense"], False, rows)
            return ln(drop(f2, i, "ff2", rows), a32, p + "output.LayerNorm", rows)

        h16, h32 = packed_embedding_layer_norm(ids, src, pid, total, P[_E + "word_embeddings.weight"], P[_E + "position_embeddings.weight"],
                                               P[_E + "token_type_embeddings.weight"][0], P[_E + "LayerNorm.weight"], P[_E + "LayerNorm.bias"], EPS,
                                               cap, PAD, True)
        if T_hid:
            h32, h16 = _dropout.packed_dropout(h32, self.hidden_dropout_prob, seed, _dropout.site_of(enc, 0, "emb"), total, True)
        for i in range(nl):
            p = f"encoder.encoder.layer.{i}."
            qkv = linear(h16, [p + "attention.self." + n for n in ("query", "key", "value")], False, total)
            if i < nl - 1:
                h16, h32 = tail(p, attn(qkv, False, i), h32, total, i)
            else:  # the CLS rows alone, gathered on the device: cu[b] is the packed row of sequence b's first token
                cls32 = h32[cu[:-1].to(torch.int64)]
                h16, h32 = tail(p, attn(qkv, True, i), cls32, None, i)
        if self.head_fp16:
            y = linear(h16, ["project.0"])
        else:
            w = P["project.0.weight"]
            y = packed_head_linear(h16, w, P["project.0.bias"], None if half is None else half(w))
        return packed_layer_norm(y, None, P["project.1.weight"], P["project.1.bias"], EPS, None, True)[1]

    def forward(self, batch, seed=None, half=None):
        """The six [B, hidden] fp32 matrices of one mhop_collate batch, in the order of RobertaRetriever.FORWARD_INPUTS. In train() mode every
        dropout site is live under the caller's `seed` (one per forward: two forwards that share a seed share their masks); in eval() mode no
        dropout call is made."""
        live = self.training and (_dropout.threshold(self.hidden_dropout_prob) or _dropout.threshold(self.attention_probs_dropout_prob))
        if live and seed is None:
            raise ValueError("a training forward with dropout needs the caller's seed")
        return {name: self.encode(batch[f"{key}_input_ids"], batch[f"{key}_mask"], half, (int(seed), ENCODE_INDEX[name]) if live else None)
                for name, key in retriever.RobertaRetriever.FORWARD_INPUTS}

    def inference(self):
        """A retriever.RobertaRetriever loaded from the current masters (device tensors; the library keeps its own fp16 copies), in eval mode."""
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        dev = sd["project.1.bias"].device
        m = retriever.RobertaRetriever(self.config, self.args)
        m.load_state_dict(sd)
        return m.to(dev).eval()


def optimizer_for(model, args, loss_scale="dynamic"):
    """The reference's two weight-decay groups (decay_groups) over model's parameters as an optim.FusedAdam with an fp16 copy of every Linear
    weight. The product computes in fp16 whether or not --fp16 is given, so the loss scale is always on (dynamic unless a number is given)."""
    P = dict(model.named_parameters())
    decay, no_decay = decay_groups(list(P))
    groups = [{"params": [P[n] for n in decay], "weight_decay": float(args.weight_decay)}, {"params": [P[n] for n in no_decay], "weight_decay": 0.0}]
    return optim.FusedAdam(groups, lr=args.learning_rate, eps=args.adam_epsilon, max_grad_norm=args.max_grad_norm, loss_scale=loss_scale,
                           fp16_copies=[P[n] for n in fp16_copy_names(list(P))])


RANK_ROWS = "_rank_rows"  # a batch that holds one rank's rows alone says so here: (lo, hi, B), widths of the full batch (mhop_arena.Feed)


def rank_outputs(model, batch, opt, seed, world):
    """This rank's part of one forward on several ranks: the six matrices of the full batch, differentiable with respect to
    this rank's rows. The rank encodes rows dist.slice_bounds(B, N)[rank] of the full-batch tensors (the widths are the full batch's, so a
    sequence's input does not depend on the rank count) under dist.rank_seed(seed, rank), and dist.gather_with_grad puts every rank's rows
    together. A rank whose slice is empty makes no encoder call, contributes zero rows and still joins the six gathers."""
    from . import dist
    if RANK_ROWS in batch:
        lo, hi, B = batch[RANK_ROWS]
        local = batch
    else:
        B = int(batch["q_input_ids"].shape[0])
        lo, hi = dist.slice_bounds(B, world.size)[world.rank]
        local = {k: v[lo:hi] if torch.is_tensor(v) and v.dim() and v.shape[0] == B else v for k, v in batch.items()}
    bounds = dist.slice_bounds(B, world.size)
    if (lo, hi) != bounds[world.rank]:
        raise ValueError(f"the batch holds rows {lo} .. {hi} of {B}, rank {world.rank} of {world.size} owns {bounds[world.rank]}")
    if hi > lo:
        outputs = model(local, seed=dist.rank_seed(seed, world.rank), half=opt.half)
    else:
        dev = next(model.parameters()).device
        outputs = {name: torch.zeros((0, model.config.hidden_size), dtype=torch.float32, device=dev) for name in ENCODE_INDEX}
    return {name: dist.gather_with_grad(world, outputs[name], bounds) for name in ENCODE_INDEX}, hi > lo


def train_step(model, batch, args, opt, seed, world=None, bucket=None):
    """One forward and backward of the in-batch loss: criterions.mhop_loss over model(batch, seed, opt.half), divided by
    gradient_accumulation_steps, scaled by the optimizer's loss scale for the backward. Returns the unscaled loss (a 0-d device tensor). The
    caller owns opt.step() and scheduler.step(); FusedAdam zeroes the gradients in place, so zero_grad() is never called.

    world (a dist.TorchWorld or a rank of dist.LoopbackWorld) and bucket (the dist.GradBucket behind the parameters' gradients): the step of
    one rank of several. The loss is the full batch's on every rank, the backward fills this rank's share of the gradients, and the caller
    runs bucket.reduce() at the accumulation boundary, immediately before opt.step()."""
    if getattr(args, "momentum", False):
        raise NotImplementedError("--momentum is not built: the reference trains it from a script of its own")
    if world is None:
        loss = criterions.mhop_loss(lambda b: model(b, seed=seed, half=opt.half), batch, args)
        has_rows = True
    else:
        if bucket is None or bucket.world is not world:
            raise ValueError("a step on several ranks needs the dist.GradBucket of this world behind the gradients")
        outputs, has_rows = rank_outputs(model, batch, opt, seed, world)
        loss = criterions.mhop_loss_outputs(outputs, args)
    if args.gradient_accumulation_steps > 1:
        loss = loss / args.gradient_accumulation_steps
    if has_rows:  # a rank without rows has nothing to differentiate: its bucket stays all zero
        opt.scale_loss(loss).backward()
    return loss.detach()
