"""Momentum training of the retriever: the second stage of the reference's recipe (scripts/train_momentum.py, "finetune the question
encoder with frozen memory bank"; RobertaMomentumRetriever, mdr/retrieval/models/mhop_retriever.py:45-129) on one rank:

    model = MomentumRetriever(config, args).cuda()       # args.k, args.init_retriever
    opt = optimizer_for(model, args)
    loss = train_step(model, batch, args, opt, seed);  opt.step();  scheduler.step()

encoder_q is a train.TrainableRetriever and the only thing that is trained. encoder_k is a retriever.RobertaRetriever INFERENCE handle, loaded
once from encoder_q's masters when the model goes to its device (after --init-retriever has been applied: the reference's
param_k.copy_(param_q)): one fp16 weight copy in the library, no masters, no moments, no gradients, never in an optimizer. The queue is a
criterions.MemoryBank of args.k rows, drawn with torch.randn from the global generator after encoder_q's initialisers. The reference's bits
for it cannot be reproduced: Hugging Face's initialisers of its two encoders draw an unknown amount from the generator before it.

The momentum update itself (momentum_update_key_encoder, param_k = m param_k + (1 - m) param_q) is NOT built, because the reference never
calls it: the call is commented out in its criterions.py:144 and its run is named freeze_k. --m is accepted and appears in the run
directory's name only, as there.

In train() mode the reference evaluates encoder_k under torch.no_grad() but with its dropout live. That forward keeps nothing for a
backward, so it is mdr_encoder_forward_dropout (include/mdr_encoder_dropout.h, bound here): the inference encoder's launch sequence with
the hidden-state dropout folded into the LayerNorm and embedding kernels that read those rows anyway and the attention dropout served by
the training attention forward. Its bits are those of TrainableRetriever.encode(..., dropout=(seed, encode)) on the same weights; it
makes no separate mask pass, no memset and no concatenation of the QKV leaves. A batch is ONE call: the hidden mask's row is the packed row
and the attention mask depends on the sequence's index in the call, so a batch above MAX_TOKENS_PER_CALL tokens is refused, not sliced, and
the call never goes through the graph cache (the seed changes every step).

Everything runs on one HIP device and is enqueued on the current stream; there is no CPU fallback.
"""
import ctypes
import functools

import torch

from . import _lib, criterions, dropout as _dropout, retriever, train as _train
from ._lib import check_hidden, check_rows, describe, is_like, ptr

_c = ctypes
# include/mdr_encoder_dropout.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_encoder_forward_dropout": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_uint64, _c.c_int,
                                               _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "mdr_test_layernorm_dropout": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_float, _c.c_int,
                                              _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "mdr_test_embed_ln_dropout": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                             _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_float, _c.c_int, _c.c_uint64, _c.c_uint32,
                                             _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_encoder_dropout.h bound

K_INPUTS = (("c1", "c1"), ("c2", "c2"), ("neg_1", "neg1"), ("neg_2", "neg2"))  # output name -> batch key prefix: the key encoder's four
Q_INPUTS = (("q", "q"), ("q_sp1", "q_sp"))                                    # and the question encoder's two


def _check_T(T):
    T = int(T)
    if not 0 <= T <= 255:
        raise ValueError(f"T = {T}: a dropout threshold lies in 0 .. 255")
    return T


def layer_norm_dropout(x16, res32, weight, bias, eps, T, seed, site, rows=None, out16=None, out32=None):
    """mdr_test_layernorm_dropout on device tensors: (y16, y32) = LayerNorm(fp32(fp16(fp32(x16) * m)) + res32), the fused form of
    dropout.packed_dropout followed by layernorm.packed_layer_norm(keep32=True). x16 fp16 [M, H], res32 None or fp32 [M, H], weight and bias
    fp32 [H]; rows None or the int32 device scalar of valid rows: rows at or behind it are NOT written (out16 / out32, when given, keep what
    they held there; fresh outputs start zeroed). Enqueued on the current stream."""
    if not (torch.is_tensor(x16) and x16.is_cuda):
        raise RuntimeError("the fused LayerNorm runs on a HIP device only (there is no CPU fallback)")
    if x16.dtype != torch.float16 or x16.dim() != 2 or not x16.is_contiguous() or x16.shape[0] < 1:
        raise ValueError(f"x16 must be a contiguous fp16 [M >= 1, H] tensor, got {describe(x16)}")
    M, H = int(x16.shape[0]), int(x16.shape[1])
    dev = x16.device
    check_hidden(H)
    if res32 is not None and not is_like(res32, (torch.float32,), (M, H), dev):
        raise ValueError(f"res32 must be None or a contiguous fp32 [{M}, {H}] tensor on x16's device, got {describe(res32)}")
    for name, t in (("weight", weight), ("bias", bias)):
        if not is_like(t, (torch.float32,), (H,), dev):
            raise ValueError(f"{name} must be a contiguous fp32 [{H}] tensor on x16's device, got {describe(t)}")
    if rows is not None:
        check_rows(rows, dev)
    seed, site = _dropout.check_seed_site(seed, site)
    out16 = torch.zeros((M, H), dtype=torch.float16, device=dev) if out16 is None else out16
    out32 = torch.zeros((M, H), dtype=torch.float32, device=dev) if out32 is None else out32
    if not (is_like(out16, (torch.float16,), (M, H), dev) and is_like(out32, (torch.float32,), (M, H), dev)):
        raise ValueError(f"out16 / out32 must be contiguous fp16 / fp32 [{M}, {H}] tensors on x16's device")
    _lib.call(lib().mdr_test_layernorm_dropout, ptr(x16), ptr(res32), M, ptr(rows), H, ptr(weight), ptr(bias), float(eps), _check_T(T), seed, site,
              ptr(out16), ptr(out32), dev=dev)
    return out16, out32


def embedding_layer_norm_dropout(ids, tok_src, tok_pid, total, word, pos, type0, weight, bias, eps, cap, T, seed, site, out16=None, out32=None):
    """mdr_test_embed_ln_dropout on device tensors: (y16, y32) with y32 = LN(word + position + type) * m and y16 = fp16(y32), the fused form of
    embedding.packed_embedding_layer_norm followed by dropout.packed_dropout(also16=True). ids int64 [B, L]; tok_src, tok_pid int32 [cap] and
    total int32 [1] as mdr_test_pack wrote them; word [vocab, H], pos [max_pos, H], type0 [H], weight, bias [H] fp32. Rows at or behind total
    are NOT written. Enqueued on the current stream."""
    if not (torch.is_tensor(word) and word.is_cuda):
        raise RuntimeError("the fused embedding runs on a HIP device only (there is no CPU fallback)")
    dev = word.device
    H = int(word.shape[1])
    check_hidden(H)
    cap = int(cap)
    if not (is_like(ids, (torch.int64,), ids.shape, dev) and is_like(tok_src, (torch.int32,), (cap,), dev) and is_like(tok_pid, (torch.int32,), (cap,), dev)):
        raise ValueError(f"ids must be int64 and tok_src / tok_pid contiguous int32 [{cap}] tensors on the tables' device")
    if ids.numel() < cap or cap < 1:
        raise ValueError(f"cap = {cap} must lie in 1 .. ids.numel() = {ids.numel()}")
    check_rows(total, dev, "total", "the tables")
    for name, t, shape in (("pos", pos, (pos.shape[0], H)), ("type0", type0, (H,)), ("weight", weight, (H,)), ("bias", bias, (H,)), ("word", word, word.shape)):
        if not is_like(t, (torch.float32,), shape, dev):
            raise ValueError(f"{name} must be a contiguous fp32 {tuple(shape)} tensor on the tables' device, got {describe(t)}")
    seed, site = _dropout.check_seed_site(seed, site)
    out16 = torch.zeros((cap, H), dtype=torch.float16, device=dev) if out16 is None else out16
    out32 = torch.zeros((cap, H), dtype=torch.float32, device=dev) if out32 is None else out32
    if not (is_like(out16, (torch.float16,), (cap, H), dev) and is_like(out32, (torch.float32,), (cap, H), dev)):
        raise ValueError(f"out16 / out32 must be contiguous fp16 / fp32 [{cap}, {H}] tensors on the tables' device")
    _lib.call(lib().mdr_test_embed_ln_dropout, ptr(ids), ptr(tok_src), ptr(tok_pid), ptr(total), cap, ptr(word), ptr(pos), ptr(type0), ptr(weight),
              ptr(bias), H, int(word.shape[0]), int(pos.shape[0]), float(eps), _check_T(T), seed, site, ptr(out16), ptr(out32), dev=dev)
    return out16, out32


def encode_dropout(encoder, input_ids, mask, T_hidden, T_attention, seed, encode, lane=0):
    """mdr_encoder_forward_dropout on an inference handle (retriever.RobertaRetriever with weights on a device): [B, hidden] fp32, the
    training-mode forward of encode number `encode` (train.ENCODE_INDEX) under `seed`, with the two thresholds (dropout.threshold of the two
    rates; 0 makes a kind's places plain, both 0 is encode_seq's result bit for bit). One call over the whole batch, eager, on `lane`'s
    workspace; never sliced and never captured (module docstring)."""
    if not encoder._h.value:
        raise RuntimeError("encoder has no weights on a device: call load_state_dict(...) and .to('cuda') first")
    if int(encoder.residual_fp32) != 2:
        raise NotImplementedError(f"the training-mode forward is built for the trunk's default numerics mode only (residual_fp32 = 2), not for "
                                  f"{encoder.residual_fp32}")
    dev = encoder.device
    ids = input_ids.to(device=dev, dtype=torch.int64).contiguous()
    msk = mask.to(device=dev, dtype=torch.int64).contiguous()
    if ids.dim() != 2 or ids.shape != msk.shape or ids.shape[0] < 1:
        raise ValueError(f"input_ids {tuple(ids.shape)} and mask {tuple(msk.shape)} must both be [B >= 1, L]")
    B, L = int(ids.shape[0]), int(ids.shape[1])
    if B * L > encoder.MAX_TOKENS_PER_CALL or L > 512:
        raise ValueError(f"a training-mode forward is one call: {B} x {L} tokens exceed MAX_TOKENS_PER_CALL = {encoder.MAX_TOKENS_PER_CALL} (or L > 512), "
                         "and a batch cannot be sliced because the dropout mask depends on a row's place in the call")
    if not 0 <= int(encode) < _dropout.ENCODES:
        raise ValueError(f"encode = {encode}: must lie in 0 .. {_dropout.ENCODES - 1}")
    seed, _ = _dropout.check_seed_site(seed, 0)
    T_hidden, T_attention = _check_T(T_hidden), _check_T(T_attention)
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("a training-mode forward is never captured: its seed changes every step")
    st = encoder._lane(lane)
    need = int(_lib.lib().mdr_encoder_workspace_bytes(encoder._h, B, L))
    if st.ws is None or st.ws.numel() < need:
        st.ws = torch.empty(need, dtype=torch.uint8, device=dev)  # (captures of this lane notice the move and are dropped: encode_seq)
    out = torch.empty((B, encoder.config.hidden_size), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib().mdr_encoder_forward_dropout(encoder._h, ptr(ids), ptr(msk), B, L, T_hidden, T_attention, seed, int(encode), ptr(out), ptr(st.ws),
                                                     st.ws.numel(), _lib.current_stream_ptr(dev)))
    return out


class MomentumRetriever(torch.nn.Module):
    """RobertaMomentumRetriever on one rank (module docstring). Parameters: encoder_q's, under the reference's `encoder_q.` prefix."""

    def __init__(self, config, args):
        super().__init__()
        self.config, self.args = config, args
        self.encoder_q = _train.TrainableRetriever(config, args)
        self.encoder_k = None  # built from encoder_q's masters when the model reaches its device
        self._q_eval = None    # encoder_q.inference() of the current eval() stretch
        if getattr(args, "init_retriever", "") != "":
            print(f"Load pretrained retriever from {args.init_retriever}")
            self.load_retriever(args.init_retriever)
        self.k, self.m = int(args.k), float(getattr(args, "m", 0.999))
        self.bank = criterions.MemoryBank(self.k, config.hidden_size)

    def load_retriever(self, path):
        """mhop_retriever.py:70-75: strip `module.`, keep the keys encoder_q knows, load strictly (a missing key raises)."""
        known = self.encoder_q.state_dict()
        strip = lambda k: k[7:] if k.startswith("module.") else k  # noqa: E731
        sd = {strip(k): v for k, v in torch.load(path, map_location="cpu").items() if strip(k) in known}
        self.encoder_q.load_state_dict(sd)

    queue = property(lambda self: self.bank.queue)
    queue_ptr = property(lambda self: self.bank.queue_ptr)

    def dequeue_and_enqueue(self, embeddings):
        self.bank.dequeue_and_enqueue(embeddings)

    def copy_key_encoder(self):
        """param_k.copy_(param_q): encoder_k as an inference handle of encoder_q's current masters. Called once, when the model reaches its
        device; nothing steps or refreshes the key encoder afterwards (freeze_k)."""
        self.encoder_k = self.encoder_q.inference()
        return self.encoder_k

    def _apply(self, fn, *a, **kw):
        super()._apply(fn, *a, **kw)
        self.bank.queue = fn(self.bank.queue)  # (queue_ptr stays on the host, where dequeue_and_enqueue reads it)
        if self.bank.queue.is_cuda and self.encoder_k is None:
            self.copy_key_encoder()
        return self

    def train(self, mode=True):
        self._q_eval = None
        return super().train(mode)

    def thresholds(self):
        return _dropout.threshold(self.encoder_q.hidden_dropout_prob), _dropout.threshold(self.encoder_q.attention_probs_dropout_prob)

    def forward(self, batch, seed=None, half=None):
        """The six [B, hidden] fp32 matrices of one mhop_collate batch. train(): q and q_sp1 from encoder_q.encode with dropout (seed,
        ENCODE_INDEX) and gradients, c1, c2, neg_1, neg_2 from the key encoder's training-mode forward under the same seed, their ENCODE_INDEX
        and encoder_q's two thresholds, without gradients. eval(): the question side from encoder_q.inference(), the passage side from
        encoder_k.encode_seq: what the reference's predict sees."""
        if self.encoder_k is None:
            raise RuntimeError("the momentum retriever runs on a HIP device only: move it there first (.cuda())")
        ids = lambda key: (batch[f"{key}_input_ids"], batch[f"{key}_mask"])  # noqa: E731
        out = {}
        if not self.training:
            if self._q_eval is None:
                self._q_eval = self.encoder_q.inference()
            for name, key in Q_INPUTS:
                out[name] = self._q_eval.encode_seq(*ids(key))
            for name, key in K_INPUTS:
                out[name] = self.encoder_k.encode_seq(*ids(key))
            return out
        T_hid, T_att = self.thresholds()
        live = bool(T_hid or T_att)
        if live and seed is None:
            raise ValueError("a training forward with dropout needs the caller's seed")
        seed = int(seed) if live else 0
        for name, key in Q_INPUTS:
            out[name] = self.encoder_q.encode(*ids(key), half, (seed, _train.ENCODE_INDEX[name]) if live else None)
        with torch.no_grad():
            for name, key in K_INPUTS:
                out[name] = encode_dropout(self.encoder_k, *ids(key), T_hid, T_att, seed, _train.ENCODE_INDEX[name])
        return out


def optimizer_for(model, args, loss_scale="dynamic"):
    """train.optimizer_for over encoder_q: the reference builds its two groups over model.named_parameters(), whose `encoder_q.` prefix changes
    no substring match of decay_groups, and encoder_k's parameters do not require a gradient there; here encoder_k has none at all."""
    return _train.optimizer_for(model.encoder_q, args, loss_scale)


def train_step(model, batch, args, opt, seed):
    """train.train_step's body over criterions.mhop_loss with args.momentum: the loss is scored against the queue as it stands, then the
    step's [c1; c2] is enqueued. Returns the unscaled loss (a 0-d device tensor); the caller owns opt.step() and scheduler.step()."""
    if not getattr(args, "momentum", False):
        raise ValueError("momentum.train_step is the --momentum step; without it the step is train.train_step")
    step = functools.partial(model, seed=seed, half=opt.half)
    step.module = model  # where mhop_loss looks for queue and dequeue_and_enqueue, as on the reference's DataParallel wrapper
    loss = criterions.mhop_loss(step, batch, args)
    if args.gradient_accumulation_steps > 1:
        loss = loss / args.gradient_accumulation_steps
    opt.scale_loss(loss).backward()
    return loss.detach()
