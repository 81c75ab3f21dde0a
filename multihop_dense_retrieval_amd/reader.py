"""The HotpotQA answer reader (mdr/qa/qa_model.py QAModel at inference) on libmdrhip.so (include/mdr_reader.h).

    model = QAModel(config, args)            # config: an ElectraConfig / BertConfig (or any object with the same fields)
    load_saved(model, args.init_checkpoint, exact=False)
    model.to("cuda")
    outputs = model(batch)                   # {'start_logits', 'end_logits', 'rank_score', 'sp_score'} as the reference returns them
                                             # (attention_mask right-padded, as qa_collate builds it; other masks raise ValueError)
    best = model.decode(batch, max_ans_len)  # + the band-limited span argmax and predict()'s masked sp sigmoid, fused on the device

The whole forward -- the ELECTRA / BERT encoder over every token, the heads and the span search -- is HIP for gfx950. There is
no CPU path: a missing library or a non-HIP device is an error. Numerics are apex O1's (the README's `--fp16` QA runs): the
outputs are fp16 tensors, as the reference's are under O1.

Model families. ELECTRA (base / large, embedding size == hidden; the pooler is QAModel's own `pooler.dense.*`) and BERT-family
checkpoints (pooler at `encoder.pooler.dense.*`) run. ELECTRA-small (`embeddings_project`), RoBERTa (position ids offset by
the padding index, no token types) and SpanBERT are refused by name.
"""
import ctypes

import torch

from . import _lib
from .retriever import _HipModule, load_saved, move_to_cuda, trunk_state_dict_shapes  # noqa: F401  (load_saved, move_to_cuda: the reference's utils)

_c = ctypes

POOLER_HEAD, POOLER_ENCODER = 0, 1


class ReaderConfig(ctypes.Structure):
    _fields_ = [("vocab", _c.c_int), ("hidden", _c.c_int), ("layers", _c.c_int), ("heads", _c.c_int), ("ffn", _c.c_int), ("max_pos", _c.c_int),
                ("type_vocab", _c.c_int), ("ln_eps", _c.c_float), ("residual_fp32", _c.c_int), ("has_sp", _c.c_int), ("pooler", _c.c_int)]


class ReaderOutputs(ctypes.Structure):
    _fields_ = [("start_logits", _c.c_void_p), ("end_logits", _c.c_void_p), ("rank_score", _c.c_void_p), ("sp_score", _c.c_void_p),
                ("sp_prob", _c.c_void_p), ("span_start", _c.c_void_p), ("span_end", _c.c_void_p), ("span_score", _c.c_void_p)]


class ReaderArena(ctypes.Structure):
    _fields_ = [("tokens_dev", _c.c_void_p), ("token_offsets_dev", _c.c_void_p), ("sent_starts_dev", _c.c_void_p), ("sent_offsets_dev", _c.c_void_p),
                ("n_passages", _c.c_int64)]


class ReaderBatch(ctypes.Structure):
    _fields_ = [("input_ids", _c.c_void_p), ("attention_mask", _c.c_void_p), ("token_type_ids", _c.c_void_p), ("paragraph_mask", _c.c_void_p),
                ("sent_offsets", _c.c_void_p), ("para_offsets", _c.c_void_p), ("lengths", _c.c_void_p)]


# include/mdr_reader.h -- bound here, apart from _lib._SIGNATURES (which is include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_reader_create": (_c.c_int, [_c.POINTER(ReaderConfig), _c.POINTER(_lib.Tensor), _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                     _c.POINTER(_c.c_void_p)]),
    "mdr_reader_free": (_c.c_int, [_c.c_void_p]),
    "mdr_reader_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int]),
    "mdr_reader_forward": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                      _c.c_int, _c.POINTER(ReaderOutputs), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "mdr_reader_span_search": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                          _c.c_void_p]),
    "mdr_reader_assemble": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                       _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
MAX_SEQ_LEN = 512  # the span kernel keeps one row of start / end logits in LDS

lib = _lib.binder(SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_reader.h bound
_ptr = _lib.ptr


def model_family(model_name, config):
    """'electra' or 'bert' (what the reference's `"electra" in args.model_name` branch decides); anything the kernels do not
    compute raises with the reason."""
    name = (model_name or "").lower()
    if "roberta" in name:
        raise NotImplementedError(f"{model_name}: RoBERTa readers are not supported (position ids offset by the padding index, no token types)")
    if "spanbert" in name:
        raise NotImplementedError(f"{model_name}: SpanBERT readers are not supported")
    emb = getattr(config, "embedding_size", None)
    if emb is not None and emb != config.hidden_size:
        raise NotImplementedError(f"{model_name}: embeddings_project (embedding_size {emb} != hidden_size {config.hidden_size}, "
                                  "ELECTRA-small) is not supported")
    act = getattr(config, "hidden_act", "gelu")
    if act != "gelu":
        raise NotImplementedError(f"{model_name}: hidden_act {act!r} is not supported (the FFN epilogue is the exact erf GELU)")
    return "electra" if "electra" in name else "bert"


def expected_state_dict_shapes(config, family, sp_pred):
    """QAModel.state_dict() of the reference (the encoder's buffers aside): encoder.embeddings.*, encoder.encoder.layer.{i}.*, the
    pooler (QAModel's for ELECTRA, the encoder's for BERT), qa_outputs.*, rank.*, sp.* with --sp-pred."""
    H = config.hidden_size
    s = trunk_state_dict_shapes(config, config.type_vocab_size)
    pool = "pooler.dense." if family == "electra" else "encoder.pooler.dense."
    s.update({pool + "weight": (H, H), pool + "bias": (H,), "qa_outputs.weight": (2, H), "qa_outputs.bias": (2,),
              "rank.weight": (1, H), "rank.bias": (1,)})
    if sp_pred:
        s.update({"sp.weight": (1, H), "sp.bias": (1,)})
    return s


class QAModel(_HipModule):
    """qa_model.py:27-109 at inference. `args` needs model_name and sp_pred (sp_weight is a training knob and is not read)."""

    _KIND = "reader"
    RESIDUAL_FP32_DEFAULT = 2  # mdr_reader_config.residual_fp32: the apex-O1 dataflow around the LayerNorms (as the retrieval encoder)

    def __init__(self, config, args):
        super().__init__()
        self.config = config
        self.model_name = args.model_name
        self.sp_pred = bool(getattr(args, "sp_pred", False))
        self.family = model_family(self.model_name, config)
        self._shapes = expected_state_dict_shapes(config, self.family, self.sp_pred)
        self.residual_fp32 = self.RESIDUAL_FP32_DEFAULT
        self._ws = None

    def load_state_dict(self, state_dict, strict=True):
        missing = [k for k in self._shapes if k not in state_dict]
        unexpected = [k for k in state_dict if k not in self._shapes]
        if missing or (strict and unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: Missing key(s): {missing}. Unexpected key(s): {unexpected}.")
        for k, shp in self._shapes.items():
            if tuple(state_dict[k].shape) != tuple(shp):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(state_dict[k].shape)} vs model {tuple(shp)}")
        self._pending = {k: state_dict[k] for k in self._shapes}
        if self.device is not None:
            self._create()
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("training is not supported: the reader runs inference only")
        return self.eval()

    # -- forward ---------------------------------------------------------------------------------------------
    def _run(self, batch, max_ans_len=None, want_logits=True):
        if not self._h.value:
            raise RuntimeError("QAModel has no weights on a device: load_state_dict(...) and .to('cuda') first")
        dev = self.device
        ids = batch["input_ids"].to(dev, torch.int64).contiguous()
        B, L = ids.shape
        if L > MAX_SEQ_LEN:
            raise ValueError(f"sequence length {L} > {MAX_SEQ_LEN}")
        mask = batch["attention_mask"].to(dev, torch.int64).contiguous()
        if B and L > 1 and bool((mask[:, 1:] > mask[:, :-1]).any()):  # the heads address position p of row b as packed token cu[b] + p
            raise ValueError("attention_mask must be right-padded (a prefix of ones in every row), as qa_collate builds it")
        tt = batch.get("token_type_ids", None)
        tt = None if tt is None else tt.to(dev, torch.int64).contiguous()
        pm = batch["paragraph_mask"].to(dev, torch.int64).contiguous()
        so = batch.get("sent_offsets", None) if self.sp_pred else None
        so = None if so is None else so.to(dev, torch.int64).contiguous()
        NS = 0 if so is None else so.shape[1]
        f16 = dict(dtype=torch.float16, device=dev)
        out = {"start_logits": torch.empty((B, L), **f16) if want_logits else None,
               "end_logits": torch.empty((B, L), **f16) if want_logits else None,
               "rank_score": torch.empty((B, 1), **f16),
               "sp_score": torch.empty((B, NS), **f16) if (self.sp_pred and so is not None) else None}
        spans = None
        if max_ans_len is not None:
            spans = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, **f16))
            out["sp_prob"] = torch.empty((B, NS), **f16) if out["sp_score"] is not None else None
        o = ReaderOutputs(_ptr(out["start_logits"]), _ptr(out["end_logits"]), _ptr(out["rank_score"]), _ptr(out["sp_score"]),
                          _ptr(out.get("sp_prob")), *([_ptr(t) for t in spans] if spans else [None, None, None]))
        L_ = lib()
        need = int(L_.mdr_reader_workspace_bytes(self._h, B, L, NS))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _lib.call(L_.mdr_reader_forward, self._h, _ptr(ids), _ptr(mask), _ptr(tt), _ptr(pm), _ptr(so), B, L, NS, -1 if max_ans_len is None else int(max_ans_len),
                  ctypes.byref(o), _ptr(self._ws), self._ws.numel(), dev=dev, device_arg=False)
        return out, spans

    def __call__(self, batch):
        """QAModel.forward(batch) in eval mode: {'start_logits' [B, L], 'end_logits' [B, L], 'rank_score' [B, 1], 'sp_score' [B, S] or
        None}, fp16 on the device, start / end already -inf outside paragraph_mask."""
        if self.training:
            raise NotImplementedError("training is not supported: the reader runs inference only")
        out, _ = self._run(batch)
        return out

    forward = __call__

    def decode(self, batch, max_ans_len, with_logits=False):
        """The forward plus predict()'s device-side work (scripts/train_qa.py:233-253), fused: {'start' [B], 'end' [B] (positions in the
        padded row, before the para_offsets shift), 'span_score' [B] (fp16), 'rank_score' [B, 1], 'sp_prob' [B, S] or None (sigmoid with
        sent_offsets == 0 masked)}; with_logits also returns the raw start / end logits and sp_score."""
        out, (s, e, sc) = self._run(batch, max_ans_len=max_ans_len, want_logits=with_logits)
        res = {"start": s, "end": e, "span_score": sc, "rank_score": out["rank_score"], "sp_prob": out.get("sp_prob")}
        if with_logits:
            res.update({k: out[k] for k in ("start_logits", "end_logits", "sp_score")})
        return res

    # -- internals -------------------------------------------------------------------------------------------
    def _create(self):
        sd = self._pending
        c = self.config
        cfg = ReaderConfig(c.vocab_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size, c.max_position_embeddings,
                           c.type_vocab_size, float(getattr(c, "layer_norm_eps", 1e-12)), int(self.residual_fp32), int(self.sp_pred),
                           POOLER_HEAD if self.family == "electra" else POOLER_ENCODER)
        names = list(sd)
        arr, keep, on_dev = _lib.tensor_table(sd, names)
        self._free()
        with torch.cuda.device(self.device):
            _lib.check(lib().mdr_reader_create(ctypes.byref(cfg), arr, len(names), int(on_dev), self.device.index, _lib.current_stream_ptr(self.device),
                                               ctypes.byref(self._h)))
        self._pending = None

    def _release(self, h):
        lib().mdr_reader_free(h)


def span_search(start_logits, end_logits, max_ans_len):
    """The device span search alone on fp16 logits [B, L] (cuda): (start [B], end [B], span_score [B] fp16) -- the kernel decode() runs."""
    if start_logits.dtype != torch.float16 or end_logits.dtype != torch.float16 or start_logits.shape != end_logits.shape:
        raise ValueError("span_search takes two fp16 [B, L] tensors of one shape")
    s16, e16 = start_logits.contiguous(), end_logits.contiguous()
    B, L = s16.shape
    dev = s16.device
    out = (torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.float16, device=dev))
    _lib.call(lib().mdr_reader_span_search, _ptr(s16), _ptr(e16), B, L, int(max_ans_len), *[_ptr(t) for t in out], dev=dev)
    return out


def span_search_reference(start_logits, end_logits, max_ans_len):
    """predict()'s formulation (scripts/train_qa.py:242-253), restated in torch on any device: the [B, L, L] matrix start[:, :, None] +
    end[:, None] in the logits' dtype, the band mask np.tril(np.triu(ones, 0), max_ans_len), the -1e10 fill through float() and back
    with type_as (-inf in fp16), then max over the end and max over the start (first index wins). Returns (start, end, score)."""
    span = start_logits[:, :, None] + end_logits[:, None]
    L = span.size(1)
    band = torch.ones((L, L), dtype=torch.bool, device=span.device).triu(0).tril(max_ans_len)
    masked = span.float().masked_fill(~band[None].expand_as(span), -1e10).type_as(span)
    row_max, row_arg = masked.max(dim=2)
    score, start = row_max.max(dim=1)
    end = row_arg.gather(1, start.unsqueeze(1)).squeeze(1)
    return start, end, score
