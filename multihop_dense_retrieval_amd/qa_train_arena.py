"""The reader's training item arena: every item of qa_train_data.QATrainDataset prepared ONCE (the character loop over the chain, WordPiece
word by word, the answer matching and the span search) and kept on the device as flat integer arrays, so that a step's batch is built by
one kernel from that step's item indices (libmdrhip.so: mdr_reader_train_assemble, include/mdr_reader_train.h) instead of re-running
__getitem__ + qa_collate on the host for every row of every batch of every epoch. What qa_arena.QAArena is for inference.

Layout: tokens int32 + token offsets int64 [N + 1] (the encoded row [CLS] q [SEP] wp [SEP], already cut); para_offset int32 [N]; the absolute
sent_offsets and their sent_labels as int32 under sent_index int64 [N + 1]; the (start, end) pairs as int32 [pairs, 2] under span_index
int64 [N + 1], at least one pair per item ((-1, -1) when the item has no span); label and ans_covered int32 [N]. The host keeps its copy:
batch_shape() reads the three widths of a batch from it, so they cost no device synchronisation. Cached as `<train file>.qa_train_arena.npz`
under train_arena_tag(); another tag means a rebuild, never a reuse.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib
from .arena import _to_device
from .qa_arena import qa_arena_tag

_c = ctypes
RULE = "qa-train-arena-v1"  # QADataset(train=True).__getitem__'s fields, one record per item
NET_KEYS = ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets", "sent_labels", "starts", "ends", "label", "ans_covered")
_ARRAYS = (("tokens", np.int32), ("offsets", np.int64), ("para_offset", np.int32), ("sent_pos", np.int32), ("sent_label", np.int32),
           ("sent_index", np.int64), ("spans", np.int32), ("span_index", np.int64), ("label", np.int32), ("ans_covered", np.int32))


class TrainArena(ctypes.Structure):
    _fields_ = [(n, _c.c_void_p) for n in ("tokens_dev", "token_offsets_dev", "para_offset_dev", "sent_pos_dev", "sent_label_dev", "sent_index_dev",
                                           "spans_dev", "span_index_dev", "label_dev", "ans_covered_dev")] + [("n_items", _c.c_int64)]


class TrainBatch(ctypes.Structure):
    _fields_ = [(n, _c.c_void_p) for n in NET_KEYS + ("para_offsets", "lengths")]


# include/mdr_reader_train.h -- bound here, apart from every other header's table
SIGNATURES = {
    "mdr_reader_train_assemble": (_c.c_int, [_c.POINTER(TrainArena), _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                             _c.POINTER(TrainBatch), _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
lib = _lib.binder(SIGNATURES)


def train_arena_tag(tokenizer, max_seq_len, max_q_len, train_file=None):
    """What a cached arena is valid for: the rule, the tokenizer (qa_arena.qa_arena_tag), the two cuts and the train file's size and mtime."""
    st = os.stat(train_file) if train_file is not None else None
    return (f"{RULE}|{qa_arena_tag(tokenizer)}|max_seq_len={int(max_seq_len)}|max_q_len={int(max_q_len)}|"
            f"file={'-' if st is None else f'{st.st_size}:{st.st_mtime_ns}'}")


def _index(counts):
    out = np.zeros(len(counts) + 1, np.int64)
    out[1:] = np.cumsum(np.asarray(counts, np.int64))
    return out


class QATrainArena:
    def __init__(self, tokens, offsets, para_offset, sent_pos, sent_label, sent_index, spans, span_index, label, ans_covered):
        """Host arrays. The three index arrays are checked here, once: the kernel trusts them."""
        given = dict(zip((n for n, _ in _ARRAYS), (tokens, offsets, para_offset, sent_pos, sent_label, sent_index, spans, span_index, label, ans_covered)))
        for name, dt in _ARRAYS:
            setattr(self, name, np.ascontiguousarray(given[name], dtype=dt))
        self.spans = self.spans.reshape(-1, 2)
        self.n = int(self.offsets.shape[0]) - 1
        for idx, arr, what in ((self.offsets, self.tokens, "tokens"), (self.sent_index, self.sent_pos, "sent_pos"), (self.span_index, self.spans, "spans")):
            if idx.shape != (self.n + 1,) or idx[0] != 0 or idx[-1] != len(arr) or (np.diff(idx) < 0).any():
                raise ValueError(f"the index of {what} must be [N + 1], start at 0, not decrease and end at len({what}) = {len(arr)}")
        if len(self.sent_label) != len(self.sent_pos) or any(len(getattr(self, k)) != self.n for k in ("para_offset", "label", "ans_covered")):
            raise ValueError("per-item arrays must hold N entries and sent_label one entry per sent_pos")
        self.lens, self.n_sents, self.n_spans = np.diff(self.offsets), np.diff(self.sent_index), np.diff(self.span_index)
        if self.n and int(self.n_spans.min()) < 1:
            raise ValueError("every item holds at least one (start, end) pair ((-1, -1) for none)")
        self.dev = None

    # -- builders -------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_items(cls, items):
        """items: an iterable of QATrainDataset.__getitem__ results (each read once)."""
        toks, lens, po, spos, slab, ns, spans, nsp, label, cov = [], [], [], [], [], [], [], [], [], []
        for it in items:
            ids = it["encodings"]["input_ids"].view(-1).tolist()
            toks.extend(ids)
            lens.append(len(ids))
            po.append(int(it["para_offset"]))
            so, sl = it["sent_offsets"].view(-1).tolist(), it["sent_labels"].view(-1).tolist()
            assert len(so) == len(sl)
            spos.extend(so)
            slab.extend(sl)
            ns.append(len(so))
            pairs = list(zip(it["starts"].view(-1).tolist(), it["ends"].view(-1).tolist()))
            spans.extend(pairs)
            nsp.append(len(pairs))
            label.append(int(it["label"].view(-1)[0]))
            cov.append(int(it["ans_covered"].view(-1)[0]))
        return cls(np.asarray(toks, np.int32), _index(lens), po, spos, slab, _index(ns), np.asarray(spans, np.int32).reshape(-1, 2), _index(nsp), label, cov)

    @classmethod
    def from_dataset(cls, ds):
        return cls.from_items(ds[i] for i in range(len(ds)))

    def save(self, path, tag=""):
        tmp = path + f".tmp{os.getpid()}.npz"  # written under another name and renamed: a reader never sees a partial file
        np.savez(tmp, tag=np.array(str(tag)), **{n: getattr(self, n) for n, _ in _ARRAYS})
        os.replace(tmp, path)

    @classmethod
    def load(cls, path, expect_tag=None):
        """None when the file carries no tag or another one (the caller rebuilds)."""
        z = dict(np.load(path))
        if expect_tag is not None and ("tag" not in z or str(z["tag"]) != str(expect_tag)):
            return None
        return cls(*(z[n] for n, _ in _ARRAYS))

    @classmethod
    def load_or_build(cls, train_file, ds, tokenizer, log=None):
        """`<train_file>.qa_train_arena.npz` when its tag is this tokenizer's, these cuts' and this file's and it holds len(ds) items; else a
        fresh build (every item's __getitem__, once) written there."""
        cache, tag = train_file + ".qa_train_arena.npz", train_arena_tag(tokenizer, ds.max_seq_len, ds.max_q_len, train_file)
        arena = None
        if os.path.exists(cache):
            try:
                arena = cls.load(cache, expect_tag=tag)
            except (OSError, ValueError, KeyError, EOFError):
                arena = None
            if arena is not None and arena.n != len(ds):
                arena = None
        if arena is None:
            if log is not None:
                log(f"Preparing the training set once for the reader ({len(ds)} items)...")
            arena = cls.from_dataset(ds)
            try:
                arena.save(cache, tag=tag)
            except OSError:
                pass  # a read-only data directory: the arena is rebuilt next time
        return arena

    def to(self, device):
        self.dev = {n: _to_device(getattr(self, n), device, torch.int32 if dt is np.int32 else torch.int64) for n, dt in _ARRAYS}
        return self

    @property
    def bytes_per_item(self):
        return sum(getattr(self, n).nbytes for n, _ in _ARRAYS) / max(1, self.n)

    # -- host geometry --------------------------------------------------------------------------------------------------------------------
    def batch_shape(self, indices):
        """(out_len, n_sent, n_span) of the padded batch qa_collate would build for these items, from host metadata only. An index outside
        [0, N) is an empty row; every width is at least what an empty batch needs (1, 0, 1)."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        ok = (idx >= 0) & (idx < self.n)
        safe = np.where(ok, idx, 0)
        width = lambda a, least: max(least, int(np.where(ok, a[safe], 0).max())) if len(idx) and self.n else least  # noqa: E731
        return width(self.lens, 1), width(self.n_sents, 0), width(self.n_spans, 1)

    def assemble_host(self, indices, out_len=None, n_sent=None, n_span=None, pad_id=0):
        """numpy statement of what mdr_reader_train_assemble writes (the yardstick of the kernel, and qa_train_collate's net_inputs when the
        widths are batch_shape's): int64 arrays under NET_KEYS plus para_offsets and lengths [R]."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        shape = self.batch_shape(idx)
        L, S, P = (shape[0] if out_len is None else out_len), (shape[1] if n_sent is None else n_sent), (shape[2] if n_span is None else n_span)
        R = len(idx)
        out = {k: np.zeros((R, L), np.int64) for k in NET_KEYS[:4]}
        out["input_ids"][:] = pad_id
        out["sent_offsets"], out["sent_labels"] = np.zeros((R, S), np.int64), np.zeros((R, S), np.int64)
        out["starts"], out["ends"] = np.full((R, P), -1, np.int64), np.full((R, P), -1, np.int64)
        out["label"], out["ans_covered"] = np.full((R, 1), -1, np.int64), np.zeros((R, 1), np.int64)
        out["para_offsets"], out["lengths"] = np.zeros(R, np.int64), np.zeros(R, np.int64)
        for r, i in enumerate(idx):
            if not 0 <= i < self.n:
                continue
            row = self.tokens[self.offsets[i]:self.offsets[i + 1]]
            n, po = len(row), int(self.para_offset[i])
            m = min(n, L)
            out["input_ids"][r, :m] = row[:m]
            out["attention_mask"][r, :m] = 1
            out["token_type_ids"][r, min(po, m):m] = 1
            out["paragraph_mask"][r, min(po, L):max(min(po, L), min(n - 1, L))] = 1
            k = min(int(self.n_sents[i]), S)
            out["sent_offsets"][r, :k] = self.sent_pos[self.sent_index[i]:self.sent_index[i] + k]
            out["sent_labels"][r, :k] = self.sent_label[self.sent_index[i]:self.sent_index[i] + k]
            k = min(int(self.n_spans[i]), P)
            pairs = self.spans[self.span_index[i]:self.span_index[i] + k]
            out["starts"][r, :k], out["ends"][r, :k] = pairs[:, 0], pairs[:, 1]
            out["label"][r, 0], out["ans_covered"][r, 0] = self.label[i], self.ans_covered[i]
            out["para_offsets"][r], out["lengths"][r] = po, n
        return out

    # -- the device op --------------------------------------------------------------------------------------------------------------------
    def assemble(self, indices_dev, out_len, n_sent, n_span, pad_id=0, out=None):
        """indices_dev int64 cuda [R] -> dict of int64 cuda tensors under NET_KEYS plus para_offsets and lengths [R]. `out`: a dict of
        preallocated contiguous tensors of exactly those shapes to write into (the tests' guarded buffers)."""
        if self.dev is None:
            raise RuntimeError("QATrainArena.to(device) first")
        dev = self.dev["offsets"].device
        if not (torch.is_tensor(indices_dev) and indices_dev.device == dev and indices_dev.dtype == torch.int64 and indices_dev.dim() == 1):
            raise ValueError("indices must be a 1-D int64 tensor on the arena's device")
        out_len, n_sent, n_span = int(out_len), int(n_sent), int(n_span)
        if out_len < 1 or n_sent < 0 or n_span < 1:
            raise ValueError(f"out_len = {out_len} (>= 1), n_sent = {n_sent} (>= 0), n_span = {n_span} (>= 1)")
        idx = indices_dev.contiguous()
        R = int(idx.shape[0])
        shapes = {**{k: (R, out_len) for k in NET_KEYS[:4]}, "sent_offsets": (R, n_sent), "sent_labels": (R, n_sent), "starts": (R, n_span),
                  "ends": (R, n_span), "label": (R, 1), "ans_covered": (R, 1), "para_offsets": (R,), "lengths": (R,)}
        if out is None:
            out = {k: torch.empty(s, dtype=torch.int64, device=dev) for k, s in shapes.items()}
        else:
            for k, s in shapes.items():
                if not _lib.is_like(out[k], (torch.int64,), s, dev):
                    raise ValueError(f"out[{k!r}] is {_lib.describe(out[k])}, not a contiguous int64 {s} on {dev}")
        d, vp = self.dev, _lib.ptr
        a = TrainArena(*(vp(d[n]) for n, _ in _ARRAYS), self.n)
        o = TrainBatch(*(vp(out[k]) if out[k].numel() else None for k in NET_KEYS + ("para_offsets", "lengths")))
        if R:
            _lib.call(lib().mdr_reader_train_assemble, ctypes.byref(a), vp(idx), R, out_len, n_sent, n_span, int(pad_id), ctypes.byref(o), dev=dev)
        return out
