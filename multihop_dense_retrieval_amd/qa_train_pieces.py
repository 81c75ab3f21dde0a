"""The reader's training PIECE arena: what qa_train_arena.QATrainArena stores as one finished row per item, stored as the pieces the rows
are made of -- one row per question, one per DISTINCT passage text -- and spliced into a step's batch on the device by one kernel
(libmdrhip.so: mdr_reader_train_compose, include/mdr_reader_train_pieces.h), byte for byte what mdr_reader_train_assemble gathers for the
same item indices.

Why. QATrainDataset keeps every candidate chain of every question as an item (the README's train file: up to 100 chains for each of
about 90 k questions). The item arena runs __getitem__ on each: prepare()'s character loop, WordPiece word by word, the answer matching.
But the chains of a question share the question and most passages, and a chain's WordPieces are `yes no [SEP] P1 [SEP] P2` with each Pi
a function of passage i alone (qa_arena.py proves it, mdr_reader_assemble uses it for inference). So here a question is tokenised once, a
passage once (qa_arena.passage_ids, through qa_arena.QAArena.from_corpus and its worker pool), and an item is five integers. Only the
items with ans_covered = 1 and an answer that is neither "yes" nor "no" still go through prepare() + qa_train_data.answer_spans, the
existing host functions, unchanged: match_answer_span collects surface strings over the WHOLE chain string, so a per-passage form would
need an exactness argument of its own. Their spans are stored uncut; the kernel does cut_spans.

Layout: q_tokens int32 + q_offsets int64 [Q + 1]; p_tokens int32 + p_offsets int64 [P + 1], p_sent_starts int32 + p_sent_offsets int64
[P + 1] (QAArena's layout); items int32 [N, 5] = question row, P1 row, P2 row, label, ans_covered; sent_label int32 under sent_label_index
int64 [N + 1] (entries only where the record carries non-empty sp_sent_labels: one per sentence of the chain); spans int32 [pairs, 2] under
span_index int64 [N + 1], uncut (first, last) in chain WordPiece positions, 0 = `yes`; special int32 [4] = cls, sep, yes, no; cuts int32
[2] = max_seq_len, max_q_len. Only chains of exactly two passages, as in mdr_reader_assemble. The host keeps its copy: batch_shape() reads
the three widths of a batch from it, so they cost no device synchronisation. Cached as `<train file>.qa_train_pieces.npz` under
train_pieces_tag(); another tag means a rebuild, never a reuse.
"""
import ctypes
import multiprocessing
import os

import numpy as np
import torch

from . import _lib, qa_arena, qa_data
from .arena import _to_device
from .qa_train_arena import NET_KEYS, TrainBatch, _index, train_arena_tag

_c = ctypes
RULE = "qa-train-pieces-v1"  # question rows, distinct qa_arena.passage_text rows, five integers per item, uncut answer_spans
MAX_WORKERS = qa_arena.MAX_WORKERS
_ARRAYS = (("q_tokens", np.int32), ("q_offsets", np.int64), ("p_tokens", np.int32), ("p_offsets", np.int64), ("p_sent_starts", np.int32),
           ("p_sent_offsets", np.int64), ("items", np.int32), ("sent_label", np.int32), ("sent_label_index", np.int64), ("spans", np.int32),
           ("span_index", np.int64), ("special", np.int32), ("cuts", np.int32))
_DEVICE_ARRAYS = _ARRAYS[:11]


class TrainPieces(ctypes.Structure):
    _fields_ = [(n + "_dev", _c.c_void_p) for n, _ in _DEVICE_ARRAYS] + [(n, _c.c_int64) for n in ("n_items", "n_questions", "n_passages", "max_q_len")]


# include/mdr_reader_train_pieces.h -- bound here, apart from every other header's table
SIGNATURES = {
    "mdr_reader_train_compose": (_c.c_int, [_c.POINTER(TrainPieces), _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                            _c.POINTER(_c.c_int32), _c.POINTER(TrainBatch), _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
lib = _lib.binder(SIGNATURES)


def train_pieces_tag(tokenizer, max_seq_len, max_q_len, train_file=None):
    """qa_train_arena.train_arena_tag's content under this module's rule string."""
    return RULE + "|" + train_arena_tag(tokenizer, max_seq_len, max_q_len, train_file).split("|", 1)[1]


class _MemoTokenizer:
    """tokenizer.tokenize cached per distinct string (exact: it is a pure function of the string), for prepare() and answer_spans of the
    covered items, which otherwise WordPiece the words of shared passages once per chain."""

    def __init__(self, tokenizer):
        self.tok, self.memo = tokenizer, {}

    def tokenize(self, text):
        out = self.memo.get(text)
        if out is None:
            out = self.memo[text] = self.tok.tokenize(text)
        return out


def _spans_of(records, tokenizer, simple_tok, lo, hi):
    """[(first, last), ...] of each covered record in records[lo:hi] whose answer is a span: qa_data.prepare + qa_train_data.answer_spans."""
    from .qa_train_data import answer_spans
    out = []
    for rec in records[lo:hi]:
        ann = qa_data.prepare(dict(rec), tokenizer)["context_processed"]
        assert ann["all_doc_tokens"][0] == "yes" and ann["all_doc_tokens"][1] == "no"
        out.append([(int(s), int(e)) for s, e in answer_spans(ann, rec["gold_answer"], simple_tok, tokenizer)])
    return out


_BUILD = None  # (records, tokenizer, simple_tok) of the forked span workers


def _worker_spans(lo_hi):
    global _BUILD
    records, tok, simple_tok = _BUILD
    if not isinstance(tok, _MemoTokenizer):
        tok = _MemoTokenizer(tok)
        _BUILD = (records, tok, simple_tok)
    return _spans_of(records, tok, simple_tok, *lo_hi)


def _chunk(n, workers, most):
    """Rows per unit of work: `most`, or less where that would leave fewer than four units per worker."""
    return max(1, min(most, -(-n // (4 * workers)))) if workers > 1 else most


class QATrainPieces:
    def __init__(self, q_tokens, q_offsets, p_tokens, p_offsets, p_sent_starts, p_sent_offsets, items, sent_label, sent_label_index, spans,
                 span_index, special, cuts):
        """Host arrays. Every index array and every row number is checked here, once: the kernel trusts them."""
        given = dict(zip((n for n, _ in _ARRAYS), (q_tokens, q_offsets, p_tokens, p_offsets, p_sent_starts, p_sent_offsets, items, sent_label,
                                                   sent_label_index, spans, span_index, special, cuts)))
        for name, dt in _ARRAYS:
            setattr(self, name, np.ascontiguousarray(given[name], dtype=dt))
        self.items, self.spans = self.items.reshape(-1, 5), self.spans.reshape(-1, 2)
        self.n, self.n_questions, self.n_passages = len(self.items), len(self.q_offsets) - 1, len(self.p_offsets) - 1
        if self.special.shape != (4,) or self.cuts.shape != (2,):
            raise ValueError("special holds the ids of cls, sep, yes, no and cuts holds max_seq_len, max_q_len")
        self.max_seq_len, self.max_q_len = int(self.cuts[0]), int(self.cuts[1])
        for idx, arr, rows, what in ((self.q_offsets, self.q_tokens, self.n_questions, "q_tokens"), (self.p_offsets, self.p_tokens, self.n_passages, "p_tokens"),
                                     (self.p_sent_offsets, self.p_sent_starts, self.n_passages, "p_sent_starts"),
                                     (self.sent_label_index, self.sent_label, self.n, "sent_label"), (self.span_index, self.spans, self.n, "spans")):
            if rows < 0 or idx.shape != (rows + 1,) or idx[0] != 0 or idx[-1] != len(arr) or (np.diff(idx) < 0).any():
                raise ValueError(f"the index of {what} must be [{rows} + 1], start at 0, not decrease and end at len({what}) = {len(arr)}")
        self.q_lens, self.p_lens, self.p_n_sents = np.diff(self.q_offsets), np.diff(self.p_offsets), np.diff(self.p_sent_offsets)
        self.longest_q = int(self.q_lens.max()) if self.n_questions else 0
        if self.max_seq_len - self.longest_q < 6:
            raise ValueError(f"max_seq_len = {self.max_seq_len} leaves no room for yes no [SEP] after a question of {self.longest_q} tokens")
        q, c = self.items[:, 0], self.items[:, 1:3]
        if self.n and (q.min() < 0 or q.max() >= self.n_questions or c.min() < 0 or c.max() >= self.n_passages):
            raise ValueError("an item names a question row or a passage row outside its table")
        # sentence starts: inside their passage and increasing, so that the sentences inside a cut are a prefix of the chain's ordinals
        owner = np.repeat(np.arange(self.n_passages), self.p_n_sents)
        s = self.p_sent_starts.astype(np.int64)
        if len(s) and ((s < 0).any() or (s >= self.p_lens[owner]).any() or ((np.diff(s) <= 0) & (np.diff(owner) == 0)).any()):
            raise ValueError("the sentence starts of a passage must increase and lie inside the passage")
        self._stride = int(self.p_lens.max()) + 1 if self.n_passages else 1
        self._sent_key = owner * self._stride + s  # increasing: one searchsorted counts the starts of a passage below a limit
        n_chain_sents = self.p_n_sents[c].sum(1) if self.n else np.zeros(0, np.int64)
        n_labels = np.diff(self.sent_label_index)
        if ((n_labels != 0) & (n_labels != n_chain_sents)).any():
            raise ValueError("an item holds either no sentence label or one per sentence of its chain")
        # host geometry of every item: para_offset, kept WordPieces, row length, sentences and spans inside the cut
        self.para_offset = self.q_lens[q] + 2 if self.n else np.zeros(0, np.int64)
        l0, l1 = (self.p_lens[c[:, 0]], self.p_lens[c[:, 1]]) if self.n else (np.zeros(0, np.int64),) * 2
        self.n_wp = np.minimum(4 + l0 + l1, np.maximum(0, self.max_seq_len - self.para_offset - 1))
        self.lens = self.para_offset + self.n_wp + 1
        self.n_sents = self._sents_below(c[:, 0], self.n_wp - 3) + self._sents_below(c[:, 1], self.n_wp - 4 - l0) if self.n else np.zeros(0, np.int64)
        pair_item = np.repeat(np.arange(self.n), np.diff(self.span_index))
        inside = self.spans[:, 0] < self.n_wp[pair_item]
        self.n_spans = np.maximum(1, np.bincount(pair_item[inside], minlength=self.n)).astype(np.int64)
        self.dev = None

    def _sents_below(self, rows, limit):
        """Per entry: how many sentence starts of passage rows[i] are < limit[i]."""
        lim = np.clip(limit, 0, self._stride - 1)
        return np.searchsorted(self._sent_key, rows.astype(np.int64) * self._stride + lim, side="left") - self.p_sent_offsets[rows]

    # -- builders -------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dataset(cls, ds, workers=0):
        """ds: a qa_train_data.QATrainDataset (its data, tokenizer, max_seq_len, max_q_len, simple_tok are read). workers > 1: that many
        forked processes (at most MAX_WORKERS) for the passages and for the covered items' spans, forked BEFORE the caller touches the
        device. The arrays do not depend on workers."""
        global _BUILD
        tok, records = ds.tokenizer, ds.data
        workers = min(MAX_WORKERS, int(workers))
        sp = qa_arena.special_ids(tok)
        q_row, q_ids, p_row, docs = {}, [], {}, []
        items = np.zeros((len(records), 5), np.int32)
        for i, rec in enumerate(records):
            if len(rec["passages"]) != 2:
                raise ValueError(f"record {i} (question {rec['qid']!r}) has a chain of {len(rec['passages'])} passages: the piece arena "
                                 "composes chains of exactly two")
            qi = q_row.get(rec["qid"])
            if qi is None:
                qi = q_row[rec["qid"]] = len(q_ids)
                q_ids.append(tok.convert_tokens_to_ids(tok.tokenize(rec["question"])[:ds.max_q_len]))
            rows = []
            for p in rec["passages"]:
                text = qa_arena.passage_text(p)
                pi = p_row.get(text)
                if pi is None:
                    pi = p_row[text] = len(docs)
                    docs.append(p)
                rows.append(pi)
            items[i] = (qi, rows[0], rows[1], int(rec["label"]), int(rec["ans_covered"]))
        passages = qa_arena.QAArena.from_corpus({str(i): d for i, d in enumerate(docs)}, tok, workers=workers, chunk=_chunk(len(docs), workers, 2048))
        n_sents = np.diff(passages.sent_offsets)
        # sentence labels, by the chain's sentence ordinal
        labels, n_labels = [], np.zeros(len(records), np.int64)
        for i, rec in enumerate(records):
            sl = rec.get("sp_sent_labels") or []
            if rec["label"]:
                assert len(sl) == n_sents[items[i, 1]] + n_sents[items[i, 2]]  # the reference's assert
            labels.extend(int(x) for x in sl)
            n_labels[i] = len(sl)
        # spans: uncut, in chain WordPiece positions
        searched = [i for i, rec in enumerate(records) if rec["ans_covered"] and rec["gold_answer"][0] not in ("yes", "no")]
        todo = [records[i] for i in searched]
        chunk = _chunk(len(todo), workers, 256)
        ranges = [(lo, min(len(todo), lo + chunk)) for lo in range(0, len(todo), chunk)]
        if min(workers, len(ranges)) > 1:
            _BUILD = (todo, tok, ds.simple_tok)
            try:
                with multiprocessing.get_context("fork").Pool(min(workers, len(ranges))) as pool:
                    parts = pool.map(_worker_spans, ranges, chunksize=1)
            finally:
                _BUILD = None
        else:
            memo = _MemoTokenizer(tok)
            parts = [_spans_of(todo, memo, ds.simple_tok, lo, hi) for lo, hi in ranges]
        found = dict(zip(searched, (s for part in parts for s in part)))
        spans, n_pairs = [], np.zeros(len(records), np.int64)
        for i, rec in enumerate(records):
            if not rec["ans_covered"]:
                continue
            pairs = {"yes": [(0, 0)], "no": [(1, 1)]}.get(rec["gold_answer"][0])
            pairs = found[i] if pairs is None else pairs
            spans.extend(pairs)
            n_pairs[i] = len(pairs)
        arena = cls(np.asarray([t for q in q_ids for t in q], np.int32), _index([len(q) for q in q_ids]), np.asarray(passages.tokens, np.int32),
                    passages.offsets, np.asarray(passages.sent_starts, np.int32), passages.sent_offsets, items, np.asarray(labels, np.int32),
                    _index(n_labels), np.asarray(spans, np.int32).reshape(-1, 2), _index(n_pairs), [sp["cls"], sp["sep"], sp["yes"], sp["no"]],
                    [ds.max_seq_len, ds.max_q_len])
        arena.searched = len(searched)  # items that went through answer_spans (a build statistic, not stored)
        return arena

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
    def load_or_build(cls, train_file, ds, tokenizer, log=None, workers=0):
        """`<train_file>.qa_train_pieces.npz` when its tag is this tokenizer's, these cuts' and this file's and it holds len(ds) items; else
        a fresh build written there."""
        cache, tag = train_file + ".qa_train_pieces.npz", train_pieces_tag(tokenizer, ds.max_seq_len, ds.max_q_len, train_file)
        arena = None
        if os.path.exists(cache):
            try:
                arena = cls.load(cache, expect_tag=tag)
            except (OSError, ValueError, KeyError, EOFError):
                arena = None
            if arena is not None and arena.n != len(ds):
                arena = None
            if arena is not None and log is not None:
                log(f"Loaded the reader's training pieces from {cache} ({arena.n} items, {arena.n_questions} questions, {arena.n_passages} passages)")
        if arena is None:
            if log is not None:
                log(f"Preparing the training set once for the reader as pieces ({len(ds)} items, {workers} workers)...")
            arena = cls.from_dataset(ds, workers=workers)
            try:
                arena.save(cache, tag=tag)
            except OSError:
                pass  # a read-only data directory: the arena is rebuilt next time
        return arena

    def to(self, device):
        self.dev = {n: _to_device(getattr(self, n), device, torch.int32 if dt is np.int32 else torch.int64) for n, dt in _DEVICE_ARRAYS}
        return self

    @property
    def bytes_per_item(self):
        return sum(getattr(self, n).nbytes for n, _ in _ARRAYS) / max(1, self.n)

    # -- host geometry --------------------------------------------------------------------------------------------------------------------
    def batch_shape(self, indices):
        """(out_len, n_sent, n_span) of the padded batch qa_collate would build for these items, from host metadata only: QATrainArena's
        semantics. An index outside [0, N) is an empty row; every width is at least what an empty batch needs (1, 0, 1)."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        ok = (idx >= 0) & (idx < self.n)
        safe = np.where(ok, idx, 0)
        width = lambda a, least: max(least, int(np.where(ok, a[safe], 0).max())) if len(idx) and self.n else least  # noqa: E731
        return width(self.lens, 1), width(self.n_sents, 0), width(self.n_spans, 1)

    def compose_host(self, indices, out_len=None, n_sent=None, n_span=None, pad_id=0, labels_per_passage=False, drop_cut=True, clamp_end=True):
        """numpy statement of what mdr_reader_train_compose writes (the yardstick of the kernel): QATrainArena.assemble_host's keys, dtypes
        and conventions. labels_per_passage / drop_cut / clamp_end exist for the tests' mutants only."""
        idx = np.asarray(indices, np.int64).reshape(-1)
        shape = self.batch_shape(idx)
        L, S, P = (shape[0] if out_len is None else out_len), (shape[1] if n_sent is None else n_sent), (shape[2] if n_span is None else n_span)
        R = len(idx)
        cls_id, sep, yes, no = (int(x) for x in self.special)
        out = {k: np.zeros((R, L), np.int64) for k in NET_KEYS[:4]}
        out["input_ids"][:] = pad_id
        out["sent_offsets"], out["sent_labels"] = np.zeros((R, S), np.int64), np.zeros((R, S), np.int64)
        out["starts"], out["ends"] = np.full((R, P), -1, np.int64), np.full((R, P), -1, np.int64)
        out["label"], out["ans_covered"] = np.full((R, 1), -1, np.int64), np.zeros((R, 1), np.int64)
        out["para_offsets"], out["lengths"] = np.zeros(R, np.int64), np.zeros(R, np.int64)
        for r, i in enumerate(idx):
            if not 0 <= i < self.n:
                continue
            qi, c0, c1, label, cov = (int(x) for x in self.items[i])
            q = self.q_tokens[self.q_offsets[qi]:self.q_offsets[qi + 1]]
            p1, p2 = (self.p_tokens[self.p_offsets[c]:self.p_offsets[c + 1]] for c in (c0, c1))
            s1, s2 = (self.p_sent_starts[self.p_sent_offsets[c]:self.p_sent_offsets[c + 1]].astype(np.int64) for c in (c0, c1))
            po = len(q) + 2
            wp = np.concatenate([[yes, no, sep], p1, [sep], p2]).astype(np.int64)
            n_wp = min(len(wp), max(0, self.max_seq_len - po - 1))
            row = np.concatenate([[cls_id], q, [sep], wp[:n_wp], [sep]]).astype(np.int64)
            n, m = len(row), min(len(row), L)
            out["input_ids"][r, :m] = row[:m]
            out["attention_mask"][r, :m] = 1
            out["token_type_ids"][r, min(po, m):m] = 1
            out["paragraph_mask"][r, min(po, L):max(min(po, L), min(n - 1, L))] = 1
            starts = np.concatenate([s1 + 3, s2 + 4 + len(p1)])
            labels = self.sent_label[self.sent_label_index[i]:self.sent_label_index[i + 1]]
            ordinal = np.concatenate([np.arange(len(s1)), np.arange(len(s2)) + (0 if labels_per_passage else len(s1))])
            kept = np.nonzero(starts < n_wp)[0][:S]
            out["sent_offsets"][r, :len(kept)] = starts[kept] + po
            if len(labels):
                out["sent_labels"][r, :len(kept)] = labels[ordinal[kept]]
            pairs = self.spans[self.span_index[i]:self.span_index[i + 1]].astype(np.int64)
            if drop_cut:
                pairs = pairs[pairs[:, 0] < n_wp]
            pairs = pairs[:P]
            out["starts"][r, :len(pairs)] = np.minimum(pairs[:, 0], n_wp - 1) + po
            out["ends"][r, :len(pairs)] = (np.minimum(pairs[:, 1], n_wp - 1) if clamp_end else pairs[:, 1]) + po
            out["label"][r, 0], out["ans_covered"][r, 0] = label, cov
            out["para_offsets"][r], out["lengths"][r] = po, n
        return out

    # -- the device op --------------------------------------------------------------------------------------------------------------------
    def assemble(self, indices_dev, out_len, n_sent, n_span, pad_id=0, out=None):
        """QATrainArena.assemble's signature and results, from the pieces: indices_dev int64 cuda [R] -> dict of int64 cuda tensors under
        NET_KEYS plus para_offsets and lengths [R]. `out`: a dict of preallocated contiguous tensors of exactly those shapes to write into."""
        if self.dev is None:
            raise RuntimeError("QATrainPieces.to(device) first")
        dev = self.dev["items"].device
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
        a = TrainPieces(*(vp(d[n]) for n, _ in _DEVICE_ARRAYS), self.n, self.n_questions, self.n_passages, self.longest_q)
        o = TrainBatch(*(vp(out[k]) if out[k].numel() else None for k in NET_KEYS + ("para_offsets", "lengths")))
        sp = (ctypes.c_int32 * 5)(*(int(x) for x in self.special), int(pad_id))
        if R:
            _lib.call(lib().mdr_reader_train_compose, ctypes.byref(a), vp(idx), R, self.max_seq_len, out_len, n_sent, n_span, sp, ctypes.byref(o), dev=dev)
        return out
