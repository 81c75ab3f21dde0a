"""QA passage arena: the corpus WordPiece-tokenised ONCE under prepare()'s rule, so that the reader's input rows
`[CLS] q [SEP] yes no [SEP] P1 [SEP] P2 [SEP]` are assembled on the device from chain ids (libmdrhip.so: mdr_reader_assemble,
include/mdr_reader.h) instead of re-running prepare() + WordPiece + qa_collate on the host for every chain.

Why it is exact. qa_data.prepare() builds "yes no [SEP] " + " [SEP] ".join(passage strings), splits it on qa_data._is_whitespace
(not str.split(): \\x0b, \\x0c, \\x1c-\\x1f, \\x85, \\u2028 and \\u2029 stay inside words) and WordPiece-tokenises word by word, keeping
[SEP], [unused1] and [unused2] whole. The separators are surrounded by blanks, so no word crosses a passage boundary and a chain's
WordPieces are `yes no [SEP] P1 [SEP] P2`, each Pi a function of passage i alone; [unused1] words (a literal one inside a sentence
included) are its sentence starts. The arena stores, per passage, the ids of Pi and those start positions relative to Pi.

Layout (mirrors arena.TokenArena): int32 tokens + int64 token offsets [N + 1], int32 sentence starts + int64 sentence offsets [N + 1].
The host keeps its copy of all four: batch shapes (the row width and sentence count qa_collate would pad to) are computed from it
without a device sync. Cached as `<corpus>.qa_arena.npz` under qa_arena_tag(); another tag means a rebuild, never a reuse.
"""
import hashlib
import json
import multiprocessing
import os
import re

import numpy as np
import torch

from . import qa_data
from .arena import _npz_memmap, _to_device

RULE = "qa-arena-v1"  # prepare()'s whitespace split, specials kept whole, WordPiece per word, [unused1] = sentence start
MAX_WORKERS = 16

_WS_RE = None


def _split_re():
    """One regex over every character qa_data._is_whitespace accepts (" \\t\\n\\r" and category Zs, all in the BMP)."""
    global _WS_RE
    if _WS_RE is None:
        ws = "".join(chr(c) for c in range(0x10000) if qa_data._is_whitespace(chr(c)))
        _WS_RE = re.compile("[" + re.escape(ws) + "]+")
    return _WS_RE


def passage_text(doc):
    """One passage's part of prepare()'s context string."""
    return doc["title"].strip() + " " + " ".join("[unused1] " + s.strip() for s in doc["sents"])


def split_words(text):
    """prepare()'s doc_tokens of `text`."""
    return [w for w in _split_re().split(text) if w]


class WordPieces:
    """word -> WordPiece ids as prepare() + convert_tokens_to_ids produce them; memo=True caches per distinct word (exact: tokenize is a
    pure function of the word)."""

    def __init__(self, tokenizer, memo=True):
        self.tok = tokenizer
        self.memo = {} if memo else None
        self.special = {t: [tokenizer.convert_tokens_to_ids(t)] for t in qa_data.SPECIAL_TOKS}

    def __call__(self, word):
        ids = self.special.get(word)
        if ids is not None:
            return ids
        if self.memo is not None:
            ids = self.memo.get(word)
            if ids is not None:
                return ids
        ids = self.tok.convert_tokens_to_ids(self.tok.tokenize(word))
        if self.memo is not None:
            self.memo[word] = ids
        return ids


def passage_ids(doc, pieces):
    """(WordPiece ids of the passage, its [unused1] positions relative to the passage)."""
    ids, starts = [], []
    for w in split_words(passage_text(doc)):
        if w == "[unused1]":
            starts.append(len(ids))
        ids.extend(pieces(w))
    return ids, starts


def _tokenize_range(id2doc, pieces, lo, hi):
    toks, lens, starts, ns = [], np.zeros(hi - lo, np.int64), [], np.zeros(hi - lo, np.int64)
    for i in range(lo, hi):
        ids, st = passage_ids(id2doc[str(i)], pieces)
        toks.extend(ids)
        starts.extend(st)
        lens[i - lo], ns[i - lo] = len(ids), len(st)
    return np.asarray(toks, np.int32), lens, np.asarray(starts, np.int32), ns


_BUILD = None  # (id2doc, tokenizer, memo) of the forked build workers


def _worker_range(lo_hi):
    global _BUILD
    id2doc, tok, memo = _BUILD
    if not isinstance(memo, WordPieces):
        memo = WordPieces(tok, memo=bool(memo))
        _BUILD = (id2doc, tok, memo)
    return _tokenize_range(id2doc, memo, *lo_hi)


def qa_arena_tag(tokenizer):
    """What a cached arena is valid for: the rule, the tokenizer class (without a trailing "Fast"), its lower-casing / accent switches and
    a hash of its vocabulary."""
    vocab = hashlib.sha256(json.dumps(sorted(tokenizer.get_vocab().items())).encode()).hexdigest()[:16]  # (no fallback: a tag must tell vocabularies apart)
    name = tokenizer.__class__.__name__
    name = name[:-4] if name.endswith("Fast") else name
    lower = getattr(tokenizer, "do_lower_case", None)
    accents = getattr(tokenizer, "strip_accents", None)
    return f"{RULE}|tokenizer={name}|lower={lower}|strip_accents={accents}|vocab={vocab}"


class QAArena:
    def __init__(self, tokens, offsets, sent_starts, sent_offsets):
        """Host arrays (numpy or read-only memmaps); `to(device)` adds the device copy."""
        self.tokens, self.offsets = tokens, np.asarray(offsets, np.int64)
        self.sent_starts, self.sent_offsets = sent_starts, np.asarray(sent_offsets, np.int64)
        self.n = int(self.offsets.shape[0]) - 1
        self.lens = np.diff(self.offsets)
        self.n_sents = np.diff(self.sent_offsets)
        self.dev = None

    # -- builders ----------------------------------------------------------------------------------------
    @classmethod
    def from_corpus(cls, id2doc, tokenizer, workers=0, memo=True, chunk=2048):
        """id2doc: {"<row id>": {"title", "sents", ...}} for row ids 0..N-1. workers > 0: that many forked processes (at most
        MAX_WORKERS), forked BEFORE the caller touches the device."""
        global _BUILD
        n = len(id2doc)
        ranges = [(lo, min(n, lo + chunk)) for lo in range(0, n, chunk)]
        workers = min(MAX_WORKERS, int(workers), len(ranges))
        if workers > 1:
            _BUILD = (id2doc, tokenizer, memo)
            try:
                with multiprocessing.get_context("fork").Pool(workers) as pool:
                    parts = pool.map(_worker_range, ranges, chunksize=1)
            finally:
                _BUILD = None
        else:
            pieces = WordPieces(tokenizer, memo=memo)
            parts = [_tokenize_range(id2doc, pieces, lo, hi) for lo, hi in ranges]
        cat = (lambda i, dt: np.concatenate([p[i] for p in parts]) if parts else np.zeros(0, dt))
        offsets = np.zeros(n + 1, np.int64)
        offsets[1:] = np.cumsum(cat(1, np.int64))
        sent_offsets = np.zeros(n + 1, np.int64)
        sent_offsets[1:] = np.cumsum(cat(3, np.int64))
        return cls(cat(0, np.int32), offsets, cat(2, np.int32), sent_offsets)

    def save(self, path, tag=""):
        tmp = path + f".tmp{os.getpid()}.npz"  # written under another name and renamed: a reader never sees a partial file
        np.savez(tmp, tokens=np.asarray(self.tokens), offsets=self.offsets, sent_starts=np.asarray(self.sent_starts),
                 sent_offsets=self.sent_offsets, tag=np.array(str(tag)))
        os.replace(tmp, path)

    @classmethod
    def load(cls, path, expect_tag=None):
        """None when the file carries no tag or another one (the caller rebuilds)."""
        z = _npz_memmap(path)
        if z is None:
            z = dict(np.load(path))
        if expect_tag is not None and ("tag" not in z or str(z["tag"]) != str(expect_tag)):
            return None
        return cls(z["tokens"], z["offsets"], z["sent_starts"], z["sent_offsets"])

    @classmethod
    def load_or_build(cls, corpus_path, id2doc, tokenizer, workers=0, log=None):
        """`<corpus_path>.qa_arena.npz` when its tag is this tokenizer's, it holds as many passages as id2doc and it is not older than the
        corpus file; else a fresh build written there."""
        cache, tag = corpus_path + ".qa_arena.npz", qa_arena_tag(tokenizer)
        arena = None
        if os.path.exists(cache) and (not os.path.exists(corpus_path) or os.path.getmtime(cache) >= os.path.getmtime(corpus_path)):
            try:
                arena = cls.load(cache, expect_tag=tag)
            except (OSError, ValueError, KeyError, EOFError):
                arena = None
            if arena is not None and arena.n != len(id2doc):
                arena = None
        if arena is None:
            if log is not None:
                log(f"Tokenising the corpus once for the reader ({len(id2doc)} passages, {workers} workers)...")
            arena = cls.from_corpus(id2doc, tokenizer, workers=workers)
            arena.save(cache, tag=tag)
        return arena

    def to(self, device):
        self.dev = {"tokens": _to_device(self.tokens, device, torch.int32), "offsets": _to_device(self.offsets, device, torch.int64),
                    "sent_starts": _to_device(self.sent_starts, device, torch.int32), "sent_offsets": _to_device(self.sent_offsets, device, torch.int64)}
        return self

    # -- host geometry ---------------------------------------------------------------------------------------
    def row_geometry(self, q_lens, chains, row_q, max_seq_len):
        """Per row: (para_offset, length, sentence count inside the cut) exactly as QAEvalDataset computes them, from host metadata only."""
        chains = np.asarray(chains, np.int64).reshape(-1, 2)
        ok = (chains >= 0) & (chains < self.n)
        safe = np.where(ok, chains, 0)
        lens = np.where(ok, self.lens[safe], 0)
        ns = np.where(ok, self.n_sents[safe], 0)
        row_q = np.asarray(row_q, np.int64)
        q_lens = np.asarray(q_lens, np.int64)
        ql = np.where((row_q >= 0) & (row_q < len(q_lens)), q_lens[np.clip(row_q, 0, max(0, len(q_lens) - 1))] if len(q_lens) else 0, 0)
        po = ql + 2
        wp = 4 + lens[:, 0] + lens[:, 1]
        cut = np.clip(np.minimum(wp, max_seq_len - po - 1), 0, None)
        cnt = ns.sum(1)
        for r in np.nonzero(cut < wp)[0]:  # only rows cut at max_seq_len lose sentence starts
            c = 0
            for k, base in ((0, 3), (1, 4 + lens[r, 0])):
                if ok[r, k]:
                    p = chains[r, k]
                    s = np.asarray(self.sent_starts[self.sent_offsets[p]:self.sent_offsets[p + 1]])
                    c += int(np.count_nonzero(base + s < cut[r]))
            cnt[r] = c
        return po, po + cut + 1, cnt

    def batch_shape(self, q_lens, chains, row_q, max_seq_len):
        """(out_len, n_sent) of the padded batch qa_collate would build for these rows."""
        _, n, cnt = self.row_geometry(q_lens, chains, row_q, max_seq_len)
        return (int(n.max()) if len(n) else 1), (int(cnt.max()) if len(cnt) else 0)


def special_ids(tokenizer):
    """{cls, sep, yes, no, pad} ids; QAEvalDataset asserts that "yes" and "no" are single WordPieces."""
    for w in ("yes", "no"):
        if tokenizer.tokenize(w) != [w]:
            raise ValueError(f"{w!r} is not a single WordPiece of this tokenizer (QAEvalDataset asserts it is)")
    ids = lambda t: int(tokenizer.convert_tokens_to_ids(t))  # noqa: E731
    return {"cls": ids(tokenizer.cls_token), "sep": ids(tokenizer.sep_token), "yes": ids("yes"), "no": ids("no"), "pad": int(tokenizer.pad_token_id)}


def question_ids(tokenizer, question, max_q_len):
    """QAEvalDataset's question: one trailing "?" stripped, WordPieces cut to max_q_len, as ids."""
    if question.endswith("?"):
        question = question[:-1]
    return tokenizer.convert_tokens_to_ids(tokenizer.tokenize(question)[:max_q_len])


def assemble_host(arena, q_ids, chains, row_q, special, max_seq_len, out_len=None, n_sent=None):
    """numpy statement of the rows mdr_reader_assemble writes (the yardstick of the kernel). q_ids: list of id lists (already cut),
    chains int [R, 2], row_q int [R]. Returns int64 input_ids / attention_mask / token_type_ids / paragraph_mask [R, out_len],
    sent_offsets [R, n_sent], para_offsets / lengths [R], and wp_ids (the cut wp part of each row, a list of arrays)."""
    chains = np.asarray(chains, np.int64).reshape(-1, 2)
    row_q = np.asarray(row_q, np.int64)
    q_lens = [len(q) for q in q_ids]
    po, n, cnt = arena.row_geometry(q_lens, chains, row_q, max_seq_len)
    R = len(chains)
    L = (int(n.max()) if R else 1) if out_len is None else out_len
    S = (int(cnt.max()) if R else 0) if n_sent is None else n_sent
    out = {k: np.zeros((R, L), np.int64) for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask")}
    out["input_ids"][:] = special["pad"]
    out["sent_offsets"] = np.zeros((R, S), np.int64)
    out["para_offsets"], out["lengths"], out["wp_ids"] = po.astype(np.int64), n.astype(np.int64), []
    for r in range(R):
        b = row_q[r]
        q = list(q_ids[b]) if 0 <= b < len(q_ids) else []
        parts, starts = [], []
        for k, p in enumerate(chains[r]):
            if 0 <= p < arena.n:
                toks = np.asarray(arena.tokens[arena.offsets[p]:arena.offsets[p + 1]], np.int64)
                ss = np.asarray(arena.sent_starts[arena.sent_offsets[p]:arena.sent_offsets[p + 1]], np.int64)
            else:
                toks, ss = np.zeros(0, np.int64), np.zeros(0, np.int64)
            base = 3 if k == 0 else 4 + len(parts[0])
            parts.append(toks)
            starts.extend((ss + base).tolist())
        wp = np.concatenate([[special["yes"], special["no"], special["sep"]], parts[0], [special["sep"]], parts[1]]).astype(np.int64)
        wp = wp[:max(0, max_seq_len - (len(q) + 2) - 1)]
        row = np.concatenate([[special["cls"]], q, [special["sep"]], wp, [special["sep"]]]).astype(np.int64)
        m = min(len(row), L)
        out["input_ids"][r, :m] = row[:m]
        out["attention_mask"][r, :m] = 1
        p0 = len(q) + 2
        out["token_type_ids"][r, p0:m] = 1
        out["paragraph_mask"][r, p0:min(len(row) - 1, L)] = 1
        so = [s + p0 for s in starts if s < len(wp)][:S]
        out["sent_offsets"][r, :len(so)] = so
        out["wp_ids"].append(wp)
    return out


def assemble(arena, q_ids, q_lens, chains, row_q, special, max_seq_len, out_len, n_sent):
    """The device op: q_ids int64 cuda [B, Lq], q_lens int64 cuda [B], chains int64 cuda [R, 2], row_q int64 cuda [R] -> dict of int64 cuda
    tensors (input_ids, attention_mask, token_type_ids, paragraph_mask [R, out_len], sent_offsets [R, n_sent], para_offsets, lengths [R])."""
    import ctypes

    from . import _lib, reader
    if arena.dev is None:
        raise RuntimeError("QAArena.to(device) first")
    dev = chains.device
    q_ids, q_lens, chains, row_q = (t.to(dev, torch.int64).contiguous() for t in (q_ids, q_lens, chains, row_q))
    R = int(chains.shape[0])
    i64 = dict(dtype=torch.int64, device=dev)
    out = {k: torch.empty((R, out_len), **i64) for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask")}
    out["sent_offsets"] = torch.empty((R, n_sent), **i64)
    out["para_offsets"], out["lengths"] = torch.empty(R, **i64), torch.empty(R, **i64)
    vp = reader._ptr
    a = reader.ReaderArena(vp(arena.dev["tokens"]), vp(arena.dev["offsets"]), vp(arena.dev["sent_starts"]), vp(arena.dev["sent_offsets"]), arena.n)
    o = reader.ReaderBatch(*(vp(out[k]) for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets", "para_offsets",
                                                  "lengths")))
    sp = (ctypes.c_int32 * 5)(special["cls"], special["sep"], special["yes"], special["no"], special["pad"])
    with torch.cuda.device(dev):
        _lib.check(reader.lib().mdr_reader_assemble(vp(q_ids), vp(q_lens), int(q_ids.shape[0]), int(q_ids.shape[1]), vp(chains), vp(row_q), R,
                                                    ctypes.byref(a), sp, int(max_seq_len), int(out_len), int(n_sent), ctypes.byref(o), dev.index,
                                                    _lib.current_stream_ptr(dev)))
    return out
