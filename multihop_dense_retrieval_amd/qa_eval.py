"""The reader's EVALUATION from a dev piece arena: what scripts/train_qa.py --eval-arena runs instead of QADataset.__getitem__ + qa_collate
on every candidate chain and get_final_text on every chain's answer, with the host path's log lines, metrics, predictions and checkpoint
decisions.

    QAEvalPieces    the predict file as QADataset(train=False) reads it, stored as pieces: one row per question (qa_arena.question_ids),
                    one per DISTINCT passage text (a qa_arena.QAArena, built by its builder and worker pool), four integers per item
                    (question row, P1 row, P2 row, label). Batches are the host path's (consecutive --predict_batch_size items in file
                    order); their rows are written on the device by qa_arena.assemble (mdr_reader_assemble), bit for bit qa_collate's.
    ScoreTable      decode()'s outputs of every batch, copied device to device into tensors of n_items rows.
    select          libmdrhip.so: mdr_reader_select (include/mdr_reader_select.h): per question and combination factor the chain
                    predict()'s in-place sorts leave on top. select_sweep_host is its yardstick (the literal list.sort calls),
                    select_host the numpy statement of the kernel's rule.
    predict_metrics, final_results
                    one read-back of the winners, a gather of the winners' rows, prepare() + qa_data.chain_results on each DISTINCT winner
                    once, then qa_data.metrics_report / qa_data.final_report: the host path's own metric arithmetic and log lines.

Only chains of exactly two passages, as in mdr_reader_assemble; an `_id` on two lines of the file is refused too (predict() merges such
lines into one question, whose chains would not be consecutive items). Cached as `<predict file>.qa_eval_pieces.npz` under
eval_pieces_tag(); another tag means a rebuild, never a reuse. The file itself is read at every start: the passages' dicts stay on the
host for the decode of the winners.
"""
import ctypes
import json
import os

import numpy as np
import torch

from . import _lib, qa_arena, qa_data
from .arena import _to_device
from .qa_train_arena import _index
from .qa_train_pieces import _chunk

_c = ctypes
RULE = "qa-eval-pieces-v1"  # question rows, distinct qa_arena.passage_text rows, four integers per item, one segment per line of the file
MAX_WORKERS = qa_arena.MAX_WORKERS
MAX_LAMBDAS = 16  # MDR_READER_SELECT_MAX_LAMBDAS
_ARRAYS = (("q_tokens", np.int32), ("q_offsets", np.int64), ("p_tokens", np.int32), ("p_offsets", np.int64), ("p_sent_starts", np.int32),
           ("p_sent_offsets", np.int64), ("items", np.int32), ("seg_offsets", np.int64), ("cuts", np.int32))

# include/mdr_reader_select.h -- bound here, apart from every other header's table
SIGNATURES = {
    "mdr_reader_select": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.c_int,
                                     _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
lib = _lib.binder(SIGNATURES)


def eval_pieces_tag(tokenizer, max_q_len, predict_file=None):
    """What a cached QAEvalPieces is valid for: the rule, the tokenizer (qa_arena.qa_arena_tag), max_q_len and the file's size and mtime
    (as qa_train_pieces.train_pieces_tag takes them). max_seq_len is not part of it: the pieces are stored uncut."""
    st = os.stat(predict_file) if predict_file is not None else None
    return f"{RULE}|{qa_arena.qa_arena_tag(tokenizer)}|max_q_len={int(max_q_len)}|file={'-' if st is None else f'{st.st_size}:{st.st_mtime_ns}'}"


def read_eval_file(data_path):
    """The predict file as qa_data.QADataset(train=False) reads it: (records, seg_offsets). records: one dict per candidate chain in file
    order, QADataset.data's keys and values; seg_offsets int64 [lines + 1]: line j owns records seg_offsets[j] .. seg_offsets[j + 1] - 1.
    ValueError for what the piece arena does not take."""
    records, counts, seen = [], [], set()
    for n, line in enumerate(open(data_path).readlines()):
        item = json.loads(line)
        if item["_id"] in seen:
            raise ValueError(f"line {n + 1} repeats the _id {item['_id']!r}: predict() merges such lines into one question, whose chains are not "
                             "consecutive items")
        seen.add(item["_id"])
        if item["question"].endswith("?"):
            item["question"] = item["question"][:-1]
        sp_titles = set(p["title"] for p in item["sp"]) if "sp" in item else None
        sp_gold = [[sp["title"], i] for sp in item.get("sp", []) for i in sp["sp_sent_ids"]]
        for chain in item["candidate_chains"]:
            if len(chain) != 2:
                raise ValueError(f"line {n + 1} (question {item['_id']!r}) has a chain of {len(chain)} passages: the piece arena assembles "
                                 "chains of exactly two")
            label = int(set(p["title"] for p in chain) == sp_titles) if sp_titles else -1
            records.append({"question": item["question"], "passages": chain, "label": label, "qid": item["_id"],
                            "gold_answer": item.get("answer", []), "sp_gold": sp_gold})
        counts.append(len(item["candidate_chains"]))
    return records, _index(counts)


def check_offsets(q_offsets, n_items):
    """The contract mdr_reader_select trusts, checked on the host: int64 [n_q + 1], starting at or above 0, non-decreasing, ending at or
    below n_items, which is below 2^31 (winners are int32 item indices)."""
    q = np.asarray(q_offsets)
    if q.ndim != 1 or len(q) < 1 or q.dtype != np.int64:
        raise ValueError("q_offsets must be an int64 array of n_q + 1 entries")
    if q[0] < 0 or (np.diff(q) < 0).any() or q[-1] > n_items or n_items >= 2 ** 31:
        raise ValueError(f"q_offsets must start at or above 0, not decrease and end at or below n_items = {n_items} < 2^31")
    return q


# ---- the selection rule on the host ------------------------------------------------------------------------------------------------------


def _f64(scores16):
    """fp16 scores (float16, or their patterns as int16 / uint16) widened exactly to float64."""
    a = np.asarray(scores16)
    if a.dtype in (np.int16, np.uint16):
        a = a.view(np.float16)
    if a.dtype != np.float16:
        raise ValueError("scores must be float16 or their int16 / uint16 bit patterns")
    return a.astype(np.float64)


def select_sweep_host(rank16, span16, q_offsets, lambdas):
    """The yardstick: predict()'s literal sorts. Per question a list of its items, sorted in place once per factor with
    list.sort(key=lambda_ * rank + (1 - lambda_) * span, reverse=True) on Python floats, its head recorded after every sort; and the head of
    the list sorted by rank alone. -> (winners int32 [n_q, n_lambda], rank_top int32 [n_q]); -1 for an empty question."""
    rank, span = _f64(rank16).tolist(), _f64(span16).tolist()
    q = np.asarray(q_offsets, np.int64)
    winners, rank_top = np.full((len(q) - 1, len(lambdas)), -1, np.int32), np.full(len(q) - 1, -1, np.int32)
    for j in range(len(q) - 1):
        if q[j + 1] <= q[j]:
            continue
        res = list(range(int(q[j]), int(q[j + 1])))
        ans_res = list(res)
        res.sort(key=lambda i: rank[i], reverse=True)
        rank_top[j] = res[0]
        for k, lambda_ in enumerate(lambdas):
            ans_res.sort(key=lambda i: lambda_ * rank[i] + (1 - lambda_) * span[i], reverse=True)
            winners[j, k] = ans_res[0]
    return winners, rank_top


def select_host(rank16, span16, q_offsets, lambdas, first_index=False):
    """numpy statement of what mdr_reader_select writes: winners[q, k] = the item with the lexicographically largest
    (key_k, key_{k-1}, ..., key_0), the lowest index among equal tuples; rank_top = the first item with the largest rank score; a question
    with a non-finite score is flagged and gets -1. -> (winners, rank_top, flags). first_index: the tests' mutant, "first item with the
    largest key_k"."""
    r, s = _f64(rank16), _f64(span16)
    q = np.asarray(q_offsets, np.int64)
    K = len(lambdas)
    with np.errstate(invalid="ignore"):  # (0 * inf in a question that is flagged below)
        keys = [np.float64(lam) * r + np.float64(1 - lam) * s for lam in lambdas]  # two products and a sum, each rounded on its own
    winners, rank_top, flags = np.full((len(q) - 1, K), -1, np.int32), np.full(len(q) - 1, -1, np.int32), np.zeros(len(q) - 1, np.int32)
    for j in range(len(q) - 1):
        lo, hi = int(q[j]), int(q[j + 1])
        if hi <= lo:
            continue
        if not (np.isfinite(r[lo:hi]).all() and np.isfinite(s[lo:hi]).all()):
            flags[j] = 1
            continue
        rank_top[j] = lo + int(np.argmax(r[lo:hi]))
        for k in range(K):
            cand = np.arange(lo, hi)
            for i in range(k, -1, -1):
                v = keys[i][cand]
                cand = cand[v == v.max()]
                if first_index or len(cand) == 1:
                    break
            winners[j, k] = cand[0]
    return winners, rank_top, flags


# ---- the device op -----------------------------------------------------------------------------------------------------------------------


def select(rank16, span16, q_offsets_dev, lambdas, out=None):
    """mdr_reader_select on torch's current stream: rank16 / span16 cuda float16 (or int16 patterns) [n_items], q_offsets_dev cuda int64
    [n_q + 1] (check_offsets' contract: the caller checked it on the host), lambdas: 1 .. 16 Python numbers. -> (winners int32
    [n_q, n_lambda], rank_top int32 [n_q], flags int32 [n_q]) on the device; `out`: three preallocated contiguous tensors of those shapes."""
    dev = q_offsets_dev.device
    for t in (rank16, span16):
        if not (torch.is_tensor(t) and t.device == dev and t.dtype in (torch.float16, torch.int16) and t.dim() == 1 and t.is_contiguous()):
            raise ValueError("rank16 and span16 must be contiguous 1-D float16 (or int16) tensors on the device of q_offsets")
    if rank16.shape != span16.shape or not _lib.is_like(q_offsets_dev, (torch.int64,), q_offsets_dev.shape, dev) or q_offsets_dev.dim() != 1 \
            or q_offsets_dev.shape[0] < 1:
        raise ValueError("rank16 and span16 must have one shape and q_offsets must be a contiguous int64 tensor of n_q + 1 entries")
    n_q, K = int(q_offsets_dev.shape[0]) - 1, len(lambdas)
    shapes = ((n_q, K), (n_q,), (n_q,))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.int32, device=dev) for s in shapes)
    for t, s in zip(out, shapes):
        if not _lib.is_like(t, (torch.int32,), s, dev):
            raise ValueError(f"an output is {_lib.describe(t)}, not a contiguous int32 {s} on {dev}")
    lam = (_c.c_double * max(1, K))(*[float(x) for x in lambdas])
    om = (_c.c_double * max(1, K))(*[float(1 - x) for x in lambdas])  # Python's 1 - lambda, rounded once, as predict()'s key has it
    _lib.call(lib().mdr_reader_select, _lib.ptr(rank16), _lib.ptr(span16), _lib.ptr(q_offsets_dev), n_q, lam, om, K, *(_lib.ptr(t) for t in out), dev=dev)
    return out


# ---- the pieces --------------------------------------------------------------------------------------------------------------------------


class QAEvalPieces:
    def __init__(self, q_tokens, q_offsets, p_tokens, p_offsets, p_sent_starts, p_sent_offsets, items, seg_offsets, cuts, records, special,
                 max_seq_len, batch_size):
        """Host arrays (the cache's), the file's records (read_eval_file), qa_arena.special_ids and the run's --max_seq_len and
        --predict_batch_size. Every index array and row number is checked here, once: the kernels trust them."""
        given = dict(zip((n for n, _ in _ARRAYS), (q_tokens, q_offsets, p_tokens, p_offsets, p_sent_starts, p_sent_offsets, items, seg_offsets, cuts)))
        for name, dt in _ARRAYS:
            setattr(self, name, np.ascontiguousarray(given[name], dtype=dt))
        self.items = self.items.reshape(-1, 4)
        self.n, self.n_questions, self.n_passages = len(self.items), len(self.q_offsets) - 1, len(self.p_offsets) - 1
        self.records, self.special = records, dict(special)
        self.max_seq_len, self.max_q_len, self.batch_size = int(max_seq_len), int(self.cuts.reshape(-1)[0]), int(batch_size)
        if len(records) != self.n:
            raise ValueError(f"the file holds {len(records)} chains and the pieces {self.n} items")
        if self.batch_size < 1:
            raise ValueError("--predict_batch_size must be at least 1")
        for idx, arr, rows, what in ((self.q_offsets, self.q_tokens, self.n_questions, "q_tokens"), (self.p_offsets, self.p_tokens, self.n_passages, "p_tokens"),
                                     (self.p_sent_offsets, self.p_sent_starts, self.n_passages, "p_sent_starts")):
            if rows < 0 or idx.shape != (rows + 1,) or idx[0] != 0 or idx[-1] != len(arr) or (np.diff(idx) < 0).any():
                raise ValueError(f"the index of {what} must be [{rows} + 1], start at 0, not decrease and end at len({what}) = {len(arr)}")
        check_offsets(self.seg_offsets, self.n)
        if self.seg_offsets.shape != (self.n_questions + 1,) or self.seg_offsets[0] != 0 or self.seg_offsets[-1] != self.n:
            raise ValueError("seg_offsets must give every question row its items and cover all of them")
        q, c = self.items[:, 0], self.items[:, 1:3]
        if self.n and (q.min() < 0 or q.max() >= self.n_questions or c.min() < 0 or c.max() >= self.n_passages):
            raise ValueError("an item names a question row or a passage row outside its table")
        if self.n and not np.array_equal(q, np.repeat(np.arange(self.n_questions), np.diff(self.seg_offsets))):
            raise ValueError("the items of a question row must be its segment")
        self.q_lens = np.diff(self.q_offsets)
        self.longest_q = int(self.q_lens.max()) if self.n_questions else 0
        if self.max_seq_len - self.longest_q < 6:
            raise ValueError(f"max_seq_len = {self.max_seq_len} leaves no room for yes no [SEP] after a question of {self.longest_q} tokens")
        self.passages = qa_arena.QAArena(self.p_tokens, self.p_offsets, self.p_sent_starts, self.p_sent_offsets)
        self.q_ids = [self.q_tokens[self.q_offsets[i]:self.q_offsets[i + 1]].tolist() for i in range(self.n_questions)]
        # host geometry of every item, once: the widths of a batch cost no synchronisation
        self.para_offset, self.lens, self.n_sents = self.passages.row_geometry(self.q_lens, c, q, self.max_seq_len)
        self.batches = [(lo, min(self.n, lo + self.batch_size)) for lo in range(0, self.n, self.batch_size)]
        self.max_sents = max([self.batch_shape(lo, hi)[1] for lo, hi in self.batches], default=0)
        self.qids = [records[int(self.seg_offsets[j])]["qid"] for j in range(self.n_questions) if self.seg_offsets[j + 1] > self.seg_offsets[j]]
        self.q_row = {records[int(self.seg_offsets[j])]["qid"]: j for j in range(self.n_questions) if self.seg_offsets[j + 1] > self.seg_offsets[j]}
        self.gold = {r["qid"]: (r["gold_answer"], r["sp_gold"]) for r in records}
        self.dev = None

    # -- builders -------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_file(cls, predict_file, tokenizer, max_seq_len, max_q_len, batch_size, workers=0, records=None):
        """workers > 1: that many forked processes (at most MAX_WORKERS) for the passages, forked BEFORE the caller touches the device. The
        arrays do not depend on workers."""
        records, seg = read_eval_file(predict_file) if records is None else records
        special = qa_arena.special_ids(tokenizer)
        workers = min(MAX_WORKERS, int(workers))
        n_q = len(seg) - 1
        q_ids = []
        for j in range(n_q):  # a line without chains keeps an empty question row: it has no item to read it
            q_ids.append(qa_arena.question_ids(tokenizer, records[int(seg[j])]["question"], max_q_len) if seg[j + 1] > seg[j] else [])
        p_row, docs = {}, []
        items = np.zeros((len(records), 4), np.int32)
        owner = np.repeat(np.arange(n_q), np.diff(seg))
        for i, rec in enumerate(records):
            rows = []
            for p in rec["passages"]:
                text = qa_arena.passage_text(p)
                pi = p_row.get(text)
                if pi is None:
                    pi = p_row[text] = len(docs)
                    docs.append(p)
                rows.append(pi)
            items[i] = (owner[i], rows[0], rows[1], int(rec["label"]))
        psg = qa_arena.QAArena.from_corpus({str(i): d for i, d in enumerate(docs)}, tokenizer, workers=workers, chunk=_chunk(len(docs), workers, 2048))
        return cls(np.asarray([t for q in q_ids for t in q], np.int32), _index([len(q) for q in q_ids]), np.asarray(psg.tokens, np.int32), psg.offsets,
                   np.asarray(psg.sent_starts, np.int32), psg.sent_offsets, items, seg, [max_q_len], records, special, max_seq_len, batch_size)

    def save(self, path, tag=""):
        tmp = path + f".tmp{os.getpid()}.npz"  # written under another name and renamed: a reader never sees a partial file
        np.savez(tmp, tag=np.array(str(tag)), **{n: getattr(self, n) for n, _ in _ARRAYS})
        os.replace(tmp, path)

    @classmethod
    def load(cls, path, records, special, max_seq_len, batch_size, expect_tag=None):
        """None when the file carries no tag or another one (the caller rebuilds)."""
        z = dict(np.load(path))
        if expect_tag is not None and ("tag" not in z or str(z["tag"]) != str(expect_tag)):
            return None
        return cls(*(z[n] for n, _ in _ARRAYS), records, special, max_seq_len, batch_size)

    @classmethod
    def load_or_build(cls, predict_file, tokenizer, max_seq_len, max_q_len, batch_size, log=None, workers=0):
        """`<predict_file>.qa_eval_pieces.npz` when its tag is this tokenizer's, this max_q_len's and this file's and it holds the file's
        chains; else a fresh build written there. The refusals (ValueError) come before either, and leave no cache."""
        parsed = read_eval_file(predict_file)
        special = qa_arena.special_ids(tokenizer)
        cache, tag = predict_file + ".qa_eval_pieces.npz", eval_pieces_tag(tokenizer, max_q_len, predict_file)
        pieces = None
        if os.path.exists(cache):
            try:
                pieces = cls.load(cache, parsed[0], special, max_seq_len, batch_size, expect_tag=tag)
            except (OSError, KeyError, EOFError):
                pieces = None
            except ValueError:
                pieces = None  # (a cache of another file under this name; a max_seq_len the questions leave no room in is raised again below)
            if pieces is not None and not np.array_equal(pieces.seg_offsets, parsed[1]):
                pieces = None
            if pieces is not None and log is not None:
                log(f"Loaded the reader's evaluation pieces from {cache} ({pieces.n} items, {pieces.n_questions} questions, {pieces.n_passages} passages)")
        if pieces is None:
            if log is not None:
                log(f"Preparing the dev set once for the reader as pieces ({len(parsed[0])} items, {workers} workers)...")
            pieces = cls.from_file(predict_file, tokenizer, max_seq_len, max_q_len, batch_size, workers=workers, records=parsed)
            try:
                pieces.save(cache, tag=tag)
            except OSError:
                pass  # a read-only data directory: the pieces are rebuilt next time
        return pieces

    def to(self, device):
        qt = np.zeros((max(1, self.n_questions), max(1, self.longest_q)), np.int64)
        for i, q in enumerate(self.q_ids):
            qt[i, :len(q)] = q
        self.passages.to(device)
        self.dev = {"q_ids": _to_device(qt, device, torch.int64), "q_lens": _to_device(self.q_lens, device, torch.int64),
                    "chains": _to_device(self.items[:, 1:3].astype(np.int64), device, torch.int64),
                    "row_q": _to_device(self.items[:, 0].astype(np.int64), device, torch.int64),
                    "label": _to_device(self.items[:, 3:4].astype(np.int64), device, torch.int64),
                    "seg_offsets": _to_device(self.seg_offsets, device, torch.int64)}
        return self

    # -- rows -----------------------------------------------------------------------------------------------------------------------------
    def batch_shape(self, lo, hi):
        """(L_b, S_b) of the padded batch qa_collate builds for items lo .. hi - 1, from host metadata only."""
        return (int(self.lens[lo:hi].max()), int(self.n_sents[lo:hi].max())) if hi > lo else (1, 0)

    def assemble_host(self, lo, hi):
        """numpy statement of assemble(lo, hi): qa_arena.assemble_host's dict plus label [R, 1]."""
        L, S = self.batch_shape(lo, hi)
        out = qa_arena.assemble_host(self.passages, self.q_ids, self.items[lo:hi, 1:3], self.items[lo:hi, 0], self.special, self.max_seq_len, L, S)
        out["label"] = self.items[lo:hi, 3:4].astype(np.int64)
        return out

    def assemble(self, lo, hi):
        """The net_inputs of the host path's batch of items lo .. hi - 1, written on the device by mdr_reader_assemble: int64 input_ids,
        attention_mask, token_type_ids, paragraph_mask [R, L_b], sent_offsets [R, S_b], label [R, 1] (plus para_offsets and lengths [R])."""
        if self.dev is None:
            raise RuntimeError("QAEvalPieces.to(device) first")
        L, S = self.batch_shape(lo, hi)
        d = self.dev
        out = qa_arena.assemble(self.passages, d["q_ids"], d["q_lens"], d["chains"][lo:hi], d["row_q"][lo:hi], self.special, self.max_seq_len, L, S)
        out["label"] = d["label"][lo:hi]
        return out

    # -- the decode of one item -----------------------------------------------------------------------------------------------------------
    def chain_result(self, i, head, s_b, tokenizer, sp_pred, final):
        """(qid, label, answer dict) of item i as qa_data.chain_results gives it for the item's row of its batch: prepare() on that chain,
        now, and the one-row batch end2end.select_and_decode builds. head: start, end (ints), span_score, rank_score (Python floats),
        sp_prob (the row of the score table, or None); s_b: the padded sentence count of the item's BATCH, which bounds _pred_sp's index."""
        rec = self.records[i]
        ann = qa_data.prepare({"passages": rec["passages"]}, tokenizer)["context_processed"]
        po = int(self.para_offset[i])
        batch = {"net_inputs": {"label": torch.tensor([[int(rec["label"])]])}, "qids": [rec["qid"]], "para_offsets": [po], "passages": [rec["passages"]],
                 "tok_to_orig_index": [ann["tok_to_orig_index"]], "doc_tokens": [ann["doc_tokens"]],
                 "wp_tokens": [ann["all_doc_tokens"][:self.max_seq_len - po - 1]]}
        one = {"start": [head["start"]], "end": [head["end"]], "span_score": [head["span_score"]], "rank_score": [head["rank_score"]],
               "sp_prob": [list(head["sp_prob"][:s_b])] if head["sp_prob"] is not None else None}
        (out,) = qa_data.chain_results(batch, one, sp_pred, final=final)
        return out


# ---- the score table ---------------------------------------------------------------------------------------------------------------------


class ScoreTable:
    """decode()'s outputs of every item: rank16, span16 (the fp16 patterns, int16), start, end (int64) [n_items], sp_prob fp16
    [n_items, max S_b] (None until a batch brings one; columns at or behind a batch's S_b stay 0 and are never read). batch_sents[b]: S_b."""

    def __init__(self, n_items, max_sents, device):
        self.n, self.max_sents, self.device = int(n_items), int(max_sents), torch.device(device)
        z = lambda dt: torch.zeros(self.n, dtype=dt, device=self.device)  # noqa: E731
        self.rank16, self.span16, self.start, self.end = z(torch.int16), z(torch.int16), z(torch.int64), z(torch.int64)
        self.sp_prob, self.batch_sents, self.batch_lo = None, [], []

    def put(self, lo, head):
        """Copy one batch's decode() outputs to rows lo .. lo + B - 1, on the tensors' device and stream: nothing is read back."""
        n = int(head["start"].shape[0])
        for name in ("rank_score", "span_score"):
            if head[name].dtype != torch.float16:
                raise ValueError(f"{name} is {head[name].dtype}: the score table keeps fp16 patterns")
        self.rank16[lo:lo + n].copy_(head["rank_score"].reshape(-1).view(torch.int16))
        self.span16[lo:lo + n].copy_(head["span_score"].reshape(-1).view(torch.int16))
        self.start[lo:lo + n].copy_(head["start"].reshape(-1))
        self.end[lo:lo + n].copy_(head["end"].reshape(-1))
        sp = head.get("sp_prob")
        s_b = 0
        if sp is not None:
            s_b = int(sp.shape[1])
            if self.sp_prob is None:
                self.sp_prob = torch.zeros((self.n, self.max_sents), dtype=torch.float16, device=self.device)
            self.sp_prob[lo:lo + n, :s_b].copy_(sp)
        self.batch_lo.append(lo)
        self.batch_sents.append(s_b)

    def sents_of(self, i):
        """S_b of the batch that holds item i."""
        return self.batch_sents[int(np.searchsorted(np.asarray(self.batch_lo), i, side="right")) - 1]


def batch_deal(n_batches, N):
    """[(first, behind)] * N: the contiguous run of whole batches each of N ranks decodes (dist.slice_bounds over the batches: balanced,
    in rank order, empty only when there are fewer batches than ranks). Batches are dealt, never rows: a batch stays the host path's, so the
    forward's kernel choice, and with it every bit, is the one-rank run's."""
    from .dist import slice_bounds
    return slice_bounds(n_batches, N)


def merge_tables(local, batches, world):
    """The complete ScoreTable from the ranks' partial ones. `local`: this rank's table of all n rows, of which it filled the
    batches batch_deal(len(batches), N)[rank]; `batches`: every (lo, hi) in order. The ranks' row ranges are contiguous and in rank order, so
    the merge is a concatenation: one gather_objects (each rank's batch_lo, batch_sents and whether it keeps sp_prob) and one gather_rows of
    [rows, 4 + max_sents] fp32 -- the int16 patterns as integers, positions up to 512 and fp16 probabilities are all exact there. The result
    is a fresh table filled by put() batch by batch in file order, as one rank fills it: nothing but a batch's own rows and its first S_b
    sp_prob columns is taken from anybody, and batch_lo and batch_sents come out as put() writes them."""
    deal = batch_deal(len(batches), world.size)
    edges = [lo for lo, _ in batches] + [local.n]
    bounds = [(edges[a], edges[b]) for a, b in deal]
    a, b = deal[world.rank]
    if list(local.batch_lo) != [lo for lo, _ in batches[a:b]]:
        raise ValueError(f"rank {world.rank} of {world.size} decodes batches {a} .. {b} and its table holds the batches at rows {local.batch_lo}")
    told = world.gather_objects((list(local.batch_lo), list(local.batch_sents), local.sp_prob is not None))
    batch_lo, batch_sents = [x for t in told for x in t[0]], [x for t in told for x in t[1]]
    has_sp = any(t[2] for t in told)
    if batch_lo != edges[:-1]:
        raise ValueError("the ranks' batches do not add up to the file's: they do not evaluate the same pieces")
    lo, hi = bounds[world.rank]
    cols = [local.rank16[lo:hi].float(), local.span16[lo:hi].float(), local.start[lo:hi].float(), local.end[lo:hi].float()]
    mine = torch.stack(cols, 1) if hi > lo else torch.zeros((0, 4), dtype=torch.float32, device=local.device)
    if has_sp and local.max_sents:
        sp = local.sp_prob[lo:hi].float() if local.sp_prob is not None else torch.zeros((hi - lo, local.max_sents), dtype=torch.float32, device=local.device)
        mine = torch.cat([mine, sp], 1)
    full = world.gather_rows(mine.contiguous(), bounds)
    merged = ScoreTable(local.n, local.max_sents, local.device)
    for (b_lo, b_hi), s_b in zip(batches, batch_sents):
        head = {"rank_score": full[b_lo:b_hi, 0].to(torch.int16).view(torch.float16), "span_score": full[b_lo:b_hi, 1].to(torch.int16).view(torch.float16),
                "start": full[b_lo:b_hi, 2].to(torch.int64), "end": full[b_lo:b_hi, 3].to(torch.int64)}
        if has_sp:
            head["sp_prob"] = full[b_lo:b_hi, 4:4 + s_b].to(torch.float16)
        merged.put(b_lo, head)
    return merged


def score_table(model, pieces, max_ans_len, world=None):
    """The arena sweep: every batch assembled on the device, decoded, its outputs kept in a ScoreTable. world (a dist.TorchWorld or a rank of
    dist.LoopbackWorld): this rank decodes its run of batches (batch_deal) and merge_tables hands every rank the complete table."""
    table = ScoreTable(pieces.n, pieces.max_sents, pieces.dev["chains"].device)
    first, behind = (0, len(pieces.batches)) if world is None else batch_deal(len(pieces.batches), world.size)[world.rank]
    for lo, hi in pieces.batches[first:behind]:
        rows = pieces.assemble(lo, hi)
        table.put(lo, model.decode({k: rows[k] for k in ("input_ids", "attention_mask", "token_type_ids", "paragraph_mask", "sent_offsets", "label")},
                                   max_ans_len))
    return table if world is None else merge_tables(table, pieces.batches, world)


# ---- evaluation on the winners -----------------------------------------------------------------------------------------------------------


class Winners:
    """The selection of one evaluation and the decode of its distinct winners: winners [n_q, n_lambda], rank_top [n_q] on the host (the
    flagged questions' rows filled in by select_sweep_host on their own scores), answers = {item: (qid, label, answer dict)}."""

    def __init__(self, pieces, table, lambdas, tokenizer, sp_pred, final, host=False):
        seg = pieces.seg_offsets
        if host:  # the tests' host half: the numpy statement of the kernel on a table that lives on the host
            winners, rank_top, flags = select_host(table.rank16.numpy(), table.span16.numpy(), seg, lambdas)
        else:
            picked = select(table.rank16, table.span16, pieces.dev["seg_offsets"], lambdas)
            flat = torch.cat([t.reshape(-1) for t in picked]).cpu().numpy()  # the one read-back of the selection
            n_q, K = len(seg) - 1, len(lambdas)
            winners, rank_top, flags = flat[:n_q * K].reshape(n_q, K).copy(), flat[n_q * K:n_q * K + n_q].copy(), flat[n_q * K + n_q:]
        for j in np.nonzero(flags)[0]:  # a non-finite score: the literal sorts, on this question's two score lists alone
            lo, hi = int(seg[j]), int(seg[j + 1])
            w, r = select_sweep_host(table.rank16[lo:hi].cpu().numpy(), table.span16[lo:hi].cpu().numpy(), [0, hi - lo], lambdas)
            winners[j], rank_top[j] = w[0] + lo, r[0] + lo
        self.winners, self.rank_top, self.flagged = winners, rank_top, int(np.count_nonzero(flags))
        chosen = np.unique(winners[winners >= 0]).astype(np.int64)
        self.answers = {}
        if len(chosen):
            at = torch.from_numpy(chosen).to(table.device)
            cols = [table.start.index_select(0, at).double(), table.end.index_select(0, at).double(),
                    table.rank16.index_select(0, at).view(torch.float16).double(), table.span16.index_select(0, at).view(torch.float16).double()]
            if table.sp_prob is not None:
                cols.append(table.sp_prob.index_select(0, at).double().reshape(len(chosen), -1))
            got = torch.cat([c.reshape(len(chosen), -1) for c in cols], 1).cpu()  # one copy: every value is exact in fp64
            start, end = got[:, 0].long().tolist(), got[:, 1].long().tolist()
            rank, span = got[:, 2].tolist(), got[:, 3].tolist()
            sp = got[:, 4:].tolist() if table.sp_prob is not None else None
            for n, i in enumerate(chosen.tolist()):
                head = {"start": start[n], "end": end[n], "rank_score": rank[n], "span_score": span[n], "sp_prob": sp[n] if sp is not None else None}
                self.answers[i] = pieces.chain_result(i, head, table.sents_of(i), tokenizer, sp_pred, final)
        self.distinct = len(chosen)


def predict_metrics(pieces, table, tokenizer, sp_pred, logger, fixed_thresh=None, host=False):
    """qa_data.predict_metrics's return value and log lines from the score table: (metrics dict, best_res)."""
    lambdas = qa_data.combination_factors(fixed_thresh)
    w = Winners(pieces, table, lambdas, tokenizer, sp_pred, final=False, host=host)
    acc = [int(pieces.items[w.rank_top[pieces.q_row[qid]], 3]) == 1 for qid in pieces.qids]
    top = lambda k, lambda_, qid: w.answers[int(w.winners[pieces.q_row[qid], k])][2]  # noqa: E731
    return qa_data.metrics_report(pieces.qids, acc, lambdas, top, pieces.gold, sp_pred, logger)


def final_results(pieces, table, tokenizer, sp_pred, weight=0.8, host=False):
    """qa_data.final_results's dict from the score table."""
    w = Winners(pieces, table, [weight], tokenizer, sp_pred, final=True, host=host)
    return qa_data.final_report(pieces.qids, lambda qid: w.answers[int(w.winners[pieces.q_row[qid], 0])][2])
