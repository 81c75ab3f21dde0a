"""The retriever's training token arena: every sequence MhopDataset / MhopTrainDataset.__getitem__ can encode, tokenised ONCE and kept on the
device as flat integer rows, so that a step's six padded (ids, mask) pairs are built by one kernel launch (libmdrhip.so: mdr_mhop_assemble,
include/mdr_mhop_train.h) from that step's choices instead of six tokenizer calls per sample on the host, every step, in the training
process. What qa_train_arena.QATrainArena is for the reader.

Rows. tokens int32 under offsets int64 [n_rows + 1]; a row is one final encoded sequence, already cut (the three cuts are fixed for a run):
    one q row per sample                 mhop_data._single(question, max_q_len), the one trailing "?" stripped
    one row per DISTINCT passage         mhop_data._pair(title.strip(), text.strip(), max_c_len) over every sample's pos_paras and neg_paras
    q_sp rows                            mhop_data._pair(question, start passage's stripped text, max_q_sp_len): one for a bridge sample, TWO
                                         for a comparison sample, one for each positive the shuffle may put first
encoded in batches by the encoders mhop_data uses (data.encode_pairs_2_11, data.prefix_space_2_11). Building draws nothing from any
generator and shuffles nothing; the samples are the dataset instance's own (`select()`: tfidf_neg for neg_paras, fewer than two negatives
dropped, a sample without the key keeps its neg_paras).

Per sample: q_row [N]; pos_rows [N, 2], the passage rows of pos_paras in FILE order; start [N], which positive a bridge sample starts from
(-1 for a comparison sample); qsp_rows [N, 2], the q_sp row for a start at positive 0 / 1 (a bridge sample: its one row, then -1);
neg_rows under neg_index [N + 1]. The host keeps all of it and every row's length.

choose(indices) makes __getitem__'s draws, in its order, on the global `random` module: a comparison sample shuffles its two-element
positive order (at eval time too), then, on the train branch, every sample shuffles its negative order and takes the first two. Both orders
are per-sample lists of small integers shuffled IN PLACE AND KEPT, as the dataset's lists are, and random.shuffle's draws depend on the
list's length alone: after any sequence of reads the orders and the generator's state are the host feed's. It returns the [B, 6] row table
(q, q_sp, c1, c2, neg1, neg2) and the six widths mhop_collate would pad to, from host metadata.

Cached as `<data file>.mhop_arena.npz` under mhop_arena_tag(); another tag means a rebuild, never a reuse.
"""
import ctypes
import os
import random
import time

import numpy as np
import torch

from . import _lib
from .arena import _to_device, arena_tag
from .data import encode_pairs_2_11, is_roberta_family, prefix_space_2_11

_c = ctypes
RULE = "mhop-arena-v1"  # the rows and the per-sample arrays of the module docstring
SLOTS = ("q", "q_sp", "c1", "c2", "neg1", "neg2")
KEYS = tuple(f"{s}_{kind}" for s in SLOTS for kind in ("input_ids", "mask"))  # mhop_collate's keys, in its order
ENCODE_BLOCK = 4096  # sequences per tokenizer call
RING = 4             # pinned staging tables of a feed
_ARRAYS = (("tokens", np.int32), ("offsets", np.int64), ("q_row", np.int32), ("pos_rows", np.int32), ("start", np.int32), ("qsp_rows", np.int32),
           ("neg_index", np.int64), ("neg_rows", np.int32))


class Arena(ctypes.Structure):
    _fields_ = [("tokens_dev", _c.c_void_p), ("offsets_dev", _c.c_void_p), ("n_rows", _c.c_int64)]


# include/mdr_mhop_train.h -- bound here, apart from every other header's table
SIGNATURES = {
    "mdr_mhop_assemble": (_c.c_int, [_c.POINTER(Arena), _c.c_void_p, _c.c_int, _c.POINTER(_c.c_int32), _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                     _c.c_int, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
lib = _lib.binder(SIGNATURES)


def require_roberta(tokenizer):
    if not is_roberta_family(tokenizer):
        raise TypeError(f"the retriever's token arena serves RoBERTa-family tokenizers only (data.encode_pairs_2_11 restates their pair template), "
                        f"not {tokenizer.__class__.__name__}: feed such a run from the host (train(..., feed=\"host\"))")


def mhop_arena_tag(tokenizer, max_q_len, max_q_sp_len, max_c_len, train, data_file=None):
    """What a cached arena is valid for: the rule, the tokenizer (arena.arena_tag: class, vocabulary, the 2.11 switches), the three cuts, the
    branch and the data file's size and mtime."""
    st = os.stat(data_file) if data_file is not None else None
    return (f"{RULE}|{arena_tag(tokenizer, False, None)}|max_q_len={int(max_q_len)}|max_q_sp_len={int(max_q_sp_len)}|max_c_len={int(max_c_len)}|"
            f"branch={'train' if train else 'eval'}|file={'-' if st is None else f'{st.st_size}:{st.st_mtime_ns}'}")


def _blocks(n):
    return ((lo, min(n, lo + ENCODE_BLOCK)) for lo in range(0, n, ENCODE_BLOCK))


def encode_singles(tokenizer, texts, max_len):
    """mhop_data._single for every text, one tokenizer call per block."""
    bos, eos, out = tokenizer.bos_token_id, tokenizer.eos_token_id, []
    for lo, hi in _blocks(len(texts)):
        raw = tokenizer([prefix_space_2_11(t) for t in texts[lo:hi]], add_special_tokens=False, truncation=False)["input_ids"]
        out += [[bos] + list(r[:max(max_len - 2, 0)]) + [eos] for r in raw]
    return out


def encode_pairs(tokenizer, pairs, max_len):
    """mhop_data._pair for every (first, second), one encode_pairs_2_11 call per block."""
    out = []
    for lo, hi in _blocks(len(pairs)):
        out += encode_pairs_2_11(tokenizer, [p[0] for p in pairs[lo:hi]], [p[1] for p in pairs[lo:hi]], max_len, False)[0]
    return out


class MhopArena:
    def __init__(self, tokens, offsets, q_row, pos_rows, start, qsp_rows, neg_index, neg_rows, train):
        """Host arrays. Every index is checked here, once: choose() and the kernel trust them."""
        given = dict(zip((n for n, _ in _ARRAYS), (tokens, offsets, q_row, pos_rows, start, qsp_rows, neg_index, neg_rows)))
        for name, dt in _ARRAYS:
            setattr(self, name, np.ascontiguousarray(given[name], dtype=dt))
        self.train = bool(train)
        self.n_rows, self.n = int(self.offsets.shape[0]) - 1, int(self.q_row.shape[0])
        self.pos_rows, self.qsp_rows = self.pos_rows.reshape(-1, 2), self.qsp_rows.reshape(-1, 2)
        o, N = self.offsets, self.n
        if self.n_rows < 0 or o[0] != 0 or o[-1] != len(self.tokens) or (np.diff(o) < 0).any():
            raise ValueError(f"offsets must be [n_rows + 1], start at 0, not decrease and end at len(tokens) = {len(self.tokens)}")
        ni = self.neg_index
        if ni.shape != (N + 1,) or ni[0] != 0 or ni[-1] != len(self.neg_rows) or (N and int(np.diff(ni).min()) < 2):
            raise ValueError(f"neg_index must be [N + 1], start at 0, end at len(neg_rows) = {len(self.neg_rows)} and give every sample at least two negatives")
        if self.pos_rows.shape != (N, 2) or self.qsp_rows.shape != (N, 2) or self.start.shape != (N,):
            raise ValueError("pos_rows and qsp_rows must be [N, 2] and start [N]")
        if not np.isin(self.start, (-1, 0, 1)).all():
            raise ValueError("start is 0 or 1 for a bridge sample and -1 for a comparison sample")
        used = np.concatenate([self.q_row, self.pos_rows.reshape(-1), self.neg_rows, self.qsp_rows[:, 0], self.qsp_rows[self.start < 0, 1]])
        if used.size and (int(used.min()) < 0 or int(used.max()) >= self.n_rows):
            raise ValueError(f"a sample names a row outside [0, {self.n_rows})")
        self.lens = np.diff(o)
        # the two orders choose() shuffles in place and keeps, as the dataset keeps its shuffled lists
        self.pos_order = [[0, 1] for _ in range(N)]
        self.neg_order = [list(range(int(ni[i + 1] - ni[i]))) for i in range(N)]
        # per sample, as plain Python for choose()'s loop: (q row, its q_sp row or two, its two positives' rows, its negatives' rows)
        self._start = self.start.tolist()
        self._rows = [(q, qsp[:2 if s < 0 else 1], pos, self.neg_rows[ni[i]:ni[i + 1]].tolist())
                      for i, (q, qsp, pos, s) in enumerate(zip(self.q_row.tolist(), self.qsp_rows.tolist(), self.pos_rows.tolist(), self._start))]
        self.dev = None
        self.build_seconds = None

    # -- builders -------------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_dataset(cls, ds, tokenizer=None):
        """From an instance of mhop_data.MhopDataset / MhopTrainDataset that has not been read yet: its samples (select()'s rules), its cuts,
        its branch. Nothing of the dataset is changed and no generator is drawn from."""
        tok = tokenizer if tokenizer is not None else ds.tokenizer
        require_roberta(tok)
        t0 = time.perf_counter()
        questions, passages, passage_row, qsp_pairs = [], [], {}, []
        pos_rows, start, qsp_at, neg_rows, neg_counts = [], [], [], [], []

        def passage(para):
            key = (para["title"].strip(), para["text"].strip())
            if key not in passage_row:
                passage_row[key] = len(passages)
                passages.append(key)
            return passage_row[key]

        for i, sample in enumerate(ds.data):
            q = sample["question"]
            q = q[:-1] if q.endswith("?") else q
            questions.append(q)
            pos, negs = sample["pos_paras"], sample["neg_paras"]
            if len(pos) != 2 or len(negs) < 2:
                raise ValueError(f"sample {i}: __getitem__ needs two pos_paras and at least two neg_paras, got {len(pos)} and {len(negs)}")
            pos_rows.append([passage(p) for p in pos])
            if sample["type"] == "comparison":
                start.append(-1)
                starts = (0, 1)
            else:
                s = [k for k, p in enumerate(pos) if p["title"] != sample["bridge"]]
                if len(s) != 1:
                    raise ValueError(f"sample {i}: exactly one of the two pos_paras must carry the bridge title {sample['bridge']!r}")
                start.append(s[0])
                starts = (s[0],)
            qsp_at.append([len(qsp_pairs) + k for k in range(len(starts))] + [-1] * (2 - len(starts)))
            qsp_pairs += [(q, pos[k]["text"].strip()) for k in starts]
            neg_rows += [passage(p) for p in negs]
            neg_counts.append(len(negs))
        rows = encode_singles(tok, questions, ds.max_q_len) + encode_pairs(tok, passages, ds.max_c_len) + encode_pairs(tok, qsp_pairs, ds.max_q_sp_len)
        N, P = len(questions), len(passages)
        offsets = np.zeros(len(rows) + 1, np.int64)
        offsets[1:] = np.cumsum([len(r) for r in rows])
        tokens = np.fromiter((t for r in rows for t in r), np.int32, int(offsets[-1]))
        neg_index = np.zeros(N + 1, np.int64)
        neg_index[1:] = np.cumsum(neg_counts)
        qsp_at = np.asarray(qsp_at, np.int64).reshape(-1, 2)
        # the rows stand in the order questions, passages, q_sp pairs
        arena = cls(tokens, offsets, np.arange(N), np.asarray(pos_rows, np.int64).reshape(-1, 2) + N, np.asarray(start, np.int64).reshape(-1),
                    np.where(qsp_at >= 0, qsp_at + N + P, -1), neg_index, np.asarray(neg_rows, np.int64) + N, ds.train)
        arena.build_seconds = time.perf_counter() - t0
        return arena

    def save(self, path, tag=""):
        tmp = path + f".tmp{os.getpid()}.npz"  # written under another name and renamed: a reader never sees a partial file
        np.savez(tmp, tag=np.array(str(tag)), train=np.array(self.train), **{n: getattr(self, n) for n, _ in _ARRAYS})
        os.replace(tmp, path)

    @classmethod
    def load(cls, path, expect_tag=None):
        """None when the file carries no tag or another one (the caller rebuilds)."""
        z = dict(np.load(path))
        if expect_tag is not None and ("tag" not in z or str(z["tag"]) != str(expect_tag)):
            return None
        return cls(*(z[n] for n, _ in _ARRAYS), train=bool(z["train"]))

    @classmethod
    def load_or_build(cls, path, dataset, tokenizer):
        """`<path>.mhop_arena.npz` when its tag is this tokenizer's, these cuts', this branch's and this file's and it holds len(dataset)
        samples; else a fresh build written there. `path` is the data file `dataset` was read from. Says what it did on stdout, as the
        dataset's own `Loading data from ...` does."""
        require_roberta(tokenizer)
        cache = path + ".mhop_arena.npz"
        tag = mhop_arena_tag(tokenizer, dataset.max_q_len, dataset.max_q_sp_len, dataset.max_c_len, dataset.train, path)
        arena = None
        if os.path.exists(cache):
            try:
                arena = cls.load(cache, expect_tag=tag)
            except (OSError, ValueError, KeyError, EOFError):
                arena = None
            if arena is not None and arena.n != len(dataset):
                arena = None
            if arena is not None:
                print(f"Loaded the token arena {cache} ({arena.n} samples, {arena.n_rows} rows)")
        if arena is None:
            print(f"Tokenising {path} once into a token arena ({len(dataset)} samples)...")
            arena = cls.from_dataset(dataset, tokenizer)
            print(f"Token arena: {arena.n_rows} rows, {arena.bytes_per_sample:.0f} bytes a sample, built in {arena.build_seconds:.2f} s")
            try:
                arena.save(cache, tag=tag)
            except OSError as e:
                print(f"The token arena is not cached ({cache}: {e.strerror or e}): it is rebuilt next time")
        return arena

    def to(self, device):
        self.dev = {n: _to_device(getattr(self, n), device, torch.int32 if dt is np.int32 else torch.int64) for n, dt in _ARRAYS}
        return self

    @property
    def bytes_per_sample(self):
        return sum(getattr(self, n).nbytes for n, _ in _ARRAYS) / max(1, self.n)

    # -- the step's choices (host) ---------------------------------------------------------------------------------------------------------
    def draw(self, i):
        """One read of sample i: __getitem__'s draws on the global `random` module, in its order. Returns (the start positive, the first
        negative, the second negative) as places in the sample's pos_paras and neg_paras of the file."""
        s = self._start[i]
        if s < 0:
            random.shuffle(self.pos_order[i])  # the global generator, in place, at eval time too
            s = self.pos_order[i][0]
        negs = self.neg_order[i]
        if self.train:
            random.shuffle(negs)  # behind the comparison shuffle: the two draw from one generator
        return s, negs[0], negs[1]

    def choose(self, indices):
        """(table int32 [B, 6] of row ids in SLOTS order, the six widths) for the samples `indices`, one draw() each in batch order."""
        lines = []
        for i in (int(i) for i in indices):
            if not 0 <= i < self.n:
                raise IndexError(f"sample {i} of {self.n}")
            s, n1, n2 = self.draw(i)
            q, qsp, pos, negs = self._rows[i]
            lines.append((q, qsp[s if len(qsp) == 2 else 0], pos[s], pos[1 - s], negs[n1], negs[n2]))
        table = np.array(lines, np.int32).reshape(-1, 6)
        return table, self.widths(table)

    def widths(self, table):
        """Each slot's longest row in the batch: the widths mhop_collate pads to (at least 1; a row id outside the arena is an empty row)."""
        table = np.asarray(table).reshape(-1, 6)
        if not len(table):
            return (1,) * 6
        ok = (table >= 0) & (table < self.n_rows)
        lens = np.where(ok, self.lens[np.where(ok, table, 0)], 0) if self.n_rows else np.zeros(table.shape, np.int64)
        return tuple(max(1, int(w)) for w in lens.max(0))

    def assemble_host(self, table, widths, pad_id=0):
        """numpy statement of what mdr_mhop_assemble writes (the yardstick of the kernel): the twelve int64 arrays under KEYS. With
        choose()'s widths and pad_id 0 they are mhop_collate's, which pads with 0 whatever its pad_id argument says."""
        table = np.asarray(table).reshape(-1, 6)
        out = {}
        for k, slot in enumerate(SLOTS):
            W = int(widths[k])
            ids, mask = np.full((len(table), W), pad_id, np.int64), np.zeros((len(table), W), np.int64)
            for b, r in enumerate(table[:, k]):
                if 0 <= r < self.n_rows:
                    row = self.tokens[self.offsets[r]:self.offsets[r + 1]][:W]
                    ids[b, :len(row)] = row
                    mask[b, :len(row)] = 1
            out[f"{slot}_input_ids"], out[f"{slot}_mask"] = ids, mask
        return out

    # -- the device op --------------------------------------------------------------------------------------------------------------------
    def assemble(self, table_dev, widths, pad_id=0, out=None):
        """table_dev int32 cuda [B, 6] -> the dict of int64 cuda tensors under KEYS, one kernel launch on the current stream. `out`: a dict of
        preallocated contiguous tensors of exactly those shapes to write into (the tests' guarded buffers)."""
        if self.dev is None:
            raise RuntimeError("MhopArena.to(device) first")
        dev = self.dev["offsets"].device
        if not (torch.is_tensor(table_dev) and table_dev.device == dev and table_dev.dtype == torch.int32 and table_dev.dim() == 2
                and table_dev.shape[1] == 6 and table_dev.is_contiguous()):
            raise ValueError("the row table must be a contiguous int32 [B, 6] tensor on the arena's device")
        widths = [int(w) for w in widths]
        if len(widths) != 6 or min(widths) < 1:
            raise ValueError(f"widths = {widths}: six widths, each >= 1")
        B = int(table_dev.shape[0])
        shapes = {f"{slot}_{kind}": (B, widths[k]) for k, slot in enumerate(SLOTS) for kind in ("input_ids", "mask")}
        if out is None:
            out = {k: torch.empty(s, dtype=torch.int64, device=dev) for k, s in shapes.items()}
        else:
            for k, s in shapes.items():
                if not _lib.is_like(out[k], (torch.int64,), s, dev):
                    raise ValueError(f"out[{k!r}] is {_lib.describe(out[k])}, not a contiguous int64 {s} on {dev}")
        a = Arena(_lib.ptr(self.dev["tokens"]), _lib.ptr(self.dev["offsets"]), self.n_rows)
        ids = (_c.c_void_p * 6)(*(out[f"{s}_input_ids"].data_ptr() for s in SLOTS))
        mask = (_c.c_void_p * 6)(*(out[f"{s}_mask"].data_ptr() for s in SLOTS))
        _lib.call(lib().mdr_mhop_assemble, ctypes.byref(a), _lib.ptr(table_dev), B, (_c.c_int32 * 6)(*widths), ids, mask, int(pad_id), dev=dev)  # B == 0: a no-op
        return out

    def feed(self, batch_size, shuffle, rank_rows=None):
        return Feed(self, batch_size, shuffle, rank_rows)


class Feed:
    """The device batches of one arena, an iterable with len(). The index order comes from a torch DataLoader over the bare indices with the
    host feed's batch_size, shuffle and num_workers=0, so torch's global generator is drawn from exactly as the host feed's loader draws (the
    sampler's seed and the iterator's base seed) and len() is that loader's. A step's only host-to-device traffic is its row table, copied
    from one of RING pinned tables; a table is written again only after the event behind its last copy has completed.

    rank_rows: None, or on one rank of several (dist.py) the function from a batch's sample count B to this rank's rows (lo, hi). Every rank
    makes the same draws and builds the same [B, 6] table, so `random` and torch's generator move as on one rank; the rank then assembles its
    rows alone, padded to the FULL table's widths, and the batch says so under train.RANK_ROWS: (lo, hi, B)."""

    def __init__(self, arena, batch_size, shuffle, rank_rows=None):
        if arena.dev is None:
            raise RuntimeError("MhopArena.to(device) first")
        self.arena = arena
        self.loader = torch.utils.data.DataLoader(range(arena.n), batch_size=batch_size, shuffle=shuffle, num_workers=0, collate_fn=list)
        self.device = arena.dev["offsets"].device
        self.ring = [torch.empty((max(1, int(batch_size)), 6), dtype=torch.int32).pin_memory() for _ in range(RING)]
        self.busy = [None] * RING
        self.at = 0
        self.rank_rows = rank_rows

    def __len__(self):
        return len(self.loader)

    def upload(self, table):
        """The table on the device, through the next pinned table of the ring, without blocking the host."""
        k, self.at = self.at, (self.at + 1) % RING
        if self.busy[k] is not None:
            self.busy[k].synchronize()  # the copy that last read this table has completed (long ago: every step ends in loss.item())
        staged = self.ring[k][:len(table)]
        staged.copy_(torch.from_numpy(table))
        with torch.cuda.device(self.device):
            on_dev = staged.to(self.device, non_blocking=True)
            self.busy[k] = torch.cuda.Event()
            self.busy[k].record()
        return on_dev

    def __iter__(self):
        for indices in self.loader:
            table, widths = self.arena.choose(indices)
            if self.rank_rows is None:
                yield self.arena.assemble(self.upload(table), widths)
            else:
                lo, hi = self.rank_rows(len(table))
                batch = self.arena.assemble(self.upload(np.ascontiguousarray(table[lo:hi])), widths)
                batch["_rank_rows"] = (lo, hi, len(table))  # train.RANK_ROWS
                yield batch
