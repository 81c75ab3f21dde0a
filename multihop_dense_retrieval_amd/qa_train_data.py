"""The reader's TRAINING data path on the host, restated from the reference's behaviour (not copied):

    QATrainDataset      mdr/qa/qa_dataset.py QADataset(train=True): __init__ (gold chain + negatives per question) and __getitem__
    MhopSampler         mdr/qa/qa_dataset.py MhopSampler
    qa_train_collate    qa_collate with its training fields (starts, ends, sent_labels, ans_covered)
    SimpleTokenizer, para_has_answer, match_answer_span, find_ans_span_with_char_offsets, _improve_answer_span
                        mdr/qa/basic_tokenizer.py, mdr/qa/utils.py

qa_data.QADataset(train=True) keeps refusing: the training dataset is this class, as mhop_data.MhopTrainDataset is for the retriever.

What is kept because the numbers depend on it (tests/test_qa_train_data.py pins each against the reference's own classes):
  * a negative is a candidate chain whose title SET differs from the gold one; its ans_covered is 1 only for a bridge question and only
    when it shares a title with a gold passage that holds the answer (distant supervision: such a row has real starts); ds_limit is unused;
  * starts / ends: "yes" -> para_offset, "no" -> para_offset + 1, else every occurrence of every matched surface string; a span that starts
    behind the cut is dropped, the end of one that crosses it is clamped to the last kept token; [-1] when nothing is left or ans_covered is 0;
  * sent_labels are zeros of sent_offsets' length for an item without sp_sent_labels (every negative);
  * MhopSampler drops len(qid2gold) % n_gpu questions per epoch with n_gpu = 8 BY DEFAULT (the script never passes it), and its len counts
    neg_num + 1 rows per question even where a question has fewer negatives: len(loader), t_total and the warm-up overstate the real
    step count and the schedule never reaches zero;
  * random.shuffle(neg_samples) shuffles the dataset's own list IN PLACE, so an epoch's negatives depend on every earlier epoch's shuffles;
    all draws come from the global `random` generator.

One deviation. match_answer_span returns list(set(...)) in the reference: with several distinct surface strings (say "London" and "london")
the order of the spans is the set's iteration order, which changes from process to process. Here it is the order of first occurrence. The
loss sums over a row's spans, so it does not depend on the order. A second one: __getitem__ reads the dataset's record and does not write the
tensors back into it (the reference replaces label and ans_covered in place; the values it returns are the same on every call).
"""
import collections
import json
import random
import unicodedata

import torch

from . import qa_data

# ---- SimpleTokenizer and the answer matching -------------------------------------------------------------------------------------------


class SimpleTokenizer:
    """Runs of letters / digits / marks, or any single character that is neither a separator nor a control character. tokenize() returns
    [(text, text followed by the whitespace up to the next token)]."""

    def __init__(self):
        import regex
        self._re = regex.compile(r"([\p{L}\p{N}\p{M}]+)|([^\p{Z}\p{C}])", flags=regex.IGNORECASE + regex.UNICODE + regex.MULTILINE)

    def tokenize(self, text):
        spans = [m.span() for m in self._re.finditer(text)]
        return [(text[s:e], text[s:(spans[i + 1][0] if i + 1 < len(spans) else e)]) for i, (s, e) in enumerate(spans)]


def _words(tokens):
    return [t[0].lower() for t in tokens]


def _nfd(text):
    return unicodedata.normalize("NFD", text)


def para_has_answer(answer, para, tokenizer):
    """Whether any answer occurs in the NFD-normalised paragraph as a run of SimpleTokenizer words, case-insensitively."""
    text = _words(tokenizer.tokenize(_nfd(para)))
    for single in answer:
        single = _words(tokenizer.tokenize(_nfd(single)))
        for i in range(0, len(text) - len(single) + 1):
            if single == text[i:i + len(single)]:
                return True
    return False


def match_answer_span(p, answer, tokenizer):
    """The distinct surface strings of `p` (NOT normalised here, as in the reference) that match an NFD-normalised answer word for word, in
    the order of first occurrence (module docstring)."""
    tokens = tokenizer.tokenize(p)
    text = _words(tokens)
    matched = []
    for single in answer:
        single = _words(tokenizer.tokenize(_nfd(single)))
        for i in range(0, len(text) - len(single) + 1):
            if single == text[i:i + len(single)]:
                s = "".join(t[1] for t in tokens[i:i + len(single)]).strip()
                if s not in matched:
                    matched.append(s)
    return matched


def _improve_answer_span(doc_tokens, input_start, input_end, tokenizer, orig_answer_text):
    tok_answer_text = " ".join(tokenizer.tokenize(orig_answer_text))
    for new_start in range(input_start, input_end + 1):
        for new_end in range(input_end, new_start - 1, -1):
            if " ".join(doc_tokens[new_start:new_end + 1]) == tok_answer_text:
                return new_start, new_end
    return input_start, input_end


def find_ans_span_with_char_offsets(detected_ans, char_to_word_offset, doc_tokens, all_doc_tokens, orig_to_tok_index, tokenizer):
    """One (first, last) WordPiece span per character span of the answer text."""
    out = []
    for char_start, char_end in detected_ans["char_spans"]:
        tok_start, tok_end = char_to_word_offset[char_start], char_to_word_offset[char_end]  # char_end is the answer's last character
        sub_start = orig_to_tok_index[tok_start]
        sub_end = orig_to_tok_index[tok_end + 1] - 1 if tok_end < len(doc_tokens) - 1 else len(all_doc_tokens) - 1
        out.append(_improve_answer_span(all_doc_tokens, sub_start, sub_end, tokenizer, detected_ans["text"]))
    return out


def answer_spans(ann, gold_answer, simple_tok, tokenizer):
    """Every (first, last) WordPiece span, in the uncut chain, of every occurrence of every matched surface string."""
    context = ann["context"]
    spans = []
    for span in match_answer_span(context, gold_answer, simple_tok):
        char_starts = [i for i in range(len(context)) if context.startswith(span, i)]
        if char_starts:
            answer = {"text": span, "char_spans": [(s, s + len(span) - 1) for s in char_starts]}
            spans.extend(find_ans_span_with_char_offsets(answer, ann["char_to_word_offset"], ann["doc_tokens"], ann["all_doc_tokens"],
                                                         ann["orig_to_tok_index"], tokenizer))
    return spans


def cut_spans(spans, n_wp, para_offset, clamp_end=True, drop_cut=True):
    """(starts, ends) in row positions of the spans that start inside the n_wp kept WordPieces, each end clamped to the last kept one; [] []
    when none is left. clamp_end / drop_cut exist for the tests' mutants only."""
    starts, ends = [], []
    for s, e in spans:
        if s >= n_wp and drop_cut:
            continue
        starts.append(min(s, n_wp - 1) + para_offset)
        ends.append((min(e, n_wp - 1) if clamp_end else e) + para_offset)
    return starts, ends


# ---- dataset ----------------------------------------------------------------------------------------------------------------------------


class QATrainDataset(torch.utils.data.Dataset):
    """qa_dataset.py QADataset with train=True. data: one record per gold chain (label 1, ans_covered 1, sp_sent_labels over all sentences of
    the sp passages) followed by that question's negatives (label 0); qid2gold / qid2neg: the records' indices per question."""

    def __init__(self, tokenizer, data_path, max_seq_len, max_q_len, no_sent_label=False):
        self.tokenizer, self.max_seq_len, self.max_q_len, self.no_sent_label = tokenizer, max_seq_len, max_q_len, no_sent_label
        self.simple_tok = SimpleTokenizer()
        self.data = []
        self.qid2gold, self.qid2neg = collections.defaultdict(list), collections.defaultdict(list)
        for item in (json.loads(line) for line in open(data_path).readlines()):
            if item["question"].endswith("?"):
                item["question"] = item["question"][:-1]
            sp_sent_labels, sp_gold = [], []
            if not no_sent_label:
                for sp in item["sp"]:
                    sp_gold.extend([sp["title"], i] for i in sp["sp_sent_ids"])
                    sp_sent_labels.extend(int(idx in sp["sp_sent_ids"]) for idx in range(len(sp["sents"])))
            self.data.append({"question": item["question"], "passages": item["sp"], "label": 1, "qid": item["_id"], "gold_answer": item["answer"],
                              "sp_sent_labels": sp_sent_labels, "ans_covered": 1, "sp_gold": sp_gold})
            self.qid2gold[item["_id"]].append(len(self.data) - 1)
            sp_titles = set(p["title"] for p in item["sp"])
            bridge = item["type"] == "bridge"
            ans_titles = set(p["title"] for p in item["sp"] if para_has_answer(item["answer"], "".join(p["sents"]), self.simple_tok)) if bridge else set()
            for chain in item["candidate_chains"]:
                titles = set(p["title"] for p in chain)
                if titles == sp_titles:
                    continue
                self.data.append({"question": item["question"], "passages": chain, "label": 0, "qid": item["_id"], "gold_answer": item["answer"],
                                  "ans_covered": self.negative_ans_covered(bridge, titles, ans_titles), "sp_gold": sp_gold})
                self.qid2neg[item["_id"]].append(len(self.data) - 1)
        print(f"Data size {len(self.data)}")

    @staticmethod
    def negative_ans_covered(bridge, titles, ans_titles):
        return int(len(titles & ans_titles) > 0) if bridge else 0

    cut_spans = staticmethod(cut_spans)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        item = dict(qa_data.prepare(dict(self.data[index]), self.tokenizer))
        ann = item["context_processed"]
        q_toks = self.tokenizer.tokenize(item["question"])[:self.max_q_len]
        para_offset = len(q_toks) + 2
        wp = ann["all_doc_tokens"]
        assert wp[0] == "yes" and wp[1] == "no"
        wp = wp[:max(0, self.max_seq_len - para_offset - 1)]
        item["wp_tokens"], item["para_offset"] = wp, para_offset
        item["encodings"] = qa_data.encode_pair(self.tokenizer, q_toks, wp)
        item["paragraph_mask"] = torch.zeros(item["encodings"]["input_ids"].size()).view(-1)
        item["paragraph_mask"][para_offset:-1] = 1
        starts, ends = [], []
        if item["ans_covered"]:
            if item["gold_answer"][0] == "yes":
                starts, ends = [para_offset], [para_offset]
            elif item["gold_answer"][0] == "no":
                starts, ends = [para_offset + 1], [para_offset + 1]
            else:
                starts, ends = self.cut_spans(answer_spans(ann, item["gold_answer"], self.simple_tok, self.tokenizer), len(wp), para_offset)
        if not starts:
            starts, ends = [-1], [-1]
        item["starts"], item["ends"] = torch.LongTensor(starts), torch.LongTensor(ends)
        if item["label"]:
            assert len(item["sp_sent_labels"]) == len(ann["sent_starts"])
        unused1 = self.tokenizer.convert_tokens_to_ids("[unused1]")
        sent_labels, sent_offsets = [], []
        for idx, s in enumerate(ann["sent_starts"]):
            if s >= len(wp):
                break
            if "sp_sent_labels" in item:
                sent_labels.append(item["sp_sent_labels"][idx])
            sent_offsets.append(s + para_offset)
            assert item["encodings"]["input_ids"].view(-1)[s + para_offset] == unused1
        item["sent_offsets"] = torch.LongTensor(sent_offsets)
        item["sent_labels"] = torch.LongTensor(sent_labels if len(sent_labels) != 0 else [0] * len(sent_offsets))
        item["ans_covered"] = torch.LongTensor([item["ans_covered"]])
        item["label"] = torch.LongTensor([item["label"]])
        return item


class MhopSampler(torch.utils.data.Sampler):
    """Shuffles the questions, not the chains: per epoch, the first q_num_per_epoch shuffled questions, each as its gold chain followed by
    the first num_neg of its negatives, which are shuffled IN PLACE in the dataset's own list first (module docstring)."""

    def __init__(self, data_source, num_neg=9, n_gpu=8):
        self.qid2gold, self.qid2neg = data_source.qid2gold, data_source.qid2neg
        self.neg_num, self.n_gpu = num_neg, n_gpu
        self.all_qids = list(self.qid2gold.keys())
        assert len(self.qid2gold) == len(self.qid2neg)
        self.q_num_per_epoch = len(self.qid2gold) - len(self.qid2gold) % self.n_gpu
        self._num_samples = self.q_num_per_epoch * (self.neg_num + 1)

    def __len__(self):
        return self._num_samples

    def negatives_of(self, qid):
        neg = self.qid2neg[qid]
        random.shuffle(neg)
        return neg

    def __iter__(self):
        out = []
        random.shuffle(self.all_qids)
        for qid in self.all_qids[:self.q_num_per_epoch]:
            neg = self.negatives_of(qid)
            out += self.qid2gold[qid]
            out += neg[:self.neg_num]
        return iter(out)


def loader_len(sampler, batch_size):
    """len(DataLoader(sampler=sampler, batch_size=batch_size)): from the sampler's len, which overstates the rows (module docstring)."""
    return (len(sampler) + batch_size - 1) // batch_size


def total_steps(sampler, batch_size, gradient_accumulation_steps, num_train_epochs):
    """The reference's t_total: len(train_dataloader) // gradient_accumulation_steps * num_train_epochs (a float: the flag is one)."""
    return loader_len(sampler, batch_size) // gradient_accumulation_steps * num_train_epochs


def epoch_batches(sampler, batch_size):
    """One epoch's index lists in batch_size slices; the last is short, and batches straddle questions."""
    idx = list(iter(sampler))
    return [idx[lo:lo + batch_size] for lo in range(0, len(idx), batch_size)]


def qa_train_collate(samples, pad_id=0):
    """qa_collate of training items: qa_data.qa_collate's fields and, in net_inputs, starts / ends (padded with -1), sent_labels and
    ans_covered (padded with 0)."""
    if len(samples) == 0:
        return {}
    out = qa_data.qa_collate(samples, pad_id=pad_id)
    net = out["net_inputs"]
    net["starts"] = qa_data.collate_tokens([s["starts"] for s in samples], -1)
    net["ends"] = qa_data.collate_tokens([s["ends"] for s in samples], -1)
    net["sent_labels"] = qa_data.collate_tokens([s["sent_labels"] for s in samples], 0)
    net["ans_covered"] = qa_data.collate_tokens([s["ans_covered"] for s in samples], 0)
    return out
