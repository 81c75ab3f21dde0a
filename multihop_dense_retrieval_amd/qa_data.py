"""The reader's CPU data path, restated from the reference (not copied):

    prepare, QADataset (eval branch), QAEvalDataset, qa_collate   mdr/qa/qa_dataset.py:17-107,188-386,424-463
    BasicTokenizer, get_final_text                                mdr/qa/utils.py:145-396
    normalize_answer, f1_score, exact_match_score, update_sp      mdr/qa/hotpot_evaluate_v1.py
    predict / eval_final (the host side of the answer decode)     scripts/train_qa.py:220-481
    add_sp_labels                                                 mdr/retrieval/utils/mhop_utils.py:173-210

Token ids with `is_pretokenized=True`. The reference calls transformers 2.11's
`encode_plus(q_toks, text_pair=wp_tokens, max_length=max_seq_len, is_pretokenized=True)` on lists of WordPiece STRINGS. The one reading
under which its own assert holds (qa_dataset.py:180: the id at `s + para_offset` is `[unused1]`) and under which its decode
(`wp_tokens[start - para_offset]`) indexes the token the model scored is: the sequence is `[CLS] q [SEP] wp [SEP]` with every WordPiece
string mapped to exactly one id (convert_tokens_to_ids, no re-tokenisation), token types 0 up to and including the first `[SEP]` and 1
after it, attention mask all ones. The caller has already cut q_toks to max_q_len and wp_tokens to max_seq_len - len(q) - 3, so
max_length never truncates. `encode_pair` below is that convention.
"""
import collections
import json
import re
import string
import unicodedata

import numpy as np
import torch

# ---- character classes and BasicTokenizer (BERT's) --------------------------------------------------------------------------------------


def _is_whitespace(c):
    return c in (" ", "\t", "\n", "\r") or unicodedata.category(c) == "Zs"


def _is_control(c):
    if c in ("\t", "\n", "\r"):
        return False
    return unicodedata.category(c).startswith("C")


def _is_punctuation(c):
    cp = ord(c)
    if 33 <= cp <= 47 or 58 <= cp <= 64 or 91 <= cp <= 96 or 123 <= cp <= 126:
        return True
    return unicodedata.category(c).startswith("P")


def _whitespace_tokenize(text):
    text = text.strip()
    return text.split() if text else []


class BasicTokenizer:
    """Punctuation splitting, lower casing and accent stripping (get_final_text's view of the original text)."""

    def __init__(self, do_lower_case=True):
        self.do_lower_case = do_lower_case

    def tokenize(self, text):
        if isinstance(text, bytes):
            text = text.decode("utf-8", "ignore")
        text = "".join(" " if _is_whitespace(c) else c for c in text if not (ord(c) in (0, 0xFFFD) or _is_control(c)))
        out = []
        for tok in _whitespace_tokenize(text):
            if self.do_lower_case:
                tok = "".join(c for c in unicodedata.normalize("NFD", tok.lower()) if unicodedata.category(c) != "Mn")
            out.extend(self._split_punc(tok))
        return _whitespace_tokenize(" ".join(out))

    @staticmethod
    def _split_punc(text):
        pieces, new_word = [], True
        for c in text:
            if _is_punctuation(c):
                pieces.append([c])
                new_word = True
            else:
                if new_word:
                    pieces.append([])
                new_word = False
                pieces[-1].append(c)
        return ["".join(p) for p in pieces]


def get_final_text(pred_text, orig_text, do_lower_case=False):
    """Project a WordPiece-detokenised prediction back onto the original words (falls back to orig_text when the alignment fails)."""
    def strip_spaces(text):
        chars, ns_to_s = [], collections.OrderedDict()
        for i, c in enumerate(text):
            if c == " ":
                continue
            ns_to_s[len(chars)] = i
            chars.append(c)
        return "".join(chars), ns_to_s

    tok_text = " ".join(BasicTokenizer(do_lower_case=do_lower_case).tokenize(orig_text))
    start = tok_text.find(pred_text)
    if start == -1:
        return orig_text
    end = start + len(pred_text) - 1
    orig_ns, orig_map = strip_spaces(orig_text)
    tok_ns, tok_map = strip_spaces(tok_text)
    if len(orig_ns) != len(tok_ns):
        return orig_text
    tok_s_to_ns = {ti: i for i, ti in tok_map.items()}
    o_start = orig_map.get(tok_s_to_ns[start]) if start in tok_s_to_ns else None
    if o_start is None:
        return orig_text
    o_end = orig_map.get(tok_s_to_ns[end]) if end in tok_s_to_ns else None
    if o_end is None:
        return orig_text
    return orig_text[o_start:o_end + 1]


# ---- HotpotQA metrics ---------------------------------------------------------------------------------------------------------------


def normalize_answer(s):
    s = s.lower()
    s = "".join(ch for ch in s if ch not in set(string.punctuation))
    s = re.sub(r"\b(a|an|the)\b", " ", s)
    return " ".join(s.split())


def f1_score(prediction, ground_truth):
    p, g = normalize_answer(prediction), normalize_answer(ground_truth)
    zero = (0, 0, 0)
    if p in ("yes", "no", "noanswer") and p != g:
        return zero
    if g in ("yes", "no", "noanswer") and p != g:
        return zero
    pt, gt = p.split(), g.split()
    same = sum((collections.Counter(pt) & collections.Counter(gt)).values())
    if same == 0:
        return zero
    prec, rec = 1.0 * same / len(pt), 1.0 * same / len(gt)
    return (2 * prec * rec) / (prec + rec), prec, rec


def exact_match_score(prediction, ground_truth):
    return normalize_answer(prediction) == normalize_answer(ground_truth)


def update_sp(metrics, prediction, gold):
    pred, gold_ = set(map(tuple, prediction)), set(map(tuple, gold))
    tp = sum(1 for e in pred if e in gold_)
    fp = len(pred) - tp
    fn = sum(1 for e in gold_ if e not in pred)
    prec = 1.0 * tp / (tp + fp) if tp + fp > 0 else 0.0
    rec = 1.0 * tp / (tp + fn) if tp + fn > 0 else 0.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    em = 1.0 if fp + fn == 0 else 0.0
    metrics["sp_em"] += em
    metrics["sp_f1"] += f1
    metrics["sp_prec"] += prec
    metrics["sp_recall"] += rec
    return em, prec, rec


# ---- dataset ----------------------------------------------------------------------------------------------------------------------------

SPECIAL_TOKS = ("[SEP]", "[unused1]", "[unused2]")


def prepare(item, tokenizer, special_toks=SPECIAL_TOKS):
    """"yes no [SEP] " + " [SEP] ".join(title + " [unused1] sent ..."), split on whitespace, WordPiece word by word with the special
    tokens kept whole; records where each [unused1] sentence marker lands."""
    contexts = [p["title"].strip() + " " + " ".join("[unused1] " + s.strip() for s in p["sents"]) for p in item["passages"]]
    context = "yes no [SEP] " + " [SEP] ".join(contexts)
    doc_tokens, char_to_word, prev_ws = [], [], True
    for c in context:
        if _is_whitespace(c):
            prev_ws = True
        else:
            if prev_ws:
                doc_tokens.append(c)
            else:
                doc_tokens[-1] += c
            prev_ws = False
        char_to_word.append(len(doc_tokens) - 1)
    sent_starts, orig_to_tok, tok_to_orig, all_tokens = [], [], [], []
    for i, tok in enumerate(doc_tokens):
        orig_to_tok.append(len(all_tokens))
        if tok in special_toks:
            if tok == "[unused1]":
                sent_starts.append(len(all_tokens))
            subs = [tok]
        else:
            subs = tokenizer.tokenize(tok)
        for s in subs:
            tok_to_orig.append(i)
            all_tokens.append(s)
    item["context_processed"] = {"doc_tokens": doc_tokens, "char_to_word_offset": char_to_word, "orig_to_tok_index": orig_to_tok,
                                 "tok_to_orig_index": tok_to_orig, "all_doc_tokens": all_tokens, "context": context, "sent_starts": sent_starts}
    return item


def encode_pair(tokenizer, q_toks, wp_tokens):
    """[CLS] q [SEP] wp [SEP], one id per WordPiece string; token types 0 through the first [SEP], 1 after (module docstring)."""
    toks = [tokenizer.cls_token] + list(q_toks) + [tokenizer.sep_token] + list(wp_tokens) + [tokenizer.sep_token]
    ids = torch.tensor([tokenizer.convert_tokens_to_ids(toks)], dtype=torch.long)
    tt = torch.zeros_like(ids)
    tt[0, len(q_toks) + 2:] = 1
    return {"input_ids": ids, "token_type_ids": tt, "attention_mask": torch.ones_like(ids)}


class _EvalItems(torch.utils.data.Dataset):
    """__getitem__ of the eval branch, shared by QADataset(train=False) and QAEvalDataset (they are the same code in the reference)."""

    def __len__(self):
        return len(self.data)

    def __getitem__(self, index):
        item = prepare(self.data[index], self.tokenizer)
        ann = item["context_processed"]
        q_toks = self.tokenizer.tokenize(item["question"])[:self.max_q_len]
        para_offset = len(q_toks) + 2
        item["wp_tokens"] = ann["all_doc_tokens"]
        assert item["wp_tokens"][0] == "yes" and item["wp_tokens"][1] == "no"
        item["para_offset"] = para_offset
        max_toks_for_doc = self.max_seq_len - para_offset - 1
        if len(item["wp_tokens"]) > max_toks_for_doc:
            item["wp_tokens"] = item["wp_tokens"][:max_toks_for_doc]
        item["encodings"] = encode_pair(self.tokenizer, q_toks, item["wp_tokens"])
        item["paragraph_mask"] = torch.zeros(item["encodings"]["input_ids"].size()).view(-1)
        item["paragraph_mask"][para_offset:-1] = 1
        item["doc_tokens"] = ann["doc_tokens"]
        item["tok_to_orig_index"] = ann["tok_to_orig_index"]
        unused1 = self.tokenizer.convert_tokens_to_ids("[unused1]")
        offsets = []
        for s in ann["sent_starts"]:
            if s >= len(item["wp_tokens"]):
                break
            offsets.append(s + para_offset)
            assert item["encodings"]["input_ids"].view(-1)[s + para_offset] == unused1
        item["sent_offsets"] = torch.LongTensor(offsets)
        item["label"] = torch.LongTensor([item["label"]])
        return item


class QADataset(_EvalItems):
    """qa_dataset.py QADataset with train=False: one item per candidate chain, label 1 if its titles are the gold sp titles."""

    def __init__(self, tokenizer, data_path, max_seq_len, max_q_len, train=False, no_sent_label=False):
        if train:
            raise NotImplementedError("training is not supported: the reader runs inference only")
        self.tokenizer, self.max_seq_len, self.max_q_len = tokenizer, max_seq_len, max_q_len
        self.data = []
        for item in (json.loads(line) for line in open(data_path).readlines()):
            if item["question"].endswith("?"):
                item["question"] = item["question"][:-1]
            sp_titles = set(p["title"] for p in item["sp"]) if "sp" in item else None
            sp_gold = [[sp["title"], i] for sp in item.get("sp", []) for i in sp["sp_sent_ids"]]
            for chain in item["candidate_chains"]:
                label = int(set(p["title"] for p in chain) == sp_titles) if sp_titles else -1
                self.data.append({"question": item["question"], "passages": chain, "label": label, "qid": item["_id"],
                                  "gold_answer": item.get("answer", []), "sp_gold": sp_gold})
        print(f"Data size {len(self.data)}")


class QAEvalDataset(_EvalItems):
    """qa_dataset.py QAEvalDataset: retrieval results in memory, no gold (label -1)."""

    def __init__(self, tokenizer, retrievel_results, max_seq_len, max_q_len):
        self.tokenizer, self.max_seq_len, self.max_q_len = tokenizer, max_seq_len, max_q_len
        self.data = []
        for item in retrievel_results:
            if item["question"].endswith("?"):
                item["question"] = item["question"][:-1]
            for chain in item["candidate_chains"]:
                self.data.append({"question": item["question"], "passages": chain, "label": -1, "qid": item["_id"],
                                  "gold_answer": item.get("answer", []), "sp_gold": []})
        print(f"Total instances size {len(self.data)}")


def collate_tokens(values, pad_idx):
    values = [v.view(-1) for v in values]
    size = max(v.size(0) for v in values)
    res = values[0].new(len(values), size).fill_(pad_idx)
    for i, v in enumerate(values):
        res[i][:len(v)].copy_(v)
    return res


def qa_collate(samples, pad_id=0):
    if len(samples) == 0:
        return {}
    batch = {"input_ids": collate_tokens([s["encodings"]["input_ids"] for s in samples], pad_id),
             "attention_mask": collate_tokens([s["encodings"]["attention_mask"] for s in samples], 0),
             "paragraph_mask": collate_tokens([s["paragraph_mask"] for s in samples], 0),
             "label": collate_tokens([s["label"] for s in samples], -1),
             "sent_offsets": collate_tokens([s["sent_offsets"] for s in samples], 0)}
    if "token_type_ids" in samples[0]["encodings"]:
        batch["token_type_ids"] = collate_tokens([s["encodings"]["token_type_ids"] for s in samples], 0)
    out = {"qids": [s["qid"] for s in samples], "passages": [s["passages"] for s in samples], "gold_answer": [s["gold_answer"] for s in samples],
           "sp_gold": [s["sp_gold"] for s in samples], "para_offsets": [s["para_offset"] for s in samples], "net_inputs": batch}
    if "doc_tokens" in samples[0]:
        out["doc_tokens"] = [s["doc_tokens"] for s in samples]
        out["tok_to_orig_index"] = [s["tok_to_orig_index"] for s in samples]
        out["wp_tokens"] = [s["wp_tokens"] for s in samples]
    return out


# ---- answer decode and metrics (the host side of predict() / eval_final()) -----------------------------------------------------------


def _answer_text(batch, idx, start, end):
    t2o, doc, wp = batch["tok_to_orig_index"][idx], batch["doc_tokens"][idx], batch["wp_tokens"][idx]
    orig_tokens = doc[t2o[start]:t2o[end] + 1]
    tok_text = " ".join(wp[start:end + 1]).replace(" ##", "").replace("##", "").strip()
    tok_text = " ".join(tok_text.split())
    return get_final_text(tok_text, " ".join(orig_tokens), do_lower_case=True).strip()


def _pred_sp(batch, idx, sp_prob, strict):
    """Sentences of the FIRST TWO passages with probability >= 0.5 (predict) or > 0.5 (eval_final); an index past the row's
    sentence slots is skipped (the reference's bare except)."""
    pred, passages = [], batch["passages"][idx]
    for passage, base in zip(passages, [0, len(passages[0]["sents"])]):
        for j, _ in enumerate(passage["sents"]):
            if j + base < len(sp_prob):
                p = sp_prob[j + base]
                if (p > 0.5) if strict else (p >= 0.5):
                    pred.append([passage["title"], j])
    return pred


def chain_results(batch, head, sp_pred, final=False):
    """Per chain of one batch: (qid, label, rank_score, answer dict) from the device outputs `head` = {'start', 'end' (positions in the
    padded row), 'span_score', 'rank_score', 'sp_prob'} as python lists (decode()'s or the reference's formula's). final: eval_final()'s
    variant (sp threshold > 0.5 instead of >= 0.5, chain titles kept)."""
    labels = batch["net_inputs"]["label"].view(-1).tolist()
    out = []
    for idx, qid in enumerate(batch["qids"]):
        start = head["start"][idx] - batch["para_offsets"][idx]
        end = head["end"][idx] - batch["para_offsets"][idx]
        ans = {"pred_str": _answer_text(batch, idx, start, end), "rank_score": head["rank_score"][idx], "span_score": head["span_score"][idx],
               "pred_sp": _pred_sp(batch, idx, head["sp_prob"][idx], final) if sp_pred else []}
        if final:
            ans["chain_titles"] = [p["title"] for p in batch["passages"][idx]]
        out.append((qid, labels[idx], ans))
    return out


def combination_factors(fixed_thresh=None):
    """predict()'s combination factors: the fixed one, or the sweep 0, 0.1, ..., 1."""
    return [fixed_thresh] if fixed_thresh else [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1]


def metrics_report(qids, acc, lambdas, top, gold, sp_pred, logger):
    """predict()'s metric arithmetic and log lines, the ONE statement of them: predict_metrics below (every chain decoded on the host) and
    qa_eval.predict_metrics (only the chosen chains decoded) both end here. qids: the questions in first-appearance order; acc: per
    question, whether the chain with the top rank score is the gold one; top(k, lambda_, qid): the answer dict on top of question qid's
    list after the sorts for lambdas[0 .. k], called once per (k, qid) in that order; gold = {qid: (gold_answer, sp_gold)}.
    Returns (metrics dict, best_res)."""
    logger.info(f"evaluated {len(qids)} questions...")
    logger.info(f"chain ranking em: {np.mean(acc)}")
    best_em, best_f1, best_joint_em, best_joint_f1, best_sp_em, best_sp_f1 = 0, 0, 0, 0, 0, 0
    best_res = None
    for k, lambda_ in enumerate(lambdas):
        ems, f1s, sp_ems, sp_f1s, joint_ems, joint_f1s = [], [], [], [], [], []
        results = collections.defaultdict(dict)
        for qid in qids:
            first = top(k, lambda_, qid)
            top_pred, top_sp = first["pred_str"], first["pred_sp"]
            results["answer"][qid] = top_pred
            results["sp"][qid] = top_sp
            ems.append(exact_match_score(top_pred, gold[qid][0][0]))
            f1, prec, recall = f1_score(top_pred, gold[qid][0][0])
            f1s.append(f1)
            if sp_pred:
                m = {"sp_em": 0, "sp_f1": 0, "sp_prec": 0, "sp_recall": 0}
                update_sp(m, top_sp, gold[qid][1])
                sp_ems.append(m["sp_em"])
                sp_f1s.append(m["sp_f1"])
                jp, jr = prec * m["sp_prec"], recall * m["sp_recall"]
                joint_f1s.append(2 * jp * jr / (jp + jr) if jp + jr > 0 else 0.)
                joint_ems.append(ems[-1] * sp_ems[-1])
        if sp_pred:
            if best_joint_f1 < np.mean(joint_f1s):
                best_joint_f1, best_joint_em = np.mean(joint_f1s), np.mean(joint_ems)
                best_sp_f1, best_sp_em = np.mean(sp_f1s), np.mean(sp_ems)
                best_f1, best_em = np.mean(f1s), np.mean(ems)
                best_res = results
        elif best_f1 < np.mean(f1s):
            best_f1, best_em = np.mean(f1s), np.mean(ems)
        logger.info(f".......Using combination factor {lambda_}......")
        logger.info(f"answer em: {np.mean(ems)}, count: {len(ems)}")
        logger.info(f"answer f1: {np.mean(f1s)}, count: {len(f1s)}")
        logger.info(f"sp em: {np.mean(sp_ems)}, count: {len(sp_ems)}")
        logger.info(f"sp f1: {np.mean(sp_f1s)}, count: {len(sp_f1s)}")
        logger.info(f"joint em: {np.mean(joint_ems)}, count: {len(joint_ems)}")
        logger.info(f"joint f1: {np.mean(joint_f1s)}, count: {len(joint_f1s)}")
    logger.info(f"Best joint F1 from combination {best_f1}")
    return {"em": best_em, "f1": best_f1, "joint_em": best_joint_em, "joint_f1": best_joint_f1, "sp_em": best_sp_em, "sp_f1": best_sp_f1}, best_res


def predict_metrics(chains, gold, sp_pred, logger, fixed_thresh=None):
    """predict()'s ranking / metrics / log lines over all chains ([(qid, label, answer dict)] in dataloader order) and
    gold = {qid: (gold_answer, sp_gold)}. Returns (metrics dict, best_res). Each question's answer list is sorted IN PLACE once per
    factor, as the reference sorts it: the sort for a factor starts from the order the factor before it left."""
    id2result, id2answer = collections.defaultdict(list), collections.defaultdict(list)
    for qid, label, ans in chains:
        id2result[qid].append((label, ans["rank_score"]))
        id2answer[qid].append(ans)
    acc = []
    for qid, res in id2result.items():
        res.sort(key=lambda x: x[1], reverse=True)
        acc.append(res[0][0] == 1)

    def top(k, lambda_, qid):
        ans_res = id2answer[qid]
        ans_res.sort(key=lambda x: lambda_ * x["rank_score"] + (1 - lambda_) * x["span_score"], reverse=True)
        return ans_res[0]

    return metrics_report(list(id2result), acc, combination_factors(fixed_thresh), top, gold, sp_pred, logger)


def final_report(qids, top):
    """eval_final()'s result dict from the chosen answer dict top(qid) of every question, for final_results below and qa_eval.final_results."""
    results = collections.defaultdict(dict)
    for qid in qids:
        first = top(qid)
        results["answer"][qid] = first["pred_str"]
        results["sp"][qid] = first["pred_sp"]
        results["titles"][qid] = first["chain_titles"]
    return results


def final_results(chains, weight=0.8):
    """eval_final()'s selection: per question the chain with the best weight * rank + (1 - weight) * span; answer, sp and titles."""
    id2answer = collections.defaultdict(list)
    for qid, _, ans in chains:
        id2answer[qid].append(ans)

    def top(qid):
        ans_res = id2answer[qid]
        ans_res.sort(key=lambda x: weight * x["rank_score"] + (1 - weight) * x["span_score"], reverse=True)
        return ans_res[0]

    return final_report(list(id2answer), top)


def add_sp_labels(raw_path, input_file, save_path, title2sent_map="data/hotpot_index/title2sents.txt"):
    """Join retrieval JSONL to raw HotpotQA: each retrieved item gets `sp` (title, sents, sp_sent_ids) and `answer` = [raw answer]."""
    raw_data = json.load(open(raw_path))
    retrieved = [json.loads(line) for line in open(input_file).readlines()]
    title2sents = {t["title"]: t["sents"] for t in (json.loads(line) for line in open(title2sent_map).readlines())}
    for inst, raw in zip(retrieved, raw_data):
        assert inst["question"] == raw["question"]
        if "supporting_facts" in raw:
            by_title = collections.defaultdict(list)
            for t, i in raw["supporting_facts"]:
                by_title[t].append(i)
            inst["sp"] = [{"title": t, "sents": title2sents[t], "sp_sent_ids": ids} for t, ids in by_title.items()]
            inst["answer"] = [raw["answer"]]
    with open(save_path, "w") as out:
        for line in retrieved:
            out.write(json.dumps(line) + "\n")
