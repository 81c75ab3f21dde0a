"""Data path of scripts/train_mhop.py, --do_predict and --do_train (mdr/retrieval/data/mhop_dataset.py:12-121 of the reference):

    MhopDataset(tokenizer, data_path, max_q_len, max_q_sp_len, max_c_len)   the eval branch; train=True raises
    MhopTrainDataset(tokenizer, data_path, max_q_len, max_q_sp_len, max_c_len)   the train branch (--do_train)
    mhop_collate(samples, pad_id=0)

JSONL records: `question`, `type`, `pos_paras` (two {title, text}), `bridge` (title of the second-hop passage, for every type but
"comparison") and `neg_paras` (at least two {title, text}; the first two are used). One trailing "?" is stripped from the question.
A passage is `encode_plus(title.strip(), text_pair=text.strip(), max_length=max_c_len)`: unlike EmDataset there is NO NFD
normalisation and NO empty-text -> title rule here. `q_sp` is the question paired with the start passage's stripped text, cut at
max_q_sp_len. Token ids follow the transformers-2.11 rules of data.py (encode_pairs_2_11 and its switches), as every CLI here.
mhop_collate right-pads every key WITH 0 to the batch maximum, whatever `pad_id` says (the reference ignores the argument too);
the masks tell the encoder where a row ends.

Comparison questions. For `type == "comparison"` the order of the two positives is a `random.shuffle` of the global `random`
module, at eval time too, on every __getitem__ (the list is shuffled in place). The CLI seeds it with `random.seed(args.seed)`;
this class calls `random.shuffle` on the same list, so reading the items once, in dataset order, after the same seed gives the
reference's order for `--num_workers 0`. With workers > 0 the reference itself is not reproducible (each worker process owns a
copy of the generator state and the items are dealt to workers in batches), so neither is any restatement of it.
"""
import json
import random

import torch

from .data import collate_tokens, encode_pairs_2_11, is_roberta_family, prefix_space_2_11


def _pair(tokenizer, first, second, max_len):
    if not is_roberta_family(tokenizer):
        return tokenizer(first, text_pair=second, max_length=max_len, truncation=True, return_tensors="pt")
    ids, mask = encode_pairs_2_11(tokenizer, [first], [second], max_len, False)
    return {"input_ids": torch.tensor(ids, dtype=torch.int64), "attention_mask": torch.tensor(mask, dtype=torch.int64)}


def _single(tokenizer, text, max_len):
    """`encode_plus(text, max_length=n)` of transformers 2.11: `<s> text </s>`, tokens dropped from the end."""
    if not is_roberta_family(tokenizer):
        return tokenizer(text, max_length=max_len, truncation=True, return_tensors="pt")
    raw = tokenizer([prefix_space_2_11(text)], add_special_tokens=False, truncation=False)["input_ids"][0]
    ids = [tokenizer.bos_token_id] + list(raw[:max(max_len - 2, 0)]) + [tokenizer.eos_token_id]
    return {"input_ids": torch.tensor([ids], dtype=torch.int64), "attention_mask": torch.ones((1, len(ids)), dtype=torch.int64)}


class MhopDataset(torch.utils.data.Dataset):
    def __init__(self, tokenizer, data_path, max_q_len, max_q_sp_len, max_c_len, train=False):
        super().__init__()
        if train:
            raise NotImplementedError("training is not supported by MhopDataset, the eval branch: the train branch is MhopTrainDataset")
        self.tokenizer = tokenizer
        self.max_q_len, self.max_c_len, self.max_q_sp_len = max_q_len, max_c_len, max_q_sp_len
        self.train = False
        print(f"Loading data from {data_path}")
        with open(data_path) as f:
            self.data = self.select([json.loads(line) for line in f.readlines()])
        print(f"Total sample count {len(self.data)}")

    def select(self, data):
        """The samples of the file this dataset keeps: all of them here; MhopTrainDataset has the train branch's rule."""
        return data

    def encode_para(self, para, max_len):
        return _pair(self.tokenizer, para["title"].strip(), para["text"].strip(), max_len)

    def __getitem__(self, index):
        sample = self.data[index]
        question = sample["question"]
        if question.endswith("?"):
            question = question[:-1]
        if sample["type"] == "comparison":
            random.shuffle(sample["pos_paras"])  # the global generator, in place, at eval time too (see the module docstring)
            start_para, bridge_para = sample["pos_paras"]
        else:
            for para in sample["pos_paras"]:
                if para["title"] != sample["bridge"]:
                    start_para = para
                else:
                    bridge_para = para
        if self.train:
            random.shuffle(sample["neg_paras"])  # behind the comparison shuffle, as in the reference: the two draw from one generator
        return {
            "q_codes": _single(self.tokenizer, question, self.max_q_len),
            "q_sp_codes": _pair(self.tokenizer, question, start_para["text"].strip(), self.max_q_sp_len),
            "start_para_codes": self.encode_para(start_para, self.max_c_len),
            "bridge_para_codes": self.encode_para(bridge_para, self.max_c_len),
            "neg_codes_1": self.encode_para(sample["neg_paras"][0], self.max_c_len),
            "neg_codes_2": self.encode_para(sample["neg_paras"][1], self.max_c_len),
        }

    def __len__(self):
        return len(self.data)


class MhopTrainDataset(MhopDataset):
    """The train=True branch of the reference's MhopDataset (mhop_dataset.py:30-39, :59-60): `neg_paras` is replaced by `tfidf_neg`, samples
    with fewer than two negatives are dropped, and every __getitem__ shuffles the sample's negatives in place with the global `random`
    generator and uses the first two. Deviations: a sample WITHOUT `tfidf_neg` keeps its `neg_paras` (the reference raises KeyError), and
    the reference's leftover `pdb.set_trace()` is not there."""

    def __init__(self, tokenizer, data_path, max_q_len, max_q_sp_len, max_c_len):
        super().__init__(tokenizer, data_path, max_q_len, max_q_sp_len, max_c_len)
        self.train = True

    def select(self, data):
        for sample in data:
            if "tfidf_neg" in sample:
                sample["neg_paras"] = sample["tfidf_neg"]
        return [s for s in data if len(s["neg_paras"]) >= 2]


_KEYS = (("q", "q_codes"), ("q_sp", "q_sp_codes"), ("c1", "start_para_codes"), ("c2", "bridge_para_codes"), ("neg1", "neg_codes_1"),
         ("neg2", "neg_codes_2"))


def mhop_collate(samples, pad_id=0):
    if len(samples) == 0:
        return {}
    batch = {}
    for name, key in _KEYS:
        batch[f"{name}_input_ids"] = collate_tokens([s[key]["input_ids"].view(-1) for s in samples], 0)
        batch[f"{name}_mask"] = collate_tokens([s[key]["attention_mask"].view(-1) for s in samples], 0)
    if "token_type_ids" in samples[0]["q_codes"]:
        for name, key in _KEYS:
            batch[f"{name}_type_ids"] = collate_tokens([s[key]["token_type_ids"].view(-1) for s in samples], 0)
    return batch
