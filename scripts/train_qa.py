"""Drop-in for the reference's scripts/train_qa.py at inference (--do_predict / --do_test) on the HIP reader.

    python scripts/train_qa.py --do_predict --predict_file <retrieval jsonl with sp / answer> --init_checkpoint qa_electra.pt \
        --model_name <ELECTRA / BERT dir or cached name> --sp-pred --fp16 --max_ans_len 35 --save-prediction out.json

Flags are the reference's (mdr/qa/config.py), parsed verbatim. --do_predict runs predict() with the fixed 0.8 combination factor and
writes its log lines and --save-prediction; --do_test runs eval_final(). --do_train exits: training is not supported. One rank; the
batches are the reference's (sequential, --predict_batch_size chains) and are loaded in this process (num_workers is accepted and not
used: the forward is on the device and data workers would fork a process that holds it). Numerics are apex O1's whether or not --fp16
is given (the README's QA command passes it). The config and the tokenizer come from --model_name, a local directory or a model in the
local cache; nothing is downloaded.
"""
import argparse
import logging
import os
import sys
from datetime import date
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def train_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--train_file", type=str, default="../data/nq-with-neg-train.txt")
    p.add_argument("--predict_file", type=str, default="../data/nq-with-neg-dev.txt")
    p.add_argument("--num_workers", default=10, type=int)
    p.add_argument("--do_train", default=False, action="store_true")
    p.add_argument("--do_predict", default=False, action="store_true")
    p.add_argument("--do_test", default=False, action="store_true")
    p.add_argument("--model_name", default="bert-base-uncased", type=str)
    p.add_argument("--init_checkpoint", type=str, default="")
    p.add_argument("--max_seq_len", default=512, type=int)
    p.add_argument("--max_q_len", default=64, type=int)
    p.add_argument("--max_ans_len", default=35, type=int)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--fp16_opt_level", type=str, default="O1")
    p.add_argument("--no_cuda", default=False, action="store_true")
    p.add_argument("--local_rank", type=int, default=-1)
    p.add_argument("--predict_batch_size", default=256, type=int)
    p.add_argument("--save-prediction", default="", type=str)
    p.add_argument("--sp-pred", action="store_true")
    p.add_argument("--prefix", type=str, default="eval")
    p.add_argument("--weight_decay", default=0.0, type=float)
    p.add_argument("--output_dir", default="./logs", type=str)
    p.add_argument("--train_batch_size", default=128, type=int)
    p.add_argument("--num_q_per_gpu", default=1)
    p.add_argument("--learning_rate", default=1e-5, type=float)
    p.add_argument("--num_train_epochs", default=5, type=float)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--eval-period", type=int, default=2500)
    p.add_argument("--max_grad_norm", default=2.0, type=float)
    p.add_argument("--adam_epsilon", default=1e-8, type=float)
    p.add_argument("--neg-num", type=int, default=9)
    p.add_argument("--shared-norm", action="store_true")
    p.add_argument("--qa-drop", default=0, type=float)
    p.add_argument("--rank-drop", default=0, type=float)
    p.add_argument("--sp-drop", default=0, type=float)
    p.add_argument("--final-metric", default="joint_f1")
    p.add_argument("--use-adam", action="store_true")
    p.add_argument("--warmup-ratio", default=0, type=float)
    p.add_argument("--sp-weight", default=0, type=float)
    return p.parse_args(argv)


def run_batches(model, loader, args, final):
    """The device work of every batch (forward + heads + span search, fused) and the host decode of each chain."""
    from multihop_dense_retrieval_amd import qa_data
    chains, gold = [], {}
    for batch in loader:
        head = model.decode(batch["net_inputs"], args.max_ans_len)
        lists = {"start": head["start"].tolist(), "end": head["end"].tolist(), "span_score": head["span_score"].float().tolist(),
                 "rank_score": head["rank_score"].view(-1).float().tolist(),
                 "sp_prob": head["sp_prob"].float().tolist() if head["sp_prob"] is not None else None}
        chains.extend(qa_data.chain_results(batch, lists, args.sp_pred, final=final))
        for idx, qid in enumerate(batch["qids"]):
            gold[qid] = (batch["gold_answer"][idx], batch["sp_gold"][idx])
    return chains, gold


def main(argv=None):
    args = train_args(argv)
    if args.do_train:
        sys.exit("training is not supported: this reader runs inference only (--do_predict / --do_test)")
    import json
    import torch
    import transformers
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import qa_data, reader
    date_curr = date.today().strftime("%m-%d-%Y")
    model_name = (f"{args.prefix}-seed{args.seed}-bsz{args.train_batch_size}-fp16{args.fp16}-lr{args.learning_rate}-decay{args.weight_decay}"
                  f"-neg{args.neg_num}-sn{args.shared_norm}-adam{args.use_adam}-warm{args.warmup_ratio}-sp{args.sp_weight}")
    args.output_dir = os.path.join(args.output_dir, date_curr, model_name)
    os.makedirs(args.output_dir, exist_ok=True)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO,
                        handlers=[logging.FileHandler(os.path.join(args.output_dir, "log.txt")), logging.StreamHandler()])
    logger = logging.getLogger(__name__)
    logger.setLevel(logging.INFO)
    logger.info(args)
    if args.no_cuda or not torch.cuda.is_available():
        sys.exit("the reader runs on a HIP device only (there is no CPU fallback)")
    device = torch.device("cuda", 0)
    logger.info("device %s n_gpu %d distributed training %r", device, 1, False)
    config = transformers.AutoConfig.from_pretrained(args.model_name, local_files_only=True)
    tokenizer = transformers.BertTokenizer.from_pretrained(args.model_name, local_files_only=True)
    model = reader.QAModel(config, args)
    collate = partial(qa_data.qa_collate, pad_id=tokenizer.pad_token_id)
    dataset = qa_data.QADataset(tokenizer, args.predict_file, args.max_seq_len, args.max_q_len)
    loader = DataLoader(dataset, batch_size=args.predict_batch_size, collate_fn=collate, num_workers=0)
    logger.info(f"Num of dev batches: {len(loader)}")
    if args.init_checkpoint != "":
        logger.info(f"Loading model from {args.init_checkpoint}")
        reader.load_saved(model, args.init_checkpoint, exact=False, map_location="cpu")
    model.to(device).eval()
    if args.do_predict:
        chains, gold = run_batches(model, loader, args, final=False)
        metrics, best_res = qa_data.predict_metrics(chains, gold, args.sp_pred, logger, fixed_thresh=0.8)
        if args.save_prediction != "":
            with open(args.save_prediction, "w") as f:
                json.dump(best_res, f)
        logger.info(f"test performance {metrics}")
    elif args.do_test:
        chains, _ = run_batches(model, loader, args, final=True)
        results = qa_data.final_results(chains, weight=0.8)
        if args.save_prediction != "":
            with open(args.save_prediction, "w") as f:
                json.dump(results, f)


if __name__ == "__main__":
    main()
