"""Drop-in for the reference's scripts/train_mhop.py at inference (--do_predict): the in-batch-negative MRR of a retriever
checkpoint on a dev set, the number the reference selects checkpoint_best.pt by, without a corpus index.

    python scripts/train_mhop.py --do_predict --predict_batch_size 3000 --model_name <roberta-base dir> --fp16 \
        --predict_file ${DEV_DATA_PATH} --init_checkpoint q_encoder.pt --seed 16 --max_c_len 300 --max_q_len 70 \
        --max_q_sp_len 350 --shared-encoder --num_workers 0

Flags are the reference's (mdr/retrieval/config.py train_args), parsed verbatim. It logs, through the same logger,
`Num of dev batches: ..`, `evaluated {n} examples...`, `MRR-1: ..`, `MRR-2: ..` and `test performance {dict}` with the keys
mrr_1, mrr_2, mrr_avg. The six forwards of a batch run on the HIP encoder (RobertaRetriever.forward) and the ranks come from
mdr_inbatch_rank (multihop_dense_retrieval_amd/criterions.py): --fp16 selects apex O1's fp16 scores, otherwise they are fp32.
--do_train exits: training is not supported. One rank.

Deviations from the reference, all outside the numbers it reports: no dated `--output_dir` directory, `log.txt` or TensorBoard
writer is created (the reference makes them even for --do_predict; an evaluation needs none); the checkpoint is loaded with
load_saved(exact=False), so buffers a newer transformers saved beside the weights are dropped instead of refused; --model_name
is a local directory (nothing is downloaded); the batches are loaded in this process whatever --num_workers says, which is also
the only setting under which the reference's order of the comparison questions' positives (a global random.shuffle at eval
time, multihop_dense_retrieval_amd/mhop_data.py) is reproducible.
"""
import logging
import os
import random
import sys
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def predict(args, model, eval_dataloader, device, logger):
    """train_mhop.py:233-250."""
    import torch
    from multihop_dense_retrieval_amd import criterions
    from multihop_dense_retrieval_amd.retriever import move_to_cuda
    model.eval()
    rrs_1, rrs_2 = [], []
    for batch in eval_dataloader:
        batch_to_feed = move_to_cuda(batch)
        with torch.no_grad():
            outputs = model(batch_to_feed)
            eval_results = criterions.mhop_eval(outputs, args)
        rrs_1 += eval_results["rrs_1"]
        rrs_2 += eval_results["rrs_2"]
    lines, acc = criterions.predict_summary(rrs_1, rrs_2)
    for ln in lines:
        logger.info(ln)
    return acc


def main(argv=None):
    from multihop_dense_retrieval_amd.config import train_args
    args = train_args(argv)
    if args.do_train:
        sys.exit("training is not supported: this retriever runs inference only (--do_predict)")
    import numpy as np
    import torch
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import data, mhop_data, retriever
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO,
                        handlers=[logging.StreamHandler()])
    logger = logging.getLogger(__name__)
    logger.setLevel(logging.INFO)
    logger.info(args)
    if args.no_cuda or not torch.cuda.is_available():
        sys.exit("the retriever runs on a HIP device only (there is no CPU fallback)")
    device = torch.device("cuda", max(args.local_rank, 0))
    torch.cuda.set_device(device)
    logger.info("device %s n_gpu %d distributed training %r", device, 1, False)
    if not os.path.isdir(args.model_name):
        sys.exit(f"--model_name {args.model_name!r} must be a local directory with the RoBERTa config and tokenizer (nothing is downloaded)")
    import transformers
    bert_config = transformers.AutoConfig.from_pretrained(args.model_name, local_files_only=True)
    model = retriever.RobertaRetriever(bert_config, args)
    tokenizer = data.load_tokenizer(args.model_name)
    collate_fc = partial(mhop_data.mhop_collate, pad_id=tokenizer.pad_token_id)
    # train_mhop.py:94-98. Seeded HERE, after the imports and the config / tokenizer loading above: importing transformers draws from the global
    # `random` generator, and the comparison questions' order of positives is the generator's state at the first __getitem__. In the reference
    # nothing between its seeding and that point draws from it (the model's initialisation uses torch's generator).
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    eval_dataset = mhop_data.MhopDataset(tokenizer, args.predict_file, args.max_q_len, args.max_q_sp_len, args.max_c_len)
    eval_dataloader = DataLoader(eval_dataset, batch_size=args.predict_batch_size, collate_fn=collate_fc, num_workers=0)
    logger.info(f"Num of dev batches: {len(eval_dataloader)}")
    if args.init_checkpoint != "":
        model = retriever.load_saved(model, args.init_checkpoint, exact=False, map_location="cpu")
    model.to(device)
    if args.do_predict:
        acc = predict(args, model, eval_dataloader, device, logger)
        logger.info(f"test performance {acc}")


if __name__ == "__main__":
    main()
