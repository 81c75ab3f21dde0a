"""Drop-in for the reference's scripts/train_momentum.py: the second stage of its retriever recipe, "finetune the question encoder with
frozen memory bank", on one rank (--do_train), and the in-batch MRR of the resulting pair of encoders (--do_predict).

    python scripts/train_momentum.py --do_train --prefix ${RUN_ID} --predict_batch_size 3000 --model_name <roberta-base dir> \
        --train_batch_size 150 --learning_rate 1e-5 --fp16 --train_file ${TRAIN_DATA_PATH} --predict_file ${DEV_DATA_PATH} --seed 16 \
        --eval-period -1 --max_c_len 300 --max_q_len 70 --max_q_sp_len 350 --momentum --k 76800 --m 0.999 --temperature 1 \
        --init-retriever ${STAGE_1}/checkpoint_best.pt

Flags are the reference's (mdr/retrieval/config.py train_args), parsed verbatim. The model is multihop_dense_retrieval_amd/momentum.py's
MomentumRetriever: encoder_q is trained, encoder_k is a frozen inference handle copied from it once, after
--init-retriever has been applied (strip `module.`, keep the known keys), and the queue holds --k earlier [c1; c2] rows. Without
--init-retriever the encoder starts from the weights in the --model_name directory, as scripts/train_mhop.py does. --m is accepted and goes
into the run directory's name only: the reference never calls its momentum update (its run is named freeze_k).

The loop is scripts/train_mhop.py's train(), which is the reference's loop in both of its scripts (Adam, the two weight-decay groups, the
linear schedule with warmup, the (batch_step + 1) % g == 0 boundary, the loss meter, --eval-period, the evaluation after every epoch, the log
lines), given the momentum step, the model itself for evaluation (question side encoder_q, passage side encoder_k) and the checkpoint names:
checkpoint_q_best.pt and checkpoint_k_best.pt, which BOTH hold encoder_q's state dict as in the reference (its lines 186-189 save encoder_q
twice), and checkpoint_q_last.pt after every epoch. They are plain fp32 CPU tensors under RobertaRetriever's keys, so --init_checkpoint of the
eval CLIs, scripts/encode_corpus.py and scripts/train_mhop.py --do_predict load them. The run directory is
output_dir/<date>/{prefix}-seed..-bsz..-fp16..-lr..-decay..-warm..-valbsz..-m{m}-k{k}-t{temperature} with log.txt inside.

Not built: several ranks (--local_rank other than -1, and the reference's DataParallel split of a batch). Inputs are checked before the
device is touched; every reason the script cannot run exits with a message. The other deviations are scripts/train_mhop.py's (no
TensorBoard without the package, local --model_name, batches built in this process: under --do_train from token arenas on the device).
"""
import logging
import os
import random
import sys
from datetime import date
from functools import partial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

CHECKPOINTS_BEST = ("checkpoint_q_best.pt", "checkpoint_k_best.pt")  # both hold encoder_q (the reference's lines 186-189)
CHECKPOINT_LAST = "checkpoint_q_last.pt"


def run_name(args):
    """train_momentum.py:34."""
    return (f"{args.prefix}-seed{args.seed}-bsz{args.train_batch_size}-fp16{args.fp16}-lr{args.learning_rate}-decay{args.weight_decay}"
            f"-warm{args.warmup_ratio}-valbsz{args.predict_batch_size}-m{args.m}-k{args.k}-t{args.temperature}")


def check_inputs(args):
    """What the command line must give, looked at before anything touches the device."""
    if args.local_rank != -1:
        sys.exit("multi-rank momentum training is not built: run one rank (--local_rank -1)")
    if not (args.do_train or args.do_predict):
        sys.exit("nothing to do: give --do_train or --do_predict")
    if not os.path.isdir(args.model_name):
        sys.exit(f"--model_name {args.model_name!r} must be a local directory with the RoBERTa config, tokenizer and weights (nothing is downloaded)")
    files = [("--predict_file", args.predict_file)] + ([("--train_file", args.train_file)] if args.do_train else [])
    for flag, path in files:
        if not (path and os.path.isfile(path)):
            sys.exit(f"momentum training needs {flag} {path!r}: no such file")
    if args.init_retriever != "" and not os.path.isfile(args.init_retriever):
        sys.exit(f"--init-retriever {args.init_retriever!r}: no such file")
    if args.k < 1:
        sys.exit(f"--k {args.k}: the queue needs at least one row")
    if args.accumulate_gradients < 1:
        raise ValueError("Invalid accumulate_gradients parameter: {}, should be >= 1".format(args.accumulate_gradients))


def build_model(args, bert_config, device):
    """MomentumRetriever on `device`: encoder_q from the --model_name directory's weights, then --init-retriever over them, then the key
    encoder copied from the result."""
    import torch
    import train_mhop
    from multihop_dense_retrieval_amd import momentum
    init, args.init_retriever = args.init_retriever, ""  # applied below, after the directory's weights
    try:
        model = momentum.MomentumRetriever(bert_config, args)  # project.* and the queue from torch's generator under --seed
    finally:
        args.init_retriever = init
    enc = model.encoder_q
    start = train_mhop.encoder_weights(args.model_name, enc.shapes)
    if init != "":
        print(f"Load pretrained retriever from {init}")
        ckpt = torch.load(init, map_location="cpu")
        start.update({(k[7:] if k.startswith("module.") else k): v for k, v in ckpt.items()})
    start = {k: v for k, v in start.items() if k in enc.shapes}
    missing = [k for k in enc.shapes if k.startswith("encoder.") and "pooler" not in k and k not in start]
    if missing:
        sys.exit(f"no encoder weights to start from: {args.model_name!r} holds none and --init-retriever gives none ({len(missing)} tensors "
                 f"missing, the first {missing[0]})")
    enc.load_state_dict(start, strict=False)
    return model.to(device)  # the key encoder is copied from encoder_q here


def main(argv=None):
    from multihop_dense_retrieval_amd.config import train_args
    args = train_args(argv)
    check_inputs(args)
    handlers = [logging.StreamHandler()]
    if args.do_train:
        args.momentum = True  # this script is the --momentum step whether or not the flag is repeated
        args.output_dir = os.path.join(args.output_dir, date.today().strftime("%m-%d-%Y"), run_name(args))
        if os.path.exists(args.output_dir) and os.listdir(args.output_dir):
            print(f"output directory {args.output_dir} already exists and is not empty.")
        os.makedirs(args.output_dir, exist_ok=True)
        handlers.insert(0, logging.FileHandler(os.path.join(args.output_dir, "log.txt")))
    import numpy as np
    import torch
    import train_mhop
    from multihop_dense_retrieval_amd import data, mhop_data, momentum
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO, handlers=handlers)
    logger = logging.getLogger(__name__)
    logger.setLevel(logging.INFO)
    logger.info(args)
    if args.no_cuda or not torch.cuda.is_available():
        sys.exit("the retriever runs on a HIP device only (there is no CPU fallback)")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    logger.info("device %s n_gpu %d distributed training %r", device, 1, False)
    import transformers
    bert_config = transformers.AutoConfig.from_pretrained(args.model_name, local_files_only=True)
    tokenizer = data.load_tokenizer(args.model_name)
    collate_fc = partial(mhop_data.mhop_collate, pad_id=tokenizer.pad_token_id)
    if args.do_train:
        args.train_batch_size = int(args.train_batch_size / args.accumulate_gradients)
        if args.max_c_len > bert_config.max_position_embeddings:
            raise ValueError("Cannot use sequence length %d because the BERT model was only trained up to sequence length %d" %
                             (args.max_c_len, bert_config.max_position_embeddings))
    # seeded after the imports and the config / tokenizer loading, as scripts/train_mhop.py explains
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    model = build_model(args, bert_config, device)
    eval_dataloader = train_mhop.dev_batches(args, tokenizer, collate_fc, device, feed="arena" if args.do_train else "host")
    logger.info(f"Num of dev batches: {len(eval_dataloader)}")
    print(f"number of trainable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
    if args.do_train:
        try:
            from torch.utils.tensorboard import SummaryWriter
            tb_logger = SummaryWriter(os.path.join(args.output_dir.replace("logs", "tflogs")))
        except ImportError:
            tb_logger = None
            logger.info("TensorBoard is not installed: its scalars are not written")
        train_mhop.train(args, model, tokenizer, collate_fc, eval_dataloader, device, logger, tb_logger, steps=momentum, eval_model=lambda: model,
                         saved=model.encoder_q.state_dict, best=CHECKPOINTS_BEST, last=CHECKPOINT_LAST)
    elif args.do_predict:
        acc = train_mhop.predict(args, model, eval_dataloader, device, logger)
        logger.info(f"test performance {acc}")


if __name__ == "__main__":
    main()
