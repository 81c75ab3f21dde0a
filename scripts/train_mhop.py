"""Drop-in for the reference's scripts/train_mhop.py: training the multi-hop retriever (--do_train) and the in-batch-negative MRR of a
retriever checkpoint on a dev set (--do_predict), the number the reference selects checkpoint_best.pt by, without a corpus index.

    python scripts/train_mhop.py --do_train --prefix ${RUN_ID} --predict_batch_size 3000 --model_name <roberta-base dir> \
        --train_batch_size 150 --learning_rate 2e-5 --fp16 --train_file ${TRAIN_DATA_PATH} --predict_file ${DEV_DATA_PATH} --seed 16 \
        --eval-period -1 --max_c_len 300 --max_q_len 70 --max_q_sp_len 350 --shared-encoder --warmup-ratio 0.1
    python scripts/train_mhop.py --do_predict --predict_batch_size 3000 --model_name <roberta-base dir> --fp16 \
        --predict_file ${DEV_DATA_PATH} --init_checkpoint q_encoder.pt --seed 16 --max_c_len 300 --max_q_len 70 \
        --max_q_sp_len 350 --shared-encoder --num_workers 0

Flags are the reference's (mdr/retrieval/config.py train_args), parsed verbatim. --do_predict logs, through the same logger,
`Num of dev batches: ..`, `evaluated {n} examples...`, `MRR-1: ..`, `MRR-2: ..` and `test performance {dict}` with the keys
mrr_1, mrr_2, mrr_avg. The six forwards of a batch run on the HIP encoder (RobertaRetriever.forward) and the ranks come from
mdr_inbatch_rank (multihop_dense_retrieval_amd/criterions.py): --fp16 selects apex O1's fp16 scores, otherwise they are fp32.

--do_train is lines 124-227 of the reference's script on multihop_dense_retrieval_amd/train.py: the two
weight-decay groups, the linear schedule with warmup, the reference's accumulation boundary ((batch_step + 1) % g == 0, quirk included),
the smoothed loss meter, --eval-period, the evaluation after every epoch, its log lines, and checkpoint_best.pt / checkpoint_last.pt (plain
fp32 CPU state dicts with the reference's keys) under output_dir/<date>/<prefix>-seed..-bsz.. with log.txt beside them. The encoder starts
from the weights in the --model_name directory, project.* from torch's default initialisers under --seed; --init_checkpoint overwrites both.
Every forward draws its dropout seed from a torch.Generator seeded with --seed. The arithmetic is fp16 with fp32 masters whether or not
--fp16 is given, so the dynamic loss scale is always on; --fp16 selects the fp16 score mode of the loss, as for --do_predict.
--momentum is refused here: the reference trains it from a script of its own, and so does this repository (scripts/train_momentum.py, which
calls this file's train() with its own step, evaluation model and checkpoint names).

Several ranks: `torchrun --nproc-per-node N scripts/train_mhop.py --do_train ...`. The rank comes from --local_rank (the
reference's flag) or from LOCAL_RANK, RANK and WORLD_SIZE; with neither, or with a world of one rank, everything above holds unchanged. Every
rank makes the same draws and sees the same batch of --train_batch_size samples, encodes its contiguous slice of it, the embeddings are
gathered, every rank evaluates the full in-batch loss (the negatives span the whole batch whatever the rank count, as under the reference's
DataParallel), backpropagates its own rows, and the gradients are summed over the ranks in rank order by mdr_rank_sum
(multihop_dense_retrieval_amd/dist.py), so the checkpoint's bytes depend on the rank count but not on the transport. --dist-backend nccl
(RCCL, the default) or gloo; --share-gpu puts every rank on device 0 (gloo only: a rehearsal on one card); --dist-timeout SECONDS goes to
init_process_group; --check-ranks compares a checksum of the parameters' bits over the ranks at every evaluation and at the end. Rank 0 alone
writes log.txt, TensorBoard, the checkpoints and the log lines; every rank evaluates the whole dev set, so nobody waits and the
best-checkpoint decision is the same everywhere. The reference's own --local_rank branch (DistributedDataParallel with one seed and no
DistributedSampler: every rank sees the same batches and the work is not split) is not reproduced, only its launch convention.

Deviations from the reference, all outside the numbers it reports: for --do_predict no dated `--output_dir` directory, `log.txt` or
TensorBoard writer is created (the reference makes them even there; an evaluation needs none); TensorBoard scalars are written only when
torch.utils.tensorboard imports; the checkpoint is loaded with load_saved(exact=False), so buffers a newer transformers saved beside the
weights are dropped instead of refused; --model_name is a local directory (nothing is downloaded); the batches are built in this process
whatever --num_workers says, which is also the only setting under which the reference's order of the comparison questions' positives and
of the training negatives (global random.shuffle calls, multihop_dense_retrieval_amd/mhop_data.py) is reproducible. Under --do_train the
train file and the dev file are each tokenised ONCE into a token arena on the device, cached beside the data file as
`<file>.mhop_arena.npz` (its status goes to stdout, not to the log), and every batch is assembled there by one kernel from the reference's
own shuffle draws (multihop_dense_retrieval_amd/mhop_arena.py): the same batches, checkpoint bytes and generator states
as the reference's per-step tokenising, which train(..., feed="host") still runs. Only RoBERTa-family tokenizers are served there.
"""
import hashlib
import logging
import os
import random
import sys
from datetime import date
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


class AverageMeter:
    """utils.py:44-60 of the reference."""

    def __init__(self):
        self.val, self.avg, self.sum, self.count = 0, 0, 0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def check_train_inputs(args):
    """What --do_train needs from the command line, looked at before anything touches the device."""
    if args.momentum:
        sys.exit("training with --momentum is not built in this script: the reference trains it from a script of its own, scripts/train_momentum.py")
    if not os.path.isdir(args.model_name):
        sys.exit(f"training is not supported with --model_name {args.model_name!r}: it must be a local directory with the RoBERTa config, "
                 "tokenizer and weights (nothing is downloaded)")
    for flag, path in (("--train_file", args.train_file), ("--predict_file", args.predict_file)):
        if not os.path.isfile(path):
            sys.exit(f"training needs {flag} {path!r}: no such file")
    if args.init_checkpoint != "" and not os.path.isfile(args.init_checkpoint):
        sys.exit(f"--init_checkpoint {args.init_checkpoint!r}: no such file")
    if args.accumulate_gradients < 1:
        raise ValueError("Invalid accumulate_gradients parameter: {}, should be >= 1".format(args.accumulate_gradients))


def rank_setup(args, environ=None):
    """(rank, world size, local rank) of a launch: from --local_rank (the reference's flag) or from the launcher's LOCAL_RANK, RANK and
    WORLD_SIZE; (0, 1, -1) with neither, which is the one-rank run. Exits on what cannot run, before anything touches a device."""
    env = os.environ if environ is None else environ
    if args.local_rank == -1 and "RANK" not in env and "LOCAL_RANK" not in env:
        if args.share_gpu:
            sys.exit("--share-gpu puts several ranks on device 0: it needs a launcher (RANK, WORLD_SIZE, LOCAL_RANK)")
        return 0, 1, -1
    world = int(env.get("WORLD_SIZE", "1"))
    local = args.local_rank if args.local_rank != -1 else int(env.get("LOCAL_RANK", env.get("RANK", "0")))
    rank = int(env.get("RANK", str(local)))
    if not (world >= 1 and 0 <= rank < world and local >= 0):
        sys.exit(f"rank {rank} (local {local}) of {world}: the launcher's RANK, LOCAL_RANK and WORLD_SIZE do not fit together")
    if args.share_gpu and args.dist_backend != "gloo":
        sys.exit(f"--share-gpu is the one-card rehearsal and runs over gloo only, not --dist-backend {args.dist_backend}: RCCL wants a device per rank")
    if world > 1:
        from multihop_dense_retrieval_amd import dist as mdr_dist
        if world > mdr_dist.MAX_RANKS:
            sys.exit(f"{world} ranks: the ordered gradient sum is built for at most {mdr_dist.MAX_RANKS}")
        if "MASTER_ADDR" not in env or "MASTER_PORT" not in env:
            sys.exit("several ranks need a launcher's MASTER_ADDR and MASTER_PORT (torchrun --nproc-per-node N scripts/train_mhop.py ...)")
        if not args.share_gpu:
            import torch
            visible = torch.cuda.device_count()
            per_node = int(env.get("LOCAL_WORLD_SIZE", str(world)))
            if per_node > visible or local >= max(visible, 1):
                sys.exit(f"{per_node} ranks on this node but {visible} visible devices: give every rank a device, or rehearse on one card with "
                         "--dist-backend gloo --share-gpu")
    return rank, world, local


def join_world(args, world_size):
    """The process group of a launch of several ranks as a dist.TorchWorld; None for one rank."""
    if world_size == 1:
        return None
    from datetime import timedelta
    import torch.distributed
    from multihop_dense_retrieval_amd import dist as mdr_dist
    torch.distributed.init_process_group(args.dist_backend, timeout=timedelta(seconds=args.dist_timeout))
    return mdr_dist.TorchWorld()


def ranks_agree(world, what, value):
    """None when every rank holds `value`, else the message that names the first rank that differs from rank 0. One all_gather_object."""
    values = world.gather_objects(value)
    for r, v in enumerate(values):
        if v != values[0]:
            return f"the ranks differ in {what}: rank 0 has {values[0]}, rank {r} has {v}"
    return None


def parameter_checksum(model):
    """The integer sum of the parameters' bit patterns modulo 2^64, summed on the device, as 16 hex digits."""
    import torch
    total = 0
    for p in model.parameters():
        total += int(p.detach().contiguous().view(torch.int32).to(torch.int64).sum().item())
    return f"{total & 0xFFFFFFFFFFFFFFFF:016x}"


def encoder_weights(model_name, wanted):
    """{`encoder.` + key: tensor} from the weights in the model directory, loaded on the CPU; {} when the directory holds none."""
    import transformers
    try:
        hf = transformers.AutoModel.from_pretrained(model_name, local_files_only=True)
    except (OSError, ValueError):
        return {}
    return {"encoder." + k: v.detach().float() for k, v in hf.state_dict().items() if "encoder." + k in wanted}


def dev_batches(args, tokenizer, collate_fc, device, feed="host"):
    """The dev set's batches, an iterable with len(): today's DataLoader over mhop_data.MhopDataset (feed="host"), or the feed of a token arena
    built or loaded once for --predict_file (feed="arena": multihop_dense_retrieval_amd/mhop_arena.py), whose batches are already on `device`.
    Both read the samples in file order and make the same draws on `random` and on torch's generator."""
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import mhop_arena, mhop_data
    eval_dataset = mhop_data.MhopDataset(tokenizer, args.predict_file, args.max_q_len, args.max_q_sp_len, args.max_c_len)
    if feed == "arena":
        return mhop_arena.MhopArena.load_or_build(args.predict_file, eval_dataset, tokenizer).to(device).feed(args.predict_batch_size, shuffle=False)
    if feed != "host":
        raise ValueError(f"feed = {feed!r}: \"arena\" or \"host\"")
    return DataLoader(eval_dataset, batch_size=args.predict_batch_size, collate_fn=collate_fc, num_workers=0)


def train(args, model, tokenizer, collate_fc, eval_dataloader, device, logger, tb_logger, steps=None, eval_model=None, saved=None,
          best=("checkpoint_best.pt",), last="checkpoint_last.pt", feed="arena", world=None):
    """train_mhop.py:124-227, and train_momentum.py:125-208 of the reference, which is the same loop. What differs between the two comes in
    from the caller: steps, the module with optimizer_for and train_step (default: multihop_dense_retrieval_amd.train); eval_model(), what
    predict() is given (default: model.inference()); saved(), the state dict a checkpoint holds (default: model's); best and last, the
    checkpoint files' names (every name of `best` gets the same tensors). feed: where a step's batch comes from. "arena": the train file is
    tokenised once into a token arena on `device` and every batch is assembled there by one kernel from that step's choices
    (multihop_dense_retrieval_amd/mhop_arena.py); "host": the reference's way, a DataLoader that tokenises six sequences per sample on every
    read. Under one seed the two leave the same checkpoint bytes and the same generator states. world: None, or this rank's dist.TorchWorld
    (module docstring: several ranks); rank 0 alone saves, and `logger` and `tb_logger` are the caller's to silence on the other ranks."""
    import torch
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import dist as mdr_dist, mhop_arena, mhop_data, optim
    from multihop_dense_retrieval_amd import train as mdr_train
    from multihop_dense_retrieval_amd.retriever import move_to_cuda
    steps = steps or mdr_train
    eval_model = eval_model or model.inference
    saved = saved or model.state_dict
    optimizer = steps.optimizer_for(model, args)
    bucket = mdr_dist.GradBucket(model.parameters(), world) if world is not None else None
    rank_rows = (lambda B: mdr_dist.slice_bounds(B, world.size)[world.rank]) if world is not None else None
    global_step, batch_step, best_mrr = 0, 0, 0  # gradient update step; forward batch count
    train_loss_meter = AverageMeter()
    model.train()
    train_dataset = mhop_data.MhopTrainDataset(tokenizer, args.train_file, args.max_q_len, args.max_q_sp_len, args.max_c_len)
    if feed == "arena":  # the batches are already on the device: step_fn's move_to_cuda is a no-op on them
        train_dataloader = mhop_arena.MhopArena.load_or_build(args.train_file, train_dataset, tokenizer).to(device).feed(args.train_batch_size, shuffle=True,
                                                                                                                           rank_rows=rank_rows)
    elif feed == "host":
        train_dataloader = DataLoader(train_dataset, batch_size=args.train_batch_size, collate_fn=collate_fc, num_workers=0, shuffle=True)
    else:
        raise ValueError(f"feed = {feed!r}: \"arena\" or \"host\"")
    t_total = len(train_dataloader) // args.gradient_accumulation_steps * args.num_train_epochs
    warmup_steps = t_total * args.warmup_ratio
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda s: optim.linear_schedule_with_warmup(s, warmup_steps, t_total))
    seeds = torch.Generator().manual_seed(args.seed)  # one dropout seed per forward
    state = {"loss": None}
    if world is not None:  # before the first step: ranks that would train on different data or settings stop here, with a message
        tag = mhop_arena.mhop_arena_tag(tokenizer, args.max_q_len, args.max_q_sp_len, args.max_c_len, True, args.train_file)
        differ = ranks_agree(world, "arena tag, sample count, seed, batch size or world size",
                             hashlib.sha256(f"{tag}|{len(train_dataset)}|{args.seed}|{args.train_batch_size}|{world.size}".encode()).hexdigest())
        if differ:
            sys.exit(differ)

    def check_ranks():
        if world is not None and args.check_ranks:
            checksum = parameter_checksum(model)
            differ = ranks_agree(world, "the parameters' checksum", checksum)
            if differ:
                sys.exit(differ)
            logger.info("ranks agree: %s", checksum)

    def save(*names):
        if world is not None and world.rank != 0:
            return
        for name in names:
            torch.save({k: v.detach().cpu() for k, v in saved().items()}, os.path.join(args.output_dir, name))

    def evaluate():
        mrrs = predict(args, eval_model(), eval_dataloader, device, logger)
        model.train()
        check_ranks()
        return mrrs

    def step_fn(batch, _batch_step):
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=seeds))
        multi = {"world": world, "bucket": bucket} if world is not None else {}
        state["loss"] = steps.train_step(model, move_to_cuda(batch), args, optimizer, seed, **multi)
        train_loss_meter.update(state["loss"].item())

    def update_fn(_batch_step):
        nonlocal global_step, best_mrr
        if bucket is not None:
            bucket.reduce()  # every rank's gradients become the ordered sum over the ranks: the one communication of an update
        optimizer.step()
        scheduler.step()
        global_step += 1
        if tb_logger is not None:
            tb_logger.add_scalar("batch_train_loss", state["loss"].item(), global_step)
            tb_logger.add_scalar("smoothed_train_loss", train_loss_meter.avg, global_step)
        if args.eval_period != -1 and global_step % args.eval_period == 0:
            mrr = evaluate()["mrr_avg"]
            logger.info("Step %d Train loss %.2f MRR %.2f on epoch=%d" % (global_step, train_loss_meter.avg, mrr * 100, epoch))
            if best_mrr < mrr:
                logger.info("Saving model with best MRR %.2f -> MRR %.2f on epoch=%d" % (best_mrr * 100, mrr * 100, epoch))
                save(*best)
                best_mrr = mrr

    logger.info("Start training....")
    for epoch in range(int(args.num_train_epochs)):
        batch_step = mdr_train.run_epoch(train_dataloader, step_fn, update_fn, args.gradient_accumulation_steps, batch_step)
        mrrs = evaluate()
        mrr = mrrs["mrr_avg"]
        logger.info("Step %d Train loss %.2f MRR-AVG %.2f on epoch=%d" % (global_step, train_loss_meter.avg, mrr * 100, epoch))
        if tb_logger is not None:
            for k, v in mrrs.items():
                tb_logger.add_scalar(k, v * 100, epoch)
        save(last)
        if best_mrr < mrr:
            logger.info("Saving model with best MRR %.2f -> MRR %.2f on epoch=%d" % (best_mrr * 100, mrr * 100, epoch))
            save(*best)
            best_mrr = mrr
    check_ranks()
    logger.info("Training finished!")


def main(argv=None):
    from multihop_dense_retrieval_amd.config import train_args
    args = train_args(argv)
    handlers = [logging.StreamHandler()]
    rank, world_size, local_rank = 0, 1, args.local_rank
    if args.do_train:
        rank, world_size, local_rank = rank_setup(args)
        check_train_inputs(args)
        model_name = (f"{args.prefix}-seed{args.seed}-bsz{args.train_batch_size}-fp16{args.fp16}-lr{args.learning_rate}-decay{args.weight_decay}"
                      f"-warm{args.warmup_ratio}-valbsz{args.predict_batch_size}-shared{args.shared_encoder}-multi{args.multi_vector}-scheme{args.scheme}")
        args.output_dir = os.path.join(args.output_dir, date.today().strftime("%m-%d-%Y"), model_name)
        if rank == 0:
            if os.path.exists(args.output_dir) and os.listdir(args.output_dir):
                print(f"output directory {args.output_dir} already exists and is not empty.")
            os.makedirs(args.output_dir, exist_ok=True)
            handlers.insert(0, logging.FileHandler(os.path.join(args.output_dir, "log.txt")))
        else:
            handlers = [logging.NullHandler()]  # rank 0 alone writes log.txt and the log lines
    import numpy as np
    import torch
    from multihop_dense_retrieval_amd import data, mhop_data, retriever
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO, handlers=handlers)
    logger = logging.getLogger(__name__)
    logger.setLevel(logging.INFO)
    logger.info(args)
    if args.no_cuda or not torch.cuda.is_available():
        sys.exit("the retriever runs on a HIP device only (there is no CPU fallback)")
    device = torch.device("cuda", 0 if args.share_gpu else max(local_rank, 0))
    torch.cuda.set_device(device)
    world = join_world(args, world_size)
    logger.info("device %s n_gpu %d distributed training %r", device, 1, world is not None)
    if not os.path.isdir(args.model_name):
        sys.exit(f"--model_name {args.model_name!r} must be a local directory with the RoBERTa config and tokenizer (nothing is downloaded)")
    import transformers
    bert_config = transformers.AutoConfig.from_pretrained(args.model_name, local_files_only=True)
    tokenizer = data.load_tokenizer(args.model_name)
    collate_fc = partial(mhop_data.mhop_collate, pad_id=tokenizer.pad_token_id)
    if args.do_train:
        args.train_batch_size = int(args.train_batch_size / args.accumulate_gradients)
        if args.max_c_len > bert_config.max_position_embeddings:
            raise ValueError("Cannot use sequence length %d because the BERT model was only trained up to sequence length %d" %
                             (args.max_c_len, bert_config.max_position_embeddings))
    # train_mhop.py:94-98. Seeded HERE, after the imports and the config / tokenizer loading above: importing transformers draws from the global
    # `random` generator, and the comparison questions' order of positives is the generator's state at the first __getitem__. In the reference
    # nothing between its seeding and that point draws from it (the model's initialisation uses torch's generator).
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    # a training run evaluates the dev set after every epoch and every --eval-period steps: tokenised once. --do_predict alone is one pass.
    eval_dataloader = dev_batches(args, tokenizer, collate_fc, device, feed="arena" if args.do_train else "host")
    logger.info(f"Num of dev batches: {len(eval_dataloader)}")
    if args.do_train:
        from multihop_dense_retrieval_amd import train as mdr_train
        model = mdr_train.TrainableRetriever(bert_config, args)  # project.* from torch's default initialisers under --seed
        start = encoder_weights(args.model_name, model.shapes)
        if args.init_checkpoint != "":
            ckpt = torch.load(args.init_checkpoint, map_location="cpu")
            start.update({(k[7:] if k.startswith("module.") else k): v for k, v in ckpt.items()})
        start = {k: v for k, v in start.items() if k in model.shapes}
        missing = [k for k in model.shapes if k.startswith("encoder.") and "pooler" not in k and k not in start]
        if missing:
            sys.exit(f"no encoder weights to start from: {args.model_name!r} holds none and --init_checkpoint gives none ({len(missing)} tensors "
                     f"missing, the first {missing[0]})")
        model.load_state_dict(start, strict=False)
        model.to(device)
        print(f"number of trainable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
        tb_logger = None
        if rank == 0:
            try:
                from torch.utils.tensorboard import SummaryWriter
                tb_logger = SummaryWriter(os.path.join(args.output_dir.replace("logs", "tflogs")))
            except ImportError:
                logger.info("TensorBoard is not installed: its scalars are not written")
        train(args, model, tokenizer, collate_fc, eval_dataloader, device, logger, tb_logger, world=world)
        if world is not None:
            import torch.distributed
            torch.distributed.destroy_process_group()
        return
    model = retriever.RobertaRetriever(bert_config, args)
    if args.init_checkpoint != "":
        model = retriever.load_saved(model, args.init_checkpoint, exact=False, map_location="cpu")
    model.to(device)
    if args.do_predict:
        acc = predict(args, model, eval_dataloader, device, logger)
        logger.info(f"test performance {acc}")


if __name__ == "__main__":
    main()
