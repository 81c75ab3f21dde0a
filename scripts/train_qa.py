"""Drop-in for the reference's scripts/train_qa.py on the HIP reader: inference (--do_predict / --do_test) and training (--do_train).

    python scripts/train_qa.py --do_predict --predict_file <retrieval jsonl with sp / answer> --init_checkpoint qa_electra.pt \
        --model_name <ELECTRA / BERT dir or cached name> --sp-pred --fp16 --max_ans_len 35 --save-prediction out.json
    python scripts/train_qa.py --do_train --prefix electra_large --model_name <ELECTRA dir> --train_file train.jsonl --predict_file dev.jsonl \
        --train_batch_size 128 --predict_batch_size 1024 --learning_rate 5e-5 --fp16 --seed 42 --eval-period 250 --max_seq_len 512 \
        --max_q_len 64 --gradient_accumulation_steps 8 --neg-num 5 --sp-pred --sp-weight 0.05 --warmup-ratio 0.1 --num_train_epochs 7

Flags are the reference's (mdr/qa/config.py), parsed verbatim. --do_predict runs predict() with the fixed 0.8 combination factor and
writes its log lines and --save-prediction; --do_test runs eval_final(). The dev batches are the reference's (sequential,
--predict_batch_size chains) and are loaded in this process (num_workers is accepted and not used: the forward is on the device and data
workers would fork a process that holds it). Numerics are apex O1's whether or not --fp16 is given (the README's QA command passes it). The
config and the tokenizer come from --model_name, a local directory or a model in the local cache; nothing is downloaded.

--do_train is lines 138-211 of the reference's script on multihop_dense_retrieval_amd/reader_train.py. The training set
(qa_train_data.QATrainDataset, the reference's QADataset(train=True)) is prepared once into an item arena on the device
(qa_train_arena.QATrainArena); every step's batch is built there by mdr_reader_train_assemble from the indices qa_train_data.MhopSampler
draws, and nothing is tokenised after start-up. Kept from the reference: the sampler's n_gpu = 8 default (len(qid2gold) % 8 questions
sit out every epoch, and len(loader), t_total and the warm-up overstate the real step count, so the schedule never reaches zero), the
negatives shuffled in place under the global `random` generator seeded once by --seed, the short last batch, the accumulation boundary
(batch_step + 1) % gradient_accumulation_steps == 0, the loss meter fed by loss.item(), the evaluation every --eval-period steps and after
every epoch (predict() over eleven combination factors), its log lines, and checkpoint_best.pt when em improves: the state dict as plain
fp32 CPU tensors with the reference's keys. The encoder starts from the weights in the --model_name directory, the pooler and the heads
from torch.nn.Linear's default initialiser under --seed (the draws are not claimed to be the reference's: it builds the encoder first, with
another transformers version); --init_checkpoint overwrites both. Every forward draws its dropout seed from a torch.Generator seeded with
--seed. One addition: checkpoint_last.pt after the last epoch, as the retriever's CLI writes; the reference saves only when em improves, so
a run whose dev em stays 0 would leave no weights. TensorBoard scalars are written only when torch.utils.tensorboard imports.

--piece-arena (not a flag of the reference, off by default) feeds the same loop from qa_train_pieces.QATrainPieces: one stored row per
question and per distinct passage, five integers per item, every batch spliced on the device by mdr_reader_train_compose, byte for byte the
batches of the default arena. It is the path for a train file with many candidate chains per question (the README's
train_retrieval_b100_k100_sp.json): the default arena runs __getitem__ on every chain of every question, in one process, before the first
step. The pieces are built before the model goes to the device (this process holds no stream, no memory there yet), with
min(16, --num_workers) forked workers, and cached beside the train file. It
takes chains of exactly two passages; another length exits and names the default arena.

--eval-arena (not a flag of the reference, off by default) runs --do_predict, --do_test and every evaluation inside --do_train from
qa_eval.QAEvalPieces instead of QADataset + qa_collate: the predict file's questions and DISTINCT passages are tokenised once (cached beside
the file as <predict file>.qa_eval_pieces.npz, built before the model goes to the device with min(16, --num_workers) forked workers), every
batch -- the same consecutive --predict_batch_size chains -- is written on the device by mdr_reader_assemble, bit for bit qa_collate's rows,
decode()'s outputs stay on the device in a score table, mdr_reader_select picks per question and combination factor the chain that predict()'s
in-place sorts leave on top (the largest (key_k, ..., key_0), lowest index among equals: DESIGN.md §32), and only the distinct winners are
decoded to strings. Log lines, metrics, --save-prediction bytes and checkpoint_best.pt decisions are the host path's. It exits with a message
that begins "--eval-arena is not supported: " and names the host path for a chain that does not have exactly two passages, an _id on two
lines of the file, or a tokenizer for which "yes" or "no" is not a single WordPiece.

Several ranks: `torchrun --nproc-per-node N scripts/train_qa.py --do_train ...`. The rank comes from --local_rank (the
reference's flag) or from LOCAL_RANK, RANK and WORLD_SIZE; with neither, or with a world of one rank, everything above holds unchanged, bit
for bit. N ranks train what one rank trains: every rank makes the same host draws and computes the full batch's widths, assembles and
forwards rows dist.slice_bounds(B, N)[rank] of it under dist.rank_seed(seed, rank) and backpropagates its partial loss -- the reference's
loss is a plain sum over the rows, so nothing is gathered before it --, the gradients are summed over the ranks in rank order by
mdr_rank_sum (dist.GradBucket) before every optimizer step, and the logged loss is the partial losses added in rank order the same way. A
DEVIATION from the reference: under DataParallel it takes loss.mean() over the replicas' sums and chunks the batch by ceil(B / N); here
there is no division by N and the slices are balanced, because the README's reader recipe runs on one device and that objective is the
published one. MhopSampler's n_gpu = 8 stays what it is: a property of the sampler, not of the launch. With --eval-arena every evaluation
(and --do_predict, --do_test) is split: rank r decodes a contiguous run of whole dev batches (qa_eval.batch_deal), the score tables' rows are
exchanged as bytes, and every rank selects, decodes the winners, computes the metrics and takes the same checkpoint_best.pt decision;
without it every rank evaluates the whole dev set by the host path and rank 0 logs a line that says so. --dist-backend nccl (RCCL, the
default) or gloo; --share-gpu puts every rank on device 0 (gloo only: a rehearsal on one card); --dist-timeout SECONDS goes to
init_process_group; --check-ranks compares a checksum of the parameters' bits over the ranks behind every evaluation and at the end
(`ranks agree: <hex>`): the meanings, defaults and code of scripts/train_mhop.py. Rank 0 alone makes the output directory and writes
log.txt, TensorBoard, the checkpoints and the log lines. The process group is joined before anything opens the device: rank 0 builds and
writes the caches (their workers are forked) while the others wait at a gloo barrier and then load them. Before the first step the ranks
compare a digest of the arena's and the dev pieces' tags, the item count, --seed, --train_batch_size, --gradient_accumulation_steps,
--neg-num and the world size.

Whatever keeps --do_train from running exits with a message that begins "training is not supported: ": a --model_name that the trainable
reader refuses (it is built for ELECTRA, from a local directory; the default bert-base-uncased is refused), no HIP device, a missing
--train_file, more than dist.MAX_RANKS ranks, --share-gpu without gloo or without a launcher, more ranks than visible devices without
--share-gpu, a launcher without MASTER_ADDR / MASTER_PORT. The command line and the launcher's environment are checked for these before any
file or device is opened.
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
if os.path.join(ROOT, "scripts") not in sys.path:  # (train_mhop.py's launch plumbing, for a caller that loads this file from elsewhere)
    sys.path.append(os.path.join(ROOT, "scripts"))


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
    p.add_argument("--piece-arena", action="store_true")  # not in the reference: the training feed's piece arena (module docstring)
    p.add_argument("--eval-arena", action="store_true")  # not in the reference: evaluation from a dev piece arena (module docstring)
    # several ranks (module docstring), not in the reference: the meanings and defaults of scripts/train_mhop.py
    p.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl")  # "nccl" is RCCL
    p.add_argument("--share-gpu", action="store_true")  # every rank on device 0, gloo only: the rehearsal on one card
    p.add_argument("--dist-timeout", type=int, default=1800)  # seconds, init_process_group's
    p.add_argument("--check-ranks", action="store_true")  # compare the parameters' checksum over the ranks at every evaluation
    return p.parse_args(argv)


def launch(args, environ=None):
    """(rank, world size, local rank) of this process: scripts/train_mhop.py's rank_setup, whose refusals exit here, under --do_train with
    the prefix every refusal of training carries. (0, 1, -1) without --local_rank and without a launcher: the one-rank run."""
    import train_mhop
    try:
        return train_mhop.rank_setup(args, environ)
    except SystemExit as e:
        if args.do_train and isinstance(e.code, str):
            sys.exit("training is not supported: " + e.code.replace("scripts/train_mhop.py", "scripts/train_qa.py"))
        raise


class Ranks:
    """What the script needs of a launch of several ranks: the dist.TorchWorld of scripts/train_mhop.py's join_world and a gloo group of its
    own, whose barrier touches no device (the pieces' workers are forked before this process opens one)."""

    def __init__(self, args, rank, size):
        from datetime import timedelta
        import torch.distributed
        import train_mhop
        self.rank, self.size = rank, size
        self.world = train_mhop.join_world(args, size)
        self.host = torch.distributed.new_group(backend="gloo", timeout=timedelta(seconds=args.dist_timeout))

    def rank_zero_first(self, fn):
        """fn() on rank 0, then on the others: rank 0 builds and writes a cache, the others wait at the barrier and load it."""
        import torch.distributed
        if self.rank == 0:
            out = fn()
            torch.distributed.barrier(group=self.host)
            return out
        torch.distributed.barrier(group=self.host)
        return fn()

    def close(self):
        import torch.distributed
        torch.distributed.destroy_process_group()


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


def eval_pieces_for(args, tokenizer, logger):
    """--eval-arena: the predict file as pieces (qa_eval.QAEvalPieces), built or loaded BEFORE this process holds the device: its workers
    are forked. Whatever the pieces do not take exits and names the host path."""
    from multihop_dense_retrieval_amd import qa_eval
    try:
        return qa_eval.QAEvalPieces.load_or_build(args.predict_file, tokenizer, args.max_seq_len, args.max_q_len, args.predict_batch_size,
                                                  log=logger.info, workers=min(16, args.num_workers))
    except ValueError as e:
        sys.exit(f"--eval-arena is not supported: {e} (run without --eval-arena: the host path, QADataset and qa_collate in this process, "
                 "takes every predict file)")


def check_train_inputs(args, environ=None):
    """What --do_train needs, read from the command line and the launcher's environment alone, before any file or device is opened: every
    refusal begins alike. Returns launch()'s (rank, world size, local rank)."""
    no = "training is not supported: "
    name = args.model_name
    if "electra" not in name.lower() or not os.path.isdir(name):
        sys.exit(f"{no}--model_name {name!r} is not a local ELECTRA directory (the trainable reader is built for ELECTRA, QAModel's own pooler; "
                 "the config, the tokenizer and the weights come from that directory and nothing is downloaded)")
    ranks = launch(args, environ)
    import torch
    if args.no_cuda or not torch.cuda.is_available():
        sys.exit(f"{no}no HIP device is visible (the reader trains on a HIP device only; there is no CPU fallback)")
    for flag, path in (("--train_file", args.train_file), ("--predict_file", args.predict_file)):
        if not os.path.isfile(path):
            sys.exit(f"{no}{flag} {path!r}: no such file")
    if args.init_checkpoint != "" and not os.path.isfile(args.init_checkpoint):
        sys.exit(f"{no}--init_checkpoint {args.init_checkpoint!r}: no such file")
    if args.gradient_accumulation_steps < 1 or args.train_batch_size < 1:
        sys.exit(f"{no}--gradient_accumulation_steps and --train_batch_size must be at least 1")
    return ranks


class AverageMeter:
    """mdr/qa/utils.py:85-101 of the reference."""

    def __init__(self):
        self.val, self.avg, self.sum, self.count = 0, 0, 0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def arena_batches(arena, pad_id, device, world=None):
    """The product's feed: one epoch's indices go to the device once; every batch is mdr_reader_train_assemble on a slice of them, its
    widths from the arena's host metadata (no synchronisation). world (a dist.TorchWorld or a rank of dist.LoopbackWorld): every rank is
    handed the same indices and computes the full batch's widths, and assembles rows dist.slice_bounds(B, N)[rank] of it alone, which the
    batch says under reader_train.RANK_ROWS; a rank without rows makes no call and yields that entry alone."""
    import torch
    from multihop_dense_retrieval_amd import dist as mdr_dist, qa_train_arena, reader_train

    def feed(indices, batch_size):
        on_dev = torch.tensor(indices, dtype=torch.int64, device=device)
        for lo in range(0, len(indices), batch_size):
            out_len, n_sent, n_span = arena.batch_shape(indices[lo:lo + batch_size])
            if world is None:
                out = arena.assemble(on_dev[lo:lo + batch_size], out_len, n_sent, n_span, pad_id)
                yield {k: out[k] for k in qa_train_arena.NET_KEYS}
                continue
            B = len(indices[lo:lo + batch_size])
            first, behind = mdr_dist.slice_bounds(B, world.size)[world.rank]
            net = {}
            if behind > first:
                out = arena.assemble(on_dev[lo + first:lo + behind], out_len, n_sent, n_span, pad_id)
                net = {k: out[k] for k in qa_train_arena.NET_KEYS}
            net[reader_train.RANK_ROWS] = (first, behind, B)
            yield net
    return feed


def host_batches(dataset, pad_id, device):
    """The reference's feed, in this process: __getitem__ per row, qa_train_collate, upload. Not reachable from the command line; the tests
    and scripts/measure/qa_train_loop_bench.py compare the product's feed with it."""
    import torch
    from multihop_dense_retrieval_amd import qa_train_data

    def feed(indices, batch_size):
        for lo in range(0, len(indices), batch_size):
            net = qa_train_data.qa_train_collate([dataset[i] for i in indices[lo:lo + batch_size]], pad_id=pad_id)["net_inputs"]
            yield {k: v.to(device=device, dtype=torch.int64) for k, v in net.items()}  # (qa_collate's paragraph_mask is float 0 / 1)
    return feed


def train(args, model, sampler, feed, evaluate, logger, tb_logger=None, loss_scale="dynamic", world=None):
    """train_qa.py:138-211. sampler: qa_train_data.MhopSampler; feed(indices, batch_size) yields the net_inputs of one epoch's batches;
    evaluate() returns predict()'s metrics on the current weights; loss_scale: reader_train.optimizer_for's (the script runs the dynamic one).
    Returns {"loss": every batch's, "epoch_means", "global_step", "skipped_steps": the
    optimizer steps the dynamic loss scale skipped while it came down from 2^16, as apex skips them (the schedule advances all the same)}.
    world: None, or this rank's dist.TorchWorld (or a rank of dist.LoopbackWorld) -- `feed` then yields this rank's rows
    (arena_batches(..., world)), the gradients live in a dist.GradBucket that is reduced before every optimizer step, rank 0 alone saves,
    --check-ranks compares the parameters' checksum behind every evaluation and at the end, and `logger` and `tb_logger` are the caller's
    to silence on the other ranks."""
    import torch
    from multihop_dense_retrieval_amd import dist as mdr_dist, optim, qa_train_data, reader_train
    from multihop_dense_retrieval_amd import train as mdr_train
    optimizer = reader_train.optimizer_for(model, args, loss_scale=loss_scale)
    bucket = mdr_dist.GradBucket(model.parameters(), world) if world is not None else None
    multi = {"world": world, "bucket": bucket} if world is not None else {}
    global_step, batch_step, best_em = 0, 0, 0  # gradient update step; forward batch count
    train_loss_meter = AverageMeter()
    model.train()
    t_total = qa_train_data.total_steps(sampler, args.train_batch_size, args.gradient_accumulation_steps, args.num_train_epochs)
    warmup_steps = t_total * args.warmup_ratio
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lambda s: optim.linear_schedule_with_warmup(s, warmup_steps, t_total))
    seeds = torch.Generator().manual_seed(args.seed)  # one dropout seed per forward
    state, losses, epoch_means = {"loss": None}, [], []

    def save(name):
        if not args.output_dir or (world is not None and world.rank != 0):  # (in-process callers that want no files)
            return
        torch.save({k: v.detach().float().cpu() for k, v in model.state_dict().items()}, os.path.join(args.output_dir, name))

    def check_ranks():
        if world is not None and getattr(args, "check_ranks", False):
            import train_mhop
            checksum = train_mhop.parameter_checksum(model)
            differ = train_mhop.ranks_agree(world, "the parameters' checksum", checksum)
            if differ:
                sys.exit(differ)
            logger.info("ranks agree: %s", checksum)

    def step_fn(batch, _batch_step):
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=seeds))
        state["loss"] = reader_train.train_step(model, batch, args, optimizer, seed, **multi)
        losses.append(state["loss"].item())
        train_loss_meter.update(losses[-1])

    def update_fn(_batch_step):
        nonlocal global_step, best_em
        if bucket is not None:
            bucket.reduce()  # every rank's gradients become the ordered sum over the ranks: the one communication of an update
        optimizer.step()
        scheduler.step()
        global_step += 1
        if tb_logger is not None:
            tb_logger.add_scalar("batch_train_loss", losses[-1], global_step)
            tb_logger.add_scalar("smoothed_train_loss", train_loss_meter.avg, global_step)
        if args.eval_period != -1 and global_step % args.eval_period == 0:
            em = evaluate()["em"]
            model.train()
            check_ranks()
            logger.info("Step %d Train loss %.2f em %.2f on epoch=%d" % (global_step, train_loss_meter.avg, em * 100, epoch))
            if best_em < em:
                logger.info("Saving model with best em %.2f -> em %.2f on step=%d" % (best_em * 100, em * 100, global_step))
                save("checkpoint_best.pt")
                best_em = em

    logger.info("Start training....")
    for epoch in range(int(args.num_train_epochs)):
        first = len(losses)
        batch_step = mdr_train.run_epoch(feed(list(iter(sampler)), args.train_batch_size), step_fn, update_fn, args.gradient_accumulation_steps,
                                         batch_step)
        epoch_means.append(sum(losses[first:]) / max(1, len(losses) - first))
        em = evaluate()["em"]
        model.train()
        check_ranks()
        logger.info("Step %d Train loss %.2f em %.2f" % (global_step, train_loss_meter.avg, em * 100))
        if tb_logger is not None:
            tb_logger.add_scalar("dev_em", em * 100, global_step)
        if best_em < em:
            logger.info("Saving model with best em %.2f -> em %.2f on epoch=%d" % (best_em * 100, em * 100, epoch))
            save("checkpoint_best.pt")
            best_em = em
    save("checkpoint_last.pt")  # not in the reference (module docstring)
    check_ranks()
    logger.info("Training finished!")
    return {"loss": losses, "epoch_means": epoch_means, "global_step": global_step, "skipped_steps": optimizer.read_state()["skipped_total"]}


def initial_state(args, config, model):
    """{name: tensor} the run starts from: the encoder of the --model_name directory (when it holds weights), the pooler and the heads from
    torch.nn.Linear's default initialiser, --init_checkpoint over both. Exits when an encoder tensor has no source."""
    import torch
    import transformers
    H = config.hidden_size
    start = {}
    for name, n_out in (("pooler.dense", H), ("qa_outputs", 2), ("rank", 1), ("sp", 1)):
        if name + ".weight" in model.shapes:
            lin = torch.nn.Linear(H, n_out)
            start[name + ".weight"], start[name + ".bias"] = lin.weight.detach(), lin.bias.detach()
    try:
        hf = transformers.AutoModel.from_pretrained(args.model_name, local_files_only=True)
        start.update({"encoder." + k: v.detach().float() for k, v in hf.state_dict().items() if "encoder." + k in model.shapes})
    except (OSError, ValueError):
        pass
    if args.init_checkpoint != "":
        ckpt = torch.load(args.init_checkpoint, map_location="cpu")
        start.update({(k[7:] if k.startswith("module.") else k): v.float() for k, v in ckpt.items()})
    start = {k: v for k, v in start.items() if k in model.shapes}
    missing = [k for k in model.shapes if k not in start]
    if missing:
        sys.exit(f"training is not supported: no weights to start from: {args.model_name!r} holds none and --init_checkpoint gives none "
                 f"({len(missing)} tensors missing, the first {missing[0]})")
    return start


def start_training(args, config, tokenizer, device, logger, ranks=None):
    """ranks: None, or the Ranks of a launch of several (module docstring). Whatever writes a cache runs on rank 0 first; the process group
    was joined before this point and the device is selected only behind the forked workers."""
    import hashlib
    import random
    import numpy as np
    import torch
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import qa_data, qa_eval, qa_train_arena, qa_train_data, qa_train_pieces, reader_train
    if args.shared_norm:
        assert (args.train_batch_size // 1) == args.neg_num + 1  # chains of each question are on the same gpu (n_gpu = 1)
    # train_qa.py:78-80. Seeded HERE, after the imports and the config / tokenizer loading: importing transformers draws from the global
    # `random` generator, and nothing between this point and the sampler's first shuffle does.
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    try:
        model = reader_train.TrainableReader(config, args)
    except NotImplementedError as e:
        sys.exit(f"training is not supported: {e}")
    eval_pieces = eval_loader = None
    world = ranks.world if ranks is not None else None
    first = ranks.rank_zero_first if ranks is not None else (lambda fn: fn())
    if args.eval_arena:  # built HERE, as the training pieces below: before model.to(device), its workers are forked processes
        eval_pieces = first(lambda: eval_pieces_for(args, tokenizer, logger))
        logger.info(f"Num of dev batches: {len(eval_pieces.batches)}")
    else:
        collate = partial(qa_data.qa_collate, pad_id=tokenizer.pad_token_id)
        eval_dataset = qa_data.QADataset(tokenizer, args.predict_file, args.max_seq_len, args.max_q_len)
        eval_loader = DataLoader(eval_dataset, batch_size=args.predict_batch_size, collate_fn=collate, num_workers=0)
        logger.info(f"Num of dev batches: {len(eval_loader)}")
        if world is not None:
            logger.info(f"every one of the {world.size} ranks evaluates the whole dev set by the host path: --eval-arena splits its batches over the ranks")
    if args.init_checkpoint != "":
        logger.info(f"Loading model from {args.init_checkpoint}")
    model.load_state_dict(initial_state(args, config, model))
    pieces = None
    if args.piece_arena:  # built HERE, before model.to(device) makes this process hold the device: its workers are forked processes
        train_dataset = qa_train_data.QATrainDataset(tokenizer, args.train_file, args.max_seq_len, args.max_q_len)
        try:
            pieces = first(lambda: qa_train_pieces.QATrainPieces.load_or_build(args.train_file, train_dataset, tokenizer, log=logger.info,
                                                                               workers=min(16, args.num_workers)))
        except ValueError as e:
            sys.exit(f"training is not supported: {e} (run without --piece-arena: the default item arena takes chains of any length)")
    if ranks is not None:
        torch.cuda.set_device(device)  # (the collectives of a device backend run on the current device)
    model.to(device)
    if eval_pieces is not None:
        eval_pieces.to(device)
    print(f"number of trainable parameters: {sum(p.numel() for p in model.parameters() if p.requires_grad)}")
    tb_logger = None
    if ranks is None or ranks.rank == 0:
        try:
            from torch.utils.tensorboard import SummaryWriter
            tb_logger = SummaryWriter(os.path.join(args.output_dir.replace("logs", "tflogs")))
        except ImportError:
            logger.info("TensorBoard is not installed: its scalars are not written")
    if pieces is None:
        train_dataset = qa_train_data.QATrainDataset(tokenizer, args.train_file, args.max_seq_len, args.max_q_len)
    sampler = qa_train_data.MhopSampler(train_dataset, num_neg=args.neg_num)
    arena = (pieces if pieces is not None else
             first(lambda: qa_train_arena.QATrainArena.load_or_build(args.train_file, train_dataset, tokenizer, log=logger.info))).to(device)
    if world is not None:  # before the first step: ranks that would train on different data or settings stop here, with a message
        import train_mhop
        tags = ((qa_train_pieces.train_pieces_tag if pieces is not None else qa_train_arena.train_arena_tag)(tokenizer, args.max_seq_len, args.max_q_len, args.train_file),
                qa_eval.eval_pieces_tag(tokenizer, args.max_q_len, args.predict_file) if eval_pieces is not None else f"host|{os.stat(args.predict_file).st_size}")
        told = (f"{tags[0]}|{tags[1]}|{len(train_dataset)}|{args.seed}|{args.train_batch_size}|{args.gradient_accumulation_steps}|{args.neg_num}|"
                f"{world.size}")
        differ = train_mhop.ranks_agree(world, "arena tag, dev pieces' tag, item count, seed, batch size, accumulation steps, negatives or world size",
                                        hashlib.sha256(told.encode()).hexdigest())
        if differ:
            sys.exit(differ)

    def evaluate():
        if eval_pieces is not None:
            table = qa_eval.score_table(model.inference(), eval_pieces, args.max_ans_len, **({"world": world} if world is not None else {}))
            return qa_eval.predict_metrics(eval_pieces, table, tokenizer, args.sp_pred, logger, fixed_thresh=None)[0]
        chains, gold = run_batches(model.inference(), eval_loader, args, final=False)
        return qa_data.predict_metrics(chains, gold, args.sp_pred, logger, fixed_thresh=None)[0]

    if world is None:
        return train(args, model, sampler, arena_batches(arena, tokenizer.pad_token_id, device), evaluate, logger, tb_logger)
    return train(args, model, sampler, arena_batches(arena, tokenizer.pad_token_id, device, world), evaluate, logger, tb_logger, world=world)


def main(argv=None):
    args = train_args(argv)
    rank, world_size, local_rank = check_train_inputs(args) if args.do_train else launch(args)
    import json
    import torch
    import transformers
    from torch.utils.data import DataLoader
    from multihop_dense_retrieval_amd import qa_data, qa_eval, reader
    date_curr = date.today().strftime("%m-%d-%Y")
    model_name = (f"{args.prefix}-seed{args.seed}-bsz{args.train_batch_size}-fp16{args.fp16}-lr{args.learning_rate}-decay{args.weight_decay}"
                  f"-neg{args.neg_num}-sn{args.shared_norm}-adam{args.use_adam}-warm{args.warmup_ratio}-sp{args.sp_weight}")
    args.output_dir = os.path.join(args.output_dir, date_curr, model_name)
    handlers = [logging.NullHandler()]  # rank 0 alone makes the output directory and writes log.txt and the log lines
    if rank == 0:
        if args.do_train and os.path.exists(args.output_dir) and os.listdir(args.output_dir):
            print(f"output directory {args.output_dir} already exists and is not empty.")
        os.makedirs(args.output_dir, exist_ok=True)
        handlers = [logging.FileHandler(os.path.join(args.output_dir, "log.txt")), logging.StreamHandler()]
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s - %(message)s", datefmt="%m/%d/%Y %H:%M:%S", level=logging.INFO, handlers=handlers)
    logger = logging.getLogger(__name__)
    logger.setLevel(logging.INFO)
    logger.info(args)
    if args.no_cuda or not torch.cuda.is_available():
        sys.exit("the reader runs on a HIP device only (there is no CPU fallback)")
    device = torch.device("cuda", 0 if args.share_gpu else max(local_rank, 0))
    # the process group is joined HERE, before anything opens the device: the pieces' workers are forked, and the ranks meet at a gloo barrier
    ranks = Ranks(args, rank, world_size) if world_size > 1 else None
    logger.info("device %s n_gpu %d distributed training %r", device, 1, ranks is not None)
    config = transformers.AutoConfig.from_pretrained(args.model_name, local_files_only=True)
    tokenizer = transformers.BertTokenizer.from_pretrained(args.model_name, local_files_only=True)
    if args.do_train:
        out = start_training(args, config, tokenizer, device, logger, ranks)
        if ranks is not None:
            ranks.close()
        return out
    model = reader.QAModel(config, args)
    pieces = loader = None
    world = ranks.world if ranks is not None else None
    if args.eval_arena:  # before model.to(device): the workers that tokenise the passages are forked
        pieces = ranks.rank_zero_first(lambda: eval_pieces_for(args, tokenizer, logger)) if ranks is not None else eval_pieces_for(args, tokenizer, logger)
        logger.info(f"Num of dev batches: {len(pieces.batches)}")
    else:
        collate = partial(qa_data.qa_collate, pad_id=tokenizer.pad_token_id)
        dataset = qa_data.QADataset(tokenizer, args.predict_file, args.max_seq_len, args.max_q_len)
        loader = DataLoader(dataset, batch_size=args.predict_batch_size, collate_fn=collate, num_workers=0)
        logger.info(f"Num of dev batches: {len(loader)}")
        if world is not None:
            logger.info(f"every one of the {world.size} ranks evaluates the whole dev set by the host path: --eval-arena splits its batches over the ranks")
    if args.init_checkpoint != "":
        logger.info(f"Loading model from {args.init_checkpoint}")
        reader.load_saved(model, args.init_checkpoint, exact=False, map_location="cpu")
    if ranks is not None:
        torch.cuda.set_device(device)
    model.to(device).eval()
    table = None
    if pieces is not None and (args.do_predict or args.do_test):
        table = qa_eval.score_table(model, pieces.to(device), args.max_ans_len, **({"world": world} if world is not None else {}))
    if args.do_predict:
        if pieces is not None:
            metrics, best_res = qa_eval.predict_metrics(pieces, table, tokenizer, args.sp_pred, logger, fixed_thresh=0.8)
        else:
            chains, gold = run_batches(model, loader, args, final=False)
            metrics, best_res = qa_data.predict_metrics(chains, gold, args.sp_pred, logger, fixed_thresh=0.8)
        if args.save_prediction != "" and rank == 0:
            with open(args.save_prediction, "w") as f:
                json.dump(best_res, f)
        logger.info(f"test performance {metrics}")
    elif args.do_test:
        if pieces is not None:
            results = qa_eval.final_results(pieces, table, tokenizer, args.sp_pred, weight=0.8)
        else:
            chains, _ = run_batches(model, loader, args, final=True)
            results = qa_data.final_results(chains, weight=0.8)
        if args.save_prediction != "" and rank == 0:
            with open(args.save_prediction, "w") as f:
                json.dump(results, f)
    if ranks is not None:
        ranks.close()


if __name__ == "__main__":
    main()
