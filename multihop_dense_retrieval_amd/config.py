"""Flag sets of the corpus-encoder CLI and of the retriever's training and dev-set evaluation: `encode_args()` = `common_args()` + two
flags, `train_args()` = `common_args()` + the optimisation flags, flag for flag as
/root/reference/mdr/retrieval/config.py:14-69,71-105,107-112 (flags a CLI does not use are accepted and ignored so
existing command lines keep working)."""
import argparse


def common_args():
    p = argparse.ArgumentParser()
    # task
    p.add_argument("--train_file", type=str, default="../data/nq-with-neg-train.txt")
    p.add_argument("--predict_file", type=str, default="../data/nq-with-neg-dev.txt")
    p.add_argument("--num_workers", default=30, type=int)
    p.add_argument("--do_train", default=False, action="store_true")
    p.add_argument("--do_predict", default=False, action="store_true")
    # model
    p.add_argument("--model_name", default="bert-base-uncased", type=str)
    p.add_argument("--init_checkpoint", type=str, default="")
    p.add_argument("--max_c_len", default=512, type=int)
    p.add_argument("--max_q_len", default=50, type=int)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--fp16_opt_level", type=str, default="O1")
    p.add_argument("--no_cuda", default=False, action="store_true")
    p.add_argument("--local_rank", type=int, default=-1)
    p.add_argument("--max_q_sp_len", default=50, type=int)
    p.add_argument("--sent-level", action="store_true")
    p.add_argument("--rnn-retriever", action="store_true")
    p.add_argument("--predict_batch_size", default=512, type=int)
    p.add_argument("--shared-encoder", action="store_true")
    # multi vector scheme / momentum / NQ trial: training-side switches, parsed for compatibility
    p.add_argument("--multi-vector", type=int, default=1)
    p.add_argument("--scheme", type=str, default="none")
    p.add_argument("--momentum", action="store_true")
    p.add_argument("--init-retriever", type=str, default="")
    p.add_argument("--k", type=int, default=38400)
    p.add_argument("--m", type=float, default=0.999)
    p.add_argument("--nq-multi", action="store_true")
    return p


def encode_args(argv=None):
    p = common_args()
    p.add_argument("--embed_save_path", type=str, default="")
    p.add_argument("--is_query_embed", action="store_true")
    # addition of this build (off by default): also write <embed_save_path>.bf16.npy, the matrix as bf16 bit patterns
    p.add_argument("--save_bf16", action="store_true")
    # addition (default behaviour is result-identical to the reference): passages are tokenised in windows of
    # predict_batch_size x this many items, sorted by token count inside a window and batched by length; every embedding
    # still lands in its own row. 1 = the reference's order-of-appearance batches.
    p.add_argument("--length_bucket_window", type=int, default=16)
    return p.parse_args(argv)


def train_args(argv=None):
    """config.py:71-105: the flags of scripts/train_mhop.py (--do_train and --do_predict)."""
    p = common_args()
    p.add_argument("--prefix", type=str, default="eval")
    p.add_argument("--weight_decay", default=0.0, type=float)
    p.add_argument("--temperature", default=1, type=float)
    p.add_argument("--output_dir", default="./logs", type=str)
    p.add_argument("--train_batch_size", default=128, type=int)
    p.add_argument("--learning_rate", default=1e-5, type=float)
    p.add_argument("--adam_epsilon", default=1e-8, type=float)
    p.add_argument("--num_train_epochs", default=50, type=float)
    p.add_argument("--save_checkpoints_steps", default=20000, type=int)
    p.add_argument("--iterations_per_loop", default=1000, type=int)
    p.add_argument("--accumulate_gradients", type=int, default=1)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--eval-period", type=int, default=2500)
    p.add_argument("--max_grad_norm", default=2.0, type=float)
    p.add_argument("--stop-drop", default=0, type=float)
    p.add_argument("--use-adam", action="store_true")
    p.add_argument("--warmup-ratio", default=0, type=float)
    # several ranks (scripts/train_mhop.py --do_train under a launcher): not the reference's flags
    p.add_argument("--dist-backend", choices=("nccl", "gloo"), default="nccl")  # "nccl" is RCCL
    p.add_argument("--share-gpu", action="store_true")  # every rank on device 0, gloo only: the rehearsal on one card
    p.add_argument("--dist-timeout", type=int, default=1800)  # seconds, init_process_group's
    p.add_argument("--check-ranks", action="store_true")  # compare the parameters' checksum over the ranks at every evaluation
    return p.parse_args(argv)
