"""GPU (-m gpu): one training step of the reader on several ranks (reader_train.train_step with a world and a bucket, dist.GradBucket,
DESIGN.md §33), the ranks emulated in one process by dist.LoopbackWorld, on the committed tiny ELECTRA and the --sp-pred batch of
tests/golden/reader_train_ref.npz (B = 4, L = 48) and its first three rows and first row. All comparisons are bit for bit but 5.

1  a hand-written composition, N in {2, 3} x B in {4, 3, 1} (uneven and empty slices), dropout off and at 0.1: per rank
   model(rows, seed=rank_seed(seed, r)), backward under the scale, dist.rank_sum_host over the ranks' flat gradients, FusedAdam. Every gradient,
   parameter and fp16 copy of every rank equals it; the returned loss is rank_sum_host of the partial losses on every rank.
   A batch whose rank-1 rows are negatives only (every starts = -1): that rank's qa_outputs gradients are exactly zero and its partial loss
   is the rank and sp terms alone.
2  under dropout rank 0's rows carry the one-rank masks and rank 1's do not; without dropout every rank's rows are the one-rank rows
3  after three steps every .grad still lies inside the bucket and every FusedAdam built its pointer table once
4  a poisoned gradient on rank 1 alone skips the step on every rank and halves every rank's scale
5  against the one-rank step on the same batch, dropout off: per tensor d_split = |g_N - g_1| / |g_1| is at most 4 x max(d_perm, median
   d_perm), d_perm being the same distance between the one-rank step on the batch and on the batch with its rows reversed (the same
   loss, another summation order): DESIGN.md §31's criterion. A lost, doubled or mis-scaled slice shows at 1 / B.
"""
import numpy as np
import pytest
import torch

import reader_train_ref as ref
from test_reader_train_step_gpu import make_model, same_bits

pytestmark = pytest.mark.gpu

SCALE = 256.0
TAG, SP = ref.SETS[0]  # the batch with sentence labels: --sp-pred on
SEEDS = (0x5EED0123456789AB, 0x0123456789ABCDEF, 7)
QA = ("qa_outputs.weight", "qa_outputs.bias")


@pytest.fixture(scope="module")
def z():
    return ref.golden()


def batch_of(z, B=None, reverse=False, negatives=None):
    batch = {k: v[:B] for k, v in ref.batch_of(z, TAG, "cuda").items()}
    if reverse:
        batch = {k: v.flip(0).contiguous() for k, v in batch.items()}
    if negatives is not None:  # rows lo .. hi - 1 as the dataset builds a negative chain's: no answer span
        batch = {k: v.clone() for k, v in batch.items()}
        batch["starts"][negatives[0]:negatives[1]] = -1
        batch["ends"][negatives[0]:negatives[1]] = -1
    return batch


def rows_of(batch, lo, hi):
    return {k: v[lo:hi] for k, v in batch.items()}


def params(model):
    return dict(model.named_parameters())


def rank_sum_of(tensors):
    from multihop_dense_retrieval_amd.dist import rank_sum_host
    host = np.stack([t.detach().cpu().numpy().reshape(-1) for t in tensors])
    return torch.from_numpy(rank_sum_host(host)).reshape(tensors[0].shape).cuda()


class Ranks:
    """N models from the same weights, their optimizers, a LoopbackWorld and the buckets."""

    def __init__(self, N, p=0.0, loss_scale=SCALE):
        from multihop_dense_retrieval_amd import dist, reader_train
        self.N, self.args = N, ref.make_args(SP)
        self.models = [make_model(SP, p).train() for _ in range(N)]
        self.opts = [reader_train.optimizer_for(m, self.args, loss_scale=loss_scale) for m in self.models]
        self.hub = dist.LoopbackWorld(N)
        self.buckets = [dist.GradBucket(m.parameters(), w) for m, w in zip(self.models, self.hub.ranks)]

    def step(self, batch, seed, between=None, update=True):
        """One train_step, reduce() and opt.step() per emulated rank. Returns per rank (loss, the gradients behind reduce())."""
        from multihop_dense_retrieval_amd import reader_train

        def fn(w):
            r = w.rank
            loss = reader_train.train_step(self.models[r], batch, self.args, self.opts[r], seed, world=w, bucket=self.buckets[r])
            if between is not None:
                between(r)
            self.buckets[r].reduce()
            grads = {k: p.grad.detach().clone() for k, p in params(self.models[r]).items()}
            if update:
                self.opts[r].step()
            return loss, grads

        return self.hub.run(fn)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
def composition(ranks, batch, seed, N, p):
    """The hand-written step on one model of the same weights: (per rank partial loss or None, per rank gradients, the model, its optimizer)."""
    from multihop_dense_retrieval_amd import dist, reader_train
    B = int(batch["input_ids"].shape[0])
    model = make_model(SP, p).train()
    opt = reader_train.optimizer_for(model, ranks.args, loss_scale=SCALE)
    P = params(model)
    parts, per_rank = [], []
    for r, (lo, hi) in enumerate(dist.slice_bounds(B, N)):
        for q in P.values():
            q.grad = torch.zeros_like(q)  # a bucket's views start as zeros and autograd adds onto them
        part = None
        if hi > lo:
            part = model(rows_of(batch, lo, hi), seed=dist.rank_seed(seed, r), half=opt.half)
            opt.scale_loss(part).backward()
            part = part.detach()
        parts.append(part)
        per_rank.append({k: q.grad.clone() for k, q in P.items()})
    return parts, per_rank, model, opt


def check_step(z, N, B, p, negatives=None):
    from multihop_dense_retrieval_amd import dist, reader_train
    seed = SEEDS[0]
    batch = batch_of(z, B, negatives=negatives)
    bounds = dist.slice_bounds(B, N)
    assert (min(hi - lo for lo, hi in bounds) == 0) == (B < N)
    ranks = Ranks(N, p)
    got = ranks.step(batch, seed)
    parts, per_rank, model, opt = composition(ranks, batch, seed, N, p)
    P = params(model)
    want = {k: rank_sum_of([g[k] for g in per_rank]) for k in P}
    host_parts = np.array([[0.0 if q is None else float(q)] for q in parts], np.float32)
    want_loss = torch.from_numpy(dist.rank_sum_host(host_parts)).cuda()
    for r in range(N):
        loss, grads = got[r]
        assert loss.shape == (1,) and same_bits(loss, want_loss), (r, "the loss", loss, want_loss)
        assert set(grads) == set(want)
        for k in want:
            assert same_bits(grads[k], want[k]), (r, k, "the gradient behind reduce()")
    assert any(bool((want[k] != 0).any()) for k in want)
    for k, q in P.items():
        q.grad = want[k].clone()
    opt.step()
    assert opt.read_state()["skipped_total"] == 0
    start = ref.checkpoint(SP)
    for r in range(N):
        mine = params(ranks.models[r])
        for k, q in P.items():
            assert same_bits(mine[k].detach(), q.detach()), (r, k, "parameter")
        assert not same_bits(mine["rank.weight"].detach(), start["rank.weight"].cuda()), (r, "the step moved nothing")
        for k in reader_train.fp16_copy_names(list(P)):
            assert same_bits(ranks.opts[r].half(mine[k]), opt.half(P[k])), (r, k, "fp16 copy")
    return parts, per_rank


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "p0.1"])
@pytest.mark.parametrize("B", [4, 3, 1])
@pytest.mark.parametrize("N", [2, 3])
def test_bit_for_bit_the_hand_written_composition(z, N, B, p):
    check_step(z, N, B, p)


def test_a_rank_of_negatives_alone_gives_qa_outputs_nothing(z):
    """Rows 2 and 3, rank 1's of two, lose their spans. The fallback of an empty marginal contributes exactly 0: no special case."""
    batch = batch_of(z, 4, negatives=(2, 4))
    assert bool((batch["starts"][:2] >= 0).any()), "rank 0 holds no span either: this test shows nothing"
    parts, per_rank = check_step(z, 2, 4, 0.0, negatives=(2, 4))
    for k in QA:
        assert not bool(per_rank[1][k].any()), (k, "a rank without spans moved qa_outputs")
        assert bool(per_rank[0][k].any()) or k == "qa_outputs.bias"  # (the bias's gradient is zero by symmetry, up to rounding)
    assert bool(per_rank[1]["rank.weight"].any()) and bool(per_rank[1]["sp.weight"].any())
    # the partial loss against the rank and sp terms in fp64 on the same fp16 scores: at most 32 non-negative terms, each within 4 ulp
    # (2^-22) of its fp64 value, added in fp32 (32 x 2^-24): 2^-17 + 2^-19 < 1e-5 of the sum
    model = make_model(SP).eval()
    rows = rows_of(batch, 2, 4)
    with torch.no_grad():
        s = model(rows)
    F = torch.nn.functional
    label = rows["label"].cpu().reshape(-1, 1).double()
    rank_term = F.binary_cross_entropy_with_logits(s["rank_score"].double().cpu().reshape(-1, 1), label, reduction="sum")
    sp_term = (F.binary_cross_entropy_with_logits(s["sp_score"].double().cpu(), rows["sent_labels"].cpu().double(), reduction="none")
               * rows["sent_offsets"].cpu() * label).sum() * float(z["meta.sp_weight"])
    want = float(rank_term + sp_term)
    print(f"rank 1's partial loss {float(parts[1]):.9g}, rank + sp terms {want:.9g}")
    assert abs(float(parts[1]) - want) <= 1e-5 * want


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
def test_rank_zero_keeps_the_one_rank_masks_and_rank_one_draws_its_own(z):
    from multihop_dense_retrieval_amd import dist, reader_train
    seed, B = SEEDS[1], 4
    batch = batch_of(z, B)
    (lo0, hi0), (lo1, hi1) = dist.slice_bounds(B, 2)
    names = ("start_logits", "end_logits", "rank_score", "sp_score")
    for p in (0.1, 0.0):
        model = make_model(SP, p).train()
        opt = reader_train.optimizer_for(model, ref.make_args(SP), loss_scale=SCALE)
        drop = seed if p else None
        with torch.no_grad():
            whole = model.scores(batch, opt.half, drop)
            first = model.scores(rows_of(batch, lo0, hi0), opt.half, dist.rank_seed(seed, 0) if p else None)  # the full batch's widths
            second = model.scores(rows_of(batch, lo1, hi1), opt.half, dist.rank_seed(seed, 1) if p else None)
            second_unshifted = model.scores(rows_of(batch, lo1, hi1), opt.half, drop)
        for name in names:
            assert same_bits(first[name], whole[name][lo0:hi0]), (p, name, "rank 0's rows are not the one-rank rows")
            if p:
                assert not same_bits(second[name], whole[name][lo1:hi1]), (p, name)
                assert not same_bits(second[name], second_unshifted[name]), (p, name, "rank 1 shares rank 0's masks")
            else:
                assert same_bits(second[name], whole[name][lo1:hi1]), (p, name, "without dropout a row's scores depend on the rank count")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_gradients_stay_in_the_bucket_and_the_pointer_table_is_built_once(z, monkeypatch):
    from multihop_dense_retrieval_amd import optim
    built = []
    real = optim.build_table
    monkeypatch.setattr(optim, "build_table", lambda rows: built.append(len(rows)) or real(rows))
    ranks = Ranks(2, 0.1)
    batch = batch_of(z, 3)
    keys = []
    for seed in SEEDS:
        ranks.step(batch, seed)
        keys.append([opt._key for opt in ranks.opts])
    assert len(built) == 2, built  # one table per rank's optimizer, at its first step
    for r in range(2):
        assert keys[0][r] is keys[1][r] is keys[2][r]
        for k, p in params(ranks.models[r]).items():
            assert p.grad is not None and ranks.buckets[r].contains(p.grad), (r, k, "the gradient left the bucket")
            assert p.grad.data_ptr() % 16 == 0, (r, k, "the optimizer reads 16 bytes at a time")
            assert not bool(p.grad.any()), (r, k, "the step did not zero the gradient in place")
        assert ranks.opts[r].read_state()["adam_step"] == 3
        assert not bool(ranks.buckets[r].flat.any())


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_an_overflow_on_one_rank_skips_the_step_on_every_rank(z):
    from multihop_dense_retrieval_amd import _lib, optim
    ranks = Ranks(3, 0.0, loss_scale="dynamic")
    for opt in ranks.opts:
        _lib.check(optim.lib().mdr_optim_state_init(_lib.ptr(opt._state), SCALE, 0, _lib.current_stream_ptr()))
    batch = batch_of(z, 4)
    start = ref.checkpoint(SP)
    seen = {}

    def poison(r):
        grads = [p.grad for p in params(ranks.models[r]).values()]
        seen[r] = all(bool(torch.isfinite(g).all()) for g in grads)
        if r == 1:
            grads[3].view(-1)[5] = float("inf")

    got = ranks.step(batch, SEEDS[2], between=poison)
    assert seen == {0: True, 1: True, 2: True}, "a gradient overflowed by itself: this test shows nothing"
    for r in range(3):
        st = ranks.opts[r].read_state()
        assert st["skipped_last"] == 1 and st["adam_step"] == 0 and st["loss_scale"] == SCALE / 2, (r, st)
        assert any(not bool(torch.isfinite(g).all()) for g in got[r][1].values()), (r, "the overflow did not reach this rank")
        for k, p in params(ranks.models[r]).items():
            assert same_bits(p.detach(), start[k].cuda()), (r, k, "a skipped step changed a parameter")
    ranks.step(batch, SEEDS[2])  # the next step, at half the scale, is clean everywhere
    assert all(ranks.opts[r].read_state()["adam_step"] == 1 for r in range(3))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_against_the_one_rank_step(z):
    """Measured on an MI355X (the tiny ELECTRA, B = 4, scale 256): the median d_perm is 6.77e-8, and the largest d_split / bound is 0.280 at
    two ranks and 0.274 at three; both columns per tensor are printed and kept in profiles/reader_multirank.md."""
    from multihop_dense_retrieval_amd import reader_train
    args = ref.make_args(SP)

    def one_rank(batch):
        model = make_model(SP).train()
        opt = reader_train.optimizer_for(model, args, loss_scale=SCALE)
        loss = reader_train.train_step(model, batch, args, opt, SEEDS[0])
        return {k: p.grad.detach().double() for k, p in params(model).items()}, loss

    g1, loss1 = one_rank(batch_of(z, 4))
    gp, _ = one_rank(batch_of(z, 4, reverse=True))
    live = [k for k in g1 if float(g1[k].norm()) > 0.0]
    assert all(ref.zero_by_symmetry(k) for k in g1 if k not in live), [k for k in g1 if k not in live]
    d_perm = {k: float((gp[k] - g1[k]).norm() / g1[k].norm()) for k in live}
    median = float(np.median(list(d_perm.values())))
    assert median > 0.0, "reversing the batch changed no bit: the yardstick is empty"
    for N in (2, 3):
        ranks = Ranks(N)
        lossN, grads = ranks.step(batch_of(z, 4), SEEDS[0], update=False)[0]
        gN = {k: g.double() for k, g in grads.items()}
        # dropout off, so the rows' scores and their terms are the one-rank step's (test 2); only the order of at most 4 x (2 + 4) fp32
        # additions differs: 24 x 2^-24 < 1e-5 of a sum of non-negative terms. A division by N would show at 1 / 2.
        assert abs(float(lossN) - float(loss1)) <= 1e-5 * abs(float(loss1))
        worst = 0.0
        print(f"N = {N}: median d_perm {median:.3e}, loss {float(lossN):.9g} against {float(loss1):.9g}")
        for k in g1:
            if k not in live:  # zero by symmetry and exactly zero on one rank: rounding noise at most, against the sibling's norm
                assert float(gN[k].norm()) <= 4.0 * median * float(g1[ref.zero_by_symmetry(k)].norm()), (N, k)
                continue
            d_split = float((gN[k] - g1[k]).norm() / g1[k].norm())
            bound = 4.0 * max(d_perm[k], median)
            worst = max(worst, d_split / bound)
            print(f"  {k:60s} d_split {d_split:.3e}  d_perm {d_perm[k]:.3e}  bound {bound:.3e}")
        print(f"N = {N}: the largest d_split / bound is {worst:.3f}")
        for k in live:
            assert float((gN[k] - g1[k]).norm() / g1[k].norm()) <= 4.0 * max(d_perm[k], median), (N, k)
