"""GPU (-m gpu): one training step on several ranks (train.train_step with a world and a bucket, dist.GradBucket), the ranks
emulated in one process by dist.LoopbackWorld, on oracle.seeded.TINY with batches of four or fewer samples.

1  bit for bit a hand-written composition, N in {2, 3} x B in {4, 3, 1} (uneven and empty slices), without and with dropout: rank-wise
   model(rows) under the rank's seed, torch.cat, mhop_loss_outputs, backward, dist.rank_sum_host over the ranks' gradients, FusedAdam. Every
   gradient, parameter and fp16 copy of every rank equals it and the loss bits are equal on all ranks.
2  under dropout rank 0's rows carry the one-rank masks and rank 1's do not; without dropout every rank's rows are the one-rank rows
3  after three steps every .grad still lies inside the bucket and every FusedAdam built its pointer table once
4  a poisoned gradient on rank 1 alone skips the step on every rank and halves every rank's scale
5  against the one-rank step on the same batch, dropout off: per tensor d_split = |g_N - g_1| / |g_1| is at most 4 x max(d_perm, median
   d_perm), d_perm being the same distance between the one-rank step on the batch and on the batch with its samples reversed (the same
   loss, another summation order). Both are reorderings of the same rounding errors; a lost, doubled or mis-scaled slice shows at 1 / B.
"""
import types

import numpy as np
import pytest
import torch

import encoder_chain_ref as ch
from encoder_chain_dev import same_bits
from oracle import seeded

pytestmark = pytest.mark.gpu

GEOM = seeded.TINY
SCALE = 256.0
SEEDS = (ch.DROP_SEED, 0x0123456789ABCDEF, 7)


def make_args(**kw):
    base = dict(learning_rate=2e-5, adam_epsilon=1e-8, max_grad_norm=2.0, weight_decay=0.01, gradient_accumulation_steps=1, fp16=True, momentum=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.fixture(scope="module")
def weights():
    return {k: torch.from_numpy(np.asarray(v)) for k, v in seeded.make_state_dict(ch.WEIGHT_SEED, GEOM).items()}


@pytest.fixture(scope="module")
def pairs():
    return ch.loss_batches(GEOM)  # {name: (ids, mask)}: four samples, widths 48 and 160


def make_model(weights, p=0.0):
    from multihop_dense_retrieval_amd import retriever, train
    cfg = retriever.RobertaConfig(vocab_size=GEOM["vocab"], hidden_size=GEOM["hidden"], num_hidden_layers=GEOM["layers"], num_attention_heads=GEOM["heads"],
                                  intermediate_size=GEOM["ffn"], max_position_embeddings=GEOM["max_pos"], layer_norm_eps=GEOM["ln_eps"], pad_token_id=GEOM["pad_id"])
    cfg.hidden_dropout_prob = cfg.attention_probs_dropout_prob = p
    m = train.TrainableRetriever(cfg, None)
    m.load_state_dict(weights)
    return m.cuda().train()


def batch_of(pairs, B=None, reverse=False):
    from multihop_dense_retrieval_amd.retriever import RobertaRetriever
    out = {}
    for name, key in RobertaRetriever.FORWARD_INPUTS:
        ids, mask = (np.asarray(a)[:B] for a in pairs[name])
        if reverse:
            ids, mask = ids[::-1].copy(), mask[::-1].copy()
        out[f"{key}_input_ids"], out[f"{key}_mask"] = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    return out


def rows_of(batch, lo, hi):
    return {k: v[lo:hi] for k, v in batch.items()}


def trainable(model):
    return {k: p for k, p in model.named_parameters() if p.requires_grad}


def rank_sum_of(tensors):
    from multihop_dense_retrieval_amd.dist import rank_sum_host
    host = np.stack([t.detach().cpu().numpy().reshape(-1) for t in tensors])
    return torch.from_numpy(rank_sum_host(host)).reshape(tensors[0].shape).cuda()


class Ranks:
    """N models from the same weights, their optimizers, a LoopbackWorld and the buckets (made inside the emulated ranks, as a process would)."""

    def __init__(self, weights, N, p=0.0, loss_scale=SCALE):
        from multihop_dense_retrieval_amd import dist, train
        self.N, self.args = N, make_args()
        self.models = [make_model(weights, p) for _ in range(N)]
        self.opts = [train.optimizer_for(m, self.args, loss_scale=loss_scale) for m in self.models]
        self.hub = dist.LoopbackWorld(N)
        self.buckets = [dist.GradBucket(m.parameters(), w) for m, w in zip(self.models, self.hub.ranks)]

    def step(self, batch, seed, between=None, update=True):
        """One train_step, reduce() and opt.step() per emulated rank. Returns per rank (loss, the gradients behind reduce())."""
        from multihop_dense_retrieval_amd import train

        def fn(w):
            r = w.rank
            loss = train.train_step(self.models[r], batch, self.args, self.opts[r], seed, world=w, bucket=self.buckets[r])
            if between is not None:
                between(r)
            self.buckets[r].reduce()
            grads = {k: p.grad.detach().clone() for k, p in trainable(self.models[r]).items()}
            if update:
                self.opts[r].step()
            return loss, grads

        return self.hub.run(fn)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, ch.DROP_P], ids=["nodrop", "p0.1"])
@pytest.mark.parametrize("B", [4, 3, 1])
@pytest.mark.parametrize("N", [2, 3])
def test_bit_for_bit_the_hand_written_composition(weights, pairs, N, B, p):
    from multihop_dense_retrieval_amd import criterions, dist, train
    seed = SEEDS[0]
    batch = batch_of(pairs, B)
    bounds = dist.slice_bounds(B, N)
    assert (min(hi - lo for lo, hi in bounds) == 0) == (B < N)
    ranks = Ranks(weights, N, p)
    got = ranks.step(batch, seed)
    # the composition, on one model of the same weights
    ref = make_model(weights, p)
    ref_opt = train.optimizer_for(ref, ranks.args, loss_scale=SCALE)
    P = trainable(ref)
    outs = [ref(rows_of(batch, lo, hi), seed=dist.rank_seed(seed, r), half=ref_opt.half) if hi > lo else None for r, (lo, hi) in enumerate(bounds)]
    losses, per_rank = [], []
    for r in range(N):
        full = {name: torch.cat([outs[j][name] if j == r else outs[j][name].detach() for j in range(N) if outs[j] is not None]) for name in train.ENCODE_INDEX}
        loss = criterions.mhop_loss_outputs(full, ranks.args)
        for q in P.values():
            q.grad = torch.zeros_like(q)  # a bucket's views start as zeros and autograd adds onto them
        if outs[r] is not None:
            ref_opt.scale_loss(loss).backward()
        losses.append(loss.detach())
        per_rank.append({k: q.grad.clone() for k, q in P.items()})
    want = {k: rank_sum_of([g[k] for g in per_rank]) for k in P}
    for r in range(N):
        loss, grads = got[r]
        assert same_bits(loss.reshape(1), losses[r].reshape(1)) and same_bits(loss.reshape(1), got[0][0].reshape(1)), (r, "the loss")
        assert set(grads) == set(want)
        for k in want:
            assert same_bits(grads[k], want[k]), (r, k, "the gradient behind reduce()")
    assert any(bool((want[k] != 0).any()) for k in want)
    for k, q in P.items():
        q.grad = want[k].clone()
    ref_opt.step()
    assert ref_opt.read_state()["skipped_total"] == 0
    for r in range(N):
        mine = trainable(ranks.models[r])
        for k, q in P.items():
            assert same_bits(mine[k].detach(), q.detach()), (r, k, "parameter")
        assert not same_bits(mine["project.0.weight"].detach(), weights["project.0.weight"].cuda()), (r, "the step moved nothing")
        for k in train.fp16_copy_names(list(P)):
            assert same_bits(ranks.opts[r].half(mine[k]), ref_opt.half(P[k])), (r, k, "fp16 copy")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
def test_rank_zero_keeps_the_one_rank_masks_and_rank_one_draws_its_own(weights, pairs):
    from multihop_dense_retrieval_amd import dist, train
    seed, B = SEEDS[1], 4
    batch = batch_of(pairs, B)
    (lo0, hi0), (lo1, hi1) = dist.slice_bounds(B, 2)
    for p in (ch.DROP_P, 0.0):
        model = make_model(weights, p)
        opt = train.optimizer_for(model, make_args(), loss_scale=SCALE)
        with torch.no_grad():
            whole = model(batch, seed=seed, half=opt.half)
            first = model(rows_of(batch, lo0, hi0), seed=dist.rank_seed(seed, 0), half=opt.half)
            second = model(rows_of(batch, lo1, hi1), seed=dist.rank_seed(seed, 1), half=opt.half)
            second_unshifted = model(rows_of(batch, lo1, hi1), seed=seed, half=opt.half)
        for name in train.ENCODE_INDEX:
            assert same_bits(first[name], whole[name][lo0:hi0]), (p, name, "rank 0's rows are not the one-rank rows")
            if p:
                assert not same_bits(second[name], whole[name][lo1:hi1]), (p, name)
                assert not same_bits(second[name], second_unshifted[name]), (p, name, "rank 1 shares rank 0's masks")
                assert not same_bits(second[name], first[name]), (p, name)
            else:
                assert same_bits(second[name], whole[name][lo1:hi1]), (p, name, "without dropout a sequence's embedding depends on the rank count")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_gradients_stay_in_the_bucket_and_the_pointer_table_is_built_once(weights, pairs, monkeypatch):
    from multihop_dense_retrieval_amd import optim
    built = []
    real = optim.build_table
    monkeypatch.setattr(optim, "build_table", lambda rows: built.append(len(rows)) or real(rows))
    ranks = Ranks(weights, 2, ch.DROP_P)
    batch = batch_of(pairs, 3)
    keys = []
    for seed in SEEDS:
        ranks.step(batch, seed)
        keys.append([opt._key for opt in ranks.opts])
    assert len(built) == 2, built  # one table per rank's optimizer, at its first step
    for r in range(2):
        assert keys[0][r] is keys[1][r] is keys[2][r]
        for k, p in trainable(ranks.models[r]).items():
            assert p.grad is not None and ranks.buckets[r].contains(p.grad), (r, k, "the gradient left the bucket")
            assert not bool(p.grad.any()), (r, k, "the step did not zero the gradient in place")
        assert ranks.opts[r].read_state()["adam_step"] == 3
        assert not bool(ranks.buckets[r].flat.any())


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
def test_an_overflow_on_one_rank_skips_the_step_on_every_rank(weights, pairs):
    from multihop_dense_retrieval_amd import _lib, optim
    ranks = Ranks(weights, 3, 0.0, loss_scale="dynamic")
    for opt in ranks.opts:
        _lib.check(optim.lib().mdr_optim_state_init(_lib.ptr(opt._state), SCALE, 0, _lib.current_stream_ptr()))
    batch = batch_of(pairs, 4)
    seen = {}

    def poison(r):
        grads = [p.grad for p in trainable(ranks.models[r]).values()]
        seen[r] = all(bool(torch.isfinite(g).all()) for g in grads)
        if r == 1:
            grads[3].view(-1)[5] = float("inf")

    got = ranks.step(batch, SEEDS[2], between=poison)
    assert seen == {0: True, 1: True, 2: True}, "a gradient overflowed by itself: this test shows nothing"
    for r in range(3):
        st = ranks.opts[r].read_state()
        assert st["skipped_last"] == 1 and st["adam_step"] == 0 and st["loss_scale"] == SCALE / 2, (r, st)
        assert any(not bool(torch.isfinite(g).all()) for g in got[r][1].values()), (r, "the overflow did not reach this rank")
        for k, p in trainable(ranks.models[r]).items():
            assert same_bits(p.detach(), weights[k].cuda()), (r, k, "a skipped step changed a parameter")
    got = ranks.step(batch, SEEDS[2])  # the next step, at half the scale, is clean everywhere
    assert all(ranks.opts[r].read_state()["adam_step"] == 1 for r in range(3))


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
def test_against_the_one_rank_step(weights, pairs):
    """Measured on an MI355X (TINY, B = 4, scale 256): the median d_perm is 1.53e-7, d_split lies between 1.9e-8 and 2.8e-7, and the largest
    d_split / bound is 0.315 at two ranks and 0.303 at three; both columns per tensor are in profiles/multirank_train.md."""
    from multihop_dense_retrieval_amd import train
    args = make_args()

    def one_rank(batch):
        model = make_model(weights)
        opt = train.optimizer_for(model, args, loss_scale=SCALE)
        train.train_step(model, batch, args, opt, SEEDS[0])
        return {k: p.grad.detach().double() for k, p in trainable(model).items()}

    g1 = one_rank(batch_of(pairs, 4))
    gp = one_rank(batch_of(pairs, 4, reverse=True))
    live = [k for k in g1 if float(g1[k].norm()) > 0.0]
    assert len(live) >= len(g1) - len(ch.zero_grad_names(GEOM))
    d_perm = {k: float((gp[k] - g1[k]).norm() / g1[k].norm()) for k in live}
    median = float(np.median(list(d_perm.values())))
    assert median > 0.0, "reversing the batch changed no bit: the yardstick is empty"
    for N in (2, 3):
        ranks = Ranks(weights, N)
        gN = {k: g.double() for k, g in ranks.step(batch_of(pairs, 4), SEEDS[0], update=False)[0][1].items()}
        worst = 0.0
        print(f"N = {N}: median d_perm {median:.3e}")
        for k in g1:
            if k not in live:
                assert not bool(gN[k].any()), (N, k, "a gradient that is exactly zero on one rank")
                continue
            d_split = float((gN[k] - g1[k]).norm() / g1[k].norm())
            bound = 4.0 * max(d_perm[k], median)
            worst = max(worst, d_split / bound)
            print(f"  {k:60s} d_split {d_split:.3e}  d_perm {d_perm[k]:.3e}  bound {bound:.3e}")
        print(f"N = {N}: the largest d_split / bound is {worst:.3f}")
        for k in live:
            assert float((gN[k] - g1[k]).norm() / g1[k].norm()) <= 4.0 * max(d_perm[k], median), (N, k)
