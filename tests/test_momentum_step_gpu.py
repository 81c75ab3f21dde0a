"""GPU (-m gpu): multihop_dense_retrieval_amd/momentum.py -- MomentumRetriever, optimizer_for and train_step -- on oracle.seeded.TINY and DEEP
with B = 4 and a queue of K = 20 rows.

1  composition: one momentum.train_step gives the loss and every encoder_q gradient of the hand-written composition (the q side through the
   trainable encoder, the c side through a SECOND TrainableRetriever of the same weights under no_grad with the same seed, then
   criterions.mhop_loss_outputs over a copy of the queue), bit for bit
2  queue and frozen key encoder over three steps: after a step rows [ptr, ptr + 2B) are that step's [c1; c2] and the rest is untouched, the
   third step writes four rows and wraps the pointer to 0, the loss is computed on the queue as it stood before the enqueue; encoder_k's
   eval outputs keep their bits, encoder_q's do not, and no tensor of encoder_k is in the optimizer
3  a non-finite gradient skips the step and halves the scale
4  against the reference: the golden first train batch, the golden initial queue, the toy checkpoint, dropout 0: the first step's loss
5  learning: the golden dev batches twice at a constant 1e-4: every second-pass loss is below its first-pass loss
"""
import json
import os
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

import encoder_chain_ref as ch
from encoder_chain_dev import same_bits
from oracle import seeded

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GEOMS = [pytest.param(seeded.TINY, id="TINY"), pytest.param(seeded.DEEP, id="DEEP")]
K = 20
SEEDS = (ch.DROP_SEED, 0x0123456789ABCDEF, 7)  # one dropout seed per step
# Case 4. MEASURED_REL is the deviation of the first run on an MI355X (device 18.438253 against the reference's 18.430634: 4.134e-4,
# profiles/momentum_train_step.md); the bound is twice that. As a condition it may not exceed 1e-2: DESIGN.md §24 records 0.1 % for the same
# comparison of scripts/train_mhop.py.
MEASURED_REL = 4.14e-4
REF_LOSS_REL_BOUND = 2 * MEASURED_REL


def config_of(geom, p=0.0):
    from multihop_dense_retrieval_amd import retriever
    cfg = retriever.RobertaConfig(vocab_size=geom["vocab"], hidden_size=geom["hidden"], num_hidden_layers=geom["layers"], num_attention_heads=geom["heads"],
                                  intermediate_size=geom["ffn"], max_position_embeddings=geom["max_pos"], layer_norm_eps=geom["ln_eps"], pad_token_id=geom["pad_id"])
    cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob = p, p
    return cfg


def make_args(**kw):
    base = dict(learning_rate=2e-5, adam_epsilon=1e-8, max_grad_norm=2.0, weight_decay=0.01, gradient_accumulation_steps=1, fp16=True, momentum=True, k=K,
                m=0.999, init_retriever="")
    base.update(kw)
    return types.SimpleNamespace(**base)


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def make_momentum(geom, args, sd=None, p=0.0, queue=None):
    from multihop_dense_retrieval_amd import momentum
    torch.manual_seed(11)  # the queue's torch.randn
    m = momentum.MomentumRetriever(config_of(geom, p), args)
    m.encoder_q.load_state_dict(tensors(seeded.make_state_dict(ch.WEIGHT_SEED, geom) if sd is None else sd))
    if queue is not None:
        m.bank.queue.copy_(torch.from_numpy(queue))
    return m.cuda().train()


def make_trainable(geom, p=0.0):
    from multihop_dense_retrieval_amd import train
    m = train.TrainableRetriever(config_of(geom, p), None)
    m.load_state_dict(tensors(seeded.make_state_dict(ch.WEIGHT_SEED, geom)))
    return m.cuda().train()


def batch_of(pairs):
    from multihop_dense_retrieval_amd.retriever import RobertaRetriever
    out = {}
    for name, key in RobertaRetriever.FORWARD_INPUTS:
        out[f"{key}_input_ids"], out[f"{key}_mask"] = (torch.from_numpy(np.asarray(a)).cuda() for a in pairs[name])
    return out


def grads_of(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_one_step_is_the_hand_written_composition(geom):
    from multihop_dense_retrieval_amd import criterions, momentum, train
    from multihop_dense_retrieval_amd.retriever import RobertaRetriever
    args = make_args()
    model = make_momentum(geom, args, p=ch.DROP_P)
    opt = momentum.optimizer_for(model, args, loss_scale=256.0)
    batch, seed = batch_of(ch.loss_batches(geom)), SEEDS[0]
    queue0 = model.queue.clone()
    assert tuple(queue0.shape) == (K, geom["hidden"]) and queue0.is_cuda and int(model.queue_ptr) == 0
    loss = momentum.train_step(model, batch, args, opt, seed)

    tq, tk = make_trainable(geom, ch.DROP_P), make_trainable(geom, ch.DROP_P)
    ref_opt = train.optimizer_for(tq, args, loss_scale=256.0)
    outs = {}
    for name, key in RobertaRetriever.FORWARD_INPUTS:
        ids, mask = batch[f"{key}_input_ids"], batch[f"{key}_mask"]
        if name in ("q", "q_sp1"):
            outs[name] = tq.encode(ids, mask, ref_opt.half, (seed, train.ENCODE_INDEX[name]))
        else:
            with torch.no_grad():
                outs[name] = tk.encode(ids, mask, None, (seed, train.ENCODE_INDEX[name]))
    ref_loss = criterions.mhop_loss_outputs(outs, args, queue=queue0.clone())
    ref_opt.scale_loss(ref_loss).backward()
    assert same_bits(loss.reshape(1), ref_loss.detach().reshape(1)), (float(loss), float(ref_loss))
    got, want = grads_of(model.encoder_q), grads_of(tq)
    assert set(got) == set(want) == set(train.trainable_names([k for k, _ in tq.named_parameters()]))
    for k in want:
        assert same_bits(got[k], want[k]), (k, "an encoder_q gradient is not the composition's")
    assert all(g is None for g in (p.grad for p in tk.parameters()))
    # the step's [c1; c2] went into the queue behind the loss
    new = torch.cat([outs["c1"], outs["c2"]])
    assert same_bits(model.queue[:8], new) and same_bits(model.queue[8:], queue0[8:]) and int(model.queue_ptr) == 8
    assert not same_bits(criterions.mhop_loss_outputs(outs, args, queue=model.queue.clone()).detach().reshape(1), loss.reshape(1)), \
        "the loss on the queue after the enqueue has the same bits: the order of score and enqueue is not shown"


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_three_steps_fill_the_queue_and_leave_the_key_encoder_frozen(geom):
    from multihop_dense_retrieval_amd import criterions, momentum, retriever
    args = make_args()
    model = make_momentum(geom, args, p=ch.DROP_P)
    opt = momentum.optimizer_for(model, args, loss_scale=256.0)
    batch = batch_of(ch.loss_batches(geom))
    ids, mask = batch["c1_input_ids"], batch["c1_mask"]
    k_before, q_before = model.encoder_k.encode_seq(ids, mask).clone(), model.encoder_q.inference().encode_seq(ids, mask).clone()
    assert same_bits(k_before, q_before)  # param_k.copy_(param_q)
    written = []
    for step, seed in enumerate(SEEDS):
        before, ptr = model.queue.clone(), int(model.queue_ptr)
        with torch.no_grad():
            outs = model(batch, seed=seed, half=opt.half)  # the step's forward again: the key side does not depend on the step before it
        want_loss = criterions.mhop_loss_outputs(outs, args, queue=before.clone()).detach()
        loss = momentum.train_step(model, batch, args, opt, seed)
        assert same_bits(loss.reshape(1), want_loss.reshape(1)), (step, "the loss is not the one on the queue before the enqueue")
        new = torch.cat([outs["c1"], outs["c2"]])
        n = min(new.shape[0], K - ptr)
        written.append(n)
        assert same_bits(model.queue[ptr:ptr + n], new[:n]), (step, "the enqueued rows")
        keep = torch.ones(K, dtype=torch.bool, device="cuda")
        keep[ptr:ptr + n] = False
        assert same_bits(model.queue[keep], before[keep]), (step, "rows outside [ptr, ptr + n) were written")
        assert int(model.queue_ptr) == (ptr + n) % K
        opt.step()
    assert written == [8, 8, 4] and int(model.queue_ptr) == 0
    st = opt.read_state()
    assert st["skipped_total"] == 0 and st["adam_step"] == len(SEEDS), st
    assert same_bits(model.encoder_k.encode_seq(ids, mask), k_before), "the key encoder moved"
    assert not same_bits(model.encoder_q.inference().encode_seq(ids, mask), q_before), "the question encoder did not move"
    # eval(): the question side is encoder_q's current weights, the passage side the frozen key encoder
    model.eval()
    with torch.no_grad():
        e = model(batch)
    assert same_bits(e["c1"], k_before) and same_bits(e["q"], model.encoder_q.inference().encode_seq(batch["q_input_ids"], batch["q_mask"]))
    model.train()
    # nothing of the key encoder can be stepped: it is an inference handle without a parameter, and the optimizer holds encoder_q's leaves
    assert isinstance(model.encoder_k, retriever.RobertaRetriever) and not isinstance(model.encoder_k, torch.nn.Module)
    mine = {id(p) for g in opt.param_groups for p in g["params"]}
    trainable = {id(p) for n, p in model.encoder_q.named_parameters() if p.requires_grad}
    assert mine == trainable and {id(p) for p in model.parameters() if p.requires_grad} == trainable
    assert all(n.startswith("encoder_q.") for n, _ in model.named_parameters())


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_gradient_skips_the_step_and_halves_the_scale():
    """The scale is put at 2^24: the loss's fp16 gradient (1 / B of it per row) overflows at once, whatever the weights."""
    from multihop_dense_retrieval_amd import _lib, momentum, optim
    from multihop_dense_retrieval_amd._lib import ptr
    geom = seeded.TINY
    args = make_args()
    model = make_momentum(geom, args)
    opt = momentum.optimizer_for(model, args)  # the dynamic scale
    set_scale = lambda s: _lib.check(optim.lib().mdr_optim_state_init(ptr(opt._state), float(s), 0, _lib.current_stream_ptr()))  # noqa: E731
    batch = batch_of(ch.loss_batches(geom))
    must = 2.0 ** 24
    set_scale(must)
    before = {k: v.detach().clone() for k, v in model.named_parameters()}
    momentum.train_step(model, batch, args, opt, seed=1)
    assert any(not bool(torch.isfinite(g).all()) for g in grads_of(model).values()), "nothing overflowed at a scale that must"
    opt.step()
    st = opt.read_state()
    assert st["skipped_last"] == 1 and st["adam_step"] == 0 and st["loss_scale"] == must / 2, st
    for k, v in model.named_parameters():
        assert same_bits(v.detach(), before[k]), (k, "a skipped step changed a parameter")
    set_scale(256.0)
    loss = momentum.train_step(model, batch, args, opt, seed=2)
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads_of(model).values())
    opt.step()
    st = opt.read_state()
    assert st["skipped_last"] == 0 and st["adam_step"] == 1, st


# ---- 4, 5 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import gen_mhop_eval_golden as gen
    with tempfile.TemporaryDirectory() as tmp:
        a = gen.build_assets(tmp)
    meta = json.load(open(os.path.join(GOLD, "momentum_train_ref.json")))
    z = np.load(os.path.join(GOLD, "momentum_train_ref.npz"))
    return a, meta, z


def golden_batch(z, prefix):
    from multihop_dense_retrieval_amd.retriever import RobertaRetriever
    keys = [f"{key}_{part}" for _, key in RobertaRetriever.FORWARD_INPUTS for part in ("input_ids", "mask")]
    return {k: torch.from_numpy(z[f"{prefix}.{k}"].astype(np.int64)).cuda() for k in keys}


def test_first_step_loss_against_the_references(toy):
    """The reference's run is fp32 on the CPU with dropout 0; the device computes in fp16 with fp32 accumulation. Same weights (the toy
    checkpoint), same batch, same queue."""
    from multihop_dense_retrieval_amd import momentum
    a, meta, z = toy
    args = make_args(learning_rate=meta["learning_rate"], weight_decay=0.0, fp16=False, k=meta["k"])
    model = make_momentum(a["geom"], args, sd=a["sd"], queue=z["queue0"])
    opt = momentum.optimizer_for(model, args, loss_scale=256.0)
    loss = float(momentum.train_step(model, golden_batch(z, "t0"), args, opt, seed=0))
    want = meta["loss"][0]
    rel = abs(loss - want) / abs(want)
    print(f"first-step loss: device {loss:.6f} reference {want:.6f} relative deviation {rel:.3e} (bound {REF_LOSS_REL_BOUND:.1e})")
    assert REF_LOSS_REL_BOUND <= 1e-2
    assert rel <= REF_LOSS_REL_BOUND, (loss, want, rel)
    assert int(model.queue_ptr) == meta["queue_ptr"][0]


def test_learning_lowers_every_loss_on_the_second_pass(toy):
    """As tests/test_train_step_gpu.py's learning case, for the q side only: constant lr 1e-4, weight decay 0, dropout 0, fp32 scores, fixed
    loss scale 2^8, K = 20 (the golden initial queue), the six committed dev batches twice. A halving is not asked for: two thirds of the
    columns' encoders are frozen, and the queue's rows change under the loss. Second-pass over first-pass loss measured on an MI355X:
    0.850 0.607 0.526 0.519 0.523 0.732 (first pass 19.47 / 24.69 / 19.99 / 20.26 / 16.46 / 30.33)."""
    from multihop_dense_retrieval_amd import momentum
    a, meta, z = toy
    dev = np.load(os.path.join(GOLD, "mhop_eval_ref.npz"))
    batches = [golden_batch(dev, f"b{bi}") for bi in range(6)]
    args = make_args(learning_rate=1e-4, weight_decay=0.0, fp16=False)
    model = make_momentum(a["geom"], args, sd=a["sd"], queue=z["queue0"])
    opt = momentum.optimizer_for(model, args, loss_scale=256.0)
    losses = [[], []]
    for rnd in range(2):
        for b in batches:
            losses[rnd].append(momentum.train_step(model, b, args, opt, seed=0))
            opt.step()
    losses = [[float(x) for x in row] for row in losses]
    for rnd in range(2):
        print(f"pass {rnd + 1}: " + " / ".join(f"{x:.2f}" for x in losses[rnd]))
    print("ratios " + " ".join(f"{b / a_:.3f}" for a_, b in zip(*losses)))
    assert opt.read_state()["skipped_total"] == 0
    for i, (first, second) in enumerate(zip(*losses)):
        assert second < first, (i, first, second)
