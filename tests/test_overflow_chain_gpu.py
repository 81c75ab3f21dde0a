"""GPU (-m gpu): the overflow contract on the whole chain: one Chain of tests/encoder_chain_dev.py, six encodes of the L48
batch (120 tokens each), the O1 in-batch loss and optim.FusedAdam over the chain's leaves in the reference's two weight-decay groups, fp16
copies kept, dynamic loss scale, lr = 2e-5. Every Linear is handed the optimizer's fp16 copy of its weight. The host side is
tests/overflow_ref.py: G1, the largest magnitude a gradient-rounding point of the reference regime is handed at scale 1, says which scales
are safe (s G1 <= 65504 / 2), which must overflow (s G1 >= 2 * 65520) and which, at most two, are undecided.

C  no poison survives a skipped step: after a step at a scale that must overflow everything keeps its bits and every .grad is +0; the next
   backward at a safe scale gives the bits of the same backward from fresh leaves on a NaN-seeded allocator.
D  the scaler finds its scale on the chain's real gradients: ten steps from 4 x the first must-overflow scale with scale_window = 2; the
   counters follow optim_ref.advance, every clean step is optim_ref.replay_update bit for bit on the device's own .grad, the backward with
   and without the fp16 copies agrees bit for bit, and after the weights moved the gradients still meet criterion E at the moved parameters.
"""
import time
import types

import numpy as np
import pytest
import torch

import encoder_chain_ref as ch
import optim_ref
import overflow_ref as ov
from encoder_chain_dev import Chain, check_e, params, poison, same_bits
from multihop_dense_retrieval_amd._lib import ptr

pytestmark = pytest.mark.gpu

CFG = ov.CHAIN
COUNTERS = ("loss_scale", "unskipped", "adam_step", "b1_pow", "b2_pow", "skipped_last", "skipped_total", "bias1", "bias2")


def make_opt(P, init_scale):
    from multihop_dense_retrieval_amd import optim
    nd = [k for k in P if any(s in k for s in ov.NO_DECAY)]
    groups = [{"params": [P[k] for k in P if k not in nd], "weight_decay": CFG["weight_decay"]}, {"params": [P[k] for k in nd], "weight_decay": 0.0}]
    assert groups[0]["params"] and groups[1]["params"]
    return optim.FusedAdam(groups, lr=CFG["lr"], betas=CFG["betas"], eps=CFG["eps"], max_grad_norm=CFG["max_grad_norm"], loss_scale="dynamic",
                           scale_window=CFG["scale_window"], fp16_copies=True, init_scale=init_scale)


def decay_of(opt):
    return {id(p): float(g["weight_decay"]) for g in opt.param_groups for p in g["params"]}


def scaled_loss(P, scale, half=None):
    """(the loss, the loss times `scale`, a device scalar, the six Chains) of six encodes through one Chain each"""
    from multihop_dense_retrieval_amd import criterions
    batches = ov.chain_batches()
    cs = {k: Chain(P, *batches[k], half=half) for k in ch.KEYS}
    loss = criterions.mhop_loss_outputs({k: cs[k].out for k in ch.KEYS}, types.SimpleNamespace(fp16=True))
    return loss, loss * scale, cs


def read_state(opt):
    from multihop_dense_retrieval_amd import optim
    raw = opt._state.cpu().numpy().view(np.uint8)[:optim.STATE_DTYPE.itemsize].view(optim.STATE_DTYPE)[0]
    return {k: raw[k] for k in optim.STATE_DTYPE.names}


def assert_counters(got, model, label):
    for k in COUNTERS:
        a, b = np.asarray(got[k]), np.asarray(model[k]).astype(got[k].dtype)
        assert a.tobytes() == b.tobytes(), (label, k, got[k], model[k])


def snapshot(P, opt):
    """clones of p, m, v and the fp16 copies"""
    snap = {}
    for k, p in P.items():
        st = opt.state[p]
        snap[k] = dict(p=p.detach().clone(), m=st["exp_avg"].clone(), v=st["exp_avg_sq"].clone(), p16=opt.half(p).clone() if p.dim() >= 2 else None)
    return snap


def assert_unchanged(P, opt, snap, label):
    now = snapshot(P, opt)
    for k in P:
        for f in ("p", "m", "v", "p16"):
            assert (snap[k][f] is None and now[k][f] is None) or same_bits(snap[k][f], now[k][f]), (label, k, f, "a skipped step changed it")


def assert_grads_plus_zero(P, label):
    for k, p in P.items():
        assert p.grad is not None and not p.grad.view(torch.int32).any(), (label, k, ".grad is not all +0")


def set_scale(opt, scale):
    from multihop_dense_retrieval_amd import _lib, optim
    _lib.check(optim.lib().mdr_optim_state_init(ptr(opt._state), float(scale), 0, _lib.current_stream_ptr()))


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------
def test_c_no_poison_survives_a_skipped_step():
    t0 = time.time()
    G1, _ = ov.chain_g1()
    safe, must, _ = ov.ladder(G1)
    P = params()
    opt = make_opt(P, must)
    # ---- step 1: must overflow
    scaled_loss(P, opt._state_f32[0], opt.half)[1].backward()
    torch.cuda.synchronize()
    dirty = [k for k in P if not bool(torch.isfinite(P[k].grad).all())]
    print(f"C step 1 at scale {must:g}: {len(dirty)} of {len(P)} .grad tensors hold a non-finite value")
    assert dirty, "nothing overflowed at a scale that must"
    snap = snapshot(P, opt)
    opt.step()
    key = opt._key
    st = read_state(opt)
    assert st["skipped_last"] == 1 and st["skipped_total"] == 1 and st["adam_step"] == 0 and st["loss_scale"] == np.float32(must / 2), st
    assert_unchanged(P, opt, snap, "step 1")
    assert_grads_plus_zero(P, "step 1")
    # ---- step 2: safe
    set_scale(opt, safe)
    scaled_loss(P, opt._state_f32[0], opt.half)[1].backward()
    torch.cuda.synchronize()
    got = {k: P[k].grad.clone() for k in P}
    # the fresh backward casts its weights itself (no weight16), the run under test reads the optimizer's fp16 copies: equal bits here also need
    # opt.half(W) == W.half() after a skipped step, which part D asserts on its own (weight16 against the plain cast) -- look there first if
    # this fails and D's comparison does too
    fresh = params()
    poison()
    loss, scaled, _ = scaled_loss(fresh, torch.tensor(float(safe), device="cuda"))
    poison()
    scaled.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    for k in P:
        assert bool(torch.isfinite(got[k]).all()), (k, "a non-finite value at a safe scale")
        assert same_bits(got[k], fresh[k].grad), (k, "the backward after a skipped step differs from the backward of a fresh state")
    snap = snapshot(P, opt)
    opt.step()
    st = read_state(opt)
    assert st["skipped_last"] == 0 and st["adam_step"] == 1, st
    assert opt._key == key, "a .grad moved: the optimizer rebuilt its table"
    assert_grads_plus_zero(P, "step 2")
    now = snapshot(P, opt)
    assert any(not same_bits(snap[k]["p"], now[k]["p"]) for k in P)
    print(f"WALL c {time.time() - t0:.2f} s")


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------
def test_d_the_scaler_finds_its_scale_on_the_chains_gradients():
    t0 = time.time()
    G1, peaks = ov.chain_g1()
    safe, must, between = ov.ladder(G1)
    start = 4 * must
    P = params()
    opt = make_opt(P, start)
    decay = decay_of(opt)
    model = optim_ref.initial_state(start)
    events, key, last_clean, halves_checked, first_seen = [], None, None, False, {}
    for step in range(CFG["steps"]):
        s = float(model["loss_scale"])
        cls = ov.scale_class(s, G1)
        loss, scaled, cs = scaled_loss(P, opt._state_f32[0], opt.half)
        scaled.backward()
        grads = {k: P[k].grad.clone() for k in P}
        finite = all(bool(torch.isfinite(g).all()) for g in grads.values())
        if finite and not halves_checked and events and not events[-1][2]:
            # (a clean step has rewritten the fp16 copies) the same backward without them: the loss and every gradient, bit for bit
            loss2, scaled2, _ = scaled_loss(P, opt._state_f32[0], None)
            g2 = torch.autograd.grad(scaled2, [P[k] for k in P])
            assert same_bits(loss.detach().reshape(1), loss2.detach().reshape(1))
            for k, g in zip(P, g2):
                assert same_bits(grads[k], g.reshape(grads[k].shape).contiguous()), (step, k, "weight16 changes the backward")
            halves_checked = True
        if not finite and not first_seen.get(s):  # where the overflow first shows, walking the tape of the last encode backwards
            first_seen[s] = next((f"{rec['label']}.{k}" for rec in reversed(cs[ch.KEYS[-1]].tape) for k, g in rec["g"].items()
                                  if not bool(torch.isfinite(g).all())), "a parameter gradient only")
            print(f"D scale {s:g}: the first non-finite gradient of an activation on the way back is that of {first_seen[s]}")
        snap = snapshot(P, opt)
        opt.step()
        st = read_state(opt)
        bad = {ov.MUST: True, ov.SAFE: False}.get(cls, bool(st["skipped_last"] == 1))
        events.append((s, cls, bad))
        print(f"D step {step}: scale {s:g} ({cls}) -> {'skipped' if st['skipped_last'] else 'clean'}; .grad finite: {finite}")
        model = optim_ref.advance(model, bad, *CFG["betas"], 1, CFG["scale_window"], opt.max_loss_scale)
        assert_counters(st, model, f"step {step}")
        assert bool(st["skipped_last"]) == (not finite), (step, "the flag and the gradients disagree")
        assert_grads_plus_zero(P, f"step {step}")
        if key is None:
            key = opt._key
        assert opt._key == key, (step, "a .grad moved: the optimizer rebuilt its table")
        if bad:
            assert_unchanged(P, opt, snap, f"step {step}")
            continue
        now = snapshot(P, opt)
        for k, p in P.items():
            want = optim_ref.replay_update(snap[k]["p"].cpu().numpy(), grads[k].cpu().numpy(), snap[k]["m"].cpu().numpy(), snap[k]["v"].cpu().numpy(),
                                           decay[id(p)], st["mult"], st["bias1"], st["bias2"], CFG["lr"], *CFG["betas"], CFG["eps"])
            for f, w in zip(("p", "m", "v", "p16"), want):
                if now[k][f] is not None:
                    a = now[k][f].cpu().numpy()
                    assert a.dtype == w.dtype and a.tobytes() == w.reshape(a.shape).tobytes(), (step, k, f, "not the replay's bits")
        last_clean = dict(step=step, scale=s, grads={k: g.cpu().numpy().astype(np.float64) / s for k, g in grads.items()},
                          sd={k: v["p"].cpu().numpy() for k, v in snap.items()})
    skipped, clean, doublings, undecided = ov.run_summary(events)
    print(f"D scales {[e[0] for e in events]}: {skipped} skipped, {clean} clean, {doublings} doublings, undecided scales met: {undecided}")
    assert skipped >= 2 and clean >= 3 and doublings >= 1 and undecided <= 2, events
    assert halves_checked
    # criterion E at the parameters the device held at its last clean step: the fp64 model and the regime are run THERE
    batches = ov.chain_batches()
    _, g64, _, _ = ch.grads_loss("model64", last_clean["sd"], ch.GEOM, batches)
    _, g_reg, _, _ = ch.grads_loss("regime", last_clean["sd"], ch.GEOM, batches)
    moved = max(float(np.abs(last_clean["sd"][k] - v).max()) for k, v in ch.state_dict().items())
    print(f"D criterion E at step {last_clean['step']} (scale {last_clean['scale']:g}); the parameters have moved by at most {moved:.3e}")
    assert 0 < moved <= 2e-4
    check_e(last_clean["grads"], g_reg, g64, list(batches.values()), f"overflow chain, step {last_clean['step']}")
    print(f"WALL d {time.time() - t0:.2f} s")
