"""The host model of the optimizer step's decoupled mode (include/mdr_optim_adamw.h, csrc/mdr_optim.hip rounding point 5w): a numpy-float32
replay of the update, operation for operation as the kernel file lists them, an fp64 version with a running error bound, and the whole step
on top of tests/optim_ref.py's norm, clip and state machine, which the two modes share. tests/test_adamw_host.py checks the replay against
the fp64 version; tests/test_adamw_gpu.py checks the kernel against the replay.

The formula is transformers.AdamW's with correct_bias=True as remembered, not captured (no copy of that class is at hand):
    m = b1 m + (1 - b1) g      v = b2 v + (1 - b2) g g      step = lr sqrt(bias2) / bias1
    p = p - step m / (sqrt(v) + eps)      p = p - lr wd p   (the updated p; only where wd != 0)
"""
import numpy as np

import optim_ref as oref
from oracle.fp import U32

F = np.float32


def replay_update(p, g, m, v, weight_decay, mult, bias1, bias2, lr, beta1, beta2, eps):
    """csrc/mdr_optim.hip, rounding point 5w, on float32 arrays: returns (p, m, v, p16). Every line is one rounded fp32 operation."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    mult, bias1, bias2, lr, beta1, beta2, eps, wd = (F(a) for a in (mult, bias1, bias2, lr, beta1, beta2, eps, weight_decay))
    with np.errstate(all="ignore"):
        omb1 = F(1) - beta1
        omb2 = F(1) - beta2
        bc2 = np.sqrt(bias2)
        t = lr * bc2
        step = t / bias1
        gh = g * mult
        t = omb1 * gh
        m = beta1 * m
        m = m + t
        t = omb2 * gh
        t = t * gh
        v = beta2 * v
        v = v + t
        denom = np.sqrt(v)
        denom = denom + eps
        q = m / denom
        t = step * q
        p = p - t
        if wd != 0:
            w = lr * wd
            t = w * p
            p = p - t
    assert p.dtype == m.dtype == v.dtype == F and type(step) is F
    return p, m, v, p.astype(np.float16)


def replay_step(state, params, grads, moments, decays, lr, beta1, beta2, eps, max_grad_norm, dynamic, scale_window, max_scale):
    """optim_ref.replay_step with the decoupled update: norm, clip, skip and the state machine are mode 0's."""
    live = [g for g in grads if g is not None]
    norm, bad = oref.host_norm(live, state["loss_scale"])
    coef, mult = oref.clip_and_mult(norm, max_grad_norm, state["loss_scale"])
    st = oref.advance(state, bad, beta1, beta2, dynamic, scale_window, max_scale)
    st.update(grad_norm=norm, clip_coef=coef, mult=mult)
    if not bad:
        for i, g in enumerate(grads):
            if g is not None:
                p, m, v, _ = replay_update(params[i], g, moments[i][0], moments[i][1], decays[i], mult, st["bias1"], st["bias2"], lr, beta1, beta2, eps)
                params[i], moments[i] = p, (m, v)
    return st


def update64(P, M, V, g, weight_decay, mult, bias1, bias2, lr, beta1, beta2, eps):
    """The same update in float64 with a running bound. P, M, V are pairs (value, bound on |fp32 replay - value|); g, mult, bias1, bias2 and
    the hyperparameters enter as the fp32 numbers the replay sees, so they carry no error. Returns the three new pairs.

    Every fp32 operation adds u = 2^-24 times its result's magnitude to the propagated error of its operands (first order; a final factor
    1 + 2^-10 per step covers the products of two error terms):
        gh = g mult                              u |gh|
        m' = b1 m + (1 - b1) gh                  b1 Em + (1 - b1) Egh + u (|b1 m| + |(1 - b1) gh| + |m'|);  1 - b1 itself is within u of its value
        v' = b2 v + ((1 - b2) gh) gh             b2 Ev + 2 (1 - b2) |gh| Egh + u (|b2 v| + 2 |(1 - b2) gh gh| + |v'|) (+ u for 1 - b2)
        s = sqrt(v')                             min(sqrt(Ev'), Ev' / (2 sqrt(v' - Ev'))) + u s      (|sqrt a - sqrt b| <= sqrt |a - b|)
        denom = s + eps                          Es + u denom
        q = m' / denom                           (Em' + |q| Ed) / (denom - Ed) + u |q|
        step = (lr sqrt(bias2)) / bias1          3 u step
        p1 = p - step q                          Ep + |step| Eq + |q| Estep + u |step q| + u |p1|
        w = lr wd,  p2 = p1 - w p1               Ep1 + |w| Ep1 + 2 u |w p1| + u |p2|
    """
    (p, Ep), (m, Em), (v, Ev) = P, M, V
    g = np.asarray(g, np.float64)
    mult, bias1, bias2, lr, b1, b2, eps, wd = (float(F(a)) for a in (mult, bias1, bias2, lr, beta1, beta2, eps, weight_decay))
    u = U32
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    gh = g * mult
    Egh = u * np.abs(gh)
    m2 = b1 * m + omb1 * gh
    Em2 = b1 * Em + omb1 * Egh + u * (np.abs(b1 * m) + 2 * np.abs(omb1 * gh) + np.abs(m2))
    v2 = b2 * v + omb2 * gh * gh
    Ev2 = b2 * Ev + 2 * omb2 * np.abs(gh) * Egh + u * (np.abs(b2 * v) + 3 * np.abs(omb2 * gh * gh) + np.abs(v2))
    s = np.sqrt(v2)
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(v2 > Ev2, Ev2 / (2 * np.sqrt(np.maximum(v2 - Ev2, 1e-300))), np.inf)
    Es = np.minimum(np.sqrt(Ev2), lin) + u * s
    denom = s + eps
    Ed = Es + u * denom
    assert (denom > Ed).all(), "the bound says nothing here: sqrt(v) + eps is not known to be positive"
    q = m2 / denom
    Eq = (Em2 + np.abs(q) * Ed) / (denom - Ed) + u * np.abs(q)
    step = lr * np.sqrt(bias2) / bias1
    Estep = 3 * u * abs(step)
    p1 = p - step * q
    Ep1 = Ep + abs(step) * Eq + np.abs(q) * Estep + u * np.abs(step * q) + u * np.abs(p1)
    if wd != 0:
        w = lr * wd
        p2 = p1 - w * p1
        Ep1 = Ep1 + abs(w) * Ep1 + 2 * u * np.abs(w * p1) + u * np.abs(p2)
        p1 = p2
    k = 1 + 2.0 ** -10
    return (p1, Ep1 * k), (m2, Em2 * k), (v2, Ev2 * k)
