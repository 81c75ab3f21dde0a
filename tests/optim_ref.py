"""The host model of the optimizer step (include/mdr_optim.h, csrc/mdr_optim.hip): a numpy-float32 replay of the update and of the EMA,
operation by operation as the kernel file lists them, the loss scaler's state machine, the chunk split, the norm's error bound, and an fp64
model (torch's own Adam and clip_grad_norm_ on the CPU). tests/test_optim_host.py checks the model against torch; tests/test_optim_gpu.py
checks the kernels against the model."""
import numpy as np
import torch

from oracle.fp import U32, gamma

F = np.float32
CHUNK = 4096


# csrc/mdr_optim.hip, rounding points 1 - 3: a term passes through at most 30 fp32 roundings on its way into a chunk sum (inv, the product and
# the square count five, the thread's 16 additions, the butterfly's 6, the waves' 3), every term is >= 0, so a chunk sum is within gamma_30 of
# its exact value; the chunk sums are added in fp64 (n_chunks * 2^-53: nothing); the square root halves a relative error; fp32(sqrt) adds u,
# and one more u pays for the fp64 steps and the second-order terms.
NORM_REL_BOUND = gamma(30) / 2 + 2 * U32


def chunks(sizes):
    """(number of chunks, first chunk of every tensor and the end): every tensor owns ceil(n / CHUNK) consecutive chunks."""
    if len(sizes) < 1 or min(sizes) < 1:
        return -1, None
    first = [0]
    for n in sizes:
        first.append(first[-1] + (n - 1) // CHUNK + 1)
    return first[-1], first


def chunk_ranges(sizes):
    """[(tensor, begin, end)] of every chunk in table order"""
    return [(i, c * CHUNK, min(n, (c + 1) * CHUNK)) for i, n in enumerate(sizes) for c in range((n - 1) // CHUNK + 1)]


def initial_state(loss_scale):
    return dict(loss_scale=F(loss_scale), unskipped=0, adam_step=0, b1_pow=F(1), b2_pow=F(1), skipped_last=0, grad_norm=F(0), clip_coef=F(0),
                mult=F(0), skipped_total=0, bias1=F(0), bias2=F(0))


def clip_and_mult(grad_norm, max_grad_norm, loss_scale):
    """the finalize kernel's fp32 expressions of grad_norm and of the scale the gradients carry"""
    with np.errstate(all="ignore"):
        coef = np.minimum(F(1), F(max_grad_norm) / (F(grad_norm) + F(1e-6)))
        return F(coef), F(F(coef) / F(loss_scale))


def bias_next(bias, beta):
    """1 - beta^(k + 1) from bias = 1 - beta^k without the cancellation of 1 - fp32(beta^(k + 1)): bias + (1 - bias) * (1 - beta), each
    operation one fp32 rounding (1 - beta is exact for beta >= 0.5)"""
    a = F(F(1) - F(bias))
    b = F(F(1) - F(beta))
    return F(F(bias) + F(a * b))


def advance(state, bad, beta1, beta2, dynamic, scale_window, max_scale):
    """the loss scaler's and Adam's counters after a step whose gradients were (bad) or were not non-finite; returns a new dict"""
    st = dict(state)
    if bad:
        st["skipped_last"] = 1
        st["skipped_total"] += 1
        if dynamic:
            st["loss_scale"] = F(st["loss_scale"] / F(2))
            st["unskipped"] = 0
    else:
        st["skipped_last"] = 0
        st["adam_step"] += 1
        st["b1_pow"] = F(st["b1_pow"] * F(beta1))
        st["b2_pow"] = F(st["b2_pow"] * F(beta2))
        st["bias1"] = bias_next(st["bias1"], beta1)
        st["bias2"] = bias_next(st["bias2"], beta2)
        st["unskipped"] += 1
        if dynamic and st["unskipped"] == scale_window:
            st["loss_scale"] = F(min(F(max_scale), F(2) * st["loss_scale"]))
            st["unskipped"] = 0
    return st


def host_norm(grads, loss_scale):
    """(fp32(sqrt(sum)), bad): the squares as the kernel forms them, fp32 (g * (1 / loss_scale))^2, added in fp64 (the order of the device's
    fp32 partial sums is not replayed: NORM_REL_BOUND covers it)"""
    inv = F(1) / F(loss_scale)
    total, bad = 0.0, False
    with np.errstate(all="ignore"):
        for g in grads:
            x = g.astype(F) * inv
            total += float((x * x).astype(np.float64).sum())
            bad |= not np.isfinite(g).all()
    return F(np.sqrt(total)), bad or not np.isfinite(total)


def replay_update(p, g, m, v, weight_decay, mult, bias1, bias2, lr, beta1, beta2, eps):
    """csrc/mdr_optim.hip, rounding point 5, on float32 arrays: returns (p, m, v, p16). Every line is one rounded fp32 operation."""
    p, g, m, v = (np.asarray(a, dtype=F) for a in (p, g, m, v))
    mult, bias1, bias2, lr, beta1, beta2, eps, wd = (F(a) for a in (mult, bias1, bias2, lr, beta1, beta2, eps, weight_decay))
    with np.errstate(all="ignore"):
        omb1 = F(1) - beta1
        omb2 = F(1) - beta2
        step_size = lr / bias1
        bc2 = np.sqrt(bias2)
        gd = g * mult
        if wd != 0:
            t = wd * p
            gd = gd + t
        t = omb1 * gd
        m = beta1 * m
        m = m + t
        t = omb2 * gd
        t = t * gd
        v = beta2 * v
        v = v + t
        denom = np.sqrt(v)
        denom = denom / bc2
        denom = denom + eps
        t = m / denom
        t = step_size * t
        p = p - t
    assert p.dtype == m.dtype == v.dtype == F
    return p, m, v, p.astype(np.float16)


def replay_ema(k, q, m):
    """k * fp32(m) + q * fp32(1 - m), the subtraction in double: (k, k16)"""
    mf, omf = F(m), F(1.0 - float(m))
    a = np.asarray(k, dtype=F) * mf
    b = np.asarray(q, dtype=F) * omf
    r = a + b
    return r, r.astype(np.float16)


def replay_step(state, params, grads, moments, decays, lr, beta1, beta2, eps, max_grad_norm, dynamic, scale_window, max_scale):
    """One whole step on the host. params, grads ((scaled) or None), moments [(m, v)] are lists of float32 arrays, replaced in the lists
    unless the step skips. Returns the new state."""
    live = [g for g in grads if g is not None]
    norm, bad = host_norm(live, state["loss_scale"])
    coef, mult = clip_and_mult(norm, max_grad_norm, state["loss_scale"])
    st = advance(state, bad, beta1, beta2, dynamic, scale_window, max_scale)
    st.update(grad_norm=norm, clip_coef=coef, mult=mult)
    if not bad:
        for i, g in enumerate(grads):
            if g is not None:
                p, m, v, _ = replay_update(params[i], g, moments[i][0], moments[i][1], decays[i], mult, st["bias1"], st["bias2"], lr, beta1, beta2, eps)
                params[i], moments[i] = p, (m, v)
    return st


# ---- the trajectory: g = S * (p - target) on 12 tensors, decay on every second one ----
TRAJ_SIZES = (4101, 768, 768, 2304, 257, 1024, 3000, 513, 640, 8193, 333, 1500)
TRAJ = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=2.0)


def trajectory_start(seed=7):
    """(params, targets): float32 arrays"""
    rng = np.random.default_rng(seed)
    params = [rng.normal(0, 0.05, n).astype(F) for n in TRAJ_SIZES]
    targets = [(p + rng.normal(0, 0.05, p.shape)).astype(F) for p in params]
    return params, targets


def traj_decays():
    return [TRAJ["weight_decay"] if i % 2 == 0 else 0.0 for i in range(len(TRAJ_SIZES))]


def torch_trajectory(params, targets, steps, dtype, device="cpu"):
    """torch.optim.Adam in the reference's two groups with clip_grad_norm_ in front, the gradient p - target formed in dtype: final params as
    float64 numpy arrays"""
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(device=device, dtype=dtype)) for p in params]
    ts = [torch.from_numpy(t).to(device=device, dtype=dtype) for t in targets]
    opt = torch.optim.Adam([{"params": ps[0::2], "weight_decay": TRAJ["weight_decay"]}, {"params": ps[1::2], "weight_decay": 0.0}], lr=TRAJ["lr"],
                           betas=TRAJ["betas"], eps=TRAJ["eps"])
    for _ in range(steps):
        for p, t in zip(ps, ts):
            p.grad = (p.detach() - t)
        torch.nn.utils.clip_grad_norm_(ps, TRAJ["max_grad_norm"])
        opt.step()
    return [p.detach().cpu().double().numpy() for p in ps]


def replay_trajectory(params, targets, steps, loss_scale=2.0 ** 16):
    """the host replay over the same trajectory, the gradients scaled by the loss scale as a scaled loss would deliver them"""
    params = [p.copy() for p in params]
    moments = [(np.zeros_like(p), np.zeros_like(p)) for p in params]
    st = initial_state(loss_scale)
    for _ in range(steps):
        grads = [F(st["loss_scale"]) * (p - t) for p, t in zip(params, targets)]
        st = replay_step(st, params, grads, moments, traj_decays(), TRAJ["lr"], *TRAJ["betas"], TRAJ["eps"], TRAJ["max_grad_norm"], 1, 2000, 2.0 ** 24)
    return [p.astype(np.float64) for p in params], st


def traj_errors(got, want64):
    """per tensor, the largest |p - p64| / (|p64| + 1e-3)"""
    return [float((np.abs(np.asarray(g, dtype=np.float64) - w) / (np.abs(w) + 1e-3)).max()) for g, w in zip(got, want64)]
