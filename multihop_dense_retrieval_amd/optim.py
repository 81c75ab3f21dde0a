"""The optimizer step of the retriever's training loop on the device, and the momentum encoder's EMA:

    opt = FusedAdam(params_or_groups, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=2.0, loss_scale="dynamic",
                    scale_window=2000, fp16_copies=False, decoupled_weight_decay=False)
    opt.scale_loss(loss).backward(); opt.step()
    momentum_update(params_k, params_q, m)
    linear_schedule_with_warmup(step, warmup_steps, total_steps)

FusedAdam does in one call what scripts/train_mhop.py of the reference does with amp.scale_loss (apex O1's dynamic loss scale),
clip_grad_norm_(max_grad_norm), torch.optim.Adam in two weight-decay groups and model.zero_grad(): mdr_optim_step of include/mdr_optim.h
(csrc/mdr_optim.hip lists its rounding points). The gradients are read once for the norm and once for the update, p, m, v are read and
written once, the fp16 copies of the weights are written in the same sweep, and the loss scale, the overflow check, the clip coefficient
and Adam's step count live in a small device struct: a step never synchronises and never reads anything back. A step that finds a
non-finite gradient changes no parameter, halves the dynamic scale and still zeroes the gradients. No atomics: two runs give the same bits.

It is a torch.optim.Optimizer, so torch.optim.lr_scheduler.LambdaLR drives param_groups[i]["lr"] and the reference's two-group
construction works as it stands. The parameters are CUDA fp32 contiguous tensors on one device; there is no CPU fallback. A parameter
without .grad takes no part in a step (torch's Adam does the same). The step zeroes .grad in place: do not call zero_grad(), which drops
the gradients and makes every step rebuild the pointer table. Every group must carry the same lr (the reference's do): the clip norm and the
loss scaler's state belong to one mdr_optim_step, and groups with different rates would need one call each.

Optimizer.state is torch's per-parameter dict (exp_avg, exp_avg_sq live there), so the readback of the device struct is read_state().
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import ptr

_c = ctypes
CHUNK = 4096  # MDR_OPTIM_CHUNK
# include/mdr_optim.h -- bound here, apart from _lib._SIGNATURES (include/mdr_hip.h's table, pinned by its own test)
SIGNATURES = {
    "mdr_optim_chunks": (_c.c_int64, [_c.c_void_p, _c.c_int, _c.c_void_p]),
    "mdr_optim_table_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int]),
    "mdr_optim_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int]),
    "mdr_optim_table_fill": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_int)]),
    "mdr_optim_state_init": (_c.c_int, [_c.c_void_p, _c.c_float, _c.c_int, _c.c_void_p]),
    "mdr_optim_step": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_float, _c.c_float, _c.c_float, _c.c_float, _c.c_float, _c.c_int,
                                  _c.c_int, _c.c_float, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "mdr_optim_ema": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_double, _c.c_int, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
# include/mdr_optim_adamw.h: mdr_optim_step with the decay's form as an argument behind zero_grads
ADAMW_SIGNATURES = {
    "mdr_optim_step_ex": (_c.c_int, SIGNATURES["mdr_optim_step"][1][:13] + [_c.c_int] + SIGNATURES["mdr_optim_step"][1][13:]),
}
ADAMW_EXPORTED_SYMBOLS = tuple(ADAMW_SIGNATURES)
DECAY_L2, DECAY_DECOUPLED = 0, 1  # MDR_OPTIM_DECAY_L2, MDR_OPTIM_DECAY_DECOUPLED
# struct mdr_optim_tensor and struct mdr_optim_state
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("p16", "<u8"), ("n", "<i8"), ("weight_decay", "<f4"),
                         ("reserved0", "<i4"), ("reserved1", "<i8")])
STATE_DTYPE = np.dtype([("loss_scale", "<f4"), ("unskipped", "<i4"), ("adam_step", "<i4"), ("b1_pow", "<f4"), ("b2_pow", "<f4"),
                        ("skipped_last", "<i4"), ("grad_norm", "<f4"), ("clip_coef", "<f4"), ("mult", "<f4"), ("skipped_total", "<i4"),
                        ("bias1", "<f4"), ("bias2", "<f4")])
_STATE_WORDS = 16  # the device buffer: 64 bytes, the struct is the first 48
lib = _lib.binder(SIGNATURES, ADAMW_SIGNATURES)  # libmdrhip.so with the signatures of include/mdr_optim.h and include/mdr_optim_adamw.h bound


def _sizes(sizes):
    return np.ascontiguousarray(np.asarray(list(sizes), dtype=np.int64))


def chunks(sizes):
    """(number of chunks, first chunk of every tensor and the end: len(sizes) + 1 entries): the split of tensors of these sizes, a function of
    the sizes alone. (-1, None) for sizes the library refuses (an empty list, a size < 1)."""
    n = _sizes(sizes)
    first = np.zeros(len(n) + 1, dtype=np.int64)
    total = int(lib().mdr_optim_chunks(n.ctypes.data, len(n), first.ctypes.data))
    return (total, first.tolist()) if total >= 0 else (-1, None)


def table_bytes(sizes):
    n = _sizes(sizes)
    return int(lib().mdr_optim_table_bytes(n.ctypes.data, len(n)))


def workspace_bytes(sizes):
    n = _sizes(sizes)
    return int(lib().mdr_optim_workspace_bytes(n.ctypes.data, len(n)))


def build_table(rows):
    """rows: (p, g, m, v, p16, n, weight_decay) per tensor, the pointers as integers (0 = NULL). Returns (the table blob as a numpy uint8
    array, the number of chunks): mdr_optim_table_fill."""
    descs = np.zeros(len(rows), dtype=TENSOR_DTYPE)
    for d, row in zip(descs, rows):
        d["p"], d["g"], d["m"], d["v"], d["p16"], d["n"], d["weight_decay"] = row
    L = lib()
    sizes = np.ascontiguousarray(descs["n"])
    nbytes = int(L.mdr_optim_table_bytes(sizes.ctypes.data, len(rows)))
    host = np.zeros(max(nbytes, 1), dtype=np.uint8)
    n_chunks = ctypes.c_int(0)
    _lib.check(L.mdr_optim_table_fill(descs.ctypes.data, len(rows), host.ctypes.data, nbytes, ctypes.byref(n_chunks)))
    return host, int(n_chunks.value)


def _check_param(p, what="parameter"):
    if not (torch.is_tensor(p) and p.is_cuda):
        raise RuntimeError(f"the fused optimizer runs on a HIP device only (there is no CPU fallback): got a {what} on "
                           f"{getattr(p, 'device', type(p).__name__)}")
    if p.dtype != torch.float32 or not p.is_contiguous() or p.numel() < 1:
        raise RuntimeError(f"every {what} must be a contiguous fp32 tensor of at least one element, got {p.dtype} {tuple(p.shape)}")


def linear_schedule_with_warmup(step, warmup_steps, total_steps):
    """The lambda of Hugging Face's get_linear_schedule_with_warmup: step / max(1, warmup) while warming up, then the straight line down to 0 at
    total_steps, 0 behind it. For torch.optim.lr_scheduler.LambdaLR(opt, lambda s: linear_schedule_with_warmup(s, w, t))."""
    if step < warmup_steps:
        return float(step) / float(max(1, warmup_steps))
    return max(0.0, float(total_steps - step) / float(max(1, total_steps - warmup_steps)))


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=2.0, loss_scale="dynamic", scale_window=2000,
                 fp16_copies=False, init_scale=2.0 ** 16, max_loss_scale=2.0 ** 24, zero_grads=True, decoupled_weight_decay=False):
        """loss_scale: "dynamic" (apex's LossScaler: init_scale, doubled after scale_window clean steps up to max_loss_scale, halved by a
        non-finite gradient) or a fixed number (a non-finite gradient still skips the step). fp16_copies: True keeps an fp16 copy of every
        parameter of two or more dimensions (the Linear weights and the embedding tables), or an iterable of the parameters to keep one of;
        half(p) returns it. decoupled_weight_decay: False is torch.optim.Adam (L2 decay into the gradient, mdr_optim_step); True is
        transformers.AdamW with correct_bias=True (mdr_optim_step_ex in mode 1, include/mdr_optim_adamw.h), the reader's optimizer."""
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"betas {betas} must lie in [0, 1)")
        if not eps > 0.0:
            raise ValueError(f"eps = {eps} must be positive")
        if not max_grad_norm > 0.0:
            raise ValueError(f"max_grad_norm = {max_grad_norm} must be positive")
        if int(scale_window) < 1:
            raise ValueError(f"scale_window = {scale_window} must be at least 1")
        self._dynamic = loss_scale == "dynamic"
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        scale0 = float(init_scale if self._dynamic else loss_scale)
        if not (scale0 > 0.0 and np.isfinite(scale0)):
            raise ValueError(f"loss_scale = {loss_scale} must be \"dynamic\" or a positive number")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay))
        self.betas, self.eps, self.max_grad_norm = (float(betas[0]), float(betas[1])), float(eps), float(max_grad_norm)
        self.scale_window, self.max_loss_scale, self.zero_grads = int(scale_window), float(max_loss_scale), bool(zero_grads)
        self._params = [p for group in self.param_groups for p in group["params"]]
        for p in self._params:
            _check_param(p)
        self._device = self._params[0].device
        if any(p.device != self._device for p in self._params):
            raise RuntimeError("every parameter must live on one device")
        want16 = set()
        if fp16_copies is True:
            want16 = {id(p) for p in self._params if p.dim() >= 2}
        elif fp16_copies:
            want16 = {id(p) for p in fp16_copies}
            if not want16 <= {id(p) for p in self._params}:
                raise ValueError("fp16_copies names a tensor that is not a parameter of this optimizer")
        self._half = {}
        for p in self._params:
            self.state[p]["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            self.state[p]["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if id(p) in want16:
                self._half[id(p)] = p.detach().to(dtype=torch.float16).contiguous()
        self._key, self._table, self._n_chunks, self._workspace = None, None, 0, None
        self.last_lr = None  # the lr of the last mdr_optim_step
        self._state = torch.zeros(_STATE_WORDS, dtype=torch.int32, device=self._device)
        self._state_f32 = self._state.view(torch.float32)
        _lib.call(lib().mdr_optim_state_init, ptr(self._state), scale0, dev=self._device)

    def half(self, p):
        """The fp16 copy of parameter p that every step keeps current (fp16_copies)."""
        if id(p) not in self._half:
            raise RuntimeError("no fp16 copy is kept of this tensor (fp16_copies)")
        return self._half[id(p)]

    def scale_loss(self, loss):
        """loss times the device's loss scale: no readback, and the product's gradient carries the scale into every .grad."""
        return loss * self._state_f32[0]

    def read_state(self):
        """The device struct (mdr_optim_state) as a dict. It synchronises: for logs and tests."""
        raw = self._state.cpu().numpy().view(np.uint8)[:STATE_DTYPE.itemsize].view(STATE_DTYPE)[0]
        return {k: raw[k].item() for k in STATE_DTYPE.names}

    def _rows(self):
        rows = []
        for group in self.param_groups:
            wd = float(group["weight_decay"])
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    if not (g.is_cuda and g.device == p.device and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape):
                        raise RuntimeError(f"a gradient must be a contiguous fp32 tensor of its parameter's shape and device, got {g.dtype} "
                                           f"{tuple(g.shape)} on {g.device}")
                st = self.state[p]
                h = self._half.get(id(p))
                rows.append((p.data_ptr(), 0 if g is None else g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                             0 if h is None else h.data_ptr(), p.numel(), wd))
        return tuple(rows)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lrs = {float(group["lr"]) for group in self.param_groups}
        if len(lrs) != 1:
            raise RuntimeError(f"every parameter group must carry the same lr, got {sorted(lrs)}")
        lr = lrs.pop()
        L, dev = lib(), self._device
        with torch.cuda.device(dev):
            rows = self._rows()
            if rows != self._key:  # some data_ptr() moved (the first backward gives every parameter its .grad): rebuild and upload
                host, self._n_chunks = build_table(rows)
                self._table = torch.from_numpy(host).to(dev)
                if self._workspace is None:
                    self._workspace = torch.empty(workspace_bytes([r[5] for r in rows]), dtype=torch.uint8, device=dev)
                self._key = rows
            head = (ptr(self._table), len(rows), self._n_chunks, ptr(self._state), lr, self.betas[0], self.betas[1], self.eps, self.max_grad_norm,
                    1 if self._dynamic else 0, self.scale_window, self.max_loss_scale, 1 if self.zero_grads else 0)
            if self.decoupled_weight_decay:
                _lib.call(L.mdr_optim_step_ex, *head, DECAY_DECOUPLED, ptr(self._workspace), self._workspace.numel(), dev=dev)
            else:
                _lib.call(L.mdr_optim_step, *head, ptr(self._workspace), self._workspace.numel(), dev=dev)
        self.last_lr = lr
        return loss


_ema_tables = {}  # pointer rows of (k, q) -> (table_k, table_q, n_tensors, n_chunks): a few encoder pairs at the most


def momentum_update(params_k, params_q, m, fp16_copies=None):
    """The momentum encoder's update, k = k * m + q * (1 - m) in place over every pair (mdr_optim_ema; torch's bits for
    param_k.data * m + param_q.data * (1. - m)). fp16_copies: None, or one fp16 tensor or None per pair, which becomes fp16(k)."""
    ks, qs = list(params_k), list(params_q)
    hs = [None] * len(ks) if fp16_copies is None else list(fp16_copies)
    if not ks or len(ks) != len(qs) or len(hs) != len(ks):
        raise ValueError(f"params_k, params_q and fp16_copies must pair up: {len(ks)}, {len(qs)}, {len(hs)} entries")
    for k, q, h in zip(ks, qs, hs):
        _check_param(k, "tensor")
        _check_param(q, "tensor")
        if q.device != ks[0].device or k.device != ks[0].device or k.shape != q.shape:
            raise RuntimeError(f"a pair must share its shape and every tensor the device: {tuple(k.shape)} and {tuple(q.shape)}")
        if h is not None and not (torch.is_tensor(h) and h.dtype == torch.float16 and h.is_contiguous() and h.device == k.device and h.shape == k.shape):
            raise RuntimeError("an fp16 copy must be a contiguous fp16 tensor of its tensor's shape and device")
    if not 0.0 <= float(m) <= 1.0:
        raise ValueError(f"m = {m} must lie in [0, 1]")
    dev = ks[0].device
    key = tuple((k.data_ptr(), q.data_ptr(), 0 if h is None else h.data_ptr(), k.numel()) for k, q, h in zip(ks, qs, hs))
    with torch.cuda.device(dev):
        if key not in _ema_tables:
            if len(_ema_tables) >= 8:
                _ema_tables.clear()
            host_k, n_chunks = build_table([(kp, 0, 0, 0, hp, n, 0.0) for kp, _, hp, n in key])
            host_q, _ = build_table([(qp, 0, 0, 0, 0, n, 0.0) for _, qp, _, n in key])
            _ema_tables[key] = (torch.from_numpy(host_k).to(dev), torch.from_numpy(host_q).to(dev), len(key), n_chunks)
        tk, tq, n_tensors, n_chunks = _ema_tables[key]
        _lib.call(lib().mdr_optim_ema, ptr(tk), ptr(tq), n_tensors, n_chunks, float(m), dev=dev)
