"""Training on several ranks: every rank encodes a slice of the batch, the embeddings are gathered, every rank evaluates the
identical full loss and backpropagates its own rows, and the parameter gradients are summed over the ranks IN RANK ORDER by a kernel of this
library (include/mdr_rank_sum.h), so the bits do not depend on a collective library's ring order or on the transport.

    bounds = slice_bounds(B, N)                         balanced contiguous row slices of a batch
    offsets, S, padded = flat_layout(sizes, N)          the parameters' places in one flat fp32 buffer of N segments of S floats
    rank_sum_host(recv)                                 numpy statement of mdr_rank_sum
    world = TorchWorld() | LoopbackWorld(N).ranks[r]    rank, size, gather_rows, exchange, publish
    x_full = gather_with_grad(world, x_local, bounds)   differentiable: the backward hands back this rank's rows
    bucket = GradBucket(model.parameters(), world);  ...backward...;  bucket.reduce();  opt.step()

The pure functions at the top touch no device. The transport moves bytes and never adds: `exchange` hands rank r every rank's values for
segment r, mdr_rank_sum adds them, `publish` hands every rank every reduced segment. After reduce() every rank's gradients hold the same bits,
so the norm, the clip, the skip decision, the loss scale and Adam stay in lockstep without a further message.
"""
import ctypes
import threading

import numpy as np
import torch

from . import _lib

_c = ctypes
SEGMENT_MULTIPLE = 1024  # floats: a segment's length is a multiple of it, so every segment starts 4 KiB-aligned in the flat buffer
MAX_RANKS = 16           # MDR_RANK_SUM_MAX_RANKS
# include/mdr_rank_sum.h -- bound here, apart from every other header's table
SIGNATURES = {
    "mdr_rank_sum": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int64, _c.c_int64, _c.c_void_p, _c.c_void_p]),
}
EXPORTED_SYMBOLS = tuple(SIGNATURES)
lib = _lib.binder(SIGNATURES)


# -- pure functions ------------------------------------------------------------------------------------------------------------------------
def slice_bounds(B, N):
    """[(lo, hi)] * N: balanced contiguous slices of B rows, the first B % N one row longer. A slice is empty only when B < N."""
    B, N = int(B), int(N)
    if B < 0 or N < 1:
        raise ValueError(f"slice_bounds({B}, {N}): B >= 0 and N >= 1")
    base, extra = divmod(B, N)
    edges = [r * base + min(r, extra) for r in range(N + 1)]
    return [(edges[r], edges[r + 1]) for r in range(N)]


def flat_layout(sizes, N, align=1):
    """(offsets, S, padded): tensor i of `sizes` elements lies at offsets[i] of one flat buffer (the running sum: no gaps), S is the per-rank
    segment, ceil(total / N) rounded up to a multiple of SEGMENT_MULTIPLE floats, and padded = N * S >= total is the buffer's length.
    align > 1: every offset is rounded up to a multiple of it (the reader's heads hold 1 and 2 elements); a gap is never written."""
    sizes, N, align = [int(s) for s in sizes], int(N), int(align)
    if N < 1 or align < 1 or not sizes or min(sizes) < 1:
        raise ValueError("flat_layout: N >= 1, align >= 1 and at least one size, every size >= 1")
    offsets, total = [], 0
    for s in sizes:
        total = -(-total // align) * align
        offsets.append(total)
        total += s
    S = -(-(-(-total // N)) // SEGMENT_MULTIPLE) * SEGMENT_MULTIPLE
    return offsets, S, N * S


def rank_sum_host(recv):
    """numpy statement of mdr_rank_sum: recv [N, n] float32 -> ((recv[0] + recv[1]) + recv[2]) + ..., one float32 addition per row behind
    the first, the accumulator starting at row 0 (one row: a copy of its bits)."""
    recv = np.asarray(recv)
    if recv.dtype != np.float32 or recv.ndim != 2 or recv.shape[0] < 1:
        raise ValueError(f"rank_sum_host: a float32 [N, n] array with N >= 1, got {recv.dtype} {recv.shape}")
    acc = recv[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(1, recv.shape[0]):
            acc = acc + recv[r]
    return acc


def rank_seed(seed, rank):
    """The dropout seed of `rank`: seed ^ (rank * 0x9E3779B97F4A7C15 mod 2^64). Rank 0 keeps the one-rank seed; without it row i of every rank
    would share one mask."""
    return int(seed) ^ ((int(rank) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)


# -- the kernel ----------------------------------------------------------------------------------------------------------------------------
def rank_sum(recv, out, n=None):
    """mdr_rank_sum: out[:n] = the ordered sum of recv's rows [N, stride] (fp32, contiguous, on one HIP device), enqueued on the current stream."""
    if not (torch.is_tensor(recv) and recv.is_cuda and recv.dtype == torch.float32 and recv.dim() == 2 and recv.is_contiguous()):
        raise ValueError(f"recv must be a contiguous fp32 [N, stride] tensor on a HIP device (there is no CPU fallback), got {_lib.describe(recv)}")
    n = int(out.numel() if n is None else n)
    if not (_lib.is_like(out, (torch.float32,), out.shape, recv.device) and out.numel() >= n):
        raise ValueError(f"out must be a contiguous fp32 tensor of at least n = {n} elements on {recv.device}, got {_lib.describe(out)}")
    _lib.call(lib().mdr_rank_sum, _lib.ptr(recv), int(recv.shape[0]), n, int(recv.shape[1]), _lib.ptr(out), dev=recv.device, device_arg=False)
    return out


# -- worlds --------------------------------------------------------------------------------------------------------------------------------
def _check_gather(x_local, bounds, rank):
    lo, hi = bounds[rank]
    if x_local.dim() != 2 or x_local.shape[0] != hi - lo:
        raise ValueError(f"rank {rank} owns rows {lo} .. {hi} and was given {tuple(x_local.shape)}")


class TorchWorld:
    """The ranks of torch.distributed's default group (or `group`). Under nccl (RCCL) exchange is all_to_all_single and publish is
    all_gather_into_tensor on device tensors. Any other backend gathers every rank's whole flat buffer and cuts out the segment (device
    tensors staged through the host, index.all_gather_dim0): slower, the same recv, and everything behind it is the same code."""

    def __init__(self, group=None):
        import torch.distributed as dist
        if not dist.is_initialized():
            raise RuntimeError("TorchWorld needs an initialised process group (torch.distributed.init_process_group)")
        self.dist, self.group = dist, group
        self.rank, self.size = dist.get_rank(group), dist.get_world_size(group)
        self.backend = dist.get_backend(group)

    def _all_gather(self, t):
        from .index import all_gather_dim0
        return all_gather_dim0(t.contiguous(), self.size, self.group)

    def gather_rows(self, x_local, bounds):
        _check_gather(x_local, bounds, self.rank)
        x = x_local.detach().to(torch.float32)
        rows = max(hi - lo for lo, hi in bounds)
        if rows == 0:
            return x.new_zeros((0, x.shape[1]))
        padded = x.new_zeros((rows, x.shape[1]))
        padded[:x.shape[0]] = x
        full = self._all_gather(padded).view(self.size, rows, x.shape[1])
        return torch.cat([full[r, :hi - lo] for r, (lo, hi) in enumerate(bounds)], dim=0)

    def exchange(self, flat):
        N, S = self.size, flat.numel() // self.size
        if self.backend == "nccl":
            recv = torch.empty_like(flat)
            self.dist.all_to_all_single(recv, flat, group=self.group)
            return recv.view(N, S)
        return self._all_gather(flat).view(N, N, S)[:, self.rank].contiguous()

    def publish(self, mine, flat):
        if self.backend == "nccl":
            self.dist.all_gather_into_tensor(flat, mine.contiguous(), group=self.group)
        else:
            flat.copy_(self._all_gather(mine))

    def gather_objects(self, obj):
        out = [None] * self.size
        self.dist.all_gather_object(out, obj, group=self.group)
        return out


class LoopbackAborted(RuntimeError):
    """Raised in the other emulated ranks when one of them has failed."""


class LoopbackWorld:
    """N ranks emulated inside one process, for tests of the whole composition without a transport. run(fn) calls fn(world_r) once per rank,
    each on a thread of its own, but ONE AFTER ANOTHER: a baton goes from rank to rank, rank r runs until it reaches a collective or its end
    and hands the baton to rank r + 1, and when the last rank has arrived the collective completes and rank 0 goes on. The order of every
    launch is therefore fixed, and a collective is a plain copy between the ranks' tensors. ranks[r] is rank r's world."""
    WAIT_SECONDS = 600.0

    class _Rank:
        def __init__(self, hub, rank):
            self.hub, self.rank, self.size = hub, rank, hub.size

        def gather_rows(self, x_local, bounds):
            _check_gather(x_local, bounds, self.rank)
            parts = self.hub._meet(self.rank, x_local.detach().to(torch.float32))
            return torch.cat(parts, dim=0)

        def exchange(self, flat):
            S = flat.numel() // self.size
            flats = self.hub._meet(self.rank, flat)
            return torch.stack([f[self.rank * S:(self.rank + 1) * S] for f in flats])

        def publish(self, mine, flat):
            S = flat.numel() // self.size
            for r, seg in enumerate(self.hub._meet(self.rank, mine)):
                flat[r * S:(r + 1) * S].copy_(seg)

        def gather_objects(self, obj):
            return list(self.hub._meet(self.rank, obj))

    def __init__(self, N):
        if not 1 <= int(N) <= MAX_RANKS:
            raise ValueError(f"LoopbackWorld({N}): 1 .. {MAX_RANKS} ranks")
        self.size = int(N)
        self.ranks = [self._Rank(self, r) for r in range(self.size)]
        self._cv = threading.Condition()
        self._turn, self._round, self._slots, self._result, self._failed = 0, 0, [None] * self.size, None, None

    def _wait(self, ready):
        if not self._cv.wait_for(lambda: self._failed is not None or ready(), timeout=self.WAIT_SECONDS):
            self._failed = self._failed or TimeoutError("an emulated rank waited too long: the ranks do not make the same collectives")
            self._cv.notify_all()
        if self._failed is not None:
            raise LoopbackAborted("another emulated rank failed") from self._failed

    def _meet(self, rank, value):
        """Rank `rank` arrives at a collective with `value`; returns every rank's value once all have arrived. The caller holds the baton."""
        with self._cv:
            self._slots[rank] = value
            if rank == self.size - 1:
                self._result, self._slots, self._round, self._turn = list(self._slots), [None] * self.size, self._round + 1, 0
            else:
                self._turn = rank + 1
            seen = self._round - (1 if rank == self.size - 1 else 0)
            self._cv.notify_all()
            self._wait(lambda: self._round > seen and self._turn == rank)
            return self._result

    def run(self, fn):
        """[fn(ranks[r]) for r in range(N)], the ranks taking turns as the class docstring says. An exception in one rank ends the others at
        their next collective and is raised here."""
        results, errors = [None] * self.size, [None] * self.size
        device = torch.cuda.current_device() if torch.cuda.is_available() else None
        self._turn, self._failed = 0, None

        def body(r):
            try:
                if device is not None:
                    torch.cuda.set_device(device)
                with self._cv:
                    self._wait(lambda: self._turn == r)
                results[r] = fn(self.ranks[r])
            except LoopbackAborted:
                pass
            except BaseException as e:  # noqa: BLE001 -- handed to the caller below
                errors[r] = e
                with self._cv:
                    self._failed = self._failed or e
                    self._cv.notify_all()
            finally:
                with self._cv:
                    if self._turn == r:
                        self._turn = r + 1
                    self._cv.notify_all()

        threads = [threading.Thread(target=body, args=(r,), name=f"loopback-rank-{r}") for r in range(self.size)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for e in errors:
            if e is not None:
                raise e
        if self._failed is not None:
            raise self._failed
        return results


# -- autograd ------------------------------------------------------------------------------------------------------------------------------
class _GatherWithGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_local, world, bounds):
        ctx.rows = bounds[world.rank]
        return world.gather_rows(x_local, bounds)

    @staticmethod
    def backward(ctx, grad):
        lo, hi = ctx.rows
        return grad[lo:hi], None, None


def gather_with_grad(world, x_local, bounds):
    """The [B, H] fp32 matrix of every rank's rows in rank order, own rows bit for bit. Its backward returns this rank's rows of the incoming
    gradient: every rank differentiates the identical full loss, so nothing is reduced there."""
    return _GatherWithGrad.apply(x_local, world, bounds)


def scalar_rank_sum(world, value):
    """The [1] fp32 tensor ((v_0 + v_1) + v_2) + ... of every rank's [1] fp32 device tensor `value`: the values are moved as bytes (one
    gather_rows of a row of four floats per rank, the kernel's smallest stride) and added in rank order by mdr_rank_sum, so every rank holds
    the same bits, dist.rank_sum_host's, whatever the transport. One collective; no library all-reduce."""
    if not (torch.is_tensor(value) and value.is_cuda and value.dtype == torch.float32 and value.numel() == 1):
        raise ValueError(f"value must be an fp32 tensor of one element on a HIP device (there is no CPU fallback), got {_lib.describe(value)}")
    row = torch.zeros((1, 4), dtype=torch.float32, device=value.device)
    row[0, :1].copy_(value.detach().reshape(1))
    recv = world.gather_rows(row, slice_bounds(world.size, world.size)).contiguous()
    return rank_sum(recv, torch.empty(4, dtype=torch.float32, device=value.device), n=1)[:1]


# -- the gradient bucket -------------------------------------------------------------------------------------------------------------------
class GradBucket:
    """One flat fp32 buffer behind every trainable parameter's .grad (flat_layout), allocated once and zeroed. The views are installed before
    the first backward: autograd then accumulates in place, optim.FusedAdam zeroes in place and its pointer table is built once. reduce():
    exchange, mdr_rank_sum, publish; afterwards every rank's .grad holds the same bits."""

    def __init__(self, model_params, world):
        self.world = world
        self.params = [p for p in model_params if p.requires_grad]
        if not self.params:
            raise ValueError("GradBucket: no trainable parameter")
        dev = self.params[0].device
        if dev.type != "cuda" or any(p.device != dev or p.dtype != torch.float32 for p in self.params):
            raise RuntimeError("GradBucket: every trainable parameter must be an fp32 tensor on one HIP device (there is no CPU fallback)")
        if not 1 <= world.size <= MAX_RANKS:
            raise ValueError(f"GradBucket: {world.size} ranks, the ordered sum is built for 1 .. {MAX_RANKS}")
        # mdr_optim_step reads 16-byte aligned gradients. Every tensor of the encoder is a multiple of 64, so the retriever's layout has no gap;
        # the reader's qa_outputs.bias, rank.bias and sp.bias are followed by one (zero for ever, summed like everything else)
        self.offsets, self.segment, padded = flat_layout([p.numel() for p in self.params], world.size, align=4)
        self.total = self.offsets[-1] + self.params[-1].numel()
        self.flat = torch.zeros(padded, dtype=torch.float32, device=dev)
        self.mine = torch.empty(self.segment, dtype=torch.float32, device=dev)
        for p, off in zip(self.params, self.offsets):
            p.grad = self.flat[off:off + p.numel()].view(p.shape)

    def contains(self, t):
        lo = self.flat.data_ptr()
        return lo <= t.data_ptr() and t.data_ptr() + t.numel() * 4 <= lo + self.flat.numel() * 4

    def reduce(self):
        recv = self.world.exchange(self.flat)
        rank_sum(recv, self.mine)
        self.world.publish(self.mine, self.flat)
