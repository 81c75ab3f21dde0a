"""CPU (-m "not gpu"): the host side of training on several ranks (multihop_dense_retrieval_amd/dist.py).

1  slice_bounds: contiguous, covering, balanced, empty only when B < N
2  flat_layout: the running sum, segments of a multiple of 1024 floats that cover the total
3  rank_sum_host is Python's float32 left-to-right addition, and on wide-exponent rows the descending order gives other bits
4  LoopbackWorld: publish(rank_sum_host(exchange(flat))) leaves the ordered sum of every rank's flat in every emulated rank; gather_rows and
   gather_with_grad with uneven and empty slices; a failing rank ends the others
5  two processes over gloo on CPU tensors: TorchWorld.gather_rows, exchange and publish leave the bytes LoopbackWorld leaves
6  scripts/train_mhop.py refuses --share-gpu with nccl and more ranks than devices, before it touches a device
7  include/mdr_rank_sum.h, the binding table and the library's exports agree
"""
import ctypes
import os
import re
import socket
import subprocess
import sys
from datetime import timedelta

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 8
CHILD_SECONDS = 120


def wide(seed, shape):
    """float32 values whose magnitudes span about 2^-20 .. 2^20: the order of a sum shows in its bits"""
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(shape) * np.exp2(rng.randint(-20, 21, shape))).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1, 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_slice_bounds_are_balanced_contiguous_and_empty_only_below_one_row_a_rank():
    from multihop_dense_retrieval_amd.dist import slice_bounds
    for B in range(21):
        for N in range(1, 17):
            b = slice_bounds(B, N)
            assert len(b) == N and b[0][0] == 0 and b[-1][1] == B
            assert all(b[r][1] == b[r + 1][0] for r in range(N - 1))
            sizes = [hi - lo for lo, hi in b]
            assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
            assert sizes[:B % N] == [B // N + 1] * (B % N)
            assert (min(sizes) == 0) == (B < N)


def test_flat_layout_is_the_running_sum_in_segments_of_1024():
    from multihop_dense_retrieval_amd.dist import flat_layout
    rng = np.random.RandomState(0)
    for N in (1, 2, 3, 8, 16):
        for sizes in ([1], [1024], [1025], [4096 * N], [4096 * N + 1], rng.randint(1, 5000, 37).tolist()):
            offsets, S, padded = flat_layout(sizes, N)
            total = sum(sizes)
            assert offsets == [sum(sizes[:i]) for i in range(len(sizes))]
            assert S % 1024 == 0 and padded == N * S >= total
            assert N * (S - 1024) < total  # the smallest such segment


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------------
def test_rank_sum_host_is_float32_addition_in_rank_order_and_the_order_shows():
    from multihop_dense_retrieval_amd.dist import rank_sum_host
    for N in (1, 2, 3, 8, 16):
        recv = wide(N, (N, 257))
        want = []
        for i in range(recv.shape[1]):
            acc = np.float32(recv[0, i])
            for r in range(1, N):
                acc = np.float32(acc + np.float32(recv[r, i]))
            want.append(acc)
        got = rank_sum_host(recv)
        assert got.dtype == np.float32 and np.array_equal(bits(got), bits(np.array(want, np.float32))), N
        if N >= 3:
            differ = int((bits(rank_sum_host(recv[::-1].copy())) != bits(got)).sum())
            print(f"N = {N}: {differ} of {recv.shape[1]} sums differ in the descending order")
            assert differ > 0, "the descending order gives the same bits: this input shows nothing"
    one = np.array([[-0.0, np.nan, np.inf, 1.5]], np.float32)
    one.view(np.uint32)[0, 1] = 0x7FC12345  # a payload
    assert np.array_equal(bits(rank_sum_host(one)), bits(one[0]))  # one rank: a copy of the bits
    assert np.array_equal(bits(rank_sum_host(np.full((3, 4), -0.0, np.float32))), bits(np.full(4, -0.0, np.float32)))
    assert np.isnan(rank_sum_host(np.array([[np.inf], [1.0], [-np.inf]], np.float32))[0])


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------------
def rank_flat(rank, sizes, N):
    """Rank `rank`'s flat gradient buffer for tensors of `sizes`: wide values in the tensors' places, zeros in the padding."""
    from multihop_dense_retrieval_amd.dist import flat_layout
    _, _, padded = flat_layout(sizes, N)
    flat = np.zeros(padded, np.float32)
    flat[:sum(sizes)] = wide(100 + rank, sum(sizes))
    return torch.from_numpy(flat)


def reduce_on(world, sizes):
    """What GradBucket.reduce() does, with the numpy statement of the kernel: returns this rank's flat afterwards."""
    from multihop_dense_retrieval_amd.dist import rank_sum_host
    flat = rank_flat(world.rank, sizes, world.size)
    recv = world.exchange(flat)
    assert tuple(recv.shape) == (world.size, flat.numel() // world.size)
    world.publish(torch.from_numpy(rank_sum_host(recv.numpy())), flat)
    return flat.numpy()


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_loopback_round_trip_leaves_the_ordered_sum_in_every_rank(N):
    from multihop_dense_retrieval_amd.dist import LoopbackWorld, rank_sum_host
    sizes = [1000, 1501, 7]  # the total is not divisible by N and not by 1024
    got = LoopbackWorld(N).run(lambda w: reduce_on(w, sizes))
    want = rank_sum_host(np.stack([rank_flat(r, sizes, N).numpy() for r in range(N)]))
    for r in range(N):
        assert np.array_equal(bits(got[r]), bits(want)), r


def gather_on(world, B):
    from multihop_dense_retrieval_amd.dist import gather_with_grad, slice_bounds
    bounds = slice_bounds(B, world.size)
    lo, hi = bounds[world.rank]
    full = torch.from_numpy(wide(7, (B, H)))
    plain = world.gather_rows(full[lo:hi], bounds)
    x = full[lo:hi].clone().requires_grad_(True)
    g = gather_with_grad(world, x, bounds)
    weight = torch.arange(B * H, dtype=torch.float32).reshape(B, H)
    if hi > lo:
        (g * weight).sum().backward()
        assert torch.equal(x.grad, weight[lo:hi])  # this rank's rows of the incoming gradient
    return plain.numpy(), g.detach().numpy()


@pytest.mark.parametrize("N,B", [(2, 5), (3, 4), (3, 1), (2, 1), (4, 0)])
def test_loopback_gather_rows_with_uneven_and_empty_slices(N, B):
    from multihop_dense_retrieval_amd.dist import LoopbackWorld
    want = wide(7, (B, H))
    for plain, g in LoopbackWorld(N).run(lambda w: gather_on(w, B)):
        assert plain.shape == (B, H) and np.array_equal(bits(plain), bits(want)) and np.array_equal(bits(g), bits(want))


def test_loopback_a_failing_rank_ends_the_others():
    from multihop_dense_retrieval_amd.dist import LoopbackWorld

    def fn(w):
        if w.rank == 1:
            raise KeyError("rank 1 fails before its first collective")
        return w.gather_objects(w.rank)

    with pytest.raises(KeyError):
        LoopbackWorld(3).run(fn)
    assert LoopbackWorld(3).run(lambda w: w.gather_objects(w.rank * 2)) == [[0, 2, 4]] * 3


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = [1000, 1501, 7]
GATHERS = (5, 1, 2, 0)  # B: uneven, an empty slice, even, nothing at all


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world_size, port, out_dir):
    import torch.distributed as dist
    from multihop_dense_retrieval_amd.dist import TorchWorld
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world_size))
    dist.init_process_group("gloo", rank=rank, world_size=world_size, timeout=timedelta(seconds=CHILD_SECONDS // 2))
    world = TorchWorld()
    assert (world.rank, world.size, world.backend) == (rank, world_size, "gloo")
    out = {f"gather{B}": gather_on(world, B)[0] for B in GATHERS}
    out["flat"] = reduce_on(world, SIZES)
    out["objects"] = np.array(world.gather_objects(rank * 3))
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    dist.destroy_process_group()


def test_two_gloo_processes_leave_the_loopback_bytes(tmp_path):
    import torch.multiprocessing as mp
    from multihop_dense_retrieval_amd.dist import LoopbackWorld
    port = _free_port()
    ctx = mp.get_context("spawn")
    children = [ctx.Process(target=_gloo_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for c in children:
        c.start()
    for c in children:
        c.join(CHILD_SECONDS)
    hung = [c for c in children if c.is_alive()]
    for c in hung:
        c.kill()
    assert not hung and [c.exitcode for c in children] == [0, 0], [c.exitcode for c in children]
    loop = LoopbackWorld(2).run(lambda w: reduce_on(w, SIZES))
    got = [np.load(tmp_path / f"rank{r}.npz") for r in range(2)]
    for r in range(2):
        assert np.array_equal(bits(got[r]["flat"]), bits(loop[r])) and np.array_equal(bits(got[r]["flat"]), bits(got[0]["flat"])), r
        for B in GATHERS:
            assert got[r][f"gather{B}"].shape == (B, H) and np.array_equal(bits(got[r][f"gather{B}"]), bits(wide(7, (B, H)))), (r, B)
        assert got[r]["objects"].tolist() == [0, 3]


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------------
def run_script(argv, **env):
    full = dict(os.environ, HIP_VISIBLE_DEVICES="0", CUDA_VISIBLE_DEVICES="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="1", **env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_mhop.py"), "--do_train"] + argv, capture_output=True, text=True,
                          timeout=300, env=full)


def test_the_script_refuses_share_gpu_with_nccl_and_more_ranks_than_devices(tmp_path):
    r = run_script(["--share-gpu", "--output_dir", str(tmp_path / "a")], RANK="1", LOCAL_RANK="1", WORLD_SIZE="2")
    assert r.returncode != 0 and "--share-gpu" in r.stderr and "gloo only" in r.stderr, r.stderr[-2000:]
    r = run_script(["--share-gpu", "--dist-backend", "nccl", "--local_rank", "0", "--output_dir", str(tmp_path / "a")], WORLD_SIZE="2")
    assert r.returncode != 0 and "gloo only" in r.stderr, r.stderr[-2000:]
    for backend in ("nccl", "gloo"):  # at most one device is visible here: two ranks without --share-gpu have nowhere to go
        r = run_script(["--dist-backend", backend, "--output_dir", str(tmp_path / "a")], RANK="1", LOCAL_RANK="1", WORLD_SIZE="2")
        assert r.returncode != 0 and "visible devices" in r.stderr and "--share-gpu" in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "a").exists()  # refused before the run directory is made


def test_the_new_flags_parse_and_default_to_one_rank():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train_mhop
    from multihop_dense_retrieval_amd import config
    d = config.train_args([])
    assert (d.dist_backend, d.share_gpu, d.dist_timeout, d.check_ranks, d.local_rank) == ("nccl", False, 1800, False, -1)
    a = config.train_args("--dist-backend gloo --share-gpu --dist-timeout 120 --check-ranks".split())
    assert (a.dist_backend, a.share_gpu, a.dist_timeout, a.check_ranks) == ("gloo", True, 120, True)
    assert train_mhop.rank_setup(d, environ={}) == (0, 1, -1)  # neither the flag nor a launcher: today's run
    env = {"RANK": "3", "LOCAL_RANK": "1", "WORLD_SIZE": "4", "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "1"}
    assert train_mhop.rank_setup(a, environ=env) == (3, 4, 1)
    a.local_rank = 2  # the reference's flag wins over LOCAL_RANK
    assert train_mhop.rank_setup(a, environ=env) == (3, 4, 2)


def test_rank_seed_keeps_rank_zero_and_separates_the_others():
    from multihop_dense_retrieval_amd.dist import rank_seed
    for seed in (0, 7, 0x5EED0123456789AB, 2 ** 62 - 1):
        seeds = [rank_seed(seed, r) for r in range(16)]
        assert seeds[0] == seed and len(set(seeds)) == 16 and all(0 <= s < 2 ** 64 for s in seeds)
        assert seeds[1] == seed ^ 0x9E3779B97F4A7C15 and seeds[3] == seed ^ ((3 * 0x9E3779B97F4A7C15) % 2 ** 64)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    from multihop_dense_retrieval_amd import _lib, build, dist, optim
    raw = open(os.path.join(ROOT, "include", "mdr_rank_sum.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mdr_rank_sum"] == sorted(dist.SIGNATURES) == sorted(dist.EXPORTED_SYMBOLS)
    assert not set(declared) & (set(optim.SIGNATURES) | set(_lib.EXPORTED_SYMBOLS))
    res, args = dist.SIGNATURES["mdr_rank_sum"]
    proto = re.search(r"\bmdr_rank_sum\s*\(([^)]*)\)", text).group(1)
    names = [a.strip().split()[-1].lstrip("*") for a in proto.split(",")]
    assert names == ["recv", "n_ranks", "n", "stride", "out", "stream"] and len(args) == len(names) and res is ctypes.c_int
    assert [a for a in args] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(build.build_lib()), "mdr_rank_sum")
    assert int(re.search(r"#define MDR_RANK_SUM_MAX_RANKS (\d+)", raw).group(1)) == dist.MAX_RANKS == 16
