"""CPU: the host model of the optimizer step (tests/optim_ref.py) against torch.optim.Adam + clip_grad_norm_, the loss scaler's state machine,
the chunk split, the warm-up schedule, and the header / binding / validation contract of include/mdr_optim.h. No device and no kernel runs
here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_ref as ref
from oracle import fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, WORKSPACE = -1, -4
C = ref.CHUNK
SIZE_LISTS = ([1], [3, 63, 64, 65], [C - 1, C, C + 1], [3 * C + 1], [5, 3 * C + 1, C, 1, 2 * C - 1])


def test_header_binding_and_library_agree():
    """The chunk size and the struct layouts of include/mdr_optim.h are the module's and the helper's (its symbol table:
    tests/test_capi_symbols.py::test_header_binding_and_library_agree)."""
    from multihop_dense_retrieval_amd import optim
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdr_optim.h")).read(), flags=re.S)
    assert int(re.search(r"#define MDR_OPTIM_CHUNK (\d+)", text).group(1)) == optim.CHUNK == ref.CHUNK
    # the struct layouts the Python side writes and reads
    assert optim.TENSOR_DTYPE.itemsize == 64 and optim.STATE_DTYPE.itemsize == 48
    fields = re.search(r"typedef struct mdr_optim_state \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(re.findall(r"(\w+);", fields)) == optim.STATE_DTYPE.names == tuple(ref.initial_state(1.0))
    fields = re.search(r"typedef struct mdr_optim_tensor \{(.*?)\}", text, flags=re.S).group(1)
    assert tuple(re.findall(r"(\w+);", fields)) == optim.TENSOR_DTYPE.names


@pytest.mark.parametrize("sizes", SIZE_LISTS, ids=lambda s: "-".join(map(str, s)))
def test_chunks_cover_every_element_once_inside_one_tensor(sizes):
    """mdr_optim_chunks and the chunk map mdr_optim_table_fill writes: every element of every tensor lies in exactly one chunk, a chunk lies
    inside one tensor, and the split depends on the sizes alone (other pointers and decays, the same map)."""
    from multihop_dense_retrieval_amd import optim
    total, first = optim.chunks(sizes)
    assert (total, first) == ref.chunks(sizes)
    assert optim.workspace_bytes(sizes) == (total * 8 + 255) // 256 * 256
    assert optim.table_bytes(sizes) == (len(sizes) * 64 + total * 8 + 255) // 256 * 256
    maps = []
    for base, wd in ((0x10000, 0.0), (0x7f0000000000, 0.5)):
        rows = [(base + 64 * i, base + 16, base + 32, base + 48, 0, n, wd) for i, n in enumerate(sizes)]
        blob, n_chunks = optim.build_table(rows)
        assert n_chunks == total and len(blob) == optim.table_bytes(sizes)
        descs = blob[:64 * len(sizes)].view(optim.TENSOR_DTYPE)
        assert descs["n"].tolist() == list(sizes) and descs["p"].tolist() == [r[0] for r in rows]
        maps.append(blob[64 * len(sizes): 64 * len(sizes) + 8 * total].view(np.int32).reshape(total, 2))
    assert np.array_equal(maps[0], maps[1])
    covered = [np.zeros(n, dtype=np.int32) for n in sizes]
    for c, (t, k) in enumerate(maps[0].tolist()):
        assert 0 <= t < len(sizes) and first[t] + k == c
        begin, end = k * C, min(sizes[t], (k + 1) * C)
        assert begin < end
        covered[t][begin:end] += 1
    assert all((cv == 1).all() for cv in covered)
    assert [(t, k * C, min(sizes[t], (k + 1) * C)) for t, k in maps[0].tolist()] == ref.chunk_ranges(sizes)


def test_chunks_refuse_what_is_not_a_size_list():
    from multihop_dense_retrieval_amd import optim
    for sizes in ([], [0], [5, -1], [4, 0, 4]):
        assert optim.chunks(sizes) == (-1, None) == ref.chunks(sizes)
        assert optim.table_bytes(sizes) == 0 and optim.workspace_bytes(sizes) == 0
    assert optim.lib().mdr_optim_chunks(None, 3, None) == -1


def test_replay_follows_torch_adam_with_clip_over_ten_steps():
    """The fp32 replay (loss scale 2^16 on the gradients, the clip, decay in one group) against torch's Adam + clip_grad_norm_ in float64.
    The bar is the GPU trajectory test's: e(replay) <= 2 e(torch fp32), e the largest |p - p64| / (|p64| + 1e-3) over the tensors; and
    torch's own fp32 run is a nonzero distance from fp64 on every tensor, so the bar says something."""
    params, targets = ref.trajectory_start()
    want = ref.torch_trajectory(params, targets, 10, torch.float64)
    e_torch = ref.traj_errors(ref.torch_trajectory(params, targets, 10, torch.float32), want)
    got, st = ref.replay_trajectory(params, targets, 10)
    e_ours = ref.traj_errors(got, want)
    print("e(replay) per tensor: " + " ".join(f"{e:.3g}" for e in e_ours))
    print("e(torch fp32) per tensor: " + " ".join(f"{e:.3g}" for e in e_torch))
    assert st["adam_step"] == 10 and st["skipped_total"] == 0 and st["loss_scale"] == 2.0 ** 16
    assert min(e_torch) > 0
    moved = max(float(np.abs(w - p).max()) for w, p in zip(want, params))
    assert moved > 5e-3  # the parameters went somewhere
    assert max(e_ours) <= 2 * max(e_torch), (max(e_ours), max(e_torch))


def _run(events, dynamic, scale_window, max_scale, scale0):
    st, seen = ref.initial_state(scale0), []
    for bad in events:
        st = ref.advance(st, bad, 0.9, 0.999, dynamic, scale_window, max_scale)
        seen.append(st)
    return seen


# clean, clean, clean (the scale doubles), inf (halves, skip), nan (halves, skip), clean
WINDOW3 = (False, False, False, True, True, False)


def test_state_machine_window_of_three():
    seen = _run(WINDOW3, 1, 3, 2.0 ** 24, 2.0 ** 16)
    assert [s["loss_scale"] for s in seen] == [2.0 ** 16, 2.0 ** 16, 2.0 ** 17, 2.0 ** 16, 2.0 ** 15, 2.0 ** 15]
    assert [s["unskipped"] for s in seen] == [1, 2, 0, 0, 0, 1]
    assert [s["adam_step"] for s in seen] == [1, 2, 3, 3, 3, 4]
    assert [s["skipped_last"] for s in seen] == [0, 0, 0, 1, 1, 0]
    assert [s["skipped_total"] for s in seen] == [0, 0, 0, 1, 2, 2]
    b1 = np.float32(0.9)
    assert seen[2]["b1_pow"] == seen[4]["b1_pow"] == b1 * b1 * b1 and seen[5]["b1_pow"] == b1 * b1 * b1 * b1
    assert seen[5]["b2_pow"] == np.float32(0.999) * np.float32(0.999) * np.float32(0.999) * np.float32(0.999)
    assert seen[3]["bias2"] == seen[4]["bias2"] == seen[2]["bias2"] != seen[5]["bias2"]
    for k, s in ((1, seen[0]), (3, seen[4]), (4, seen[5])):  # the carried bias terms keep their relative precision; 1 - b2_pow does not
        for name, beta in (("bias1", 0.9), ("bias2", 0.999)):
            exact = 1.0 - float(np.float32(beta)) ** k
            assert abs(float(s[name]) - exact) <= 4 * k * fp.U32 * exact, (k, name)
    assert abs(float(np.float32(1) - seen[5]["b2_pow"]) - (1.0 - float(np.float32(0.999)) ** 4)) > 1e-6 * (1.0 - 0.999 ** 4)


def test_state_machine_clamps_at_max_scale_and_static_scale_never_moves():
    seen = _run((False,) * 5, 1, 1, 2.0 ** 18, 2.0 ** 16)
    assert [s["loss_scale"] for s in seen] == [2.0 ** 17, 2.0 ** 18, 2.0 ** 18, 2.0 ** 18, 2.0 ** 18]
    seen = _run((False, True, False, False, True), 0, 1, 2.0 ** 24, 128.0)
    assert [s["loss_scale"] for s in seen] == [128.0] * 5
    assert [s["skipped_last"] for s in seen] == [0, 1, 0, 0, 1] and [s["adam_step"] for s in seen] == [1, 1, 2, 3, 3]
    assert [s["unskipped"] for s in seen] == [1, 1, 2, 3, 3]


def test_replay_step_skips_on_a_non_finite_gradient():
    p0 = [np.linspace(-1, 1, 70, dtype=np.float32)]
    for poison in (np.inf, np.nan):
        params, moments = [p0[0].copy()], [(np.zeros(70, np.float32), np.zeros(70, np.float32))]
        g = np.ones(70, np.float32)
        g[-1] = poison
        st = ref.replay_step(ref.initial_state(2.0 ** 16), params, [g], moments, [0.0], 1e-3, 0.9, 0.999, 1e-8, 2.0, 1, 2000, 2.0 ** 24)
        assert st["skipped_last"] == 1 and st["loss_scale"] == 2.0 ** 15 and st["adam_step"] == 0
        assert np.array_equal(params[0], p0[0]) and not moments[0][0].any()


def test_clip_and_mult_are_fp32_expressions():
    coef, mult = ref.clip_and_mult(np.float32(8.0), 2.0, 2.0 ** 16)
    assert coef == np.float32(2.0) / (np.float32(8.0) + np.float32(1e-6)) and mult == coef / np.float32(2.0 ** 16)
    assert ref.clip_and_mult(np.float32(0.5), 2.0, 4.0) == (np.float32(1.0), np.float32(0.25))


def test_linear_schedule_with_warmup_closed_form():
    from multihop_dense_retrieval_amd.optim import linear_schedule_with_warmup as f
    w, t = 10, 110
    assert f(0, w, t) == 0.0 and f(5, w, t) == 0.5 and f(w, w, t) == 1.0
    assert f(60, w, t) == 0.5 and f(t, w, t) == 0.0 and f(t + 7, w, t) == 0.0
    for s in range(0, 130):
        assert f(s, w, t) == (s / w if s < w else max(0.0, (t - s) / (t - w)))
    assert f(0, 0, 10) == 1.0 and f(3, 0, 0) == 0.0  # no warm-up; a zero-length run does not divide by zero
    sched_lrs = []
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=2.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: f(s, 2, 6))
    for _ in range(7):
        sched_lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert sched_lrs == [0.0, 1.0, 2.0, 1.5, 1.0, 0.5, 0.0]


def test_arguments_are_validated_without_a_device():
    """What the host can see gives MDR_E_INVALID, a short workspace MDR_E_WORKSPACE, each with a message and before anything touches a
    device (this machine may have none)."""
    from multihop_dense_retrieval_amd import optim
    L = optim.lib()
    T, S, W = 0x100000, 0x200000, 0x300000  # never dereferenced: every call below is refused first
    good = dict(table=T, n_tensors=2, n_chunks=5, state=S, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, max_grad_norm=2.0, dynamic=1,
                scale_window=2000, max_scale=2.0 ** 24, zero_grads=1, ws=W, ws_bytes=40)

    def step(**kw):
        a = dict(good, **kw)
        return L.mdr_optim_step(a["table"], a["n_tensors"], a["n_chunks"], a["state"], a["lr"], a["beta1"], a["beta2"], a["eps"], a["max_grad_norm"],
                                a["dynamic"], a["scale_window"], a["max_scale"], a["zero_grads"], a["ws"], a["ws_bytes"], 0, None)

    bad = [dict(table=None), dict(state=None), dict(n_tensors=0), dict(n_tensors=-3), dict(n_chunks=1), dict(n_chunks=-1), dict(table=T + 4),
           dict(state=S + 8), dict(ws=W + 2), dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=1.5), dict(eps=0.0), dict(eps=-1e-8),
           dict(eps=float("nan")), dict(scale_window=0), dict(dynamic=2), dict(zero_grads=-1), dict(max_grad_norm=0.0), dict(lr=float("inf")),
           dict(max_scale=0.0)]
    for kw in bad:
        assert step(**kw) == INVALID, kw
        assert b"mdr_optim_step" in L.mdr_last_error(), kw
    for kw in (dict(ws=None), dict(ws_bytes=39), dict(ws_bytes=0)):
        assert step(**kw) == WORKSPACE, kw
        assert b"workspace" in L.mdr_last_error()
    for args in ((None, T, 2, 5, 0.5), (T, None, 2, 5, 0.5), (T, T, 0, 5, 0.5), (T, T, 2, 1, 0.5), (T + 8, T, 2, 5, 0.5), (T, T, 2, 5, 1.5), (T, T, 2, 5, -0.1)):
        assert L.mdr_optim_ema(*args, 0, None) == INVALID, args
    for args in ((None, 65536.0), (S + 4, 65536.0), (S, 0.0), (S, -1.0), (S, float("inf"))):
        assert L.mdr_optim_state_init(*args, 0, None) == INVALID, args
    # the table: a NULL p, n < 1, a misaligned pointer, a g without moments, a short buffer
    ok = (0x1000, 0x2000, 0x3000, 0x4000, 0x5008, 7, 0.0)
    optim.build_table([ok])
    for i, v in ((0, 0), (5, 0), (5, -2), (0, 0x1004), (1, 0x2008), (4, 0x5004), (2, 0), (3, 0)):
        row = list(ok)
        row[i] = v
        with pytest.raises(RuntimeError):
            optim.build_table([tuple(row)])
    descs = np.zeros(1, dtype=optim.TENSOR_DTYPE)
    descs["p"], descs["n"] = 0x1000, 7
    out, n_chunks = np.zeros(256, np.uint8), ctypes.c_int(0)
    assert L.mdr_optim_table_fill(descs.ctypes.data, 1, out.ctypes.data, 255, ctypes.byref(n_chunks)) == INVALID
    assert L.mdr_optim_table_fill(descs.ctypes.data, 1, out.ctypes.data, 256, ctypes.byref(n_chunks)) == 0 and n_chunks.value == 1


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import optim
    p = torch.nn.Parameter(torch.zeros(4, 4))
    with pytest.raises(RuntimeError):
        optim.FusedAdam([p], lr=1e-3)
    with pytest.raises(RuntimeError):
        optim.momentum_update([p], [torch.nn.Parameter(torch.zeros(4, 4))], 0.999)


def test_packed_linear_checks_weight16_before_anything_runs():
    from multihop_dense_retrieval_amd import linear
    import inspect
    assert list(inspect.signature(linear.packed_linear).parameters) == ["x", "weight", "bias", "gelu", "rows", "weight16"]
    assert inspect.signature(linear.packed_linear).parameters["weight16"].default is None
