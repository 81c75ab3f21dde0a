"""GPU (-m gpu): dropout in isolation (include/mdr_dropout.h) against the host restatement of tests/dropout_ref.py: the device generator bit
for bit, the row kernel's output bits, the mask of EVERY (sequence, head, query, key) read out of the attention kernels, and the training
forward and its backward against the fp64 model inside the derived bound. No tolerance here was read off a device. Every output buffer starts as
a finite sentinel between guard rows, which must keep their bits.

The bound and the one-hot cases run at two heads and five short lengths, and again at the geometry training uses: 12 and 16 heads, L = 512, the
edge lengths of tests/attention_grad_ref.py in one ragged call (eight chunks, eight owner blocks, row strides of 3 x 768 and 3 x 1024 halves, a
mask counter in the hundreds); the row kernel at 2051 rows of 768 and 1024. Almost all of a case's time is its fp64 reference on the host.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attention_grad_ref as agr
import dropout_ref as ref
from guarded import E_INVALID, E_WORKSPACE, OK, SENTINEL, Guarded, dev
from multihop_dense_retrieval_amd._lib import ptr
from oracle import attention_oracle as ao
from oracle import fp
from oracle.fp import bits

pytestmark = pytest.mark.gpu

GUARD = 8
SEED, SITE = 0x9abcdef012345678, 7   # (the seed's high word is set)


def libs():
    from multihop_dense_retrieval_amd import _lib, attention, dropout
    return _lib, attention, dropout


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [5, SEED], ids=["low", "high-word"])
@pytest.mark.parametrize("c2", [0, 65535 * 16 + 15])
def test_device_generator_is_the_replica(seed, c2):
    _lib, _, dropout = libs()
    out = torch.full((GUARD + 128 * 128 + GUARD, 16), 0xa5, dtype=torch.uint8, device="cuda")
    own = out[GUARD:GUARD + 128 * 128]
    _lib.check(dropout.lib().mdr_test_dropout_bytes(seed, c2, SITE, 128, 128, ptr(own), 0, _lib.current_stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:GUARD] == 0xa5).all() and (got[GUARD + 128 * 128:] == 0xa5).all()
    want = ref.call_bytes(seed, np.arange(128)[:, None], np.arange(128)[None, :], c2, SITE).reshape(128 * 128, 16)
    assert np.array_equal(got[GUARD:GUARD + 128 * 128], want)


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
def rows_call(x, T, seed, site, y, y16=None, add16=None, rows=None, M=None, N=None):
    _lib, _, dropout = libs()
    return dropout.lib().mdr_dropout_rows(ptr(x), 1 if x.dtype == torch.float16 else 0, ptr(add16), x.shape[0] if M is None else M, ptr(rows),
                                          x.shape[1] if N is None else N, T, seed, site, ptr(y), ptr(y16), 0, _lib.current_stream_ptr())


# The small grid, then the widths training calls it at: 2051 rows of 768 and 1024 are 385 and 513 workgroups, the last one partial, where the
# small grid has at most four; a thread's (row, group) comes from a division of an index that runs past 131 000.
ROWS_WIDE = [(2051, 768), (2051, 1024)]
ROWS_GRID = ([(M, N, x16, p) for p in (0.1, 0.5) for x16 in (True, False) for N in (64, 192) for M in (1, 5, 67)] +
             [(M, N, x16, 0.1) for x16 in (True, False) for M, N in ROWS_WIDE])


@pytest.mark.parametrize("M,N,x16,p", ROWS_GRID, ids=[f"{M}-{N}-{'fp16' if x16 else 'fp32-also16'}-{p}" for M, N, x16, p in ROWS_GRID])
def test_rows_forward_bits(M, N, x16, p):
    """y bits == x * m in numpy from the replica's mask; fp32: y16 == fp16(y32); with a row count, the rows behind it and the guards keep the
    sentinel (the wide cases: also a count of 0, for which nothing is written); an inf at a dropped position gives NaN."""
    _lib, _, dropout = libs()
    T = dropout.threshold(p)
    dt, tdt = (np.float16, torch.float16) if x16 else (np.float32, torch.float32)
    x = (np.random.default_rng([M, N, T]).standard_normal((M, N)) * 3).astype(dt)
    keep = ref.hidden_keep(M, N, T, SEED, SITE)
    assert (~keep).any()
    at = tuple(np.argwhere(~keep)[0])
    x[at] = np.inf
    m = np.where(keep, ref.scale(T), np.float32(0))
    with np.errstate(invalid="ignore"):
        want = (x.astype(np.float32) * m).astype(dt)
    assert np.isnan(want[at])
    for valid in sorted({M, max(M - 2, 0)} | ({0} if (M, N) in ROWS_WIDE else set())):
        y = Guarded(M, (N,), tdt, GUARD, GUARD, name="y")
        y16 = None if x16 else Guarded(M, (N,), torch.float16, GUARD, GUARD, name="y16")
        rows = None if valid == M else torch.tensor([valid], dtype=torch.int32, device="cuda")
        _lib.check(rows_call(dev(x), T, SEED, SITE, y.own, None if x16 else y16.own, rows=rows))
        torch.cuda.synchronize()
        got = y.checked(valid=valid)
        assert np.array_equal(bits(got[:valid]), bits(want[:valid])), (M, N, valid)
        if not x16:
            with np.errstate(over="ignore"):
                assert np.array_equal(bits(y16.checked(valid=valid)[:valid]), bits(want[:valid].astype(np.float16)))
    # T = 0 keeps every bit
    y = Guarded(M, (N,), tdt, GUARD, GUARD)
    _lib.check(rows_call(dev(x), 0, SEED, SITE, y.own))
    torch.cuda.synchronize()
    assert np.array_equal(bits(y.checked()), bits(x))


@pytest.mark.parametrize("x16", [True, False], ids=["fp16", "fp32-also16"])
def test_rows_autograd_backward_replays_the_mask(x16):
    """packed_dropout's backward is zero exactly where the forward's mask is zero and carries the scale elsewhere; with also16 the two gradients
    are added in fp32 under one mask; rows behind the count get a zero gradient; p with T = 0 returns x itself."""
    _, _, dropout = libs()
    M, N, p = 67, 192, 0.1
    T = dropout.threshold(p)
    rng = np.random.default_rng(9)
    x_h = rng.standard_normal((M, N)).astype(np.float16 if x16 else np.float32)
    keep = ref.hidden_keep(M, N, T, SEED, SITE)
    m = np.where(keep, ref.scale(T), np.float32(0))
    for valid in (M, M - 3):
        rows = None if valid == M else torch.tensor([valid], dtype=torch.int32, device="cuda")
        x = dev(x_h).requires_grad_(True)
        g_h = fp.grid((M, N), 3, dtype=x_h.dtype) + x_h.dtype.type(5)   # 3 .. 7: never zero, also with a g16 in -2 .. 2 added
        if x16:
            y = dropout.packed_dropout(x, p, SEED, SITE, rows=rows)
            y.backward(dev(g_h))
            want = (g_h.astype(np.float32) * m).astype(np.float16)
        else:
            y, y16 = dropout.packed_dropout(x, p, SEED, SITE, rows=rows, also16=True)
            g16_h = fp.grid((M, N), 4, dtype=np.float16)
            torch.autograd.backward([y, y16], [dev(g_h), dev(g16_h)])
            want = (g_h + g16_h.astype(np.float32)) * m
            assert np.array_equal(bits(y16.detach().cpu().numpy()), bits(y.detach().cpu().numpy().astype(np.float16)))
        torch.cuda.synchronize()
        got, out = x.grad.cpu().numpy(), y.detach().cpu().numpy()
        assert got.dtype == x_h.dtype
        want[valid:] = 0
        assert np.array_equal(bits(got + got.dtype.type(0)), bits(want + want.dtype.type(0)))
        assert ((got[:valid] == 0) == ~keep[:valid]).all()
        assert ((out[:valid] == 0) == (~keep[:valid] | (x_h[:valid] == 0))).all() and (out[valid:] == 0).all()
    x = dev(x_h).requires_grad_(True)
    assert dropout.packed_dropout(x, 0.001, SEED, SITE) is x and dropout.threshold(0.001) == 0


# ---- attention: plumbing ---------------------------------------------------------------------------------------------------------------------
def fwd_call(qkv, cu, heads, L, mode, T, seed, site, out, B=None, hidden=None, stream="current"):
    _lib, _, dropout = libs()
    return dropout.lib().mdr_attention_dropout_forward(ptr(qkv), ptr(cu), cu.numel() - 1 if B is None else B, L, 64 * heads if hidden is None else hidden, heads,
                                                       mode, T, seed, site, ptr(out), 0, _lib.current_stream_ptr() if stream == "current" else stream)


def bwd_call(qkv, dctx, cu, heads, L, mode, T, seed, site, out, ws="auto"):
    _lib, attention, dropout = libs()
    B = cu.numel() - 1
    need = int(attention.lib().mdr_attention_backward_workspace_bytes(B, L, heads, mode))
    w = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda") if ws == "auto" else ws
    return dropout.lib().mdr_attention_dropout_backward(ptr(qkv), ptr(dctx), ptr(cu), B, L, 64 * heads, heads, mode, T, seed, site, ptr(out), ptr(w),
                                                        w.numel() if w is not None else 0, 0, _lib.current_stream_ptr())


def run(qkv, dctx, cu, heads, L, mode, T, seed=SEED, site=SITE):
    """(ctx, dqkv) of one forward and (dctx given) one backward call, numpy float16, after asserting MDR_OK, that the guard rows kept their bits
    and that the ctx rows of empty sequences (mode 3) were not written."""
    _lib = libs()[0]
    cu = np.asarray(cu, np.int32)
    lens = np.diff(cu)
    assert lens.max() <= L and lens.min() >= 0
    Tn, hidden, B = int(cu[-1]), 64 * heads, len(cu) - 1
    q, c = dev(qkv), dev(cu)
    ctx = Guarded(B if mode == 3 else Tn, (hidden,), torch.float16, GUARD, GUARD, name="ctx")
    _lib.check(fwd_call(q, c, heads, L, mode, T, seed, site, ctx.own))
    dqkv = None
    if dctx is not None:
        dqkv = Guarded(Tn, (3 * hidden,), torch.float16, GUARD, GUARD, name="dqkv")
        _lib.check(bwd_call(q, dev(dctx), c, heads, L, mode, T, seed, site, dqkv.own))
    torch.cuda.synchronize()
    got = ctx.checked().copy()
    if mode == 3:
        assert (got[lens == 0] == SENTINEL).all(), "the ctx row of an empty sequence was written"
        got[lens == 0] = 0
    return got, None if dqkv is None else dqkv.checked()


# ---- attention: the mask, read out of the kernels --------------------------------------------------------------------------------------------
READOUT = [[1, 0, 63, 129], [3, 64, 0, 130], [5, 65, 512, 0]]


def readout_inputs(lens, heads, seed):
    """Q and K from the grid, small enough that no probability underflows fp16 (|s| <= 1/2, so p >= e^-1 / n); V is filled by the caller."""
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    qkv = fp.grid((int(cu[-1]), 3 * 64 * heads), seed, 0.125, np.float16)
    return qkv, cu


def keep_of(cu, heads, mode, T):
    return [None if m is None else m != 0 for m in ref.attn_masks(cu, heads, mode, T, SEED, SITE)]


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("lens", READOUT, ids=lambda v: "-".join(map(str, v)))
@pytest.mark.parametrize("mode", [0, 3])
def test_forward_mask_read_out_for_every_probability(mode, lens, heads):
    """V_j = e_(j - w) inside a window of 64 keys and 0 elsewhere: ctx[i, j - w] != 0 iff (i, j) was kept, whatever p's bits are. The window
    sweeps the sequence; every (b, h, i, j) is compared with the replica."""
    T, hidden, L = 128, 64 * heads, max(lens)
    qkv, cu = readout_inputs(lens, heads, 21)
    keep = keep_of(cu, heads, mode, T)
    for w in range(0, L, 64):
        qkv[:, 2 * hidden:] = 0
        for b, n in enumerate(lens):
            for j in range(w, min(n, w + 64)):
                qkv[int(cu[b]) + j, 2 * hidden + (j - w) + 64 * np.arange(heads)] = 1
        ctx, _ = run(qkv, None, cu, heads, L, mode, T)
        for b, n in enumerate(lens):
            if n <= w:
                continue
            rows = ctx[b:b + 1] if mode == 3 else ctx[int(cu[b]):int(cu[b + 1])]
            got = rows.reshape(rows.shape[0], heads, 64).transpose(1, 0, 2)[:, :, :min(n, w + 64) - w] != 0
            assert np.array_equal(got, keep[b][:, :, w:w + 64]), (b, n, w, np.argwhere(got != keep[b][:, :, w:w + 64])[0])


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("lens", READOUT, ids=lambda v: "-".join(map(str, v)))
def test_backward_column_pass_mask_read_out(lens, heads):
    """dO_i = e_(i - w) inside a window of 64 queries: dV[j, i - w] = Pd_ij != 0 iff (i, j) was kept."""
    T, hidden, L = 128, 64 * heads, max(lens)
    qkv, cu = readout_inputs(lens, heads, 22)
    keep = keep_of(cu, heads, 0, T)
    for w in range(0, L, 64):
        dctx = np.zeros((int(cu[-1]), hidden), np.float16)
        for b, n in enumerate(lens):
            for i in range(w, min(n, w + 64)):
                dctx[int(cu[b]) + i, (i - w) + 64 * np.arange(heads)] = 1
        _, dqkv = run(qkv, dctx, cu, heads, L, 0, T)
        for b, n in enumerate(lens):
            if n <= w:
                continue
            rows = dqkv[int(cu[b]):int(cu[b + 1]), 2 * hidden:]
            got = rows.reshape(n, heads, 64).transpose(1, 2, 0)[:, :min(n, w + 64) - w] != 0   # [h, i - w, j]
            assert np.array_equal(got, keep[b][:, w:w + 64]), (b, n, w, np.argwhere(got != keep[b][:, w:w + 64])[0])


@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("lens", READOUT, ids=lambda v: "-".join(map(str, v)))
def test_backward_first_query_mask_read_out(lens, heads):
    """Mode 3 with dO = 1: dV[j, c] = Pd_0j != 0 iff (0, j) was kept, in every column."""
    T, hidden, L = 128, 64 * heads, max(lens)
    qkv, cu = readout_inputs(lens, heads, 23)
    keep = keep_of(cu, heads, 3, T)
    _, dqkv = run(qkv, np.ones((len(lens), hidden), np.float16), cu, heads, L, 3, T)
    for b, n in enumerate(lens):
        if n:
            got = dqkv[int(cu[b]):int(cu[b + 1]), 2 * hidden:].reshape(n, heads, 64) != 0
            assert np.array_equal(got, np.broadcast_to(keep[b][:, 0].T[:, :, None], got.shape)), (b, n)


# ---- attention: inside the derived bound ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("scale", [1.0, 256.0], ids=["unit", "x256"])
@pytest.mark.parametrize("family", ["realistic1", "spike16"])
@pytest.mark.parametrize("mode", [0, 3])
def test_forward_and_backward_within_the_derived_bound(mode, family, scale, p):
    check_bound(2, max(ref.LENS_BOUND), ref.LENS_BOUND, mode, family, scale, p)


@functools.lru_cache(maxsize=1)
def family_inputs(family, heads, lens):
    """(qkv, cu) of a family over the lengths `lens` (a tuple), made once for the consecutive cases that differ in scale and p alone (a hundred
    sequences at twelve heads take longer to draw than to check); nobody writes to them."""
    return ao.FAMILIES[family](list(lens), heads, 11)


def dqkv_locator(cu, heads):
    """index (row, column) of dqkv -> "sequence b, len n, head h, dQ | dK | dV": the `where` of fp.assert_within"""
    return lambda at: f"{ao.locator(cu, 1)((at[0], at[1] % (64 * heads)))}, {'dQ dK dV'.split()[at[1] // (64 * heads)]}"


def check_bound(heads, L, lens, mode, family, scale, p):
    """One forward and one backward call over the ragged batch `lens`: EVERY element of ctx and of dqkv inside the derived bound of the fp64 model
    under the replica's masks. Prints the two worst ratios."""
    T = ref.threshold(p)
    qkv, cu = family_inputs(family, heads, tuple(lens))
    dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 2, scale)
    ctx, dqkv = run(qkv, dctx, cu, heads, L, mode, T)
    ctx_r, ctx_b, dqkv_r, dqkv_b = ref.reference_and_bound(qkv, dctx, cu, heads, mode, ref.attn_masks(cu, heads, mode, T, SEED, SITE))
    label = f"mode={mode} heads={heads} L={L} family={family} scale={scale} p={p}"
    print(f"RATIO {label} ctx {fp.worst_ratio(ctx, ctx_r, ctx_b)[0]:.4f} dqkv {fp.worst_ratio(dqkv, dqkv_r, dqkv_b)[0]:.4f}")
    fp.assert_within(ctx, ctx_r, ctx_b, "ctx " + label, ao.locator(cu, 3 if mode == 3 else 1))
    fp.assert_within(dqkv, dqkv_r, dqkv_b, "dqkv " + label, dqkv_locator(cu, heads))


# The geometry training runs at, which the two heads and five short lengths above do not reach: 12 heads (the retriever) and 16 heads (the
# answer reader: a row stride of 3 x 1024 halves in qkv and dqkv, 1024 in ctx), L = 512, the lengths -1, 0, +1 around every multiple of the MFMA
# tile up to 512 in attention_grad_ref's four interleaved groups. A call holds 25 sequences (mode 3: 100), so the forward's and the backward's
# running (max, sum) go over up to eight chunks of 64 keys -- under stair_up the maximum rises in every one --, the owner blocks 0 .. 7 meet a
# sequence's end at every tile edge, and the mask counter b * heads + h runs to 24 * 12 + 11 (mode 3: 99 * 12 + 11), where a counter of any
# other stride in `heads` draws another mask than the replica's. The gradient carries a loss scale of 256, as in training.
BOUND_TRAINING = [(12, 0, "stair_up", 256.0, 0.1), (12, 1, "realistic4", 256.0, 0.1), (12, 2, "spike16", 256.0, 0.1), (12, 3, "stair_down", 256.0, 0.1),
                  (12, 1, "realistic4", 1.0, 0.5), (16, 1, "realistic4", 256.0, 0.1), (16, 1, "spike16", 256.0, 0.1)]


def scale_id(scale):
    return {1.0: "unit", 256.0: "x256"}[scale]


@pytest.mark.parametrize("heads,group,family,scale,p", BOUND_TRAINING,
                         ids=[f"h{h}-L512-edges{g}-{f}-{scale_id(s)}-p{p}" for h, g, f, s, p in BOUND_TRAINING])
def test_every_query_within_the_derived_bound_at_training_geometry(heads, group, family, scale, p):
    check_bound(heads, 512, agr.LENS_EDGES[group::4], 0, family, scale, p)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("scale", [1.0, 256.0], ids=scale_id)
@pytest.mark.parametrize("family", agr.FAMILY_NAMES)
@pytest.mark.parametrize("heads,lens", [pytest.param(12, agr.LENS_EDGES, id="h12-L512-edges"), pytest.param(16, agr.LENS_EDGES[1::4], id="h16-L512-edges1")])
def test_first_query_within_the_derived_bound_at_training_geometry(heads, lens, family, scale, p):
    """Mode 3: one ragged call of every edge length (100 sequences at 12 heads). The dQ rows behind a sequence's first have bound 0."""
    check_bound(heads, 512, lens, 3, family, scale, p)


# ---- attention: bit-known outputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("heads,L,lens", [pytest.param(1, 129, agr.LENS_SWEEP, id="h1-L129-sweep"), pytest.param(12, 512, agr.LENS_EDGES[1::4], id="h12-L512-edges1"),
                                          pytest.param(16, 512, agr.LENS_EDGES[1::4], id="h16-L512-edges1")])
def test_onehot_permutation_under_half_dropout_is_bit_known(heads, L, lens, mode):
    """q_i = code(pi(i)): the fp16-rounded p is exactly a permutation matrix, and at T = 128 the factor is exactly 2. So ctx[i] == fp16(2 V[pi(i)])
    where the replica keeps (i, pi(i)) and +0 where it drops it, and dV[pi(i)] == fp16(2 dO[i]) or 0 likewise, bit for bit: the query -> key ->
    mask byte map of every tile, chunk, lane slot, owner block, head and sequence at once, where a bound can only say it loosely. dQ and dK stay
    within the derived bound. Mode 3 (the first query: ctx[b], and dV in row pi(0)) gives the same pattern -- e = 1, inv = 1 and m = 2 make its
    two products exact, as tests/test_dropout_host.py shows on the emulation; its dK and dV rows are single products, whose zero takes the
    operands' signs, so dV compares there with -0 counted as +0."""
    qkv, cu, expected = ao.onehot(lens, heads, 3)
    hidden = 64 * heads
    dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), hidden, 4)
    ctx, dqkv = run(qkv, dctx, cu, heads, L, mode, 128)
    masks = ref.attn_masks(cu, heads, mode, 128, SEED, SITE)
    ctx_w, dV_w, kept, pairs = ref.onehot_pattern(expected, dctx, cu, heads, mode, [m != 0 for m in masks])
    assert 0.3 * pairs < kept < 0.7 * pairs, (kept, pairs)   # both outcomes are well populated
    bad = np.argwhere(bits(ctx) != bits(ctx_w))
    assert not len(bad), ("ctx", len(bad), bad[0], ao.locator(cu, 3 if mode == 3 else 1)(bad[0]), float(ctx[tuple(bad[0])]), float(ctx_w[tuple(bad[0])]))
    dV = dqkv[:, 2 * hidden:] + np.float16(0) if mode == 3 else dqkv[:, 2 * hidden:]
    bad = np.argwhere(bits(dV) != bits(dV_w))
    assert not len(bad), ("dV", len(bad), bad[0], ao.locator(cu, 1)(bad[0]), float(dV[tuple(bad[0])]), float(dV_w[tuple(bad[0])]))
    _, _, dqkv_r, dqkv_b = ref.reference_and_bound(qkv, dctx, cu, heads, mode, masks)
    label = f"mode={mode} heads={heads} L={L} family=onehot p=0.5"
    print(f"RATIO {label} kept {kept} of {pairs} dQ|dK {fp.worst_ratio(dqkv[:, :2 * hidden], dqkv_r[:, :2 * hidden], dqkv_b[:, :2 * hidden])[0]:.4f}")
    fp.assert_within(dqkv[:, :2 * hidden], dqkv_r[:, :2 * hidden], dqkv_b[:, :2 * hidden], "dQ | dK " + label, dqkv_locator(cu, heads))


# ---- attention: edge cases -------------------------------------------------------------------------------------------------------------------
def test_a_sequence_whose_only_key_is_dropped_gives_zeros():
    """Length 1, the seed found on the host so that (0, 0) of sequence 1 is dropped in both heads: ctx, dQ, dK and dV are exactly +0 in mode 0 (an
    MFMA accumulator starts at +0). Mode 3 forms dK and dV as single products, whose zero takes the operands' signs: zero by value there."""
    heads, T, lens = 2, 128, [5, 1, 3]
    seed = next(s for s in range(1, 4096) if not ref.attn_keep(0, 0, 2, T, s, SITE) and not ref.attn_keep(0, 0, 3, T, s, SITE))
    qkv, cu = ao.realistic(lens, heads, 4, 1.0)
    for mode in (0, 3):
        dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 5)
        ctx, dqkv = run(qkv, dctx, cu, heads, 8, mode, T, seed=seed)
        row = ctx[1] if mode == 3 else ctx[int(cu[1])]
        if mode == 0:
            assert (bits(row) == 0).all() and (bits(dqkv[int(cu[1])]) == 0).all()
        else:
            assert (row == 0).all() and (dqkv[int(cu[1])] == 0).all() and (bits(row) == 0).all()
        assert (ctx[0] != 0).any() and (dqkv[0] != 0).any()


@pytest.mark.parametrize("mode", [0, 3])
def test_two_runs_repeat_the_bits_and_another_seed_or_site_another_mask(mode):
    heads, lens, T = 2, [130, 0, 1, 64, 17], 26
    qkv, cu = ao.realistic(lens, heads, 6, 1.0)
    dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 7)
    a = run(qkv, dctx, cu, heads, 130, mode, T)
    b = run(qkv, dctx, cu, heads, 130, mode, T)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    for kw in (dict(seed=SEED + 1), dict(site=SITE + 1), dict(seed=SEED ^ (1 << 40))):
        c = run(qkv, dctx, cu, heads, 130, mode, T, **kw)
        assert not np.array_equal(bits(a[0]), bits(c[0])) and not np.array_equal(bits(a[1]), bits(c[1])), kw


@pytest.mark.parametrize("mode", [0, 3])
def test_non_finite_gradients_stay_in_their_sequence_and_head(mode):
    """One head's dO block of one sequence non-finite: every dQ (mode 3: the first query's), dK and dV element of that head in that sequence is
    non-finite -- also at dropped positions, 0 * Inf being NaN: the mask is a factor, not a select -- and everything else keeps its bits."""
    heads, lens, T = 2, [1, 64, 65, 130], 128
    L, hidden = max(lens), 64 * heads
    qkv, cu = ao.realistic(lens, heads, 24, 1.0)
    dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), hidden, 9)
    _, clean = run(qkv, dctx, cu, heads, L, mode, T)
    assert np.isfinite(clean.astype(np.float32)).all()
    for k, (victim, h) in enumerate([(0, 1), (1, 0), (2, 1), (3, 0)]):
        lo, hi = int(cu[victim]), int(cu[victim + 1])
        dirty = dctx.copy()
        (dirty[victim:victim + 1] if mode == 3 else dirty[lo:hi])[:, 64 * h:64 * (h + 1)] = [np.inf, -np.inf, np.nan][k % 3]
        _, got = run(qkv, dirty, cu, heads, L, mode, T)
        hit = np.zeros(got.shape, bool)
        for part in range(3):
            hit[slice(lo, lo + 1) if (mode == 3 and part == 0) else slice(lo, hi), part * hidden + 64 * h:part * hidden + 64 * (h + 1)] = True
        assert not np.isfinite(got[hit].astype(np.float32)).any(), (victim, h, "an element of the planted head stayed finite")
        assert np.array_equal(bits(got)[~hit], bits(clean)[~hit]), (victim, h, "the other head or another sequence changed")


def test_bad_arguments_are_errors_without_a_launch():
    _lib, attention, dropout = libs()
    L = dropout.lib()
    heads, T = 2, 26
    qkv = torch.zeros((8, 3 * 128), dtype=torch.float16, device="cuda")
    dctx = torch.zeros((8, 128), dtype=torch.float16, device="cuda")
    cu = torch.tensor([0, 3, 8], dtype=torch.int32, device="cuda")
    ctx = torch.full((8, 128), SENTINEL, dtype=torch.float16, device="cuda")
    out = torch.full((8, 3 * 128), SENTINEL, dtype=torch.float16, device="cuda")
    need = int(attention.lib().mdr_attention_backward_workspace_bytes(2, 8, 2, 0))
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def fwd(q=p(qkv), c=p(cu), B=2, Lx=8, hidden=128, heads=2, mode=0, T=T, o=p(ctx)):
        return L.mdr_attention_dropout_forward(q, c, B, Lx, hidden, heads, mode, T, SEED, SITE, o, 0, None)

    def bwd(q=p(qkv), d=p(dctx), c=p(cu), B=2, Lx=8, hidden=128, heads=2, mode=0, T=T, o=p(out), w=p(ws), wb=need):
        return L.mdr_attention_dropout_backward(q, d, c, B, Lx, hidden, heads, mode, T, SEED, SITE, o, w, wb, 0, None)

    shape_cases = ((dict(q=None), "NULL"), (dict(c=None), "NULL"), (dict(o=None), "NULL"), (dict(B=0), "B"), (dict(Lx=0), "L"), (dict(Lx=513), "L"),
                   (dict(hidden=96), "head dim"), (dict(heads=3), "head dim"), (dict(mode=1), "mode"), (dict(T=0), "T"), (dict(T=256), "T"), (dict(T=-1), "T"),
                   (dict(o=ctypes.c_void_p(ctx.data_ptr() + 2)), "aligned"))
    for kw, word in shape_cases:
        assert fwd(**kw) == E_INVALID, kw
        assert word in L.mdr_last_error().decode(), (kw, L.mdr_last_error())
    for kw, word in shape_cases[:-1] + ((dict(d=None), "NULL"), (dict(o=ctypes.c_void_p(out.data_ptr() + 2)), "aligned")):
        assert bwd(**kw) == E_INVALID, kw
        assert word in L.mdr_last_error().decode(), (kw, L.mdr_last_error())
    for kw in (dict(wb=2 * 8 * 2 * 8 - 1), dict(w=None), dict(w=None, wb=0)):
        assert bwd(**kw) == E_WORKSPACE, kw
        assert "workspace" in L.mdr_last_error().decode()
    x = torch.zeros((4, 64), dtype=torch.float32, device="cuda")
    y = torch.full((4, 64), SENTINEL, dtype=torch.float32, device="cuda")
    h = torch.full((4, 64), SENTINEL, dtype=torch.float16, device="cuda")

    def rows(xp=p(x), x16=0, a=None, M=4, N=64, T=T, yp=p(y), y16=None):
        return L.mdr_dropout_rows(xp, x16, a, M, None, N, T, SEED, SITE, yp, y16, 0, None)

    for kw, word in ((dict(xp=None), "NULL"), (dict(yp=None), "NULL"), (dict(x16=2), "x_is_fp16"), (dict(x16=1, y16=p(h)), "fp32 x only"),
                     (dict(x16=1, a=p(h)), "fp32 x only"), (dict(M=0), "M"), (dict(N=0), "N"), (dict(N=24), "N"), (dict(T=256), "T"), (dict(T=-1), "T"),
                     (dict(yp=ctypes.c_void_p(y.data_ptr() + 4)), "aligned")):
        assert rows(**kw) == E_INVALID, kw
        assert word in L.mdr_last_error().decode(), (kw, L.mdr_last_error())
    byt = torch.full((16, 16), 0xa5, dtype=torch.uint8, device="cuda")
    for n0, n1, o in ((0, 4, p(byt)), (4, 65537, p(byt)), (4, 4, None)):
        assert L.mdr_test_dropout_bytes(SEED, 0, SITE, n0, n1, o, 0, None) == E_INVALID
    assert L.mdr_dropout_threshold(ctypes.c_float(1.0)) == -1 and L.mdr_dropout_threshold(ctypes.c_float(0.1)) == 26
    torch.cuda.synchronize()
    assert (ctx == SENTINEL).all() and (out == SENTINEL).all() and (y == SENTINEL).all() and (h == SENTINEL).all() and (byt == 0xa5).all(), "a rejected call launched"
    assert fwd() == OK and bwd() == OK and fwd(mode=3) == OK and bwd(mode=3, w=None, wb=0) == OK and rows(y16=p(h)) == OK
    torch.cuda.synchronize()
    assert (ctx != SENTINEL).all() and (out != SENTINEL).all() and (y == 0).all() and (h == 0).all()


@pytest.mark.parametrize("cls_only", [False, True])
def test_autograd_function_with_and_without_dropout(cls_only):
    """packed_self_attention: dropout=None and dropout=(0.0, ...) give the bits of the existing forward and backward; dropout=(p, seed, site) gives
    the bits of direct calls of the two new entry points."""
    _lib, attention, dropout = libs()
    heads, L, lens = 2, 130, [70, 130, 1, 64]
    mode = 3 if cls_only else 0
    qkv_h, cu_h = ao.realistic(lens, heads, 25, 1.0)
    g_h = agr.dctx_grid(len(lens) if cls_only else int(cu_h[-1]), 64 * heads, 10)
    cu, g = dev(cu_h), dev(g_h)

    def through(**kw):
        qkv = dev(qkv_h).requires_grad_(True)
        out = attention.packed_self_attention(qkv, cu, heads, L, cls_only=cls_only, **kw)
        out.backward(g)
        torch.cuda.synchronize()
        return out.detach().cpu().numpy(), qkv.grad.cpu().numpy()

    q = dev(qkv_h)
    want = torch.zeros((len(lens) if cls_only else q.shape[0], 64 * heads), dtype=torch.float16, device="cuda")
    base = through()
    _lib.check(_lib.lib().mdr_test_attention(q.data_ptr(), cu.data_ptr(), None, len(lens), L, 64 * heads, heads, mode, want.data_ptr(), 0, _lib.current_stream_ptr()))
    direct = attention.attention_backward(q, g, cu, heads, L, mode)
    torch.cuda.synchronize()
    assert np.array_equal(bits(base[0]), bits(want.cpu().numpy())) and np.array_equal(bits(base[1]), bits(direct.cpu().numpy()))
    for kw in (dict(dropout=None), dict(dropout=(0.0, SEED, SITE)), dict(dropout=(0.001, SEED, SITE))):
        got = through(**kw)
        assert np.array_equal(bits(got[0]), bits(base[0])) and np.array_equal(bits(got[1]), bits(base[1])), kw
    got = through(dropout=(0.1, SEED, SITE))
    ctx, dqkv = run(qkv_h, g_h, cu_h, heads, L, mode, 26)
    assert np.array_equal(bits(got[0]), bits(ctx)) and np.array_equal(bits(got[1]), bits(dqkv))
    assert not np.array_equal(bits(got[0]), bits(base[0]))
