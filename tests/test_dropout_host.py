"""CPU (-m "not gpu"): the host restatement of dropout (tests/dropout_ref.py) -- the generator's known answers and drop rate, the fp64 model
against torch.autograd, the emulation of the kernels' dataflow inside the derived bound and every mutation outside it, the block-wise mask
builder against the per-element mapping, the one-hot family's bit-known pattern under p = 0.5, the two defects that need more than two heads
or a rising maximum -- and the agreement of include/mdr_dropout.h, dropout.SIGNATURES and the built library."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import attention_grad_ref as agr
import dropout_ref as ref
from oracle import attention_oracle as ao
from oracle import fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, SITE = 0x9abcdef012345678, 7


def test_philox_known_answers():
    """Philox4x32-10's known answers (the Random123 test vectors): zeros, all ones, and the digits of pi."""
    for ctr, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(w) for w in ref.philox(*ctr, *key)) == want
    # the byte order of a call, and the key of a seed
    w = ref.philox(1, 2, 3, 4, 0x12345678, 0x9abcdef0)
    b = ref.call_bytes(0x9abcdef012345678, 1, 2, 3, 4)
    assert [int(x) for x in b] == [(int(w[k >> 2]) >> (8 * (k & 3))) & 0xff for k in range(16)]
    assert int(ref.byte_of(0x9abcdef012345678, 1, 2, 3, 4, 9)) == int(b[9])


def test_threshold_scale_and_module_agree():
    from multihop_dense_retrieval_amd import dropout
    assert [ref.threshold(p) for p in (0.0, 0.001, 0.002, 0.1, 0.5, 0.997, 0.999, 1.0, -0.1, float("nan"))] == [0, 0, 1, 26, 128, 255, -1, -1, -1, -1]
    for p in (0.0, 0.001, 0.002, 0.1, 0.25, 0.5, 0.9, 0.997):
        assert dropout.threshold(p) == ref.threshold(p) and dropout.effective_p(p) == ref.threshold(p) / 256.0
    assert dropout.effective_p(0.1) == 26 / 256
    for p in (1.0, -0.1, 0.999, float("nan")):
        with pytest.raises(ValueError):
            dropout.threshold(p)
    assert ref.scale(26) == np.float32(256.0 / 230.0) and ref.scale(128) == 2.0


@pytest.mark.parametrize("T", [1, 26, 128, 255])
def test_drop_rate_over_a_million_bytes(T):
    """2^20 bytes of the hidden site: the drop count within 5 binomial sigmas of T / 256."""
    keep = ref.hidden_keep(256, 4096, T, SEED, SITE)
    n, q = keep.size, T / 256.0
    assert n == 2 ** 20
    assert abs(int((~keep).sum()) - n * q) <= 5 * np.sqrt(n * q * (1 - q)), (T, int((~keep).sum()), n * q)


def test_other_sites_and_seeds_give_other_masks():
    """Two independent masks of rate q differ on a fraction 2 q (1 - q) of the elements: within 5 sigmas, for both sites."""
    T = 26
    q = T / 256.0
    f = 2 * q * (1 - q)
    i, j = np.arange(512)[:, None], np.arange(512)[None, :]
    for a, b in ((ref.hidden_keep(512, 512, T, SEED, SITE), ref.hidden_keep(512, 512, T, SEED, SITE + 1)),
                 (ref.hidden_keep(512, 512, T, SEED, SITE), ref.hidden_keep(512, 512, T, SEED + 1, SITE)),
                 (ref.hidden_keep(512, 512, T, SEED, SITE), ref.hidden_keep(512, 512, T, SEED ^ (1 << 63), SITE)),
                 (ref.attn_keep(i, j, 3, T, SEED, SITE), ref.attn_keep(i, j, 3, T, SEED, SITE + 1)),
                 (ref.attn_keep(i, j, 3, T, SEED, SITE), ref.attn_keep(i, j, 3, T, SEED + 1, SITE)),
                 (ref.attn_keep(i, j, 3, T, SEED, SITE), ref.attn_keep(i, j, 4, T, SEED, SITE))):
        n = a.size
        assert abs(int((a != b).sum()) - n * f) <= 5 * np.sqrt(n * f * (1 - f))


def test_site_mappings_are_the_documented_bytes():
    T = 128
    keep = ref.hidden_keep(5, 64, T, SEED, SITE)
    for row, col in ((0, 0), (4, 63), (2, 17), (3, 48)):
        assert keep[row, col] == (ref.call_bytes(SEED, col >> 4, row, 0, SITE)[col & 15] >= T)
    for i, j, bh in ((0, 0, 0), (5, 130, 3), (511, 510, 65535 * 16 + 15), (7, 2, 1)):
        assert bool(ref.attn_keep(i, j, bh, T, SEED, SITE)) == (ref.call_bytes(SEED, i >> 2, j >> 2, bh, SITE)[4 * (i & 3) + (j & 3)] >= T)
    cu = np.array([0, 9, 9, 14])
    ms = ref.attn_masks(cu, 2, 0, T, SEED, SITE)
    assert ms[1] is None and ms[0].shape == (2, 9, 9) and ms[2].shape == (2, 5, 5)
    assert set(np.unique(ms[2])) <= {0.0, 2.0}
    assert (ms[2][1, 3, 4] != 0) == bool(ref.attn_keep(3, 4, 2 * 2 + 1, T, SEED, SITE))
    m3 = ref.attn_masks(cu, 2, 3, T, SEED, SITE)
    assert np.array_equal(m3[2][:, 0], ms[2][:, 0])  # mode 3 is the same function at i = 0


@pytest.mark.parametrize("mode", [0, 3])
def test_model_against_autograd(mode):
    """The fp64 model equals torch.autograd in float64 on softmax(Q K^T / 8) * mask @ V."""
    heads, lens = 2, [1, 5, 17, 66]
    qkv, cu = ao.realistic(lens, heads, 3, 1.0)
    dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 4)
    masks = ref.attn_masks(cu, heads, mode, 26, SEED, SITE)
    ctx, dqkv = ref.model(qkv, dctx, cu, heads, mode, masks)
    hidden = 64 * heads
    for b, n in enumerate(lens):
        rows = torch.from_numpy(qkv[int(cu[b]):int(cu[b + 1])].astype(np.float64)).requires_grad_(True)
        Q, K, V = (rows[:, i * hidden:(i + 1) * hidden].reshape(n, heads, 64).transpose(0, 1) for i in range(3))
        if mode == 3:
            Q = Q[:, :1]
        P = torch.softmax(Q @ K.transpose(1, 2) / 8.0, dim=2) * torch.from_numpy(masks[b])
        out = (P @ V).transpose(0, 1).reshape(-1, hidden)
        g = torch.from_numpy((dctx[b:b + 1] if mode == 3 else dctx[int(cu[b]):int(cu[b + 1])]).astype(np.float64))
        out.backward(g)
        want_ctx = ctx[b:b + 1] if mode == 3 else ctx[int(cu[b]):int(cu[b + 1])]
        assert np.allclose(out.detach().numpy(), want_ctx, rtol=1e-12, atol=1e-13)
        assert np.allclose(rows.grad.numpy(), dqkv[int(cu[b]):int(cu[b + 1])], rtol=1e-11, atol=1e-12)


CASES = [(mode, family, scale, p) for mode in (0, 3) for family in ("realistic1", "spike16") for scale in (1.0, 256.0) for p in (0.1, 0.5)]


def _case(mode, family, scale, heads=2):
    qkv, cu = ao.FAMILIES[family](ref.LENS_BOUND, heads, 11)
    dctx = agr.dctx_grid(len(ref.LENS_BOUND) if mode == 3 else int(cu[-1]), 64 * heads, 2, scale)
    return qkv, dctx, cu, heads


def _worst(got, want):
    return max(fp.worst_ratio(got[0], want[0], want[1])[0], fp.worst_ratio(got[1], want[2], want[3])[0])


@pytest.mark.parametrize("mode,family,scale,p", CASES)
def test_emulation_inside_the_bound_at_the_gpu_tests_lengths(mode, family, scale, p):
    qkv, dctx, cu, heads = _case(mode, family, scale)
    T = ref.threshold(p)
    want = ref.reference_and_bound(qkv, dctx, cu, heads, mode, ref.attn_masks(cu, heads, mode, T, SEED, SITE))
    worst = _worst(ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE), want)
    print(f"RATIO emulation mode={mode} {family} scale={scale} p={p}: {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("mode,mutation", [(mode, mu) for mode in (0, 3) for mu in ref.MUTATIONS
                                           if mu not in ref.GEOMETRY_MUTATIONS and (mode == 3 or mu != "cls_row1")])
def test_every_mutation_leaves_the_bound(mode, mutation):
    for p in (0.1, 0.5):
        qkv, dctx, cu, heads = _case(mode, "realistic1", 1.0)
        T = ref.threshold(p)
        want = ref.reference_and_bound(qkv, dctx, cu, heads, mode, ref.attn_masks(cu, heads, mode, T, SEED, SITE))
        worst = _worst(ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE, mutation), want)
        assert worst > 1.0, (mutation, mode, p, worst)


# ---- the block-wise mask builder -------------------------------------------------------------------------------------------------------------
def _masks_per_element(cu, heads, mode, T, mutation=None):
    """attn_masks as attn_keep states it: one generator call per (query, key) element."""
    out = []
    for b in range(len(cu) - 1):
        n = int(cu[b + 1] - cu[b])
        if n == 0:
            out.append(None)
            continue
        qi = np.arange(1 if mode == 3 else n)[:, None] + (1 if (mode == 3 and mutation == "cls_row1") else 0)
        kj = np.arange(n)[None, :]
        ms = []
        for h in range(heads):
            bh = b * 2 + h if mutation == "bh_stride_2" else b * heads + h + {"mask_next_head": 1, "mask_next_sequence": heads}.get(mutation, 0)
            keep = (ref.attn_keep(kj, qi, bh, T, SEED, SITE) if mutation == "mask_transposed" else
                    ref.attn_keep(qi, kj, bh, T, SEED, SITE, mutation == "byte_swapped"))
            ms.append(keep.astype(np.float64) * float(ref.scale(T)))
        out.append(np.stack(ms))
    return out


@pytest.mark.parametrize("mutation", (None,) + ref.MASK_MUTATIONS)
@pytest.mark.parametrize("mode", [0, 3])
def test_block_wise_masks_are_the_per_element_mapping(mode, mutation):
    """attn_masks makes one generator call per 4 x 4 block; attn_keep one per element. Equal for every length of the mask read-out (a sequence of
    length 0 between them), three heads (so that bh_stride_2 is not the identity), both thresholds, and under every mask-side mutation."""
    heads = 3
    lens = ref.LENS_READOUT[:4] + [0] + ref.LENS_READOUT[4:]
    cu = np.concatenate([[0], np.cumsum(lens)])
    for T in (26, 128):
        got, want = ref.attn_masks(cu, heads, mode, T, SEED, SITE, mutation), _masks_per_element(cu, heads, mode, T, mutation)
        assert len(got) == len(want) == len(lens)
        for b, n in enumerate(lens):
            if n == 0:
                assert got[b] is None and want[b] is None
                continue
            assert got[b].dtype == want[b].dtype and got[b].shape == want[b].shape == (heads, 1 if mode == 3 else n, n)
            assert np.array_equal(got[b], want[b]), (b, n, np.argwhere(got[b] != want[b])[0])
    if mutation is not None and not (mode == 0 and mutation == "cls_row1"):
        plain = ref.attn_masks(cu, heads, mode, 128, SEED, SITE)
        assert any(not np.array_equal(a, b) for a, b in zip(got, plain) if a is not None), "the mutation left every mask as it was"
    assert set(ref.MASK_MUTATIONS) <= set(ref.MUTATIONS)


# ---- the one-hot family under p = 0.5 --------------------------------------------------------------------------------------------------------
def _onehot_case(lens, heads, mode):
    qkv, cu, expected = ao.onehot(lens, heads, 3)
    dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 4)
    return qkv, cu, expected, dctx


def _onehot_mismatches(got, want):
    """(ctx elements whose bits differ, dV elements that differ): ctx bit for bit; dV bit for bit in mode 0 -- a sum from +0 -- and, as single
    products in mode 3, with -0 counted as +0 (`want` carries +0)"""
    (ctx, dqkv), (ctx_w, dV_w, mode) = got, want
    dV = dqkv[:, 2 * ctx_w.shape[1]:]
    if mode == 3:
        dV = dV + np.float16(0)
    return int((fp.bits(ctx) != fp.bits(ctx_w)).sum()), int((fp.bits(dV) != fp.bits(dV_w)).sum())


@pytest.mark.parametrize("mode", [0, 3])
def test_onehot_emulation_gives_the_bit_known_pattern(mode):
    """With p a permutation matrix and T = 128 the emulated kernels return ctx[i] = 2 V[pi(i)] and dV[pi(i)] = 2 dO[i] where (i, pi(i)) is kept and
    zero where it is not, bit for bit, at the lengths of the bound tests and two heads (what tests/test_dropout_gpu.py asks of the device at 1, 12
    and 16 heads). Mode 3 forms p = e * inv and p * m as two products: e = 1, inv = 1 and m = 2 for the winner, so the pattern holds there too;
    its dV rows are single products, whose zero takes the operands' signs: zero by value."""
    heads, lens = 2, ref.LENS_BOUND
    qkv, cu, expected, dctx = _onehot_case(lens, heads, mode)
    keep = [m != 0 for m in ref.attn_masks(cu, heads, mode, 128, SEED, SITE)]
    ctx_w, dV_w, kept, pairs = ref.onehot_pattern(expected, dctx, cu, heads, mode, keep)
    assert 0 < kept < pairs and pairs == heads * (len(lens) if mode == 3 else int(cu[-1]))
    assert (ctx_w != 0).any() and (dV_w != 0).any()
    assert _onehot_mismatches(ref.emulate(qkv, dctx, cu, heads, mode, 128, SEED, SITE), (ctx_w, dV_w, mode)) == (0, 0)
    # the pattern is the mask's: another site's mask does not fit it
    other = ref.emulate(qkv, dctx, cu, heads, mode, 128, SEED, SITE + 1)
    assert min(_onehot_mismatches(other, (ctx_w, dV_w, mode))) > 0


# ---- the defects that only the training geometry shows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 3])
def test_a_head_stride_of_two_is_invisible_at_two_heads_and_caught_at_twelve(mode):
    """bh_stride_2 (the counter's third word b * 2 + h): at two heads it IS the correct mask, so every case of two heads passes with it -- shown
    on the old bound case's inputs. At twelve heads on a short ragged batch it leaves the derived bound and breaks the one-hot pattern."""
    for p in (0.1, 0.5):
        qkv, dctx, cu, heads = _case(mode, "realistic1", 1.0)
        T = ref.threshold(p)
        for a, b in zip(ref.attn_masks(cu, heads, mode, T, SEED, SITE), ref.attn_masks(cu, heads, mode, T, SEED, SITE, "bh_stride_2")):
            assert np.array_equal(a, b)
        got, plain = ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE, "bh_stride_2"), ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE)
        assert fp.same_bits(got[0], plain[0]) and fp.same_bits(got[1], plain[1])
    heads, lens = 12, [65, 130, 300]
    for p in (0.1, 0.5):
        T = ref.threshold(p)
        qkv, cu = ao.FAMILIES["realistic1"](lens, heads, 11)
        dctx = agr.dctx_grid(len(lens) if mode == 3 else int(cu[-1]), 64 * heads, 2)
        want = ref.reference_and_bound(qkv, dctx, cu, heads, mode, ref.attn_masks(cu, heads, mode, T, SEED, SITE))
        assert _worst(ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE), want) <= 1.0
        worst = _worst(ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE, "bh_stride_2"), want)
        assert worst > 1.0, (mode, p, worst)
    qkv, cu, expected, dctx = _onehot_case(lens, heads, mode)
    keep = [m != 0 for m in ref.attn_masks(cu, heads, mode, 128, SEED, SITE)]
    ctx_w, dV_w, _, _ = ref.onehot_pattern(expected, dctx, cu, heads, mode, keep)
    assert _onehot_mismatches(ref.emulate(qkv, dctx, cu, heads, mode, 128, SEED, SITE), (ctx_w, dV_w, mode)) == (0, 0)
    assert min(_onehot_mismatches(ref.emulate(qkv, dctx, cu, heads, mode, 128, SEED, SITE, "bh_stride_2"), (ctx_w, dV_w, mode))) > 0


def test_a_forward_sum_without_the_rescale_leaves_the_bound_under_a_rising_maximum():
    """fwd_no_rescale (the forward's l_run + csum without alpha): under stair_up the maximum rises by 16 in every chunk of 64 keys, so over five
    and eight chunks lse is too large by about log(chunks) and ctx too small by that factor; the backward keeps its own sweep 0, so dqkv keeps
    its bits. Mode 3 has no running sum: the mutation changes nothing there.

    Do the old LENS_BOUND inputs (two heads, at most three chunks, realistic1 and spike16) catch it too? Computed below, not assumed: YES, both
    do (ctx lands 473 and 782 bounds away: the lengths 65 and 130 have rows whose maximum sits in a later chunk). So a value comparison of two or
    three chunks already sees this defect; what the longer cases add is the rescale chained over five to eight chunks, which the mutant misses
    by 353 bounds here."""
    heads, lens, mode, T = 2, [300, 512], 0, 26
    qkv, cu = ao.FAMILIES["stair_up"](lens, heads, 11)
    dctx = agr.dctx_grid(int(cu[-1]), 64 * heads, 2)
    want = ref.reference_and_bound(qkv, dctx, cu, heads, mode, ref.attn_masks(cu, heads, mode, T, SEED, SITE))
    plain = ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE)
    got = ref.emulate(qkv, dctx, cu, heads, mode, T, SEED, SITE, "fwd_no_rescale")
    assert _worst(plain, want) <= 1.0
    ctx_ratio = fp.worst_ratio(got[0], want[0], want[1])[0]
    print(f"RATIO fwd_no_rescale stair_up lens={lens}: ctx {ctx_ratio:.1f}")
    assert ctx_ratio > 1.0 and fp.same_bits(got[1], plain[1])
    for b, n in enumerate(lens):   # every sequence of five or more chunks by itself
        rows = slice(int(cu[b]), int(cu[b + 1]))
        assert n > 4 * ref.CHUNK and fp.worst_ratio(got[0][rows], want[0][rows], want[1][rows])[0] > 1.0
    caught = {}
    for family in ("realistic1", "spike16"):
        qkv, dctx, cu, heads = _case(0, family, 1.0)
        want = ref.reference_and_bound(qkv, dctx, cu, heads, 0, ref.attn_masks(cu, heads, 0, T, SEED, SITE))
        got = ref.emulate(qkv, dctx, cu, heads, 0, T, SEED, SITE, "fwd_no_rescale")
        caught[family] = fp.worst_ratio(got[0], want[0], want[1])[0]
        print(f"RATIO fwd_no_rescale LENS_BOUND {family}: ctx {caught[family]:.1f}")
    assert caught["realistic1"] > 1.0 and caught["spike16"] > 1.0, caught
    qkv, dctx, cu, heads = _case(3, "realistic1", 1.0)
    a, b = ref.emulate(qkv, dctx, cu, heads, 3, T, SEED, SITE), ref.emulate(qkv, dctx, cu, heads, 3, T, SEED, SITE, "fwd_no_rescale")
    assert fp.same_bits(a[0], b[0]) and fp.same_bits(a[1], b[1])


def test_header_binding_and_library_agree():
    """include/mdr_dropout.h declares exactly what dropout.SIGNATURES binds and the library exports, apart from include/mdr_hip.h's table and from
    every other header's; each signature has the prototype's number of arguments; dropout.lib() binds (what
    tests/test_capi_symbols.py::test_header_binding_and_library_agree asserts for the other headers)."""
    import importlib
    from multihop_dense_retrieval_amd import _lib, build, dropout
    import test_capi_symbols as capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdr_dropout.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mdr_[a-z0-9_]+)\s*\(", text)))
    expected = ["mdr_attention_dropout_backward", "mdr_attention_dropout_forward", "mdr_dropout_rows", "mdr_dropout_threshold", "mdr_test_dropout_bytes"]
    assert sorted(dropout.SIGNATURES) == declared == expected
    assert sorted(dropout.EXPORTED_SYMBOLS) == declared
    assert not set(dropout.SIGNATURES) & set(_lib.EXPORTED_SYMBOLS)
    for h, m, a, _ in capi.HEADER_TABLES:
        assert not set(dropout.SIGNATURES) & set(getattr(importlib.import_module("multihop_dense_retrieval_amd." + m), a)), h
    for name, (_, args) in dropout.SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1)
        assert len(args) == proto.count(",") + 1, name
    lib = ctypes.CDLL(build.build_lib())
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/mdr_dropout.h but not exported"
    dropout.lib()
    # the headers the existing tests pin kept their tables
    from multihop_dense_retrieval_amd import attention
    assert sorted(attention.SIGNATURES) == ["mdr_attention_backward", "mdr_attention_backward_workspace_bytes"]
    # the constants of the device header are the replica's
    dev = open(os.path.join(ROOT, "multihop_dense_retrieval_amd", "csrc", "mdr_dropout.h")).read()
    for c in (ref.M0, ref.M1, ref.W0, ref.W1):
        assert f"0x{c:08X}u" in dev


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import attention, dropout
    with pytest.raises(RuntimeError):
        dropout.packed_dropout(torch.zeros(4, 64), 0.1, 1, 2)
    with pytest.raises(RuntimeError):
        dropout.packed_dropout(torch.zeros(4, 64), 0.0, 1, 2)
    with pytest.raises(RuntimeError):
        attention.packed_self_attention(torch.zeros(4, 192, dtype=torch.float16), torch.tensor([0, 4], dtype=torch.int32), 1, 8, dropout=(0.1, 1, 2))
    with pytest.raises(ValueError):
        dropout.check_seed_site(2 ** 64, 0)
    with pytest.raises(ValueError):
        dropout.check_seed_site(0, 2 ** 32)
