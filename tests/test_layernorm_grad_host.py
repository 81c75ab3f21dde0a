"""CPU: the fp64 statement of the LayerNorm backward (tests/layernorm_grad_ref.py) against torch.autograd in float64, the emulation of the
kernel's dataflow against the derived bound, each mutation against the same bound, and the header / binding / split contract of
include/mdr_layernorm_grad.h. No device and no kernel runs here."""

import numpy as np
import pytest
import torch

import layernorm_grad_ref as ref
from oracle import fp
from oracle import trunk_rows_oracle as tr

OUTPUTS = ("dx", "dg", "db")


def _ratios(emu, rb):
    """the emulation's (dx16, dx32, dg, db) against reference_and_bound: dx16 by the monotonic fp16 rule (an assertion), the fp32 outputs as
    their largest share of the bound"""
    dx16, dx32, dg, db = emu
    tr.assert_f16(dx16, *rb["dx"], "dx16")
    return {k: fp.worst_ratio(got, *rb[k]) for k, got in zip(OUTPUTS, (dx32, dg, db))}


def _outside(emu, rb):
    """whether any output leaves the bound (dx16 by the monotonic rule)"""
    dx16, dx32, dg, db = emu
    if max(fp.worst_ratio(got, *rb[k])[0] for k, got in zip(OUTPUTS, (dx32, dg, db))) > 1.0:
        return True
    try:
        tr.assert_f16(dx16, *rb["dx"], "dx16")
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("combo", ref.COMBOS, ids=lambda c: "-".join(map(str, c)))
def test_fp64_statement_agrees_with_torch_autograd(combo):
    """F.layer_norm(in + res) in float64 with the two output gradients summed. Both sides are fp64 and differ only in the order of operations:
    |a - b| <= 1e-9 max|b| per output."""
    M, H = 37, 192
    case = ref.make_case("unit", combo, M, H, 1)
    g, b = case["g"].astype(np.float64), np.zeros(H)
    tin = torch.from_numpy(case["inp"].astype(np.float64)).requires_grad_(True)
    leaves = [tin]
    x = tin
    if case["res"] is not None:
        tres = torch.from_numpy(case["res"].astype(np.float64)).requires_grad_(True)
        leaves.append(tres)
        x = tin + tres
    tg, tb = torch.from_numpy(g).requires_grad_(True), torch.from_numpy(b).requires_grad_(True)
    y = torch.nn.functional.layer_norm(x, (H,), tg, tb, ref.EPS)
    outs, grads = [], []
    for part in (case["dy16"], case["dy2"]):  # the output is used twice: autograd sums the two gradients
        if part is not None:
            outs.append(y * 1.0)
            grads.append(torch.from_numpy(part.astype(np.float64)))
    want = torch.autograd.grad(outs, leaves + [tg, tb], grads)
    rb = ref.reference_and_bound(**case)
    for w in want[:len(leaves)]:  # dx is the gradient of `in` and of the residual alike
        assert np.abs(rb["dx"][0] - w.numpy()).max() <= 1e-9 * np.abs(w.numpy()).max()
    for k, w in zip(("dg", "db"), want[len(leaves):]):
        assert np.abs(rb[k][0] - w.numpy()).max() <= 1e-9 * np.abs(w.numpy()).max(), k


def test_stats_restate_the_forward_derivation():
    """stats() returns the intermediate terms of oracle/trunk_rows_oracle.py's bound: at g = 1, b = 0 they give that bound itself."""
    for family in ref.FAMILIES:
        case = ref.make_case(family, ref.TRUNK_COMBOS[0], 9, 192, 3)
        x, ex = tr.ln_inputs(case["inp"], case["res"])
        st = ref.stats(x, ex, ref.EPS)
        t, Et = np.abs(st["t"]), st["Et"]
        mine = (Et + fp.U32 * (t + Et) + fp.U32 * (t + Et)) * (1 + 2.0 ** -10)
        theirs = tr.bound(x, ex, np.ones(192), np.zeros(192), ref.EPS)
        assert np.allclose(mine, theirs, rtol=1e-12, atol=0), family
        assert np.allclose(st["t"], tr.layer_norm(x, np.ones(192), np.zeros(192), ref.EPS), rtol=1e-12, atol=1e-300), family


def _scales(family):
    return (1.0, 256.0) if ref.FAMILIES[family] else (1.0,)


@pytest.mark.parametrize("family", list(ref.FAMILIES))
@pytest.mark.parametrize("H", ref.HS)
def test_emulation_stays_inside_the_bound(H, family):
    """A second implementation of the listed dataflow, on every family and every shape the GPU tests use, every operand combination, unit and
    loss scale, with and without a valid-row count and old values."""
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for M in ref.M_SWEEP + (ref.split_ms(H) if H == 64 else []):
        for combo in (ref.COMBOS if M in (5, 300) else ref.TRUNK_COMBOS):
            for scale in _scales(family):
                case = ref.make_case(family, combo, M, H, 11, scale)
                old_dg, old_db = fp.grid((H,), 12, 4.0), fp.grid((H,), 13, 4.0)
                for m, odg, odb in ((None, None, None), (max(M - 1, 0), old_dg, old_db)):
                    rb = ref.reference_and_bound(**case, m=m, old_dg=odg, old_db=odb)
                    for k, (w, at) in _ratios(ref.emulate(**case, m=m, old_dg=odg, old_db=odb), rb).items():
                        assert w <= 1.0, (M, H, family, combo, scale, m, k, w, at)
                        worst[k] = max(worst[k], w)
    print(f"RATIO emulation H={H} {family}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("family", list(ref.FAMILIES))
@pytest.mark.parametrize("H,M", ref.LARGE_HM, ids=lambda v: str(v))
def test_emulation_stays_inside_the_bound_at_training_row_counts(H, M, family):
    """The same at LARGE_HM, where a wave walks three rows and the strands add hundreds of chunks: the three trunk combinations, one of them
    with a valid-row count in the middle and old values; the unit family under the loss scale, as in training. One fp64 reference per
    combination keeps a case at a few seconds."""
    worst = dict.fromkeys(OUTPUTS, 0.0)
    old_dg, old_db = fp.grid((H,), 12, 4.0), fp.grid((H,), 13, 4.0)
    for combo, (m, odg, odb) in zip(ref.TRUNK_COMBOS, ((None, None, None), (None, None, None), (ref.large_ms(M, H)[1], old_dg, old_db))):
        case = ref.make_case(family, combo, M, H, 11, 256.0 if family == "unit" else 1.0)
        rb = ref.reference_and_bound(**case, m=m, old_dg=odg, old_db=odb)
        for k, (w, at) in _ratios(ref.emulate(**case, m=m, old_dg=odg, old_db=odb), rb).items():
            assert w <= 1.0, (M, H, family, combo, m, k, w, at)
            worst[k] = max(worst[k], w)
    print(f"RATIO emulation H={H} M={M} {family}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("mutation", ref.MUTATIONS)
def test_each_mutation_leaves_the_bound(mutation):
    """The bound is worth something: every formula, operand, row-count, chunk and accumulate defect is thrown out."""
    M, H = 23, 192
    S, rpc = ref.chunks(M, H)
    assert S > 1
    family = "const" if mutation == "no_eps" else "unit"
    case = ref.make_case(family, ref.TRUNK_COMBOS[0], M, H, 21)
    old_dg, old_db = fp.grid((H,), 22, 4.0), fp.grid((H,), 23, 4.0)
    m = M - 2
    rb = ref.reference_and_bound(**case, m=m, old_dg=old_dg, old_db=old_db)
    assert not _outside(ref.emulate(**case, m=m, old_dg=old_dg, old_db=old_db), rb)
    emu = ref.emulate(**case, m=m, old_dg=old_dg, old_db=old_db, mutation=mutation)
    r = {k: fp.worst_ratio(got, *rb[k])[0] for k, got in zip(OUTPUTS, emu[1:])}
    print(f"mutation {mutation}: worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0, mutation
    assert _outside(emu, rb)


def test_split_is_a_function_of_the_shape_and_workspace_covers_it():
    """mdr_layernorm_backward_chunks equals the helper's restatement, S > 1 on a tested shape, the workspace holds [S][2][H]."""
    from multihop_dense_retrieval_amd import layernorm
    lib = layernorm.lib()
    some_split = False
    for H in range(64, 1025, 64):
        for M in ref.M_SWEEP + ref.split_ms(64) + [38, 1023, 1024, 1025, 2048, 2731, 4096, 4097, 8608, 11400, 100000, 2 ** 22 + 5]:
            S, rpc = layernorm.backward_chunks(M, H)
            assert (S, rpc) == ref.chunks(M, H) and S >= 1 and rpc >= 4 and rpc % 4 == 0 and (S - 1) * rpc < M <= S * rpc, (M, H, S, rpc)
            assert S * 2 * H * 4 <= ref.MAX_PARTIAL_BYTES
            some_split |= S > 1
            for want in (1, 2, 3):
                assert lib.mdr_layernorm_backward_workspace_bytes(M, H, want) == (0 if S == 1 else (S * 2 * H * 4 + 255) // 256 * 256)
            assert lib.mdr_layernorm_backward_workspace_bytes(M, H, 0) == 0
    assert some_split
    for M in ref.split_ms(64):
        S, rpc = ref.chunks(M, 64)
        assert S >= 3 and rpc >= 8 and M % rpc
    assert ref.assert_large(chunks_of=layernorm.backward_chunks) == ref.assert_large()  # the large shapes keep their properties under the LIBRARY's split
    for M, H in ((0, 64), (-1, 64), (5, 0), (5, 32), (5, 96), (5, 1088), (5, -64)):
        assert lib.mdr_layernorm_backward_workspace_bytes(M, H, 3) == 0
        assert layernorm.backward_chunks(M, H) == (0, 0) == ref.chunks(M, H)


def test_module_fails_loudly_without_a_device():
    from multihop_dense_retrieval_amd import layernorm
    x, w, b = torch.zeros(4, 64), torch.ones(64), torch.zeros(64)
    with pytest.raises(RuntimeError):
        layernorm.packed_layer_norm(x, None, w, b)
    with pytest.raises(RuntimeError):
        layernorm.layer_norm_backward(x, None, torch.zeros(4, 64, dtype=torch.float16), None, w)
    with pytest.raises(RuntimeError):
        layernorm.gather_cls_backward(torch.zeros(2, 64, dtype=torch.float16), torch.zeros(3, dtype=torch.int32), torch.zeros(5, 64, dtype=torch.float16))
