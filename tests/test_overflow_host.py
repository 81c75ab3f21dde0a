"""Host: tests/overflow_ref.py -- the classification on hand-made arrays, the loss scaler's ladder, and, ON THE REFERENCES ALONE, that the inputs
which tests/test_overflow_gpu.py and tests/test_overflow_chain_gpu.py put on the device meet the caps: per output at most 2 % of the live
elements left out, the finite and the Inf class at least 5 % each, an overflowed dZ for the GELU Linear, an overflowed dS16 for the attention
(modes 0 and 3) and an overflowed g for the O1 loss; and a ladder on which ten steps from
4 x the first must-overflow scale hold at least 2 skipped steps, 3 clean steps and a doubling, whatever the undecided scales turn out to do."""
import numpy as np
import pytest

import encoder_chain_ref as ch
import overflow_ref as ov
from oracle import fp

E = fp.F16_EDGE


def test_classify_on_hand_made_arrays():
    r = np.array([0.0, 100.0, -65000.0, 65519.0, 65519.5, 65520.0, 65521.0, -65521.0, -70000.0, 1e9])
    b = np.array([0.0, 1.0, 100.0, 0.5, 0.5, 0.0, 1.0, 2.0, 4000.0, 0.0])
    #             fin  fin   fin     fin     out(=E)  inf     inf(=E) out      inf       inf
    want = [ov.FINITE, ov.FINITE, ov.FINITE, ov.FINITE, ov.LEFT_OUT, ov.INF, ov.INF, ov.LEFT_OUT, ov.INF, ov.INF]
    assert ov.classify(r, b).tolist() == want
    # 65520 itself: the tie rounds to even, which is out of range
    with np.errstate(over="ignore"):
        assert np.isinf(np.float16(np.float32(65520.0))) and np.isfinite(np.float16(np.float32(65519.99)))
        assert np.isinf(np.float64(65520.0).astype(np.float16)) and np.float64(65519.9).astype(np.float16) == np.float16(65504.0)
    r2, b2 = np.array([[1.0, 70000.0], [2.0, 80000.0], [3.0, -90000.0]]), np.zeros((3, 2))
    cls = ov.classify(r2, b2, poisoned=np.array([[False], [True], [False]]), doubtful=np.array([[False], [False], [True]]))
    assert cls.tolist() == [[ov.FINITE, ov.INF], [ov.POISON, ov.POISON], [ov.LEFT_OUT, ov.LEFT_OUT]]
    with pytest.raises(AssertionError):
        ov.classify(np.array([np.inf]), np.array([0.0]))


def test_verdicts_accept_and_reject():
    r = np.array([10.0, 70000.0, -70000.0, 5.0, 7.0])
    b = np.array([1.0, 10.0, 10.0, 0.0, 0.0])
    cls = np.array([ov.FINITE, ov.INF, ov.INF, ov.POISON, ov.LEFT_OUT], np.int8)
    good = np.array([10.5, np.inf, -np.inf, np.nan, 12345.0], np.float16)
    assert ov.verdicts(good, r, b, cls) == []
    assert ov.verdicts(np.array([10.5, np.inf, -np.inf, -np.inf, np.nan], np.float16), r, b, cls) == []
    # a bound on the value in front of the last rounding: the fp16 neighbours of r -+ b are the limits
    r3, b3 = np.array([-46509.98, 1000.3]), np.array([0.07, 0.3])
    c3 = np.array([ov.FINITE, ov.FINITE], np.int8)
    assert ov.verdicts(np.array([-46496.0, 1000.0], np.float16), r3, b3, c3, final_rounding_in_b=False) == []
    assert ov.verdicts(np.array([-46496.0, 1000.5], np.float16), r3, b3, c3, final_rounding_in_b=False) == []
    assert len(ov.verdicts(np.array([-46528.0, 1000.0], np.float16), r3, b3, c3, final_rounding_in_b=False)) == 1
    assert len(ov.verdicts(np.array([-46496.0, 1001.0], np.float16), r3, b3, c3, final_rounding_in_b=False)) == 1
    assert len(ov.verdicts(np.array([-46496.0, 1000.0], np.float16), r3, b3, c3)) == 1
    for i, v, word in ((0, 12.0, "finite"), (0, np.inf, "finite"), (0, np.nan, "finite"), (1, 65504.0, "inf"), (1, -np.inf, "inf"), (1, np.nan, "inf"),
                       (2, np.inf, "inf"), (2, -65504.0, "inf"), (3, 5.0, "poison"), (3, 65504.0, "poison")):
        bad = good.copy()
        bad[i] = v
        out = ov.verdicts(bad, r, b, cls)
        assert len(out) == 1 and f"class {word}" in out[0], (i, v, out)


def test_caps_helper():
    cls = np.array([ov.FINITE] * 90 + [ov.INF] * 8 + [ov.LEFT_OUT] * 2, np.int8)
    assert ov.cap_failures(cls) == [] and len(ov.cap_failures(cls, need_poison=True)) == 1
    assert len(ov.cap_failures(np.array([ov.FINITE] * 96 + [ov.INF] * 4, np.int8))) == 1
    assert len(ov.cap_failures(np.array([ov.FINITE] * 50 + [ov.INF] * 47 + [ov.LEFT_OUT] * 3, np.int8))) == 1


@pytest.mark.parametrize("M,rows,N,K,gelu", ov.LINEAR_CASES)
def test_linear_case_meets_the_caps(M, rows, N, K, gelu):
    c = ov.linear_case(M, rows, N, K, gelu)
    print(f"CAPS linear M={M} N={N} K={K} gelu={gelu} s_dy={c['s_dy']:g} s_w={c['s_w']:g} {ov.shares(c['cls'])}")
    assert ov.cap_failures(c["cls"], need_poison=gelu) == []
    assert c["cls"].shape == (rows, K) and np.isfinite(c["dy"]).all() and np.isfinite(c["w"]).all()
    if gelu:  # the poisoned rows are those whose dZ certainly overflows, and the dZ reference says which columns
        dz, edz = c["ref"]["dz"]
        over = np.abs(dz) - edz >= E
        assert over.any() and np.array_equal(over.any(axis=1), c["poisoned"][:, 0])
        assert (np.abs(c["dy"][:rows].astype(np.float64)) <= fp.F16_MAX).all()   # dy itself stays inside: the overflow is dZ's own


@pytest.mark.parametrize("form", list(ov.LN_FORMS))
@pytest.mark.parametrize("M,rows,H", ov.LN_SHAPES)
def test_layernorm_case_meets_the_caps(M, rows, H, form):
    c = ov.layernorm_case(M, rows, H, form)
    print(f"CAPS layernorm M={M} H={H} {form} s={c['s']:g} {ov.shares(c['cls'])}")
    assert ov.cap_failures(c["cls"]) == [] and c["cls"].shape == (rows, H)
    # the parameter gradients stay far inside fp32: the overflow is dx16's alone
    assert all(np.abs(c["ref"][k][0]).max() < 1e30 for k in ("dg", "db"))


@pytest.mark.parametrize("mode", [0, 3])
def test_attention_case_meets_the_caps(mode):
    """dQ | dK | dV as one output; a dS16 that certainly overflows exists (the POISON class), the fp16 p operand cannot; and the host emulation of
    the kernels' dataflow (attention_grad_ref.emulate, a second implementation) is what its classes say"""
    import attention_grad_ref as aref
    c = ov.attention_case(mode)
    hidden = 64 * c["heads"]
    live, cls = c["live"], c["cls"]
    parts = {n: ov.shares(cls[:, i * hidden:(i + 1) * hidden][live[:, i * hidden:(i + 1) * hidden]]) for i, n in enumerate(("dQ", "dK", "dV"))}
    print(f"CAPS attention mode={mode} (a, v, e)={ov.ATTN_POWERS[mode]} {ov.shares(cls[live])} parts {parts}")
    assert ov.cap_failures(cls[live], need_poison=True) == []
    assert c["poisoned"].any() and not c["poisoned"][:, 2 * hidden:].any() and (cls[~live] == ov.FINITE).all()
    assert np.isfinite(c["dctx"]).all() and np.isfinite(c["qkv"]).all()
    if mode == 3:  # p <= 1: no dV element can leave fp16
        assert np.abs(c["ref"][0][:, 2 * hidden:]).max() <= np.abs(c["dctx"].astype(np.float64)).max() <= fp.F16_MAX
    with np.errstate(all="ignore"):
        emu = aref.emulate(c["qkv"], c["dctx"], c["cu"], c["heads"], mode)
    assert ov.verdicts(emu, *c["ref"], cls, "emulation") == []
    # and a saturating store is thrown out
    sat = np.where(np.isinf(emu), np.copysign(np.float16(65504.0), emu), emu)
    assert any("class inf" in f for f in ov.verdicts(sat, *c["ref"], cls))


def test_loss_case_meets_the_caps():
    """the six O1 gradients as one output, classified from what mhop_loss_ref hands its fp16 rounding points; the O1 regime itself (the helper's
    own evaluation, one valid order of summation) is what its classes say"""
    import mhop_loss_ref
    c = ov.loss_case()
    every = np.concatenate([c["cls"][k].ravel() for k in mhop_loss_ref.KEYS])
    print(f"CAPS loss shape={ov.LOSS_SHAPE} a={ov.LOSS_A} g0={c['g0']:g} {ov.shares(every)} " + str({k: ov.shares(c["cls"][k]) for k in c["cls"]}))
    assert ov.cap_failures(every, need_poison=True) == []
    regime = mhop_loss_ref.loss_and_grads(c["inp"], c["queue"], g0=c["g0"], o1=True)["grads"]
    for k in mhop_loss_ref.KEYS:
        assert ov.verdicts(regime[k], *c["ref"][k], c["cls"][k], k) == []
    # hand-made: one overflowing term makes Inf of its sign, two of opposite signs NaN -- what the classes rest on
    with np.errstate(invalid="ignore", over="ignore"):
        f = lambda x: np.float32(np.float16(np.float32(x)))  # noqa: E731
        assert f(70000.0) + f(-3.0) == np.inf and f(-70000.0) + f(65000.0) == -np.inf and np.isnan(f(70000.0) + f(-70000.0))


def test_the_ladder():
    for G1 in (0.393, 1.0, 0.5, 0.49999, 3.0e-5, 7.7):
        safe, must, between = ov.ladder(G1)
        assert safe * G1 <= fp.F16_MAX / 2 < 2 * safe * G1 and must * G1 >= 2 * E > must / 2 * G1
        assert must / safe in (4.0, 8.0) and len(between) == (1 if must / safe == 4.0 else 2)
    assert ov.scale_class(2.0 ** 14, 1.0) == ov.SAFE and ov.scale_class(2.0 ** 15, 1.0) == ov.UNDECIDED and ov.scale_class(2.0 ** 16, 1.0) == ov.UNDECIDED
    assert ov.scale_class(2.0 ** 17, 1.0) == ov.MUST


def test_the_recorder_sees_every_gradient_rounding_point_and_nothing_outside_the_block():
    assert ch.GRAD_PEAKS is None
    G1, peaks = ov.chain_g1()
    assert ch.GRAD_PEAKS is None
    nl = ch.GEOM["layers"]
    for want in ["emb.y16", "loss:g", "loss:operand", "project.0:x", "project.0:y"] + [f"encoder.encoder.layer.{i}.attention:dS" for i in range(nl)] + \
            [f"encoder.encoder.layer.{i}.intermediate.dense:dZ" for i in range(nl)] + [f"encoder.encoder.layer.{i}.attention:ctx" for i in range(nl)]:
        assert want in peaks and peaks[want] > 0, want
    assert "?" not in peaks and G1 == max(peaks.values()) and 0 < G1 < 65504
    # recording changes nothing: the gradients are those of an unrecorded run
    a = ch.grads_loss("regime", ch.state_dict(), ch.GEOM, ov.chain_batches())
    with ch.record_grad_peaks():
        b = ch.grads_loss("regime", ch.state_dict(), ch.GEOM, ov.chain_batches())
    assert a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])


def test_the_chain_run_holds_its_events_whatever_the_undecided_scales_do():
    G1, peaks = ov.chain_g1()
    safe, must, between = ov.ladder(G1)
    print(f"LADDER G1={G1:.6g} at {max(peaks, key=peaks.get)} last safe {safe:g} first must-overflow {must:g} undecided {between}")
    start = 4 * must
    choices = [lambda s: True, lambda s: False] + [lambda s, t=t: s >= t for t in between] + [lambda s, t=t: s < t for t in between]
    for pick in choices:
        ev, st = ov.simulate(G1, start, ov.CHAIN["steps"], ov.CHAIN["scale_window"], pick)
        skipped, clean, doublings, undecided = ov.run_summary(ev)
        assert skipped >= 2 and clean >= 3 and doublings >= 1 and undecided <= 2, ev
        assert ev[0][1] == ev[1][1] == ov.MUST and st["skipped_total"] == skipped and st["adam_step"] == clean
    # parts C: step 1 at a scale that must overflow, step 2 at a safe one
    assert ov.scale_class(must, G1) == ov.MUST and ov.scale_class(safe, G1) == ov.SAFE
    # the regime itself agrees with its own prediction: finite at the last safe scale, not at the first that must overflow
    assert must * G1 >= 2 * E and safe * G1 <= fp.F16_MAX / 2


def test_the_o1_loss_regime_at_b1_overflows_at_2_16_and_not_at_2_12():
    """the claim of tests/test_inbatch_grad_gpu.py's docstring, in the reference regime (the device's turn is tests/test_overflow_gpu.py)"""
    import mhop_loss_ref
    inp, _ = mhop_loss_ref.make_inputs(1, 32, 0, seed=7 + 32)
    hi = mhop_loss_ref.loss_and_grads(inp, None, g0=2.0 ** 16, o1=True)["grads"]
    lo = mhop_loss_ref.loss_and_grads(inp, None, g0=2.0 ** 12, o1=True)["grads"]
    assert any(not np.isfinite(hi[k]).all() for k in hi) and all(np.isfinite(lo[k]).all() for k in lo)
    # and not by a hair: some unrounded term is a factor 1.5 outside, every term at 2^12 a factor 4 inside
    peak = max(np.abs(v).max() for v in mhop_loss_ref.loss_and_grads(inp, None, g0=1.0, o1=False)["grads"].values())
    print(f"LOSS B=1: largest |gradient| at g0 = 1: {peak:.4f}")
    assert peak * 2.0 ** 16 >= 1.5 * E and peak * 2.0 ** 12 <= fp.F16_MAX / 4
