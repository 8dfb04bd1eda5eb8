"""GPU tests of ``KWhisperForConditionalGeneration.forward`` (the teacher's no-grad pass of a distillation step) and of
``kwhisper.distill.kd_loss`` on its logits, on the tiny fp32 and bf16 engines.

References: transformers' own forward on the same model (tests/golden/forward_tiny.npz, tools/make_forward_fixtures.py:
per-position top-8 logits, log-sum-exp, ``.loss`` and the float64 distillation loss) and, for whole [3][24][V] tensors,
the in-repo oracle, which tests/test_distill_cpu.py holds to that fixture within 1e-4 (measured 9.5e-6).

Bars: fp32 logits 1e-3 (the project's fp32 bar, test_tiny_fp32_logits); bf16 top-8 error max 0.25 / mean 0.03 (the
project's tiny bf16 bar, test_tiny_bf16_logits_and_tokens), for each of the bf16 engine's two many-row plans."""
import os

import numpy as np
import pytest
import torch

import _distill_ref as DR
from _util import oracle_features
from conftest import GOLD, gpu_available

from kwhisper.config import TINY, generation_constants
from kwhisper.synthetic import synthetic_state_dict

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

FP32_BAR = 1e-3
BF16_MAX, BF16_MEAN = 0.25, 0.03


def _model(cross_kv_dtype, dtype=torch.bfloat16):
    from kwhisper.generation import KWhisperForConditionalGeneration

    return KWhisperForConditionalGeneration.from_state_dict(
        TINY, synthetic_state_dict(TINY, 0), dtype=dtype, generation_config=generation_constants(TINY),
        cross_kv_dtype=cross_kv_dtype)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLD, "forward_tiny.npz")))


@pytest.fixture(scope="module")
def feats(fx):
    return torch.from_numpy(oracle_features(TINY, fx["cases"])).cuda()


@pytest.fixture(scope="module")
def oracle(fx):
    """The oracle's f32 logits [3][24][V] for the fixture's decoder ids and for the shifted labels; computed once."""
    from oracle.whisper_np import WhisperNP

    o = WhisperNP(synthetic_state_dict(TINY, 0), TINY)
    enc = o.encode(oracle_features(TINY, fx["cases"]))
    ids2 = DR.shift_right(fx["labels"], TINY.pad_token_id, TINY.decoder_start_token_id)
    return dict(ids=o.decode(fx["decoder_input_ids"], o.new_cache(enc)), shifted=o.decode(ids2, o.new_cache(enc)))


@pytest.fixture(scope="module")
def tiny32():
    return _model(None, torch.float32)


@pytest.fixture(scope="module")
def tiny16():
    return _model(None, torch.bfloat16)


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _top8(logits, fx):
    return np.take_along_axis(logits, fx["top_idx"].astype(np.int64), -1)


def _lse(logits):
    m = logits.max(-1, keepdims=True).astype(np.float64)
    return (m + np.log(np.exp(logits - m).sum(-1, keepdims=True)))[..., 0]


# --------------------------------------------------------------------------------------------------- 1. fp32
def test_fp32_logits_loss_and_shift(tiny32, fx, feats, oracle):
    with torch.enable_grad():  # no grad, whatever the mode around the call
        out = tiny32(input_features=feats, labels=_t(fx["labels"]), decoder_input_ids=_t(fx["decoder_input_ids"]))
    assert out.logits.dtype == torch.float32 and tuple(out.logits.shape) == (3, 24, TINY.vocab_size)
    assert out.logits.is_cuda and not out.logits.requires_grad and out.logits.grad_fn is None
    lg = out.logits.cpu().numpy()
    e_top, e_lse = np.abs(_top8(lg, fx) - fx["top_val"]).max(), np.abs(_lse(lg) - fx["lse"]).max()
    e_all = np.abs(lg - oracle["ids"]).max()
    print(f"fp32 forward: top-8 error {e_top:.3g}, log-sum-exp error {e_lse:.3g}, whole tensor vs the oracle {e_all:.3g}; "
          f"loss {float(out.loss):.7f} (HF {float(fx['loss']):.7f})")
    assert e_top <= FP32_BAR and e_lse <= FP32_BAR and e_all <= FP32_BAR
    assert abs(float(out.loss) - float(fx["loss"])) <= 1e-3
    # HF's tuple form and the encoder output
    assert out[0] is out.loss and out[1] is out.logits
    enc = out.encoder_last_hidden_state
    assert tuple(enc.shape) == (3, TINY.max_source_positions, TINY.d_model) and out[2] is enc
    # the labels alone: shift_tokens_right inside
    out2 = tiny32(input_features=feats, labels=_t(fx["labels"]))
    lg2 = out2.logits.cpu().numpy()
    assert np.abs(lg2 - oracle["shifted"]).max() <= FP32_BAR
    assert np.abs(np.sort(lg2, -1)[..., ::-1][..., :8] - fx["shift_top_val"]).max() <= FP32_BAR
    assert abs(float(out2.loss) - float(fx["shift_loss"])) <= 1e-3
    # without labels: no loss, out[0] is the logits
    out3 = tiny32(input_features=feats, decoder_input_ids=_t(fx["decoder_input_ids"]))
    assert out3.loss is None and out3[0] is out3.logits and torch.equal(out3.logits, out.logits)
    # an output is the caller's: a later forward does not write into it
    assert np.array_equal(out.logits.cpu().numpy(), lg)


# --------------------------------------------------------------------------------------------------- 2. bf16
@pytest.mark.parametrize("plan", ["wide", "chunk"])
def test_bf16_logits_both_plans(tiny16, fx, feats, plan):
    tiny16.forward_plan = plan
    try:
        out = tiny16(input_features=feats, labels=_t(fx["labels"]), decoder_input_ids=_t(fx["decoder_input_ids"]))
    finally:
        tiny16.forward_plan = None
    assert tiny16._fwd_sessions[3].forward_plan_last == plan
    assert out.logits.dtype == torch.float32 and tuple(out.logits.shape) == (3, 24, TINY.vocab_size)
    err = np.abs(_top8(out.logits.cpu().numpy(), fx) - fx["top_val"])
    print(f"bf16 forward, {plan} plan: top-8 error max {err.max():.4f} mean {err.mean():.4f}; "
          f"loss {float(out.loss):.5f} (HF {float(fx['loss']):.5f})")
    assert err.max() < BF16_MAX and err.mean() < BF16_MEAN
    assert bool(torch.isfinite(out.logits).all())


def test_bf16_default_plan_is_chosen_by_rows(tiny16, fx, feats):
    """The measured crossover (profiles/distill_forward.txt, large-v3): the chunk plan wins up to 128 rows, the wide plan
    from 256 rows on."""
    ids = _t(fx["decoder_input_ids"])
    tiny16(input_features=feats, decoder_input_ids=ids)                      # 72 rows
    assert tiny16._fwd_sessions[3].forward_plan_last == "chunk"
    sess = tiny16._fwd_sessions[3]
    wide = sess.forward_all(ids.repeat(1, 4)[:, :86])                         # 258 rows
    assert sess.forward_plan_last == "wide" and tuple(wide.shape) == (3, 86, TINY.vocab_size)
    small = sess.forward_all(ids.repeat(1, 4)[:, :85])                        # 255 rows
    assert sess.forward_plan_last == "chunk"
    # the two plans on either side of the threshold (causal: the first 85 positions are the same rows): each is within
    # the bf16 bar of the exact logits, so they are within twice the bar of each other
    err = (wide[:, :85] - small).abs()
    print(f"wide (258 rows) vs chunk (255 rows): max |logit difference| {float(err.max()):.4f}")
    assert float(err.max()) < 2 * BF16_MAX


@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_one_position_forward(which, tiny32, tiny16, fx, feats, oracle):
    """T == 1 takes the one-token step plan and its own LM head: position 0 of the 24-position pass (causal, so the
    same arithmetic up to the plan's rounding), held to the same references and bars."""
    m = tiny32 if which == "fp32" else tiny16
    ids = _t(fx["decoder_input_ids"])
    one = m(input_features=feats, decoder_input_ids=ids[:, :1]).logits
    assert tuple(one.shape) == (3, 1, TINY.vocab_size) and one.dtype == torch.float32
    lg = one.cpu().numpy()
    err = np.abs(_top8(np.broadcast_to(lg, (3, 24, TINY.vocab_size)), fx)[:, 0] - fx["top_val"][:, 0])
    print(f"{which} one-position forward: top-8 error at position 0 max {err.max():.3g} mean {err.mean():.3g}")
    if which == "fp32":
        assert err.max() <= FP32_BAR and np.abs(lg[:, 0] - oracle["ids"][:, 0]).max() <= FP32_BAR
    else:
        assert err.max() < BF16_MAX and err.mean() < BF16_MEAN


# ----------------------------------------------------------------------------------------- 3. encoder_outputs
@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_encoder_outputs_is_bitwise_the_features_call(which, tiny32, tiny16, fx, feats):
    m = tiny32 if which == "fp32" else tiny16
    labels = _t(fx["labels"])
    a = m(input_features=feats, labels=labels)
    enc = m.get_encoder()(feats)
    b = m(encoder_outputs=enc, labels=labels)
    assert torch.equal(a.logits, b.logits)
    c = m(encoder_outputs=(a.encoder_last_hidden_state,), labels=labels)  # a tuple, as HF takes it
    d = m(encoder_outputs=a.encoder_last_hidden_state, labels=labels)    # a tensor
    assert torch.equal(a.logits, c.logits) and torch.equal(a.logits, d.logits)
    assert torch.equal(a.loss, b.loss)


# --------------------------------------------------------------------------------------------- 4. / 5. end to end
def _student(fx):
    shape = (3, 24, TINY.vocab_size)
    return np.random.RandomState(int(fx["student_seed"])).standard_normal(shape).astype(np.float32) * np.float32(3)


@pytest.mark.parametrize("T", [1.0, 2.0])
def test_kd_loss_end_to_end_fp32(tiny32, fx, feats, T):
    """kd_loss on the fp32 engine's logits within 1e-3 relative of the float64 value on transformers' logits: the logit
    bar is 1e-3 and the worst-case first-order sensitivity sum |dL/dt| 1e-3 / L is 4.5e-4 for this fixture recipe."""
    from kwhisper.distill import kd_loss

    out = tiny32(input_features=feats, labels=_t(fx["labels"]), decoder_input_ids=_t(fx["decoder_input_ids"]))
    student = _t(_student(fx)).requires_grad_(True)
    loss = kd_loss(student, out.logits, _t(fx["labels"]), T)
    want = float(fx[f"kd_loss_T{T:g}"])
    print(f"fp32 end to end, T = {T:g}: kd loss {float(loss.detach()):.7f}, float64 on HF's logits {want:.7f}")
    assert abs(float(loss.detach()) - want) <= 1e-3 * want
    loss.backward()
    assert student.grad is not None and bool(torch.isfinite(student.grad).all())


@pytest.mark.parametrize("T", [1.0, 2.0])
def test_kd_loss_end_to_end_bf16(tiny16, fx, feats, oracle, T):
    """|loss(bf16 logits) - loss(f32 logits)| <= 1.5 x sum |dL/dt| x max |logit error|: the first-order bound with
    half again for the curvature.  Both factors are computed here: the sensitivity by float64 autograd on the host at
    the oracle's logits, the logit error from the engine's own output (the strided view goes to kd_loss as it is)."""
    from kwhisper.distill import kd_loss

    labels = fx["labels"]
    out = tiny16(input_features=feats, labels=_t(labels), decoder_input_ids=_t(fx["decoder_input_ids"]))
    student = _student(fx)
    loss = float(kd_loss(_t(student), out.logits, _t(labels), T))
    t64 = torch.from_numpy(oracle["ids"]).double().requires_grad_(True)
    p = torch.nn.functional.softmax(t64 / T, dim=-1)
    lq = torch.nn.functional.log_softmax(torch.from_numpy(student).double() / T, dim=-1)
    mask = torch.from_numpy(labels >= 0).unsqueeze(-1)
    ref = (torch.nn.KLDivLoss(reduction="none")(lq, p) * mask).sum() / mask.sum() * T ** 2
    ref.backward()
    sens = float(t64.grad.abs().sum())
    dlogit = float(np.abs(out.logits.cpu().numpy() - oracle["ids"])[labels >= 0].max())
    print(f"bf16 end to end, T = {T:g}: kd loss {loss:.6f}, float64 on the oracle's logits {ref.item():.6f}; "
          f"sum |dL/dt| = {sens:.4f}, max |logit error| on valid rows = {dlogit:.4f}, bound {1.5 * sens * dlogit:.4f}")
    assert abs(loss - ref.item()) <= 1.5 * sens * dlogit


# ------------------------------------------------------------------------------------------ 6. generate() isolation
@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_generate_is_untouched_by_a_forward(which, fx, feats):
    m = _model(None, torch.float32 if which == "fp32" else torch.bfloat16)
    kw = dict(language="ja", task="transcribe", max_length=32)
    before = m.generate(feats[:2], **kw).cpu().numpy()      # (bf16: the step graphs are captured here)
    m(input_features=feats[:2], labels=_t(fx["labels"][:2]))
    m(input_features=feats, labels=_t(fx["labels"]))
    after = m.generate(feats[:2], **kw).cpu().numpy()
    np.testing.assert_array_equal(before, after)
    assert m._fwd_sessions[2] is not m._sessions[(2, 1)]


# ------------------------------------------------------------------------------------------------------- 7. fp8
def test_fp8_engine_refuses_forward_and_default_engine_is_untouched(tiny16, fx, feats):
    m = _model("fp8_e4m3")
    with pytest.raises(NotImplementedError, match="fp8"):
        m(input_features=feats, labels=_t(fx["labels"]))
    sess = m.engine.new_session(2)
    with pytest.raises(NotImplementedError, match="fp8"):
        sess.forward_all(_t(fx["decoder_input_ids"][:2]))
    # the default engine's step plan, after forward() has run on it, is the one test_fp8_default_untouched lists
    tiny16(input_features=feats[:2], labels=_t(fx["labels"][:2]))
    s2 = tiny16._session(2)
    kinds = [type(p).__name__ for p in s2._step_plans(1)]
    assert "XqCrossPlan" in kinds and "XqCrossFp8Plan" not in kinds
    assert s2.cross.dtype == torch.bfloat16 and s2.cross_scale is None


def test_forward_refuses_ids_outside_the_vocabulary(tiny32, fx, feats):
    bad = fx["decoder_input_ids"].copy()
    bad[1, 3] = TINY.vocab_size
    with pytest.raises(IndexError):
        tiny32(input_features=feats, decoder_input_ids=_t(bad))
    bad[1, 3] = -100
    with pytest.raises(IndexError):
        tiny32(input_features=feats, decoder_input_ids=_t(bad))
