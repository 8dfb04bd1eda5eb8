"""CPU tests of the distillation feature: HF's label shift, forward()'s argument checks on a host stub, the plain
float64 restatement of the KD loss (tests/_distill_ref.py) against torch's KLDivLoss expression, and the in-repo oracle
against transformers' own forward (tests/golden/forward_tiny.npz, tools/make_forward_fixtures.py) -- the yardstick the
GPU tests (tests/test_distill_gpu.py, tests/test_gpu_kd_loss.py) compare full tensors against."""
import os
import types

import numpy as np
import pytest
import torch

import _distill_ref as DR
from _util import oracle_features
from conftest import GOLD

from kwhisper.config import TINY, generation_constants
from kwhisper.synthetic import synthetic_state_dict


def _host_model():
    """forward()'s argument checks run before anything touches the device: a model over a stub engine."""
    from kwhisper.generation import KWhisperForConditionalGeneration

    gen = generation_constants(TINY)
    m = object.__new__(KWhisperForConditionalGeneration)
    m.engine = types.SimpleNamespace(shape=TINY, generation_config=gen, device="cpu")
    m.generation_config = gen
    m._fwd_sessions, m.forward_plan = {}, None
    return m


def test_shift_equals_transformers():
    from transformers.models.whisper.modeling_whisper import shift_tokens_right as hf_shift

    from kwhisper.generation import shift_tokens_right

    labels = torch.tensor([[-100, -100, 50258, 7, 8, 50257],       # -100 at the front
                           [50258, 5, -100, 6, 9, 50257],          # in the middle
                           [50258, 5, 6, 50257, -100, -100],       # at the end
                           [-100, 3, -100, 4, -100, -100]], dtype=torch.int64)
    want = hf_shift(labels, TINY.pad_token_id, TINY.decoder_start_token_id)
    got = shift_tokens_right(labels, TINY.pad_token_id, TINY.decoder_start_token_id)
    assert torch.equal(got, want)
    assert (got >= 0).all() and labels[0, 0] == -100  # the input is left alone
    np.testing.assert_array_equal(DR.shift_right(labels.numpy(), TINY.pad_token_id, TINY.decoder_start_token_id),
                                  want.numpy())


def test_forward_argument_errors_on_a_host_model():
    m = _host_model()
    feats = torch.zeros(1, 80, 3000)
    with pytest.raises(ValueError, match="Labels' sequence length 449 cannot exceed the maximum allowed length of 448 "
                                         "tokens."):
        m.forward(input_features=feats, labels=torch.zeros((1, 449), dtype=torch.int64))
    with pytest.raises(ValueError, match="You cannot specify both decoder_input_ids and decoder_inputs_embeds at the "
                                         "same time"):
        m(input_features=feats)
    with pytest.raises(NotImplementedError, match="decoder_attention_mask"):
        m(input_features=feats, labels=torch.zeros((1, 4), dtype=torch.int64),
          decoder_attention_mask=torch.ones((1, 4), dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="output_attentions"):
        m(input_features=feats, labels=torch.zeros((1, 4), dtype=torch.int64), output_attentions=True)
    for k in ("past_key_values", "decoder_inputs_embeds", "output_hidden_states", "use_cache"):
        with pytest.raises(NotImplementedError, match=k):
            m(input_features=feats, labels=torch.zeros((1, 4), dtype=torch.int64), **{k: True})
    with pytest.raises(ValueError, match="input_features"):
        m(labels=torch.zeros((1, 4), dtype=torch.int64))
    # an fp8-cache engine has no many-row cross-attention: refused before anything touches the device
    m.engine.cross_kv_fp8 = True
    with pytest.raises(NotImplementedError, match="fp8"):
        m(input_features=feats, labels=torch.zeros((1, 4), dtype=torch.int64))


def test_forward_output_reads_like_hf():
    from kwhisper.generation import ForwardOutput

    logits = torch.tensor([[[2.0, 0.0, -1.0], [0.5, 0.5, 3.0]]])
    enc = torch.zeros(1, 2, 4)
    out = ForwardOutput(logits, enc)
    assert out.loss is None and out[0] is logits and out[1] is enc and len(out) == 2
    assert list(out) == ["logits", "encoder_last_hidden_state"] and out["logits"] is logits
    labels = torch.tensor([[0, -100]])
    out = ForwardOutput(logits, enc, labels)
    want = torch.nn.CrossEntropyLoss()(logits.view(-1, 3), labels.reshape(-1))
    assert abs(float(out.loss) - float(want)) < 1e-6
    assert out[0] is out.loss and out[1] is logits and out.to_tuple()[2] is enc and out[:2] == (out.loss, logits)


def test_kd_restatement_equals_torch_kldivloss_at_f64():
    """tests/_distill_ref.kd_ref against the reference's expression (softmax, log_softmax, KLDivLoss(reduction="none"),
    the labels >= 0 mask, the mean, T^2) in float64, and its gradient by autograd: 1e-12."""
    rng = np.random.RandomState(2)
    N, V = 4, 1000
    t = rng.standard_normal((N, V)) * 3
    s = rng.standard_normal((N, V)) * 3
    labels = np.array([5, -100, 7, 999])
    for T in (0.5, 1.0, 2.0):
        st = torch.from_numpy(s).requires_grad_(True)
        p = torch.nn.functional.softmax(torch.from_numpy(t) / T, dim=-1)
        lq = torch.nn.functional.log_softmax(st / T, dim=-1)
        div = torch.nn.KLDivLoss(reduction="none")(lq, p)
        mask = (torch.from_numpy(labels) >= 0).unsqueeze(-1)
        div = div * mask
        want = div.sum() / mask.sum() * T ** 2
        want.backward()
        loss, rows, grad = DR.kd_ref(t, s, labels, T)
        assert abs(loss - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
        np.testing.assert_allclose(rows, div.sum(-1).detach().numpy(), rtol=0, atol=1e-12)
        np.testing.assert_allclose(grad, st.grad.numpy(), rtol=0, atol=1e-12)
        assert rows[1] == 0 and (grad[1] == 0).all()
    loss, rows, grad = DR.kd_ref(t, s, np.full(N, -100), 2.0)
    assert np.isnan(loss) and (rows == 0).all() and (grad == 0).all()


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLD, "forward_tiny.npz")))


def test_fixture_is_the_collators_shape(fx):
    labels, ids, full = fx["labels"], fx["decoder_input_ids"], fx["labels_full"]
    assert labels.shape == ids.shape == (3, 24) and full.shape == (3, 25)
    np.testing.assert_array_equal(ids, full[:, :-1])
    assert (labels[:, 0] == -100).sum() == 2 and (labels[:, -1] == -100).sum() == 2  # prompt prefixes, padded tails
    keep = labels != -100
    np.testing.assert_array_equal(labels[keep], full[:, 1:][keep])
    assert (ids >= 0).all() and fx["top_val"].shape == (3, 24, 8) and fx["lse"].shape == (3, 24)


def test_oracle_full_sequence_logits_match_transformers(fx):
    """The oracle's logits of every position on the fixture's inputs: within 1e-4 of transformers' top-8 values and
    log-sum-exp (measured 9.5e-6), and its cross-entropy and KD losses at the stored ones.  It passes without the
    feature: it is what lets the GPU tests hold full [3][24][V] tensors to the oracle."""
    from oracle.whisper_np import WhisperNP

    o = WhisperNP(synthetic_state_dict(TINY, 0), TINY)
    enc = o.encode(oracle_features(TINY, fx["cases"]))
    lg = o.decode(fx["decoder_input_ids"], o.new_cache(enc))
    got_top = np.take_along_axis(lg, fx["top_idx"].astype(np.int64), -1)
    assert np.abs(got_top - fx["top_val"]).max() <= 1e-4
    m = lg.max(-1, keepdims=True).astype(np.float64)
    lse = (m + np.log(np.exp(lg - m).sum(-1, keepdims=True)))[..., 0]
    assert np.abs(lse - fx["lse"]).max() <= 1e-4
    assert abs(DR.cross_entropy64(lg, fx["labels"]) - float(fx["loss"])) <= 1e-4
    # labels alone: the shifted ids
    ids2 = DR.shift_right(fx["labels"], TINY.pad_token_id, TINY.decoder_start_token_id)
    lg2 = o.decode(ids2, o.new_cache(enc))
    assert np.abs(np.sort(lg2, -1)[..., ::-1][..., :8] - fx["shift_top_val"]).max() <= 1e-4
    assert abs(DR.cross_entropy64(lg2, fx["labels"]) - float(fx["shift_loss"])) <= 1e-4
    # the stored KD values are the restatement's on these logits (first-order sensitivity to 1e-5 logit error: ~1e-5)
    V = lg.shape[-1]
    student = np.random.RandomState(int(fx["student_seed"])).standard_normal(lg.shape).astype(np.float32) * np.float32(3)
    for T in fx["temperatures"]:
        loss, rows, _ = DR.kd_ref(lg.reshape(-1, V), student.reshape(-1, V), fx["labels"].reshape(-1), T)
        assert abs(loss - float(fx[f"kd_loss_T{T:g}"])) <= 1e-4 * loss
        assert np.abs(rows - fx[f"kd_rows_T{T:g}"].reshape(-1)).max() <= 1e-3
