"""The fp8 (e4m3) cross K/V option without a GPU: the format's CPU restatement (tests/_fp8_ref.py), what the
quantisation alone costs in accuracy on the tiny fixture model, and the engine option's validation."""
import numpy as np
import pytest
import torch

from kwhisper.config import TINY
from kwhisper.synthetic import synthetic_state_dict

import _fp8_ref as R
from _util import oracle_features


def test_exact_inputs_round_trip():
    """Values the format holds exactly -- e4m3 codes with one +-448 per channel, times a power-of-two channel scale,
    all exact in bf16 -- quantise back to those codes, with exactly the powers of two as scales."""
    rng = np.random.default_rng(0)
    for n, S in ((3, 1500), (2, 77), (4, 1)):
        x, codes, scales = R.exact_case(rng, n, S)
        assert np.array_equal(torch.from_numpy(x).bfloat16().float().numpy(), x)  # exact in bf16
        c, s = R.quantize(torch.from_numpy(x).bfloat16())
        assert np.array_equal(c, codes)
        assert np.array_equal(s, scales)
        assert np.array_equal(R.dequantize(c, s), x)


def test_zero_channel():
    """A channel of zeros (of either sign) gives zero codes and a zero scale; its neighbours are untouched."""
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal((2, 50, 64)).astype(np.float32)).bfloat16()
    x[0, :, 5] = 0.0
    x[1, :, 9] = -0.0
    c, s = R.quantize(x)
    assert s[0, 5] == 0 and s[1, 9] == 0 and not c[0, :, 5].any() and not c[1, :, 9].any()
    others = np.ones((2, 64), bool)
    others[0, 5] = others[1, 9] = False
    assert (s[others] > 0).all()
    d = R.dequantize(c, s)
    assert np.isfinite(d).all() and not d[0, :, 5].any()
    # a channel whose maximum is negative: the scale is its magnitude / 448 and the peak's code is -448
    x[0, :, 7] = -x[0, :, 7].abs() - 1
    c, s = R.quantize(x)
    k = int(x[0, :, 7].float().abs().argmax())
    assert s[0, 7] == np.float32(x[0, k, 7].float().abs().item()) / np.float32(448.0) and c[0, k, 7] == 0xFE


@pytest.fixture(scope="module")
def tiny_oracle():
    from oracle.whisper_np import WhisperNP

    return WhisperNP(synthetic_state_dict(TINY, 0), TINY)


def test_quantisation_only_accuracy(gold, tiny_oracle):
    """What the cache format alone costs: the fp32 oracle on the tiny fixture model with its cross K/V replaced by
    their bf16-rounded, fake-quantised values, teacher-forced along the fixture's greedy sequences; top-8 logits
    against transformers' fp32.  Bars: twice the measured 0.0098 (max) / 0.0019 (mean) over the 4,096 values (the
    computation is deterministic up to BLAS summation order); bf16 rounding alone gives 0.0004 / 0.00008."""
    g = gold("tiny_fp32")
    m = tiny_oracle
    feats = oracle_features(TINY, g["cases"])
    seq = g["greedy_sequences"]
    cache = m.new_cache(m.encode(feats))
    cache["cross"] = [(R.fake_quant(k), R.fake_quant(v)) for k, v in cache["cross"]]
    logits = m.decode(seq[:, :-1], cache)[:, 3:]
    idx, val = g["greedy_logits_top_idx"], g["greedy_logits_top_val"]
    got = np.take_along_axis(logits[:, : idx.shape[1]], idx.astype(np.int64), axis=-1)
    err = np.abs(got - val)
    print("fp8 cross K/V, quantisation only: top-8 logit err max %.4f mean %.5f over %d values"
          % (err.max(), err.mean(), err.size))
    assert err.max() < 0.02 and err.mean() < 0.004


def test_option_validation():
    """cross_kv_dtype="fp8_e4m3" needs the bf16 engine, and an unknown string is refused -- both before anything
    touches the weights or the device."""
    from kwhisper.engine import WhisperEngine

    with pytest.raises(ValueError, match="bfloat16"):
        WhisperEngine(TINY, {}, dtype=torch.float32, cross_kv_dtype="fp8_e4m3")
    with pytest.raises(ValueError, match="cross_kv_dtype"):
        WhisperEngine(TINY, {}, dtype=torch.bfloat16, cross_kv_dtype="fp8")
    with pytest.raises(ValueError, match="cross_kv_dtype"):
        WhisperEngine(TINY, {}, dtype=torch.bfloat16, cross_kv_dtype="int8")
