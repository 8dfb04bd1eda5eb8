"""GPU tests of assisted (speculative) generate, end to end on the tiny engine: generate(assistant_model=...) against
the same engine's greedy generate() with ``begin_suppress_tokens=None`` -- the contract of kwhisper/spec.py -- with three
assistants (the main model's own weights, other weights, the main model's weights with 5 % noise on the decoder), both
timestamp modes, short-form and a two-pass long-form clip; and one bf16 case that bounds the K + 1-position verify
forward against the one-position step.
"""
import copy
import math

import numpy as np
import pytest
import torch

from conftest import gpu_available

from kwhisper.config import TINY, generation_constants

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

NEW_TOKENS = 30
NOISE_SEED = 0  # (c): chosen so that some but not all drafts are accepted on the clips below
# the bf16 teacher-forced bound of tests/test_gpu_workloads.py (test_config3_large_v3_bf16): logits within 0.2 of the
# reference at the worst, 0.03 on average
BF16_MAX, BF16_MEAN = 0.2, 0.03


def _model(sd, dtype=torch.float32):
    from kwhisper.generation import KWhisperForConditionalGeneration

    return KWhisperForConditionalGeneration.from_state_dict(TINY, sd, dtype=dtype,
                                                            generation_config=generation_constants(TINY))


def _noisy(sd, seed, rel=0.05):
    """``sd`` with Gaussian noise of ``rel`` times each tensor's own standard deviation on every decoder weight."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, w in sd.items():
        if "decoder" in k and w.dtype.kind == "f":
            w = (w + rel * float(w.std()) * rng.standard_normal(w.shape)).astype(w.dtype)
        out[k] = w
    return out


@pytest.fixture(scope="module")
def models():
    from kwhisper.synthetic import synthetic_state_dict

    sd0 = synthetic_state_dict(TINY, 0)
    main = _model(sd0)
    main.record_pass_ids = True  # stats["pass_ids"]: every pass's ids with the prompt, for the tokens generated
    return dict(main=main, same=_model(sd0), other=_model(synthetic_state_dict(TINY, 1)),
                noisy=_model(_noisy(sd0, NOISE_SEED)))


@pytest.fixture(scope="module")
def clips(gold):
    """Two of the short-form clips of tools/make_fixtures.py fallback_features() (dummy:0, tone:0), one row each."""
    from _util import oracle_features

    cases = [str(c) for c in gold("fallback_tiny")["cases"]]
    f = torch.from_numpy(oracle_features(TINY, [cases[0], cases[2]])).cuda()
    return [f[0:1], f[1:2]]


@pytest.fixture(scope="module")
def long_clip():
    """One 36 s clip: two seek passes (the first window's last timestamp pair moves the seek to frame 2384)."""
    from _util import long_audio
    from oracle.mel import log_mel_padded

    feats, _ = log_mel_padded([long_audio("tone", 0, 36.0)], TINY.num_mel_bins)
    assert feats.shape[-1] == 3600
    return torch.from_numpy(feats).cuda()


_REF = {}


def _reference(main, key, feats, **kw):
    """The main model's greedy generate() with begin_suppress_tokens=None, computed once per input and mode."""
    if key not in _REF:
        gen = copy.deepcopy(main.generation_config)
        gen.begin_suppress_tokens = None
        res = main.generate(feats, generation_config=gen, **kw)
        _REF[key] = ({k: v for k, v in res.items()} if isinstance(res, dict) else res.cpu().numpy(), dict(main.stats))
    return _REF[key]


def _generated(main):
    """Tokens generated in every pass of the last call (the prefill's first token included)."""
    return [int(ids.shape[1]) - int(P) for ids, P in zip(main.stats["pass_ids"], main.stats["pass_P"])]


def _all_accepted(g, K, g_max=NEW_TOKENS):
    """(rounds, accepted) of one pass that generates ``g`` tokens (of at most ``g_max``) when every draft agrees: the
    first token is the prefill's; a round is issued while K + 1 more positions fit below max_length and keeps K drafts
    and the bonus token -- or, when the row's EOS (g < g_max) falls inside it, the drafts up to and including the EOS;
    the rest is the plain-step tail."""
    n, rounds, accepted = 1, 0, 0
    while n < g and n + K + 1 <= g_max:
        take = min(K + 1, g - n)
        rounds, accepted, n = rounds + 1, accepted + min(take, K), n + take
    return rounds, accepted


def _check_counters(assistant, K, st, generated, passes):
    rounds, drafted, accepted = st["rounds"], st["drafted"], st["accepted"]
    assert drafted == K * rounds and 0 <= accepted <= drafted
    if assistant == "same":
        # every draft is accepted: the counters are exactly those of the round schedule
        want = [_all_accepted(g, K) for g in generated]
        assert (rounds, accepted) == (sum(w[0] for w in want), sum(w[1] for w in want)), (st, generated)
        assert math.ceil(sum(generated) / (K + 1)) - 2 * passes <= rounds <= math.ceil(sum(generated) / (K + 1))
    elif assistant == "other":
        assert accepted < drafted / 2, st
    else:
        assert 0 < accepted < drafted, st


@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("assistant", ["same", "other", "noisy"])
def test_short_form_equals_greedy(models, clips, assistant, K, rt):
    main = models["main"]
    total = dict(rounds=0, drafted=0, accepted=0)
    generated = []
    for i, f in enumerate(clips):
        kw = dict(language="ja", task="transcribe", return_timestamps=rt, max_new_tokens=NEW_TOKENS,
                  return_dict_in_generate=True)
        ref, _ = _reference(main, ("short", i, rt), f, **kw)
        got = main.generate(f, assistant_model=models[assistant], num_assistant_tokens=K, **kw)
        want_seq, got_seq = ref["sequences"].cpu().numpy(), got["sequences"].cpu().numpy()
        np.testing.assert_array_equal(got_seq, want_seq, err_msg=f"clip {i}")
        st = main.stats["assisted"]
        print(f"{assistant} K={K} rt={rt} clip {i}: {st}, {main._spec_session(models[assistant]).last_steps} plain steps")
        for k in total:
            total[k] += st[k]
        generated += _generated(main)
    sess = main._spec_session(models[assistant])
    assert sess.last_rounds >= 1
    _check_counters(assistant, K, total, generated, passes=len(clips))


@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("assistant", ["same", "other", "noisy"])
def test_long_form_two_passes_equals_greedy(models, long_clip, assistant, K):
    main = models["main"]
    kw = dict(language="ja", task="transcribe", return_timestamps=True, max_new_tokens=NEW_TOKENS, return_segments=True)
    ref, ref_stats = _reference(main, ("long",), long_clip, **kw)
    got = main.generate(long_clip, assistant_model=models[assistant], num_assistant_tokens=K, **kw)
    np.testing.assert_array_equal(got["sequences"].cpu().numpy(), ref["sequences"].cpu().numpy())
    assert main.stats["passes"] == ref_stats["passes"] == 2
    assert [(s["start"], s["end"]) for s in got["segments"][0]] == [(s["start"], s["end"]) for s in ref["segments"][0]]
    st = main.stats["assisted"]
    print(f"long-form {assistant} K={K}: {st}")
    _check_counters(assistant, K, st, _generated(main), passes=2)


def test_repeat_calls_replay_the_same_graphs(models, clips):
    """A second call with the same configuration captures nothing new, and a plain call in between is untouched."""
    main, a = models["main"], models["same"]
    kw = dict(language="ja", task="transcribe", return_timestamps=False, max_new_tokens=NEW_TOKENS)
    first = main.generate(clips[0], assistant_model=a, num_assistant_tokens=5, **kw).cpu().numpy()
    sess = main._spec_session(a)
    graphs = {k: id(v) for c in sess._cfg.values() for k, v in c.items() if "graph" in str(k)}
    plain = main.generate(clips[0], **kw).cpu().numpy()
    assert plain.shape[0] == 1 and "assisted" not in main.stats
    again = main.generate(clips[0], assistant_model=a, num_assistant_tokens=5, **kw).cpu().numpy()
    np.testing.assert_array_equal(first, again)
    assert graphs and graphs == {k: id(v) for c in sess._cfg.values() for k, v in c.items() if "graph" in str(k)}
    assert main.stats["assisted"]["rounds"] > 0


def test_many_k_on_one_pair_keep_their_buffers(models, clips):
    """K >= 8 makes the verify forward longer than DecodeSession.LONG_Q, whose lengths a plain session evicts two
    behind.  The paired session keeps every buffer set, because its cached round graphs hold their addresses: three such
    K and back to the first -- the same tokens every time, the first K's buffers and graph where they were."""
    main, a = models["main"], models["noisy"]
    kw = dict(language="ja", task="transcribe", return_timestamps=True, max_new_tokens=NEW_TOKENS,
              return_dict_in_generate=True)
    ref, _ = _reference(main, ("short", 0, True), clips[0], **kw)
    want = ref["sequences"].cpu().numpy()
    sess = main._spec_session(a)
    seen = {}
    for K in (8, 12, 16, 8, 12):
        got = main.generate(clips[0], assistant_model=a, num_assistant_tokens=K, **kw)["sequences"].cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"K={K}")
        assert main.stats["assisted"]["rounds"] > 0
        now = ({k: t.data_ptr() for k, t in sess.main._bufs[K + 1].items() if t is not None},
               [id(c["round_graph"]) for k, c in sess._cfg.items() if k[0] == K])
        assert seen.setdefault(K, now) == now, K
    assert {9, 13, 17} <= set(sess.main._bufs)


def test_pipeline_forwards_the_assistant(models):
    """ASRPipeline(generate_kwargs=...) hands ``assistant_model`` to generate() unchanged: a 20 s clip in two windows,
    one row per call; the text equals the pipeline's without an assistant on a model without SuppressTokensAtBegin."""
    from _util import OracleFeatureExtractor, StubTok
    from kwhisper.pipeline import ASRPipeline
    from kwhisper.synthetic import dummy_audio, synthetic_state_dict

    plain = _model(synthetic_state_dict(TINY, 0))
    plain.generation_config.begin_suppress_tokens = None
    audio = {"array": dummy_audio(0)[: 16000 * 20], "sampling_rate": 16000}
    kw = dict(language="ja", task="transcribe", max_new_tokens=12, num_beams=1)  # (the pipeline's default is beam search)

    def run(model, **extra):
        pipe = ASRPipeline(model, feature_extractor=OracleFeatureExtractor(TINY.num_mel_bins),
                           tokenizer=StubTok(generation_constants(TINY)), chunk_length_s=15, batch_size=1,
                           generate_kwargs=dict(kw, **extra))
        return pipe(dict(audio))

    main = models["main"]
    main.stats = {}
    got = run(main, assistant_model=models["noisy"], num_assistant_tokens=3)
    assert main.stats["assisted"]["rounds"] > 0
    assert got["text"] == run(plain)["text"]


def test_bf16_verify_rows_match_the_one_position_step(clips):
    """bf16 engine: the verify forward's K + 1 logits rows against the q = 1 step's logits at the same positions, within
    the bound of the bf16 teacher-forced tests; assisted tokens equal the greedy ones before the first position whose
    fp32 top-2 margin is under that bound."""
    from kwhisper.synthetic import synthetic_state_dict

    sd0 = synthetic_state_dict(TINY, 0)
    m16, a16, m32 = _model(sd0, torch.bfloat16), _model(sd0, torch.bfloat16), _model(sd0)
    f = clips[1]
    gen = copy.deepcopy(m16.generation_config)
    gen.begin_suppress_tokens = None
    kw = dict(language="ja", task="transcribe", return_timestamps=False, max_new_tokens=NEW_TOKENS,
              return_dict_in_generate=True)
    want = m16.generate(f, generation_config=gen, **kw)["sequences"].cpu().numpy()
    got = m16.generate(f, assistant_model=a16, num_assistant_tokens=5, **kw)["sequences"].cpu().numpy()
    P = 4
    # ---- the verify plan against the one-position step, teacher-forced on the greedy sequence ----
    K = 5
    eng = m16.engine
    sess = eng.new_session(1, eng.encode(f))
    seq = torch.from_numpy(want)
    lg = sess.teacher_forced_logits(seq[:, :-1], P)[0]  # row i predicts position P + i; the cache now holds the sequence
    buf = torch.empty((K + 1, TINY.vocab_size), device="cuda", dtype=torch.float32)
    vlen = torch.zeros((1,), device="cuda", dtype=torch.int32)
    plan = sess._step_plans(K + 1, all_rows=buf)
    errs = []
    for L in (P + 1, P + 7, want.shape[1] - K - 1):  # rows predict positions L .. L + K
        vlen.fill_(L + K)
        sess._run(plan, cur_len=vlen)
        errs.append((buf - lg[L - P: L - P + K + 1]).abs().cpu().numpy())
    err = np.stack(errs)
    print(f"bf16 verify rows vs one-position step: max {err.max():.5f} mean {err.mean():.6f}")
    assert err.max() < BF16_MAX and err.mean() < BF16_MEAN
    # ---- tokens: equal before the first position the fp32 engine decides by less than the bound ----
    s32 = m32.engine.new_session(1, m32.engine.encode(f))
    l32 = s32.teacher_forced_logits(seq[:, :-1], P)[0].clone()
    l32[:, torch.tensor(gen.suppress_tokens, device=l32.device)] = -float("inf")
    top2 = l32.topk(2, -1).values
    margin = (top2[:, 0] - top2[:, 1]).cpu().numpy()[: want.shape[1] - P]
    low = np.nonzero(margin < BF16_MAX)[0]
    n = P + int(low[0]) if low.size else want.shape[1]
    print(f"bf16 assisted vs greedy: compared up to position {n} of {want.shape[1]}; accepted "
          f"{m16.stats['assisted']}")
    np.testing.assert_array_equal(got[0, :n], want[0, :n])
