"""CPU checks of assisted (speculative) generate: the numpy restatement tests/_spec_ref.py of the accept rule and the
round loop against plain greedy decoding, generation.py's argument handling over a stub paired session, and the C layout
of kw_spec_accept_args."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import _spec_ref as R
from conftest import ROOT

from kwhisper.config import TINY, generation_constants

G = generation_constants(TINY)
GD = dict(G.to_dict(), begin_suppress_tokens=None)
TS, EOS, PAD = G.timestamp_begin, G.eos_token_id, G.pad_token_id
V = TINY.vocab_size


# ---- the accept walk -------------------------------------------------------------------------------------------------
def _row(L, drafts, width=40):
    ids = np.full(width, 7, np.int64)
    ids[L: L + len(drafts)] = drafts
    return ids


def test_accept_none_some_all():
    L, K = 10, 4
    toks = [100, 101, 102, 103, 104]
    r = R.accept(_row(L, [9, 101, 102, 103]), L, K, toks, GD, 40)  # the first draft is wrong: the correction only
    assert (r["n"], r["new_len"], r["done"]) == (0, 11, False) and r["ids"][10] == 100
    assert r["ids"][11:14].tolist() == [101, 102, 103]  # drafts behind the correction stay (beyond the length)
    r = R.accept(_row(L, [100, 101, 9, 103]), L, K, toks, GD, 40)
    assert (r["n"], r["new_len"], r["done"]) == (2, 13, False) and r["ids"][10:13].tolist() == [100, 101, 102]
    r = R.accept(_row(L, toks[:4]), L, K, toks, GD, 40)  # n == K: the bonus token
    assert (r["n"], r["new_len"], r["done"]) == (4, 15, False) and r["ids"][10:15].tolist() == toks


def test_accept_eos_and_max_length():
    L, K = 10, 4
    toks = [100, EOS, 102, 103, 104]
    r = R.accept(_row(L, [100, EOS, 102, 103]), L, K, toks, GD, 40)  # an accepted EOS ends the row there
    assert (r["n"], r["new_len"], r["done"]) == (2, 12, True)
    assert r["ids"][10:15].tolist() == [100, EOS, PAD, PAD, PAD] and r["ids"][15] == 7
    r = R.accept(_row(L, [100, 55, 102, 103]), L, K, toks, GD, 40)  # EOS as the correction
    assert (r["n"], r["new_len"], r["done"]) == (1, 12, True) and r["ids"][10:15].tolist() == [100, EOS, PAD, PAD, PAD]
    toks = [100, 101, 102, None, None]
    r = R.accept(_row(L, [100, 101, 102, 103]), L, K, toks, GD, 13)  # max_length inside the window
    assert (r["n"], r["new_len"], r["done"]) == (3, 13, True)
    assert r["ids"][13:].tolist() == _row(L, [100, 101, 102, 103])[13:].tolist()  # nothing at or beyond max_length
    r = R.accept(_row(L, [100, 9, 102, 103]), L, K, toks, GD, 12)  # the correction is the last position
    assert (r["n"], r["new_len"], r["done"]) == (1, 12, True) and r["ids"][11] == 101 and r["ids"][12] == 102


def test_position_tokens_see_the_drafts():
    """A draft that closes a timestamp pair changes the rule of the position behind it: after (TS + 3, TS + 3) the
    next token may not be a timestamp below TS + 3 and, as a pair has just closed, may be text or a later timestamp;
    after a lone timestamp it must be a timestamp or EOS."""
    P, L, K = 3, 8, 2
    ids = np.zeros(20, np.int64)
    ids[:L] = [G.decoder_start_token_id, 50259, 50359, TS, 100, 101, 102, TS + 3]
    logits = np.zeros((K + 1, V), np.float32)
    logits[:, 200] = 25.0  # text wins wherever it is allowed (and outweighs the timestamps' mass)
    logits[:, TS + 3] = 24.0
    logits[:, TS + 9] = 23.0
    ids[L: L + K] = [TS + 3, 200]  # the draft closes the pair, then text
    toks = R.position_tokens(ids, L, K, logits, GD, P, True, 40)
    assert toks == [TS + 3, 200, 200]  # position 0: text is banned after a lone timestamp
    ids[L: L + K] = [200, 200]  # a draft the main model rejects at once
    assert R.position_tokens(ids, L, K, logits, GD, P, True, 40)[0] == TS + 3


# ---- the round loop: assisted decoding is the main model's greedy decoding ------------------------------------------
# (a small vocabulary keeps the loop quick: text [0, 880), EOS 880, specials, <|notimestamps|> 899, timestamps [900, 1000))
TOY = dict(eos_token_id=880, pad_token_id=879, no_timestamps_token_id=899, max_initial_timestamp_index=50,
           suppress_tokens=[1, 2, 7, 300, 511, 512] + list(range(881, 899)), begin_suppress_tokens=None)
TOY_V, TOY_PROMPT = 1000, [890, 891, 892]


def _toy(seed, noise=0.0, eos_after=None):
    """A deterministic toy model: logits from a hash of the last two tokens and the length (+ a fixed perturbation)."""
    V, EOS = TOY_V, TOY["eos_token_id"]
    def f(history):
        h = np.asarray(history, np.int64)
        key = (int(h[-1]) * 1000003 + int(h[-2]) * 10007 + len(h) * 101 + seed) % (2 ** 31)
        rng = np.random.default_rng(key)
        x = (rng.standard_normal(V) * 3).astype(np.float32)
        if noise:
            x += (np.random.default_rng(key + 17).standard_normal(V) * noise).astype(np.float32)
        if eos_after is not None and len(h) >= eos_after:
            x[EOS] += 30.0
        return x
    return f


@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("assistant", ["same", "other", "noisy"])
def test_round_loop_equals_plain_greedy(assistant, K, rt):
    GD, prompt = TOY, TOY_PROMPT + ([] if rt else [TOY["no_timestamps_token_id"]])
    for max_length, eos_after in ((24, None), (30, 17), (len(prompt) + 1, None), (len(prompt) + K + 1, None)):
        main = _toy(0, eos_after=eos_after)
        draft = {"same": main, "other": _toy(1, eos_after=eos_after),
                 "noisy": _toy(0, noise=1.5, eos_after=eos_after)}[assistant]
        want = R.plain_greedy(main, prompt, GD, rt, max_length)
        got, st = R.assisted_decode(main, draft, prompt, K, GD, rt, max_length)
        np.testing.assert_array_equal(got, want)
        assert st["drafted"] == K * st["rounds"] and 0 <= st["accepted"] <= st["drafted"]
        if assistant == "same":
            assert st["accepted"] >= st["drafted"] - K  # every draft agrees; only a round cut by EOS / max_length differs
            n_gen = len(want) - len(prompt) - 1
            assert st["rounds"] <= -(-n_gen // (K + 1)) + 1 and st["steps"] <= K + 1
        if assistant == "other" and max_length == 24:
            assert st["accepted"] < st["drafted"]


def test_rounds_stop_before_the_cache_ends():
    """Near max_target_positions the loop leaves 2K + 1 positions: a replay issued behind a row that has just finished
    drafts K + 1 more positions from the final length."""
    prompt = TOY_PROMPT + [TOY["no_timestamps_token_id"]]
    main = _toy(0)
    K, t_max = 4, 40
    got, st = R.assisted_decode(main, main, prompt, K, TOY, False, 40, t_max=t_max)
    np.testing.assert_array_equal(got, R.plain_greedy(main, prompt, TOY, False, 40))
    assert st["steps"] >= 1 and len(got) == 40


# ---- generation.py's host logic over a stub paired session -----------------------------------------------------------
class _StubSpec:
    def __init__(self, script):
        self.script, self.calls, self.enc = script, [], []

    def set_encoder_output(self, enc_main, enc_asst):
        self.enc.append((enc_main, enc_asst))

    def generate(self, prompt, gen, *, K, max_length, return_timestamps):
        ids, stats = self.script[len(self.calls)]
        self.calls.append(dict(K=K, max_length=max_length, return_timestamps=return_timestamps,
                               begin_suppress=gen.begin_suppress_tokens, prompt=prompt.numpy().copy()))
        self.last_stats = dict(zip(("rounds", "drafted", "accepted"), stats))
        return np.asarray(ids, np.int64)


def _stub_model(shape=TINY, tag=0.0):
    from kwhisper.generation import KWhisperForConditionalGeneration

    eng = types.SimpleNamespace(shape=shape, device=torch.device("cpu"), dtype=torch.float32,
                                generation_config=generation_constants(shape),
                                encode=lambda x: torch.full((1,), tag), new_session=lambda B, beams=1: None)
    return KWhisperForConditionalGeneration(eng)


def _pair(script):
    model, assistant = _stub_model(tag=1.0), _stub_model(tag=2.0)
    spec = _StubSpec(script)
    model._spec_session = lambda a: spec if a is assistant else None
    return model, assistant, spec


PROMPT = [G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"]]


def test_generate_takes_an_assistant_and_keeps_the_counters():
    """Long-form, 45 s: the paired session is called once per seek pass with the pass's encoder outputs of both models,
    K from the call, no SuppressTokensAtBegin; stats["assisted"] sums the passes' counters."""
    body = [TS, 100, 101, TS + 50, EOS]
    row = [PROMPT + body]
    model, assistant, spec = _pair([(row, (3, 9, 7)), (row, (2, 6, 1))])
    assert model.generation_config.begin_suppress_tokens  # the config has some; the call drops them
    res = model.generate(torch.zeros((1, 80, 4500)), language="ja", task="transcribe", return_timestamps=True,
                         assistant_model=assistant, num_assistant_tokens=3, return_segments=True)
    assert [c["K"] for c in spec.calls] == [3, 3] and all(c["begin_suppress"] is None for c in spec.calls)
    assert all(c["return_timestamps"] for c in spec.calls) and spec.calls[0]["prompt"].tolist() == [PROMPT]
    assert [(float(m), float(a)) for m, a in spec.enc] == [(1.0, 2.0)] * 2  # each model's own encoder
    assert model.stats["assisted"] == {"rounds": 5, "drafted": 15, "accepted": 8}
    assert model.stats["passes"] == 2 and res["sequences"][0].tolist() == [TS, 100, 101, TS + 50] * 2
    assert model.generation_config.begin_suppress_tokens  # (the model's own config is untouched)


def test_num_assistant_tokens_resolution():
    row = [PROMPT + [G.no_timestamps_token_id, 10, EOS]]
    f = torch.zeros((1, 80, 3000))
    model, assistant, spec = _pair([(row, (1, 5, 5))] * 3)
    model.generate(f, language="ja", task="transcribe", assistant_model=assistant)
    assistant.generation_config.num_assistant_tokens = 7
    model.generate(f, language="ja", task="transcribe", assistant_model=assistant)
    model.generate(f, language="ja", task="transcribe", assistant_model=assistant, num_assistant_tokens=2)
    assert [c["K"] for c in spec.calls] == [5, 7, 2]
    for bad in (0, 32, 2.5, True):
        with pytest.raises(ValueError, match="num_assistant_tokens"):
            model.generate(f, language="ja", assistant_model=assistant, num_assistant_tokens=bad)


def test_without_an_assistant_nothing_changes():
    model = _stub_model()
    called = []
    model._spec_session = lambda a: called.append(a)
    sess = types.SimpleNamespace(set_encoder_output=lambda enc, key=None: None,
                                 generate=lambda prompt, gen, **kw: called.append(("plain", gen.begin_suppress_tokens, kw))
                                 or np.asarray([PROMPT + [G.no_timestamps_token_id, 10, EOS]], np.int64))
    model.engine.new_session = lambda B, beams=1: sess
    model.generate(torch.zeros((1, 80, 3000)), language="ja", task="transcribe", num_assistant_tokens=4)
    (tag, bsup, kw), = called
    assert tag == "plain" and bsup == G.begin_suppress_tokens and set(kw) == {"max_length", "return_timestamps", "key_start"}
    assert "assisted" not in model.stats


def test_argument_errors_on_the_host():
    model, assistant, spec = _pair([])
    f = torch.zeros((1, 80, 3000))
    with pytest.raises(ValueError, match="assisted generate is only supported for batch_size = 1"):
        model.generate(torch.zeros((2, 80, 3000)), language="ja", assistant_model=assistant)
    from kwhisper.config import WhisperShape
    import dataclasses

    other = _stub_model(dataclasses.replace(TINY, vocab_size=TINY.vocab_size + 1))
    assert isinstance(other.engine.shape, WhisperShape)
    with pytest.raises(ValueError, match="vocabular"):
        model.generate(f, language="ja", assistant_model=other)
    for bad in (dict(num_beams=2), dict(temperature=(0.0, 0.2), logprob_threshold=-1.0), dict(temperature=0.4),
                dict(return_token_timestamps=True), dict(prompt_ids=torch.tensor([1, 2])),
                dict(condition_on_prev_tokens=True), dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=3)):
        with pytest.raises(NotImplementedError):
            model.generate(f, language="ja", assistant_model=assistant, **bad)
    with pytest.raises(NotImplementedError, match="KWhisperForConditionalGeneration"):
        model.generate(f, language="ja", assistant_model=object())
    model.engine.cross_kv_fp8 = True
    with pytest.raises(NotImplementedError, match="fp8"):
        model.generate(f, language="ja", assistant_model=assistant)
    model.engine.cross_kv_fp8 = False
    assistant.engine.cross_kv_fp8 = True
    with pytest.raises(NotImplementedError, match="fp8"):
        model.generate(f, language="ja", assistant_model=assistant)
    assert not spec.calls


def test_keywords_are_known():
    from kwhisper.generation import _SUPPORTED

    assert {"assistant_model", "num_assistant_tokens"} <= _SUPPORTED


def test_assistant_on_another_device_is_refused():
    from kwhisper.spec import SpecDecodeSession

    eng = lambda dev: types.SimpleNamespace(shape=TINY, device=torch.device(dev))  # noqa: E731
    with pytest.raises(ValueError, match="device"):
        SpecDecodeSession(eng("cuda:0"), eng("cuda:1"))


# ---- ABI -------------------------------------------------------------------------------------------------------------
def test_spec_accept_args_layout_matches_c(tmp_path):
    """The ctypes mirror of kw_spec_accept_args has the C header's size and field offsets."""
    from kwhisper import _lib

    cls = _lib.SpecAcceptArgs
    fields = [f for f, _ in cls._fields_]
    code = "#include <stdio.h>\n#include <stddef.h>\n#include \"kwhisper.h\"\nint main(){"
    code += 'printf("%zu\\n", sizeof(kw_spec_accept_args));'
    for f in fields:
        code += f'printf("%zu\\n", offsetof(kw_spec_accept_args, {f}));'
    code += "return 0;}"
    src, exe = str(tmp_path / "kw_layout.c"), str(tmp_path / "kw_layout")
    with open(src, "w") as fh:
        fh.write(code)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(cls)
    for f, off in zip(fields, got[1:]):
        assert getattr(cls, f).offset == off, f
    assert "kw_spec_accept" in _lib.EXPORTS and "kw_spec_accept_workspace" in _lib.EXPORTS
    assert "spec_accept" in _lib.TORCH_OPS
    lib = _lib.load()
    assert lib.kw_spec_accept_workspace(0) == 0 and lib.kw_spec_accept_workspace(32) == 0
    assert lib.kw_spec_accept_workspace(5) == 6 * 8 * 8 * 4 + 4
    assert lib.kw_spec_accept(None, None) == 1 and b"kw_spec_accept" in lib.kw_last_error()
