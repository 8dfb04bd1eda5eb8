"""CPU tests of ``repetition_penalty`` / ``no_repeat_ngram_size``: the numpy restatement tests/_repeat_ref.py against
transformers' own RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor (bit for bit), generate()'s host
logic over a stub session (where the two arguments come from, where they go, what they refuse), and the conditions
tests/golden/repeat_tiny.npz has to meet to prove anything (tools/make_repeat_fixture.py)."""
import json
import types

import numpy as np
import pytest
import torch

import _repeat_ref as RR

from kwhisper.config import TINY, generation_constants

F32 = np.float32
G = generation_constants(TINY)
TS = G.timestamp_begin
PROMPT_TS = [G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"]]
LOGIT_BAR = 1e-3  # tests/test_prompt_gpu.py's


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


# ---- the restatement against transformers ---------------------------------------------------------------------------
def _rows(V, L, rng):
    """(4, L) histories with duplicates, the ids 0 and V-1, and -- from L = 12 on -- a tail that repeats an earlier
    run, so n-grams up to 6 do recur; scores with 0.0, -0.0, -inf and NaN at history tokens."""
    pool = np.concatenate([[0, V - 1], rng.choice(np.arange(1, V - 1), max(1, L // 3), replace=False)])
    ids = rng.choice(pool, (4, L))
    ids[0, 0], ids[1, -1] = 0, V - 1
    if L >= 12:
        ids[:, -5:] = ids[:, 3:8]
    x = (rng.standard_normal((4, V)) * 4).astype(F32)
    for r in range(4):
        toks = list(dict.fromkeys(ids[r].tolist()))
        for t, v in zip(toks, [0.0, -0.0, -np.inf, np.nan]):
            x[r, t] = v
    return ids.astype(np.int64), x


@pytest.mark.parametrize("n", [1, 2, 3, 6])
@pytest.mark.parametrize("penalty", [1.3, 0.7])
def test_restatement_equals_transformers(penalty, n):
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

    V = 97
    seen_ban = False
    for L in sorted({1, max(1, n - 1), n, 40}):
        ids, x = _rows(V, L, np.random.default_rng(100 * n + L))
        ti, tx = torch.from_numpy(ids), torch.from_numpy(x)
        want_p = RepetitionPenaltyLogitsProcessor(penalty)(ti, tx.clone()).numpy()
        assert (_bits(RR.repetition_penalty(ids, x, penalty)) == _bits(want_p)).all(), L
        want_n = NoRepeatNGramLogitsProcessor(n)(ti, tx.clone()).numpy()
        assert (_bits(RR.no_repeat_ngram(ids, x, n)) == _bits(want_n)).all(), L
        both = NoRepeatNGramLogitsProcessor(n)(ti, torch.from_numpy(want_p)).numpy()  # the reference's order
        assert (_bits(RR.repeat_process(ids, x, penalty, n)) == _bits(both)).all(), L
        seen_ban |= bool((np.isneginf(want_n) & ~np.isneginf(x)).any())
        if L < n:
            assert (_bits(want_n) == _bits(x)).all()
    assert seen_ban
    ids, x = _rows(V, 40, np.random.default_rng(7))
    assert (_bits(RR.repeat_process(ids, x, 1.0, 0)) == _bits(x)).all()


def test_restatement_penalises_a_repeated_token_once_and_skips_foreign_ids():
    ids = np.array([[5, 5, 5, 200, -1, 7]], np.int64)
    x = np.zeros((1, 10), F32)
    x[0, 5], x[0, 7] = 2.6, -2.0
    got = RR.repeat_process(ids, x, 1.3, 0)
    assert got[0, 5] == F32(2.6) / F32(1.3) and got[0, 7] == F32(-2.0) * F32(1.3)
    assert RR.has_repeated_ngram([1, 2, 3, 1, 2, 3], 3) and not RR.has_repeated_ngram([1, 2, 3, 1, 2, 4], 3)


# ---- generate()'s host logic over a stub session -----------------------------------------------------------------------
class _StubSession:
    """Scripted decodes that record what each call was given: ``script[call]`` = (ids with the prompt, avg_logprob)."""

    def __init__(self, script):
        self.script, self.calls, self.avg_logprob = script, [], None

    def set_encoder_output(self, enc, key=None):
        pass

    def _next(self, kind, prompt, gen, kw):
        ids, lp = self.script[len(self.calls) % len(self.script)]
        self.calls.append(dict(kind=kind, repeat=kw.get("repeat", "absent"), has_repeat="repeat" in kw,
                               sample=kw.get("sample")))
        self.avg_logprob = np.asarray(lp, np.float64)
        return np.asarray(ids, np.int64).copy()

    def generate(self, prompt, gen, *, max_length, return_timestamps, **kw):
        return self._next("greedy", prompt, gen, kw)

    def generate_beam(self, prompt, gen, *, num_beams, max_length, return_timestamps, **kw):
        return self._next("beam", prompt, gen, kw)


def _stub_model(script, gen=None):
    from kwhisper.generation import KWhisperForConditionalGeneration

    sess = _StubSession(script)
    eng = types.SimpleNamespace(shape=TINY, device=torch.device("cpu"), dtype=torch.float32,
                                generation_config=gen or generation_constants(TINY),
                                encode=lambda x: torch.zeros(1), new_session=lambda B, beams=1: sess)
    return KWhisperForConditionalGeneration(eng), sess


def _row(body, L=12):
    r = PROMPT_TS + list(body)
    return r + [G.pad_token_id] * (L - len(r))


BODY = [TS, 100, 101, TS + 50, G.eos_token_id]
KW = dict(language="ja", task="transcribe", return_timestamps=True)


def test_generate_takes_the_arguments_parent_refuses():
    """On the parent commit both names land in the "not used by the model" ValueError."""
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(torch.zeros((1, 80, 3000)), repetition_penalty=1.3, **KW)
    assert [c["repeat"] for c in sess.calls] == [(1.3, 0)]
    sess.calls.clear()
    model.generate(torch.zeros((1, 80, 3000)), no_repeat_ngram_size=3, **KW)
    assert [c["repeat"] for c in sess.calls] == [(1.0, 3)]


def test_repeat_reaches_every_pass_attempt_and_beam_call():
    # long-form, 45 s: two passes
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(torch.zeros((1, 80, 4500)), repetition_penalty=1.3, no_repeat_ngram_size=3, **KW)
    assert len(sess.calls) == 2 and all(c["repeat"] == (1.3, 3) and c["kind"] == "greedy" for c in sess.calls)
    # the fallback: every attempt of the schedule (the row never passes the threshold)
    model, sess = _stub_model([([_row(BODY)], [-2.0])])
    model.generate(torch.zeros((1, 80, 3000)), repetition_penalty=1.3, no_repeat_ngram_size=2, temperature=(0.0, 0.2, 0.4),
                   logprob_threshold=-1.0, **KW)
    assert [c["sample"]["temperature"] for c in sess.calls] == [0.0, 0.2, 0.4]
    assert all(c["repeat"] == (1.3, 2) for c in sess.calls)
    # beams
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(torch.zeros((1, 80, 3000)), num_beams=3, no_repeat_ngram_size=4, **KW)
    assert [(c["kind"], c["repeat"]) for c in sess.calls] == [("beam", (1.0, 4))]
    # conditioned long-form passes (key_start travels beside it)
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(torch.zeros((1, 80, 4500)), condition_on_prev_tokens=True, repetition_penalty=0.7, **KW)
    assert len(sess.calls) == 2 and all(c["repeat"] == (0.7, 0) for c in sess.calls)


def test_values_come_from_the_call_else_the_config():
    gen = generation_constants(TINY)
    gen.repetition_penalty, gen.no_repeat_ngram_size = 1.2, 4
    model, sess = _stub_model([([_row(BODY)], [-0.5])], gen)
    x = torch.zeros((1, 80, 3000))
    model.generate(x, **KW)
    model.generate(x, repetition_penalty=1.5, **KW)
    model.generate(x, no_repeat_ngram_size=2, **KW)
    model.generate(x, generation_config={**generation_constants(TINY).to_dict(), "no_repeat_ngram_size": 5}, **KW)
    assert [c["repeat"] for c in sess.calls] == [(1.2, 4), (1.5, 4), (1.2, 2), (1.0, 5)]
    # the dataclass carries the fields (from_pretrained copies generation_config.json's keys onto it)
    assert generation_constants(TINY).repetition_penalty is None and generation_constants(TINY).no_repeat_ngram_size is None


@pytest.mark.parametrize("off", [dict(), dict(repetition_penalty=None, no_repeat_ngram_size=None),
                                 dict(repetition_penalty=1.0, no_repeat_ngram_size=0), dict(repetition_penalty=1.0),
                                 dict(no_repeat_ngram_size=0)])
def test_off_values_make_the_call_without_them(off):
    """None / 1.0 / 0: the session is called exactly as before (no ``repeat`` keyword at all)."""
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(torch.zeros((1, 80, 3000)), **off, **KW)
    model.generate(torch.zeros((1, 80, 3000)), num_beams=2, **off, **KW)
    model.generate(torch.zeros((1, 80, 3000)), temperature=(0.0, 0.4), logprob_threshold=-1.0, **off, **KW)
    assert len(sess.calls) == 3 and not any(c["has_repeat"] for c in sess.calls)


@pytest.mark.parametrize("bad", [0.0, -1.3, 2, 0, "1.3"])
def test_penalty_must_be_a_strictly_positive_float(bad):
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    with pytest.raises(ValueError, match="`penalty` has to be a strictly positive float, but is"):
        model.generate(torch.zeros((1, 80, 3000)), repetition_penalty=bad, **KW)
    assert not sess.calls  # refused before any device work


def test_other_refusals_stay():
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    x = torch.zeros((1, 80, 3000))
    with pytest.raises(ValueError, match="not used by the model.*repetition_penalti"):
        model.generate(x, repetition_penalti=1.3, **KW)
    with pytest.raises(ValueError, match="`ngram_size` has to be a strictly positive integer"):
        model.generate(x, no_repeat_ngram_size=2.5, **KW)
    with pytest.raises(NotImplementedError, match="fallback"):
        model.generate(x, repetition_penalty=1.3, num_beams=2, temperature=(0.0, 0.4), **KW)
    with pytest.raises(NotImplementedError, match="prompt_ids"):
        model.generate(x, repetition_penalty=1.3, num_beams=2, prompt_ids=torch.tensor([G.prev_sot_token_id, 5]), **KW)
    assert not sess.calls
    # a negative size builds no processor in the reference (utils.py:1182), so it is "off" here too
    model.generate(x, no_repeat_ngram_size=-1, **KW)
    assert not sess.calls[0]["has_repeat"]


def test_session_repeat_normalisation():
    from kwhisper.decode import _norm_repeat

    assert _norm_repeat(None) is None and _norm_repeat((1.0, 0)) is None
    assert _norm_repeat((1.3, 0)) == (1.3, 0) and _norm_repeat((1, 2)) == (1.0, 2)
    for bad in [(0.0, 0), (-1.0, 2), (float("inf"), 0), (float("nan"), 0), (1.3, -1)]:
        with pytest.raises(ValueError):
            _norm_repeat(bad)


# ---- the fixture proves something ----------------------------------------------------------------------------------------
def _rows_differ(a, b):
    n = max(a.shape[1], b.shape[1])
    pa, pb = np.full((a.shape[0], n), -1, np.int64), np.full((b.shape[0], n), -1, np.int64)
    pa[:, : a.shape[1]], pb[:, : b.shape[1]] = a, b
    return (pa != pb).any(1)


def _first_attempt(passes):
    at = passes[0]["attempts"][0]
    n = max(len(t) for t in at["tokens"])
    out = np.full((len(at["tokens"]), n), -1, np.int64)
    for r, t in enumerate(at["tokens"]):
        out[r, : len(t)] = t
    return out


def test_fixture_differs_from_the_call_without_the_arguments(gold):
    """In every case at least half of the rows differ from the same call's tokens without the two arguments (case e:
    the temperature-0 attempt's tokens; the sampled rows would differ anyway)."""
    g = gold("repeat_tiny")
    pairs = {"a": (g["a_tokens"], g["a_base_tokens"]), "b": (g["b_sequences"], g["b_base_sequences"]),
             "c": (g["c_tokens"], g["c_base_tokens"]), "d": (g["d_sequences"], g["d_base_sequences"]),
             "e": (_first_attempt(json.loads(str(g["e_passes"]))), _first_attempt(json.loads(str(g["e_base_passes"]))))}
    for case, (a, b) in pairs.items():
        d = _rows_differ(np.asarray(a), np.asarray(b))
        assert 2 * int(d.sum()) >= len(d), (case, d)
    args = json.loads(str(g["args"]))
    assert set(args["a"]) == {"repetition_penalty"} and set(args["b"]) == {"no_repeat_ngram_size"}
    assert all(set(args[c]) == {"repetition_penalty", "no_repeat_ngram_size"} for c in "cde")


def test_fixture_margins_and_structure(gold):
    """At most one (case, row) of the greedy cases has a step under the fp32 logit bar (the GPU test compares a row only
    up to such a step); case e's first attempt has rows on both sides of its threshold, none within 0.05 of it, and no
    row of it holds an n-gram twice (one pass's tokens; an output that spans seek passes may repeat across them)."""
    g = gold("repeat_tiny")
    low = [(c, b) for c in "abd" for b in range(g[f"{c}_margin"].shape[0]) if (g[f"{c}_margin"][b] < LOGIT_BAR).any()]
    assert len(low) <= 1, low
    args = json.loads(str(g["args"]))
    at = json.loads(str(g["e_passes"]))[0]["attempts"][0]
    thr = json.loads(str(g["e_kwargs"]))["logprob_threshold"]
    assert any(at["needs_fallback"]) and not all(at["needs_fallback"])
    assert all(abs(x - thr) >= 0.05 for x in at["avg_logprob"])
    for toks in at["tokens"]:
        assert not RR.has_repeated_ngram(PROMPT_TS + toks, args["e"]["no_repeat_ngram_size"])
