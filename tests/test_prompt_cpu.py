"""CPU checks of prompt conditioning (``prompt_ids``, ``prompt_condition_type``, ``condition_on_prev_tokens``):
kwhisper.generation.build_pass_input and the plain restatement tests/_prompt_ref.py against every seek pass that
transformers recorded in tests/golden/prompt_tiny.npz (tools/make_prompt_fixture.py), the fixture's own top-2 margins,
the argument errors and the refusals, and generate()'s host loop over a stub session."""
import json
import types

import numpy as np
import pytest
import torch

import _prompt_ref as R

from kwhisper.config import TINY, generation_constants

G = generation_constants(TINY)
INIT = [G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"]]
CASES = ["a", "b", "c", "d", "f"]


def _builder_inputs(g, case, p, toks):
    kw = R.CASE_KWARGS[case]
    prompt = g["prompt_ids"] if kw.get("prompt_ids") else None
    segs = R.segments_before(case, p, toks, g["prompt_ids"], G.prev_sot_token_id)
    return prompt, segs, kw.get("prompt_condition_type", "first-segment")


@pytest.mark.parametrize("case", CASES + ["e"])
def test_builder_reproduces_every_recorded_pass(gold, case):
    """decoder_input_ids and key_start (the number of zeros of the recorded mask) of every pass, from the fixture's own
    segments and the ``do_condition_on_prev_tokens`` list the reference held at that pass.  Case e (the fallback) is
    fed the same way: its passes depend on sampled tokens, but the builder's rule does not."""
    from kwhisper.generation import build_pass_input

    g = gold("prompt_tiny")
    seqs, _, passes, toks = R.fixture_case(g, case)
    B = seqs.shape[0]
    init = np.tile(np.asarray(INIT, np.int64), (B, 1))
    assert len(passes) >= 3
    masked = 0
    for p in passes:
        prompt, segs, ptype = _builder_inputs(g, case if case != "e" else "a", p, toks)
        ids, ks = build_pass_input(init, [[{"tokens": np.asarray(t, np.int64)} for t in row] for row in segs], p["rows"],
                                   p["do_condition"], prompt, G, TINY.max_target_positions, ptype)
        np.testing.assert_array_equal(ids, np.asarray(p["ids"], np.int64))
        want_ks = R.key_start_of(p["mask"])
        assert (ks is None) == (want_ks is None)
        if ks is not None:
            assert [int(k) for k in ks] == want_ks
            masked += any(want_ks)
        # and the restatement the GPU tests use
        rid, rks = R.pass_input(INIT, segs, p["rows"], p["do_condition"], prompt, pad=G.pad_token_id,
                                prev_sot=G.prev_sot_token_id, ts_begin=G.timestamp_begin, all_segments=ptype == "all-segments")
        assert rid == p["ids"] and rks == want_ks
    # what each case is there for: padded rows in a, c, d and e; none in b (no mask at all) and f (one row)
    assert (masked > 0) == (case in "acde")


def test_fixture_covers_the_cases_it_is_there_for(gold):
    g = gold("prompt_tiny")
    shapes = {c: [np.asarray(p["ids"]).shape for p in json.loads(str(g[f"{c}_passes"]))] for c in CASES + ["e"]}
    assert shapes["a"][0] == (3, 3) and max(s[1] for s in shapes["a"]) > 100
    n = len(g["prompt_ids"])
    assert all(s[1] == n + 3 for s in shapes["b"])                       # the prompt on every pass
    assert max(s[1] for s in shapes["c"]) == 223 + n + 3                 # the cut to 448 // 2 - 1 previous tokens
    assert max(s[1] for s in shapes["d"]) == 223 + 1 + 3
    assert all(s[0] == 1 for s in shapes["f"]) and max(s[1] for s in shapes["f"]) > 8
    # e: a pass where one row carries previous text and another only <|startofprev|>, having fallen back at >= 0.5
    found = False
    for p in json.loads(str(g["e_passes"])):
        if p["mask"] is None:
            continue
        kept = [sum(r) for r in p["mask"]]
        off = [not p["do_condition"][a] for a in p["rows"]]
        found |= any(k > 4 for k in kept) and any(k == 4 and o for k, o in zip(kept, off))
    assert found and max(json.loads(str(g["e_kwargs"]))["temperature"]) >= 0.5


def test_fixture_margins_allow_exact_comparison(gold):
    """The fp32 engine is compared token for token up to the first step whose top-2 margin is under the fp32 logit bar
    (1e-3); at most one (case, row) of the fixture may be cut short that way."""
    g = gold("prompt_tiny")
    short = [(c, b) for c in CASES for b, row in enumerate(g[f"{c}_margin"]) if (row < 1e-3).any()]
    assert len(short) <= 1, short


# ---- generate(): errors and refusals ---------------------------------------------------------------------------------
class _StubSession:
    """Scripted decodes: call k returns ``script[k]`` behind the prompt it was given (right-padded with pad)."""

    def __init__(self, script):
        self.script, self.calls = script, []

    def set_encoder_output(self, enc, key=None):
        pass

    def generate(self, prompt, gen, *, max_length, return_timestamps, key_start=None, sample=None):
        body = self.script[len(self.calls)]
        self.calls.append(dict(prompt=prompt.numpy().copy(), key_start=key_start, max_length=max_length))
        L = max(len(b) for b in body)
        ids = np.full((prompt.shape[0], prompt.shape[1] + L), gen.pad_token_id, np.int64)
        ids[:, : prompt.shape[1]] = prompt.numpy()
        for i, b in enumerate(body):
            ids[i, prompt.shape[1]: prompt.shape[1] + len(b)] = b
        return ids


def _stub_model(script, fp8=False):
    from kwhisper.generation import KWhisperForConditionalGeneration

    sess = _StubSession(script)
    eng = types.SimpleNamespace(shape=TINY, device=torch.device("cpu"), dtype=torch.float32, cross_kv_fp8=fp8,
                                generation_config=generation_constants(TINY),
                                encode=lambda x: torch.zeros(1), new_session=lambda B, beams=1: sess)
    return KWhisperForConditionalGeneration(eng), sess


def test_validation_errors_are_transformers():
    """_set_prompt_condition_type (generation_whisper.py:1732-1748): the same ValueErrors, word for word."""
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    model, _ = _stub_model([])
    f = torch.zeros((1, 80, 3000))
    for cond, ptype in [(None, "every-segment"), (None, "all-segments"), (False, "all-segments")]:
        cfg = types.SimpleNamespace(condition_on_prev_tokens=cond)
        with pytest.raises(ValueError) as want:
            gw.WhisperGenerationMixin._set_prompt_condition_type(cfg, ptype)
        with pytest.raises(ValueError) as got:
            model.generate(f, language="ja", prompt_ids=torch.tensor([G.prev_sot_token_id, 5]),
                           prompt_condition_type=ptype, condition_on_prev_tokens=cond)
        assert str(got.value) == str(want.value)


def test_max_new_tokens_error_uses_the_pass_length():
    """_set_max_new_tokens_and_length (:1920-1931): the prompt counts."""
    model, _ = _stub_model([])
    prompt = torch.tensor([G.prev_sot_token_id] + [7] * 9)
    with pytest.raises(ValueError, match=r"is 14,  and `max_new_tokens` is 440.*is: 454"):
        model.generate(torch.zeros((1, 80, 3000)), language="ja", prompt_ids=prompt, max_new_tokens=440)


def test_refusals():
    model, _ = _stub_model([])
    f = torch.zeros((1, 80, 3000))
    prompt = torch.tensor([G.prev_sot_token_id, 5, 6])
    for arg in (dict(prompt_ids=prompt), dict(condition_on_prev_tokens=True)):
        with pytest.raises(NotImplementedError, match="num_beams"):
            model.generate(f, language="ja", num_beams=2, **arg)
        with pytest.raises(NotImplementedError, match="return_token_timestamps"):
            model.generate(f, language="ja", return_token_timestamps=True, **arg)
        # with the fallback the arguments are built for the long-form loop; one window stays refused
        with pytest.raises(NotImplementedError, match="long-form"):
            model.generate(f, language="ja", temperature=(0.0, 0.2), logprob_threshold=-1.0, **arg)
    with pytest.raises(ValueError, match="rank-1"):
        model.generate(f, language="ja", prompt_ids=torch.zeros((2, 2), dtype=torch.long))


# ---- generate()'s host loop over a stub session -------------------------------------------------------------------------
TS = G.timestamp_begin
EOS = G.eos_token_id


def test_host_loop_conditions_each_pass_on_the_previous_ones():
    """Two clips (70 s and 35 s of frames), conditioning on: pass 1 has the bare init tokens and no mask; pass 2
    carries each row's text behind <|startofprev|>, left-padded, with the ending double timestamp counted once; in
    pass 3 the only row left is unpadded."""
    a1 = [TS, 100, 101, 102, TS + 1500, EOS]          # 30 s, a single ending timestamp: the window is consumed
    b1 = [TS, 200, TS + 1500, TS + 1500, EOS]  # a double ending timestamp
    a2 = [TS, 110, TS + 1500, EOS]
    b2 = [TS, 210, TS + 250, EOS]
    a3 = [TS, 120, TS + 500, EOS]
    model, sess = _stub_model([[a1, b1], [a2, b2], [a3]])
    mask = torch.zeros((2, 7000), dtype=torch.long)
    mask[0, :7000] = 1
    mask[1, :3500] = 1
    res = model.generate(torch.zeros((2, 80, 7000)), attention_mask=mask, language="ja", return_timestamps=True,
                         condition_on_prev_tokens=True, return_segments=True)
    sot = G.prev_sot_token_id
    p2 = sess.calls[1]["prompt"]
    assert sess.calls[0]["prompt"].tolist() == [INIT, INIT] and sess.calls[0]["key_start"] is None
    assert p2[0].tolist() == [sot] + a1[:-1] + INIT
    assert p2[1].tolist() == [G.pad_token_id] * 2 + [sot] + b1[:-2] + INIT
    assert list(sess.calls[1]["key_start"]) == [0, 2]
    assert sess.calls[2]["prompt"].tolist() == [[sot] + a1[:-1] + a2[:-1] + INIT]
    assert list(sess.calls[2]["key_start"]) == [0]
    assert model.stats["pass_P"] == [3, 9, 12] and model.stats["pass_key_start"] == [None, [0, 2], [0]]
    # max_length grows by min(223, P) per pass (:1935-1941), from the config's 448: capped at once
    assert [c["max_length"] for c in sess.calls] == [448, 448, 448]
    assert [len(s["tokens"]) for s in res["segments"][0]] == [5, 3, 3]


def test_first_segment_prompt_is_seeded_and_removed():
    """"first-segment" with conditioning: the prompt's text (without its <|startofprev|>) heads the first pass as a
    segment would, stays at the head of later passes' previous text, and is no part of the result."""
    a1 = [TS, 100, TS + 1500, EOS]
    a2 = [TS, 110, TS + 500, EOS]
    model, sess = _stub_model([[a1], [a2]])
    sot = G.prev_sot_token_id
    res = model.generate(torch.zeros((1, 80, 4000)), language="ja", return_timestamps=True, return_segments=True,
                         prompt_ids=torch.tensor([sot, 7, 8]), condition_on_prev_tokens=True)
    assert sess.calls[0]["prompt"].tolist() == [[sot, 7, 8] + INIT]
    assert sess.calls[1]["prompt"].tolist() == [[sot, 7, 8] + a1[:-1] + INIT]
    assert res["sequences"].tolist() == [a1[:-1] + a2[:-1]]
    # without conditioning the prompt goes on every pass, and no mask is passed
    model, sess = _stub_model([[a1], [a2]])
    model.generate(torch.zeros((1, 80, 4000)), language="ja", return_timestamps=True, prompt_ids=torch.tensor([sot, 7, 8]))
    assert [c["prompt"].tolist() for c in sess.calls] == [[[sot, 7, 8] + INIT]] * 2
    assert all(c["key_start"] is None for c in sess.calls)
