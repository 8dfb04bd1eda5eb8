"""GPU tests of prompt conditioning in generate(): ``prompt_ids``, ``prompt_condition_type`` and
``condition_on_prev_tokens`` on the tiny model against transformers (tests/golden/prompt_tiny.npz,
tools/make_prompt_fixture.py).

fp32 engine: sequences, segments and every pass's prompt length and key_start equal the fixture, up to the first step
whose top-2 margin in the fixture is under the fp32 logit bar of 1e-3 (at most one (case, row) may be cut short there:
tests/test_prompt_cpu.py checks the fixture for that).  bf16 engine: teacher-forced logits under a key_start against the
fp32 engine, at the tiny bf16 bar of test_gpu_generate.py.  The fp8-cache engine and the fallback run on their own
tokens and are checked against the restatement tests/_prompt_ref.py.
"""
import json

import numpy as np
import pytest
import torch

import _fallback_ref as FR
import _prompt_ref as R
from conftest import gpu_available

from kwhisper.config import TINY, generation_constants

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

G = generation_constants(TINY)
INIT = [G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"]]
CASES = ["a", "b", "c", "d", "f"]
LOGIT_BAR = 1e-3
LP_TOL = 2e-3  # avg_logprob: tests/test_fallback_gpu.py's bar (the fp32 logit bar on the token's score and the normaliser)


def _model(dtype, **kw):
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import synthetic_state_dict

    return KWhisperForConditionalGeneration.from_state_dict(TINY, synthetic_state_dict(TINY, 0), dtype=dtype,
                                                            generation_config=generation_constants(TINY), **kw)


@pytest.fixture(scope="module")
def tiny32():
    return _model(torch.float32)


@pytest.fixture(scope="module")
def inputs(gold):
    """The fixture's clips as oracle log-mel: (batched features, frame mask, the single clip of case f), on the GPU."""
    from _util import longform_inputs

    feats, mask, one = longform_inputs(gold("prompt_tiny")["clips"])
    return torch.from_numpy(feats).cuda(), torch.from_numpy(mask).cuda(), torch.from_numpy(one).cuda()


def _kwargs(g, case):
    kw = dict(R.CASE_KWARGS[case])
    if kw.get("prompt_ids"):
        kw["prompt_ids"] = torch.from_numpy(g["prompt_ids"])
    return kw


def _run(model, inputs, g, case, **extra):
    feats, mask, one = inputs
    kw = dict(_kwargs(g, case), **extra)
    model.record_pass_ids = True
    try:
        if case == "f":
            res = model.generate(one, language="ja", return_timestamps=True, return_segments=True, **kw)
        else:
            res = model.generate(feats, attention_mask=mask, language="ja", return_timestamps=True, return_segments=True,
                                 **kw)
    finally:
        model.record_pass_ids = False
    return res, model.stats


@pytest.mark.parametrize("case", CASES)
def test_fp32_generate_equals_transformers(gold, tiny32, inputs, case):
    g = gold("prompt_tiny")
    res, stats = _run(tiny32, inputs, g, case)
    want, segs, passes, _ = R.fixture_case(g, case)
    got = res["sequences"].cpu().numpy()
    margin = g[f"{case}_margin"]
    cut = {}
    for b in range(want.shape[0]):
        low = np.nonzero(margin[b] < LOGIT_BAR)[0]
        n = int(low[0]) if low.size else want.shape[1]
        if low.size:
            cut[b] = n
        np.testing.assert_array_equal(got[b, :n], want[b, :n], err_msg=f"case {case} row {b}")
    print(f"case {case}: rows compared only up to a low-margin step: {cut}")
    full = [b for b in range(want.shape[0]) if b not in cut]
    assert got.shape == want.shape or cut
    for b in full:
        assert [len(s["tokens"]) for s in res["segments"][b]] == [s[2] for s in segs[b]]
        if segs[b]:
            np.testing.assert_allclose([(s["start"], s["end"]) for s in res["segments"][b]], [s[:2] for s in segs[b]],
                                       atol=1e-9)
    if not cut:
        # every pass: the running rows, the prompt length and the per-row first key are transformers'
        assert [p[0] for p in stats["pass_log"]] == [p["rows"] for p in passes]
        assert stats["pass_P"] == [len(p["ids"][0]) for p in passes]
        assert stats["pass_key_start"] == [R.key_start_of(p["mask"]) for p in passes]
        for (ids, cond), p in zip(stats["pass_prompt"], passes):
            assert ids.tolist() == p["ids"] and cond == p["do_condition"]


def _replay(stats, gen, prompt_ids=None, seeded=False, skipped=()):
    """Every pass's prompt and key_start from the engine's own decoded ids of the passes before it, by the
    restatement: (ids, key_start) per pass."""
    from kwhisper.generation import _retrieve_segment, _strip_pass_row

    B = int(max(max(rows) for rows, _, _ in stats["pass_log"])) + 1
    seed = None
    if seeded:
        pt = [int(t) for t in prompt_ids]
        seed = pt[1:] if pt[0] == gen.prev_sot_token_id else pt
    segments = [[seed] if seeded else [] for _ in range(B)]
    out = []
    for k, ((rows, seeks, frames), ids, (prompt, cond)) in enumerate(zip(stats["pass_log"], stats["pass_ids"],
                                                                         stats["pass_prompt"])):
        out.append(R.pass_input(INIT, segments, rows, cond, prompt_ids, pad=gen.pad_token_id,
                                prev_sot=gen.prev_sot_token_id, ts_begin=gen.timestamp_begin))
        P = prompt.shape[1]
        for i, a in enumerate(rows):
            if (k, a) in skipped:
                continue
            seq = _strip_pass_row(ids[i, P:], gen.pad_token_id, gen.eos_token_id)
            segs, _ = _retrieve_segment(seq, gen.timestamp_begin, frames[i], 0.0)
            segments[a] += [[int(t) for t in s["tokens"]] for s in segs]
    return out


def _check_replay(stats, gen, **kw):
    masked = 0
    for (ids, ks), (prompt, _), got_ks, P in zip(_replay(stats, gen, **kw), stats["pass_prompt"], stats["pass_key_start"],
                                                 stats["pass_P"]):
        assert prompt.tolist() == ids and got_ks == ks and P == len(ids[0])
        masked += bool(ks and any(ks))
    return masked


def test_bf16_masked_logits_against_fp32(gold, tiny32, inputs):
    """teacher_forced_logits(key_start=...) along pass 2 of case a (two rows, one left-padded by far more than a
    tile): the bf16 engine against the fp32 engine on the same tokens, top 8 of every step; the tiny bf16 bar (max
    0.25, mean 0.03).  The fp32 engine's own first steps are the fixture's tokens (its generate test), so it stands
    for the reference here."""
    g = gold("prompt_tiny")
    _, _, passes, toks = R.fixture_case(g, "a")
    p = passes[1]
    ks = R.key_start_of(p["mask"])
    assert len(p["rows"]) == 2 and max(ks) > 64 and min(ks) == 0
    nxt = passes[2]["nsegs"] if len(passes) > 2 else [len(t) for t in toks]
    body = [sum(toks[a][p["nsegs"][a]: nxt[a]], []) for a in p["rows"]]
    # each row is fed its own tokens of that pass (the shorter one filled up with EOS) and compared on the steps that
    # predict them and the one after: the prefill's last position and every fed token of the row
    T = max(len(b) for b in body)
    assert min(len(b) for b in body) >= 2
    seq = torch.tensor([row + b + [G.eos_token_id] * (T - len(b)) for row, b in zip(p["ids"], body)], dtype=torch.int64)
    valid = torch.tensor([[t <= len(b) for t in range(T + 1)] for b in body])
    P = len(p["ids"][0])
    feats, mask, _ = inputs
    # the window pass 2 decoded: each row's 30 s from its seek (the fp32 run's log has the fixture's seeks)
    _run(tiny32, inputs, g, "a")
    rows, seeks, frames = tiny32.stats["pass_log"][1]
    assert rows == p["rows"]
    seg = torch.zeros((2, feats.shape[1], 3000), device="cuda")
    for i, a in enumerate(rows):
        seg[i, :, : frames[i]] = feats[a, :, seeks[i]: seeks[i] + frames[i]]
    out = {}
    for name, model in (("f32", tiny32), ("bf16", _model(torch.bfloat16))):
        eng = model.engine
        sess = eng.new_session(2, eng.encode(seg))
        out[name] = sess.teacher_forced_logits(seq, P, key_start=ks).float().cpu()
        assert torch.isfinite(out[name]).all()
    idx = out["f32"].topk(8, -1).indices
    err = (out["bf16"].gather(-1, idx) - out["f32"].gather(-1, idx)).abs()[valid].numpy()
    print("tiny bf16 masked teacher-forced top-8 logit err: max %.4f mean %.4f over %d values" % (err.max(), err.mean(),
                                                                                                  err.size))
    assert err.max() < 0.25 and err.mean() < 0.03
    # the mask matters: the same tokens without key_start give other logits for the padded row only
    sess = tiny32.engine.new_session(2, tiny32.engine.encode(seg))
    plain = sess.teacher_forced_logits(seq, P).float().cpu()
    pad_row = int(np.argmax(ks))
    assert torch.equal(plain[1 - pad_row], out["f32"][1 - pad_row])
    assert (plain[pad_row] - out["f32"][pad_row])[valid[pad_row]].abs().max() > 10 * LOGIT_BAR


def test_fp8_cache_engine_runs_case_a(gold, inputs):
    """Conditioning over the fp8 cross cache (cross-attention is unchanged by the mask): case a end to end; the result
    is well formed and every pass's prompt and key_start are the restatement's for the engine's own tokens."""
    g = gold("prompt_tiny")
    model = _model(torch.bfloat16, cross_kv_dtype="fp8_e4m3")
    res, stats = _run(model, inputs, g, "a")
    seqs = res["sequences"].cpu().numpy()
    assert seqs.shape[0] == 3 and ((seqs >= 0) & (seqs < TINY.vocab_size)).all()
    assert all(np.isfinite([s["start"], s["end"]]).all() for row in res["segments"] for s in row)
    assert stats["passes"] >= 3 and max(stats["pass_P"]) > 8
    assert _check_replay(stats, G) >= 1  # at least one pass ran masked


def test_fallback_with_conditioning(gold, tiny32, inputs):
    """Case e, the fallback's schedule and thresholds with conditioning.  Sampled tokens are the engine's own, so (as
    tests/test_fallback_gpu.py does) the decisions are checked against the recorded numbers, and on top: a row
    accepted at a temperature >= 0.5 carries only <|startofprev|> in its next pass, every other row its previous
    text, and every pass's prompt and key_start are the restatement's for the engine's own tokens."""
    g = gold("prompt_tiny")
    kw = json.loads(str(g["e_kwargs"]))
    kw["temperature"] = tuple(kw["temperature"])
    tiny32.manual_seed(7)
    res, stats = _run(tiny32, inputs, g, "a", **kw)
    thr = {k: kw.get(k) for k in ("compression_ratio_threshold", "logprob_threshold", "no_speech_threshold")}
    cond = [True] * 3
    skipped = set()
    fell = 0
    for k, (ps, (prompt, cond_k)) in enumerate(zip(stats["fallback"], stats["pass_prompt"])):
        assert cond_k == cond, k  # what the pass was built with follows from the attempts before it
        for at in ps:
            for j, a in enumerate(at["rows"]):
                want = FR.need_fallback(compression=at["compression_ratio"][j], avg_lp=at["avg_logprob"][j],
                                        no_speech_prob=at["no_speech_prob"][j], **thr)
                assert (at["needs_fallback"][j], at["should_skip"][j]) == want
                cond[a] = at["temperature"] < 0.5
                if at["should_skip"][j]:
                    skipped.add((k, a))
        fell += any(not c for c in cond)
    assert fell, "no row was accepted at a temperature >= 0.5: the case does not exercise the rule"
    assert _check_replay(stats, G, skipped=skipped) >= 1
    # a pass in which a row lost its conditioning: that row is <|startofprev|> + init behind its pads
    seen = False
    for (prompt, cond_k), rows in zip(stats["pass_prompt"], [p[0] for p in stats["pass_log"]]):
        for i, a in enumerate(rows):
            if not cond_k[a] and prompt.shape[1] > 4:
                assert prompt[i, -4:].tolist() == [G.prev_sot_token_id] + INIT
                assert (prompt[i, :-4] == G.pad_token_id).all()
                seen = True
    print(f"case e on the engine: {stats['passes']} passes, P {stats['pass_P']}, key_start {stats['pass_key_start']}, "
          f"a row without conditioning in a padded pass: {seen}")
    assert seen, "no padded pass held a row without conditioning"
    # the sampled attempts' log-probabilities (tests/test_fallback_gpu.py's method): every row accepted from a sampled
    # attempt is teacher-forced along its own tokens -- here through the fp32 engine's greedy plans under the pass's
    # key_start, the path the fixture test holds to transformers -- and the pinned processors; the reported
    # avg_logprob is that reference's within the fp32 bar, and every sampled token has a finite processed score
    from oracle.generate import process_logits

    feats = inputs[0]
    gd, eng = G.to_dict(), tiny32.engine
    checked = masked_checked = 0
    for k, ps in enumerate(stats["fallback"]):
        last = ps[-1]
        if last["temperature"] <= 0.0:
            continue
        rows, seeks, frames = stats["pass_log"][k]
        ids, P, ks = stats["pass_ids"][k], stats["pass_P"][k], stats["pass_key_start"][k]
        seg = torch.zeros((len(rows), feats.shape[1], 3000), device="cuda")
        for i, a in enumerate(rows):
            seg[i, :, : frames[i]] = feats[a, :, seeks[i]: seeks[i] + frames[i]]
        sess = eng.new_session(len(rows), eng.encode(seg))
        logits = sess.teacher_forced_logits(torch.from_numpy(ids), P, key_start=ks).float().cpu().numpy()
        for j, a in enumerate(last["rows"]):
            i = rows.index(a)
            body = FR.strip_padding(ids[i, P:], G.pad_token_id, G.eos_token_id)
            total = 0.0
            for t in range(len(body)):
                sc = process_logits(ids[i: i + 1, : P + t], logits[i, t][None], gd, P, True)[0]
                assert np.isfinite(sc[body[t]]), (k, a, t)
                total += FR.log_softmax64(sc)[body[t]]
            print(f"   pass {k} row {a}: {len(body)} sampled tokens, avg_logprob {last['avg_logprob'][j]:.4f} "
                  f"reference {total / len(body):.4f} (key_start {None if ks is None else ks[i]})")
            assert abs(last["avg_logprob"][j] - total / len(body)) <= LP_TOL
            checked += 1
            masked_checked += bool(ks and any(ks))
    assert checked >= 1 and masked_checked >= 1, (checked, masked_checked)


def test_unmasked_pass_after_a_masked_one_is_a_fresh_session(tiny32, inputs):
    """One session: a masked pass with a long prompt, then an unmasked one -- the unmasked pass gives the tokens of a
    session that never ran masked (plan and graph keys, the key_start buffer, buffer reuse).  Two more prompt lengths
    then push the first one's prefill buffers, plans and graphs out; asked again, it gives its first result."""
    feats, _, _ = inputs
    eng = tiny32.engine
    enc = eng.encode(feats[:2, :, :3000].contiguous()).clone()
    short = torch.tensor([INIT, INIT], dtype=torch.int64)
    text = list(range(1000, 1040))

    def padded(n0, n1):
        ids, ks = R.pass_input(INIT, [[text[:n0]], [text[:n1]]], [0, 1], [True, True], None, pad=G.pad_token_id,
                               prev_sot=G.prev_sot_token_id, ts_begin=G.timestamp_begin)
        return torch.tensor(ids), ks

    (ids44, ks44), (ids24, ks24), (ids34, ks34) = padded(40, 7), padded(20, 3), padded(30, 29)
    assert (ks44, ks24, ks34) == ([0, 33], [0, 17], [0, 1]) and ids44.shape[1] == 44
    kw = dict(max_length=64, return_timestamps=True)
    fresh = eng.new_session(2, enc).generate(short, G, **kw)
    fresh44 = eng.new_session(2, enc).generate(ids44, G, key_start=ks44, **kw)
    sess = eng.new_session(2, enc)
    m1 = sess.generate(ids44, G, key_start=ks44, **kw)
    np.testing.assert_array_equal(m1, fresh44)
    np.testing.assert_array_equal(sess.generate(short, G, **kw), fresh)
    sess.generate(ids24, G, key_start=ks24, **kw)
    sess.generate(ids34, G, key_start=ks34, **kw)
    assert sess._long_q == [24, 34] and 44 not in sess._bufs and not any(k[0] == 44 for k in sess._plans)
    np.testing.assert_array_equal(sess.generate(ids44, G, key_start=ks44, **kw), m1)
    np.testing.assert_array_equal(sess.generate(short, G, **kw), fresh)
    assert len(sess._long_q) == sess.LONG_KEEP


def test_pipeline_and_pseudo_label_take_prompt_ids(inputs):
    """ASRPipeline's generate_kwargs and pseudo_label's gen_kwargs hand prompt_ids to generate(): the prompt shows in
    the pass's prompt length."""
    from _util import OracleFeatureExtractor, StubTok
    from kwhisper.pipeline import ASRPipeline
    from kwhisper.pseudo_label import pseudo_label
    from kwhisper.synthetic import dummy_audio

    model = _model(torch.bfloat16)
    prompt = torch.tensor([G.prev_sot_token_id, 1012, 2044])
    pipe = ASRPipeline(model, feature_extractor=OracleFeatureExtractor(TINY.num_mel_bins),
                       tokenizer=StubTok(generation_constants(TINY)), chunk_length_s=15, batch_size=2,
                       generate_kwargs=dict(prompt_ids=prompt, language="ja", task="transcribe", max_new_tokens=12,
                                            num_beams=1))  # (the pipeline's default is 5 beams: refused with a prompt)
    out = pipe({"array": dummy_audio(0)[: 16000 * 20], "sampling_rate": 16000})
    assert isinstance(out["text"], str) and model.stats["pass_P"][0] == 3 + 4
    feats = inputs[0][:2, :, :3000].contiguous()
    model.stats = {}
    ids, preds = pseudo_label(model, lambda idx: feats[list(idx)], 2, batch_size=2, pad_token_id=50257,
                              gen_kwargs=dict(prompt_ids=prompt, language="ja", task="transcribe", max_length=24))
    assert list(ids) == [0, 1] and len(preds) == 2 and model.stats["pass_P"][0] == 3 + 4


def test_generate_multitask_memo_with_a_prompt(tiny32, inputs):
    """generate_multitask's shared-encoder memo holds the first pass's encoder output and cross K/V only, which a
    prompt does not touch: with prompt_ids every task's result is the separate generate() call's."""
    feats = inputs[0][:2, :, :3000].contiguous()
    prompt = torch.tensor([G.prev_sot_token_id, 500, 600])
    tasks = [("ja", "transcribe"), ("en", "translate")]
    kw = dict(prompt_ids=prompt, return_timestamps=True, max_length=40)
    want = [tiny32.generate(feats, language=l, task=t, **kw).cpu() for l, t in tasks]
    got = tiny32.generate_multitask(feats, tasks, **kw)
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b)
    assert tiny32.stats["pass_P"][0] == 3 + 3
