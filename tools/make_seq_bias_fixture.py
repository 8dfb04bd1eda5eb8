"""tests/golden/seq_bias_tiny.npz: transformers' generate with ``sequence_bias`` and ``bad_words_ids`` on the seeded
tiny model (CPU, fp32), for tests/test_gpu_seq_bias.py.

  case a   greedy, no timestamps                                          (make_fixtures.FALLBACK_CLIPS' four clips)
  case a2  case a's call with other values of the same shape (the graph-reuse test runs a, a2, a)
  case b   greedy, timestamps, long-form make_fixtures.LONG_CLIPS: more than one seek pass
  case c   num_beams=3, timestamps                                        (the four clips)
  case d   long-form, condition_on_prev_tokens=True
  case e   a two-temperature fallback schedule                            (make_fixtures.fallback_features)
  case f   case a with repetition_penalty=1.3 and no_repeat_ngram_size=3 beside both arguments

A fixture of this kind passes vacuously if no entry ever applies, so a case's entries are cut, one after the other,
from the output of the same call with the entries before them (the first from the UNBIASED output, kept as
``{case}_base_*``), one per kind:
  len1      a length-1 boost on a text token z the model emitted late in some row;
  boost     a positive multi-token boost: (row 2's first generated token, z);
  ban2      a two-token ban: row 0's second and third generated tokens;
  ban3      a ban of three tokens that crosses the prompt boundary: the last prompt token and row 1's first two;
  shared    two entries sharing a last token: len1 and boost both end in z.
While the reference runs, SequenceBiasLogitsProcessor.__call__ is shadowed by a counter of the entries that apply
(tests/_seq_bias_ref.applies) per kind; the tool asserts that every kind fires in every case and that every case's
output differs from its unbiased output, and stores the counts (the test asserts them non-zero again).  Greedy cases
record the top-1 / top-2 margin of every step; the GPU test holds token ids equal without exception, so the tool takes
the first scale of the length-1 boost (SCALES) whose run has no live step under the fp32 logit bar of 1e-3.

    python tools/make_seq_bias_fixture.py            # about ten minutes
"""
import json
import os
import sys
import time

import numpy as np
import torch

from make_fixtures import (FALLBACK_CLIPS, FALLBACK_MAX_LENGTH, GOLD, LONG_CLIPS, ROOT, TINY, fallback_features,
                           fallback_run, features, hf_gen_config, hf_model, long_audio, run_generate)
from make_prompt_fixture import run_case
from make_repeat_fixture import first_attempt_tokens, rows_differ, short_greedy
from transformers import WhisperFeatureExtractor
from transformers.generation.logits_process import NoBadWordsLogitsProcessor, SequenceBiasLogitsProcessor

sys.path[:0] = [os.path.join(ROOT, "tests"), ROOT]  # (the restatement imports the oracle package)
import _seq_bias_ref as SR  # noqa: E402

MAX_LENGTH = 40
LEN1, BOOST = 2.0, 25.0
LEN1_2, BOOST_2 = 1.0, 30.0  # case a2
SCALES = (1.0, 0.75, 1.25, 0.5, 1.5, 0.875, 1.125, 0.625)  # of the length-1 boost: see first_ok
E_TEMPERATURES = (0.0, 0.4)
KINDS = ("len1", "ban2", "ban3", "boost", "shared")
_, GC = hf_gen_config(TINY)
EOS = GC.eos_token_id
PROMPT = [GC.decoder_start_token_id, GC.lang_to_id["<|ja|>"], GC.task_to_id["transcribe"]]


class Firing:
    """Counts, while installed, the entries that apply per kind over every row of every processor call."""

    def __init__(self, labels):
        self.labels, self.counts = labels, dict.fromkeys(KINDS, 0)
        inner = self.inner = SequenceBiasLogitsProcessor.__call__
        me = self

        def call(proc, input_ids, scores):
            bad = isinstance(proc, NoBadWordsLogitsProcessor)
            for row in input_ids.tolist():
                hit = [ids for ids in proc.sequence_bias if SR.applies(ids, row)]
                for ids in hit:
                    kind = me.labels.get((bad, tuple(ids)))
                    if kind:
                        me.counts[kind] += 1
                if not bad:
                    me.counts["shared"] += int(any(len(a) > 1 and (a[-1],) in hit for a in hit))
            return inner(proc, input_ids, scores)

        SequenceBiasLogitsProcessor.__call__ = call

    def close(self):
        SequenceBiasLogitsProcessor.__call__ = self.inner


def generated(row, skip=0):
    """A row's generated tokens up to its first EOS, without the forced prompt tokens a result may lead with."""
    forced = set(PROMPT) | {GC.no_timestamps_token_id}
    row = [int(t) for t in row]
    while row and row[0] in forced:
        row = row[1:]
    out = []
    for t in row:
        if t == EOS or t < 0:
            break
        out.append(t)
    return out


def derive(run, prompt_last, skip=0, len1=LEN1, boost=BOOST, shift=0):
    """The entries of a case, each cut from the output of the call with the entries before it (``run(kwargs)`` ->
    token matrix; the first run is the unbiased one), so that the prefix an entry waits for does occur when it is
    added -> (generate kwargs, labels, unbiased tokens).  ``shift``: take the banned tokens one step later (case a2:
    other values of the same shape; its three-token ban then lies inside the generated text)."""
    bias, bad, labels = {}, [], {}

    def kwargs():
        kw = {}
        if bias:
            kw["sequence_bias"] = [[list(k), v] for k, v in bias.items()]
        if bad:
            kw["bad_words_ids"] = [list(w) for w in bad]
        return kw

    def rows():
        toks = np.asarray(run(kwargs()))
        gen = [generated(r, skip) for r in toks]
        assert all(len(g) >= 4 + shift for g in gen), [len(g) for g in gen]
        return toks, gen

    base, gen = rows()
    B = len(gen)
    z = next(t for g in gen[::-1] for t in g[3:] if t < EOS and t not in gen[2 % B][:2])
    bias[(z,)] = len1
    labels[(False, (z,))] = "len1"
    _, gen = rows()
    g2 = gen[2 % B]
    bias[(g2[0], z)] = boost
    labels[(False, (g2[0], z))] = "boost"
    _, gen = rows()
    g1 = gen[1 % B]
    ban3 = (prompt_last, g1[0], g1[1]) if not shift else (g1[0], g1[1], g1[2])
    bad.insert(0, ban3)
    labels[(True, ban3)] = "ban3"
    # (the two-token ban last: the rows often start alike, and a ban added after it could keep row 0 off its prefix)
    _, gen = rows()
    ban2 = (gen[0][1 + shift], gen[0][2 + shift])
    bad.insert(0, ban2)
    labels[(True, ban2)] = "ban2"
    return kwargs(), labels, base


class LowMargin(Exception):
    pass


def first_ok(name, case):
    """``case(scale)`` with the first scale of the length-1 boost whose run has no step under the logit bar."""
    for scale in SCALES:
        try:
            return case(scale)
        except LowMargin as e:
            print(f"  {name}: length-1 boost x {scale}: {e}", flush=True)
    raise SystemExit(f"case {name}: every candidate has a low-margin step")


def live_margin(tokens, margin):
    """The margins of the steps that decide a token: +inf behind a row's first EOS (a finished row is padded)."""
    mg = np.array(margin, np.float32)
    toks = tokens[:, tokens.shape[1] - mg.shape[1]:]
    for r, row in enumerate(toks):
        hit = np.nonzero(row == EOS)[0]
        if hit.size:
            mg[r, hit[0] + 1:] = np.inf
    return mg


def checked(name, fire, got, base, margin=None, kinds=KINDS):
    d = rows_differ(np.asarray(got), np.asarray(base))
    low = None if margin is None else int((margin < 1e-3).sum())
    print(f"  {name}: fired {fire.counts}; rows that differ from the unbiased call {d.astype(int).tolist()}; "
          f"steps with a margin < 1e-3: {low}", flush=True)
    assert all(fire.counts[k] > 0 for k in kinds), f"case {name}: a kind never fired"
    assert d.any(), f"case {name}: the output is the unbiased output"
    if low:
        raise LowMargin(f"case {name}: a step's top-2 margin is under the fp32 logit bar")
    return np.array(json.dumps(fire.counts))


def with_firing(labels, fn):
    fire = Firing(labels)
    try:
        return fn(), fire
    finally:
        fire.close()


def main():
    t0 = time.time()
    m = hf_model(TINY)
    feats = features(TINY.num_mel_bins, FALLBACK_CLIPS)
    out = {"cases": np.array([f"{k}:{s}" for k, s in FALLBACK_CLIPS]), "max_length": MAX_LENGTH}
    args = {}

    # a, a2, f: short greedy without timestamps (the prompt ends in <|notimestamps|>)
    P = len(PROMPT) + 1
    for name, dkw, extra in (("a", dict(len1=LEN1, boost=BOOST), {}),
                             ("a2", dict(len1=LEN1_2, boost=BOOST_2, shift=1), {}),
                             ("f", dict(len1=LEN1, boost=BOOST), dict(repetition_penalty=1.3, no_repeat_ngram_size=3))):
        def case(scale, name=name, dkw=dkw, extra=extra):
            kw, labels, base = derive(lambda k: short_greedy(m, feats, **k, **extra)["tokens"],
                                      GC.no_timestamps_token_id, **dict(dkw, len1=dkw["len1"] * scale))
            args[name] = dict(kw, **extra)
            got, fire = with_firing(labels, lambda: short_greedy(m, feats, **args[name]))
            got["margin"] = live_margin(got["tokens"], got["margin"])
            # (a2's three-token ban sits inside the generated text: only case a's crosses the prompt boundary)
            out[f"{name}_fired"] = checked(name, fire, got["tokens"], base, got["margin"])
            out[f"{name}_tokens"], out[f"{name}_margin"], out[f"{name}_base_tokens"] = got["tokens"], got["margin"], base

        first_ok(name, case)
        print(f"  {name}: {args[name]} ({time.time() - t0:.1f}s)", flush=True)
    assert args["a"] != args["a2"] and rows_differ(out["a_tokens"], out["a2_tokens"]).any()

    # c: beams
    call = dict(language="ja", task="transcribe", return_timestamps=True, num_beams=3, max_length=MAX_LENGTH)

    def beams(k):
        m.generation_config, _ = hf_gen_config(TINY)
        return run_generate(m, feats, **call, **k).numpy().astype(np.int64)

    kw, labels, out["c_base_tokens"] = derive(beams, PROMPT[-1], skip=len(PROMPT))
    args["c"] = kw
    got, fire = with_firing(labels, lambda: beams(kw))
    out["c_fired"] = checked("c", fire, got, out["c_base_tokens"])
    out["c_tokens"] = got
    print(f"  c: {got.shape} ({time.time() - t0:.1f}s)", flush=True)

    # e: the fallback; the threshold is placed in the widest gap of the temperature-0 average log-probabilities
    ff = fallback_features()
    kw0 = dict(return_timestamps=True, temperature=E_TEMPERATURES)
    _, base_passes = fallback_run(m, ff, dict(kw0, logprob_threshold=-1.0e4), None)

    def attempt0(k):  # (a threshold nothing reaches: the temperature-0 attempt alone; the silent fifth row left out)
        return first_attempt_tokens(fallback_run(m, ff, dict(kw0, logprob_threshold=-1.0e4, **k), None)[1], ff.shape[0])[:4]

    akw, labels, _ = derive(attempt0, PROMPT[-1])
    base0 = first_attempt_tokens(base_passes, ff.shape[0])
    args["e"] = akw
    _, passes = fallback_run(m, ff, dict(kw0, logprob_threshold=-1.0e4, **akw), None)
    lp = np.sort(np.array(passes[0]["attempts"][0]["avg_logprob"]))
    gap = int(np.argmax(np.diff(lp)))
    thr = float(np.round((lp[gap] + lp[gap + 1]) / 2, 2))
    print(f"  e: temperature-0 avg_logprob {np.round(lp, 3).tolist()} -> logprob_threshold {thr}", flush=True)
    assert min(thr - lp[gap], lp[gap + 1] - thr) >= 0.05, "case e: no gap of 0.1 between the rows' log-probabilities"
    kw = dict(kw0, logprob_threshold=thr)
    (res, passes), fire = with_firing(labels, lambda: fallback_run(m, ff, dict(kw, **akw), None))
    at0 = passes[0]["attempts"][0]
    assert any(at0["needs_fallback"]) and not all(at0["needs_fallback"]), at0["needs_fallback"]
    out["e_fired"] = checked("e", fire, first_attempt_tokens(passes, ff.shape[0]), base0)
    out["e_kwargs"] = np.array(json.dumps(dict(kw, temperature=list(E_TEMPERATURES))))
    out["e_max_length"] = FALLBACK_MAX_LENGTH
    out["e_passes"], out["e_base_passes"] = np.array(json.dumps(passes)), np.array(json.dumps(base_passes))
    print(f"  e: first attempt falls back {at0['needs_fallback']} ({time.time() - t0:.1f}s)", flush=True)

    # b, d: long-form with timestamps (the prompt of a row's first pass ends in <|transcribe|>)
    fe = WhisperFeatureExtractor(feature_size=TINY.num_mel_bins)
    audio = [long_audio(k, s, sec) for k, s, sec in LONG_CLIPS]
    inp = fe(audio, sampling_rate=16000, return_tensors="pt", truncation=False, padding="longest",
             return_attention_mask=True)
    out["clips"] = np.array([f"{k}:{s}:{sec}" for k, s, sec in LONG_CLIPS])
    for name, extra in (("b", {}), ("d", dict(condition_on_prev_tokens=True))):
        def case(scale, name=name, extra=extra):
            kw, labels, base = derive(lambda k: run_case(m, inp, **extra, **k)[0]["sequences"], PROMPT[-1],
                                      len1=LEN1 * scale)
            args[name] = kw
            (res, _), fire = with_firing(labels, lambda: run_case(m, inp, **extra, **kw))
            out[f"{name}_fired"] = checked(name, fire, res["sequences"], base, res["margin"])
            out[f"{name}_sequences"], out[f"{name}_base_sequences"] = res["sequences"], base
            out[f"{name}_margin"] = res["margin"]
            out[f"{name}_segments"] = np.array(json.dumps(res["segments"]))
            out[f"{name}_passes"] = np.array(json.dumps(res["passes"]))
            assert len(res["passes"]) > 1, "one seek pass only"
            print(f"  {name}: {res['sequences'].shape} passes {[np.asarray(p['ids']).shape for p in res['passes']]} "
                  f"({time.time() - t0:.1f}s)", flush=True)

        first_ok(name, case)

    out["args"] = np.array(json.dumps(args))
    np.savez_compressed(os.path.join(GOLD, "seq_bias_tiny.npz"), **out)
    print(f"seq_bias_tiny fixtures done in {time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
