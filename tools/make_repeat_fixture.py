"""tests/golden/repeat_tiny.npz: transformers' generate with ``repetition_penalty`` and ``no_repeat_ngram_size`` on
the seeded tiny model (CPU, fp32), for tests/test_repeat_cpu.py and tests/test_gpu_repeat.py.

  case a  greedy, no timestamps, repetition_penalty=1.3                       (make_fixtures.FALLBACK_CLIPS' four clips)
  case b  greedy, timestamps, no_repeat_ngram_size=3                          (the same clips)
  case c  both, num_beams=3, timestamps                                       (the same clips)
  case d  long-form make_fixtures.LONG_CLIPS, condition_on_prev_tokens=True, both (the first of D_CANDIDATES that
          leaves at most one row with a low-margin step: (1.2, 3); the values used are stored under ``args``)
  case e  a two-temperature fallback schedule with both                       (make_fixtures.fallback_features)

Every case also runs the same call WITHOUT the two arguments (``{case}_base_*``).  The fixture is only worth something
if the arguments change the result, so the tool asserts that in every case at least half of the rows differ from their
no-argument tokens (tests/test_repeat_cpu.py asserts it again on the file).  Greedy cases record, per output token, the
top-1 / top-2 margin of the processed scores of the step that produced it.  Case e's log-probability threshold is
placed by the tool in the widest gap of the rows' temperature-0 average log-probabilities (so that some rows fall back
and some do not, every row at least 0.05 from the threshold) and stored with the case.

    python tools/make_repeat_fixture.py            # about two minutes
"""
import json
import os
import time

import numpy as np
import torch

from make_fixtures import (FALLBACK_CLIPS, FALLBACK_MAX_LENGTH, GOLD, LONG_CLIPS, TINY, fallback_features, fallback_run,
                           features, hf_gen_config, hf_model, long_audio, run_generate)
from make_prompt_fixture import run_case
from transformers import WhisperFeatureExtractor

PENALTY, NGRAM = 1.3, 3
MAX_LENGTH = 40
ARGS = {
    "a": dict(repetition_penalty=PENALTY),
    "b": dict(no_repeat_ngram_size=NGRAM),
    "c": dict(repetition_penalty=PENALTY, no_repeat_ngram_size=NGRAM),
    "d": dict(repetition_penalty=PENALTY, no_repeat_ngram_size=NGRAM),
    "e": dict(repetition_penalty=PENALTY, no_repeat_ngram_size=NGRAM),
}
E_TEMPERATURES = (0.0, 0.4)
# case d: the first (penalty, n) whose run has at most one row with a step whose top-2 margin is under the fp32 logit
# bar of 1e-3 (tests/test_gpu_repeat.py compares a row only up to such a step, and allows one such row in all)
D_CANDIDATES = [(1.3, 3), (1.2, 3), (1.5, 3), (1.3, 4), (1.2, 4), (1.5, 4), (1.3, 2), (1.1, 3)]


def rows_differ(a, b):
    """Per row, whether two right-padded token matrices differ (the shorter one padded with -1)."""
    n = max(a.shape[1], b.shape[1])
    pa, pb = np.full((a.shape[0], n), -1, np.int64), np.full((b.shape[0], n), -1, np.int64)
    pa[:, : a.shape[1]], pb[:, : b.shape[1]] = a, b
    return (pa != pb).any(1)


def enough(name, a, b):
    d = rows_differ(a, b)
    print(f"  {name}: rows that differ from the no-argument call: {d.astype(int).tolist()}", flush=True)
    assert 2 * int(d.sum()) >= len(d), f"case {name}: fewer than half of the rows differ; change its penalty / n"


def short_greedy(m, feats, **kw):
    """One short-form greedy call without timestamps: the plain call's tokens and the per-step margins."""
    m.generation_config, _ = hf_gen_config(TINY)
    call = dict(language="ja", task="transcribe", return_timestamps=False, max_length=MAX_LENGTH, **kw)
    res = run_generate(m, feats, return_dict_in_generate=True, output_scores=True, **call)
    seq = res["sequences"]
    sc = torch.stack(list(res["scores"]), 1).float()  # (B, T, V) processed
    assert torch.equal(sc.argmax(-1), seq[:, seq.shape[1] - sc.shape[1]:]), "greedy step != argmax of its scores"
    top = sc.topk(2, -1).values
    m.generation_config, _ = hf_gen_config(TINY)
    return dict(tokens=run_generate(m, feats, **call).numpy().astype(np.int64),
                margin=(top[..., 0] - top[..., 1]).numpy().astype(np.float32))


def first_attempt_tokens(passes, n_rows):
    """row -> the tokens of its temperature-0 attempt in the first pass."""
    at = passes[0]["attempts"][0]
    assert at["temperature"] == 0.0 and at["rows"] == list(range(n_rows))
    n = max(len(t) for t in at["tokens"])
    out = np.full((n_rows, n), -1, np.int64)
    for r, t in enumerate(at["tokens"]):
        out[r, : len(t)] = t
    return out


def main():
    t0 = time.time()
    m = hf_model(TINY)
    feats = features(TINY.num_mel_bins, FALLBACK_CLIPS)
    out = {"cases": np.array([f"{k}:{s}" for k, s in FALLBACK_CLIPS]), "max_length": MAX_LENGTH,
           "args": np.array(json.dumps(ARGS))}
    got, base = short_greedy(m, feats, **ARGS["a"]), short_greedy(m, feats)
    enough("a", got["tokens"], base["tokens"])
    out["a_tokens"], out["a_margin"], out["a_base_tokens"] = got["tokens"], got["margin"], base["tokens"]
    low = [int((got["margin"][b] < 1e-3).sum()) for b in range(len(got["margin"]))]
    print(f"  a: {got['tokens'].shape} margins < 1e-3 per row {low} ({time.time() - t0:.1f}s)", flush=True)

    # case b, with timestamps: through the segment loop (sequences without the prompt, segments, aligned margins)
    short = {"input_features": feats}
    res, _ = run_case(m, short, max_length=MAX_LENGTH, **ARGS["b"])
    base, _ = run_case(m, short, max_length=MAX_LENGTH)
    enough("b", res["sequences"], base["sequences"])
    out["b_sequences"], out["b_margin"], out["b_base_sequences"] = res["sequences"], res["margin"], base["sequences"]
    out["b_segments"] = np.array(json.dumps(res["segments"]))
    low = [int((res["margin"][b] < 1e-3).sum()) for b in range(len(res["margin"]))]
    print(f"  b: {res['sequences'].shape} margins < 1e-3 per row {low} ({time.time() - t0:.1f}s)", flush=True)

    call = dict(language="ja", task="transcribe", return_timestamps=True, num_beams=3, max_length=MAX_LENGTH)
    m.generation_config, _ = hf_gen_config(TINY)
    out["c_tokens"] = run_generate(m, feats, **call, **ARGS["c"]).numpy().astype(np.int64)
    m.generation_config, _ = hf_gen_config(TINY)
    out["c_base_tokens"] = run_generate(m, feats, **call).numpy().astype(np.int64)
    enough("c", out["c_tokens"], out["c_base_tokens"])
    print(f"  c: {out['c_tokens'].shape} ({time.time() - t0:.1f}s)", flush=True)

    fe = WhisperFeatureExtractor(feature_size=TINY.num_mel_bins)
    audio = [long_audio(k, s, sec) for k, s, sec in LONG_CLIPS]
    inp = fe(audio, sampling_rate=16000, return_tensors="pt", truncation=False, padding="longest",
             return_attention_mask=True)
    out["clips"] = np.array([f"{k}:{s}:{sec}" for k, s, sec in LONG_CLIPS])
    for pen, n in D_CANDIDATES:
        ARGS["d"] = dict(repetition_penalty=pen, no_repeat_ngram_size=n)
        res, _ = run_case(m, inp, condition_on_prev_tokens=True, **ARGS["d"])
        low = [np.nonzero(res["margin"][b] < 1e-3)[0].tolist() for b in range(len(res["margin"]))]
        print(f"  d: {ARGS['d']} -> steps with a margin < 1e-3 per row {low} ({time.time() - t0:.1f}s)", flush=True)
        if sum(bool(x) for x in low) <= 1:
            break
    else:
        raise SystemExit("case d: every candidate has two rows with a low-margin step")
    out["args"] = np.array(json.dumps(ARGS))
    base, _ = run_case(m, inp, condition_on_prev_tokens=True)
    enough("d", res["sequences"], base["sequences"])
    out["d_sequences"], out["d_margin"], out["d_base_sequences"] = res["sequences"], res["margin"], base["sequences"]
    out["d_segments"] = np.array(json.dumps(res["segments"]))
    out["d_passes"] = np.array(json.dumps(res["passes"]))
    low = [int((res["margin"][b] < 1e-3).sum()) for b in range(len(res["margin"]))]
    print(f"  d: {res['sequences'].shape} passes {[np.asarray(p['ids']).shape for p in res['passes']]} margins < 1e-3 "
          f"per row {low} ({time.time() - t0:.1f}s)", flush=True)

    # case e: first with a threshold nothing reaches, to see the rows' temperature-0 average log-probabilities
    ff = fallback_features()
    probe = dict(return_timestamps=True, temperature=E_TEMPERATURES, logprob_threshold=-1.0e4, **ARGS["e"])
    _, passes = fallback_run(m, ff, probe, None)
    lp = np.sort(np.array(passes[0]["attempts"][0]["avg_logprob"]))
    gap = int(np.argmax(np.diff(lp)))
    thr = float(np.round((lp[gap] + lp[gap + 1]) / 2, 2))
    print(f"  e: temperature-0 avg_logprob {np.round(lp, 3).tolist()} -> logprob_threshold {thr}", flush=True)
    assert min(thr - lp[gap], lp[gap + 1] - thr) >= 0.05, "case e: no gap of 0.1 between the rows' log-probabilities"
    kw = dict(return_timestamps=True, temperature=E_TEMPERATURES, logprob_threshold=thr)
    res, passes = fallback_run(m, ff, dict(kw, **ARGS["e"]), None)
    base, base_passes = fallback_run(m, ff, kw, None)
    at0 = passes[0]["attempts"][0]
    assert any(at0["needs_fallback"]) and not all(at0["needs_fallback"]), at0["needs_fallback"]
    assert all(abs(x - thr) >= 0.05 for ps in passes for x in ps["attempts"][0]["avg_logprob"])
    enough("e", first_attempt_tokens(passes, ff.shape[0]), first_attempt_tokens(base_passes, ff.shape[0]))
    out["e_kwargs"] = np.array(json.dumps(dict(kw, temperature=list(E_TEMPERATURES))))
    out["e_max_length"] = FALLBACK_MAX_LENGTH
    out["e_sequences"], out["e_base_sequences"] = (x["sequences"].numpy().astype(np.int64) for x in (res, base))
    out["e_passes"], out["e_base_passes"] = np.array(json.dumps(passes)), np.array(json.dumps(base_passes))
    print(f"  e: {out['e_sequences'].shape} first attempt falls back {at0['needs_fallback']} "
          f"({time.time() - t0:.1f}s)", flush=True)
    np.savez_compressed(os.path.join(GOLD, "repeat_tiny.npz"), **out)
    print(f"repeat_tiny fixtures done in {time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
