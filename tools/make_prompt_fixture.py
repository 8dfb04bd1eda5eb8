"""tests/golden/prompt_tiny.npz: transformers' long-form generate with ``prompt_ids`` and
``condition_on_prev_tokens`` on the seeded tiny model (CPU, fp32), for tests/test_prompt_cpu.py and
tests/test_prompt_gpu.py.

Every case runs the real ``generate`` over make_fixtures.LONG_CLIPS (batched, with the attention mask; case f: one
clip) with language "ja", timestamps and segments, and records
  * ``sequences`` and the segments as (start, end, token count);
  * every seek pass as ``_prepare_decoder_input_ids`` (generation_whisper.py:1853-1918) built it: the batch map, the
    ``decoder_input_ids``, the ``decoder_attention_mask`` (None where the reference passes none), the
    ``do_condition_on_prev_tokens`` list it was given and how many segments every audio had by then;
  * per output token the top-1 / top-2 margin of the processed scores of the step that produced it (greedy cases).

    python tools/make_prompt_fixture.py            # ~15 s per case
"""
import json
import os
import time

import numpy as np
import torch

from make_fixtures import GOLD, LONG_CLIPS, TINY, hf_gen_config, hf_model, long_audio, run_generate
from transformers import WhisperFeatureExtractor

# <|startofprev|> + 4 text tokens, as WhisperProcessor.get_prompt_ids returns them
PROMPT_TEXT = [500, 600, 700, 800]
# case e: the thresholds and the schedule found by the search below (the first candidate whose run has a pass where
# one row carries previous text and another only <|startofprev|>, having been accepted at a temperature >= 0.5)
FALLBACK_SEED = 11
FALLBACK_CANDIDATES = [
    dict(temperature=(0.0, 0.6), logprob_threshold=lp, compression_ratio_threshold=cr)
    for cr in (1.6, 1.8, 2.0, 2.4, 1.45, 1.35) for lp in (-20.0,)
] + [dict(temperature=(0.0, 0.6), logprob_threshold=lp) for lp in (-10.6, -10.7, -10.8, -10.5, -10.9, -10.4, -11.0)]


class PromptRecorder:
    """Shadows ``_prepare_decoder_input_ids`` on one model for one run and keeps what it was given and returned."""

    def __init__(self, m):
        self.m, self.passes = m, []
        inner = type(m)._prepare_decoder_input_ids

        def prepare(**kw):
            ids, kwargs = inner(**kw)
            mask = kwargs.get("decoder_attention_mask")
            self.passes.append(dict(
                rows=[int(i) for i in kw["batch_idx_map"]], ids=ids.tolist(),
                mask=None if mask is None else mask.long().tolist(),
                do_condition=[bool(x) for x in kw["do_condition_on_prev_tokens"]],
                nsegs=[len(x) for x in kw["current_segments"]]))
            return ids, kwargs

        m._prepare_decoder_input_ids = prepare

    def close(self):
        del self.m._prepare_decoder_input_ids


def margins(segs):
    """make_fixtures._aligned_margins with the prompt length of every pass taken from its own result."""
    groups = []
    for s in segs:
        if groups and groups[-1][0] is s["result"]:
            groups[-1][1].append(s)
        else:
            groups.append((s["result"], [s]))
    out = []
    for res, ss in groups:
        n = sum(len(s["tokens"]) for s in ss)
        sc = torch.stack(list(res["scores"]), 0).float()
        P = len(res["sequences"]) - sc.shape[0]
        assert torch.equal(sc[:n].argmax(-1), res["sequences"][P: P + n]), "greedy step != argmax of its scores"
        top = sc[:n].topk(2, -1).values
        out.append((top[:, 0] - top[:, 1]).numpy())
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def run_case(m, inp, greedy=True, **kw):
    m.generation_config, gc = hf_gen_config(TINY)
    rec = PromptRecorder(m)
    try:
        extra = dict(return_dict_in_generate=True, output_scores=True) if greedy else {}
        res = run_generate(m, inp["input_features"], attention_mask=inp.get("attention_mask"), language="ja",
                           return_timestamps=True, return_segments=True, **extra, **kw)
    finally:
        rec.close()
    toks = res["sequences"].numpy().astype(np.int64)
    out = {"sequences": toks,
           "segments": [[(float(x["start"]), float(x["end"]), len(x["tokens"])) for x in row] for row in res["segments"]],
           "passes": rec.passes}
    if greedy:
        mg = np.full(toks.shape, np.inf, np.float32)
        for b, segs in enumerate(res["segments"]):
            x = margins(segs)
            mg[b, : len(x)] = x
        out["margin"] = mg
    return out, gc


def mixed_pass(passes, n_init):
    """A pass where one row carries previous text and another only <|startofprev|> because its conditioning is off."""
    for p in passes:
        if p["mask"] is None:
            continue
        n = [sum(r) for r in p["mask"]]
        off = [not p["do_condition"][a] for a in p["rows"]]
        if any(k > 1 + n_init for k in n) and any(k == 1 + n_init and o for k, o in zip(n, off)):
            return True
    return False


def main():
    t0 = time.time()
    m = hf_model(TINY)
    fe = WhisperFeatureExtractor(feature_size=TINY.num_mel_bins)
    audio = [long_audio(k, s, sec) for k, s, sec in LONG_CLIPS]
    inp = fe(audio, sampling_rate=16000, return_tensors="pt", truncation=False, padding="longest",
             return_attention_mask=True)
    one = fe([audio[1]], sampling_rate=16000, return_tensors="pt", truncation=False, padding="longest")
    _, gc = hf_gen_config(TINY)
    prompt = torch.tensor([gc.prev_sot_token_id] + PROMPT_TEXT)
    cases = {
        "a": (inp, dict(condition_on_prev_tokens=True)),
        "b": (inp, dict(prompt_ids=prompt)),
        "c": (inp, dict(prompt_ids=prompt, prompt_condition_type="all-segments", condition_on_prev_tokens=True)),
        "d": (inp, dict(prompt_ids=prompt, prompt_condition_type="first-segment", condition_on_prev_tokens=True)),
        "f": (one, dict(condition_on_prev_tokens=True)),
    }
    out = {"clips": np.array([f"{k}:{s}:{sec}" for k, s, sec in LONG_CLIPS]), "prompt_ids": prompt.numpy(),
           "n_init": 3}
    for name, (x, kw) in cases.items():
        res, _ = run_case(m, x, **kw)
        out[f"{name}_sequences"], out[f"{name}_margin"] = res["sequences"], res["margin"]
        out[f"{name}_segments"] = np.array(json.dumps(res["segments"]))
        out[f"{name}_passes"] = np.array(json.dumps(res["passes"]))
        shapes = [np.asarray(p["ids"]).shape for p in res["passes"]]
        low = [(b, int((res["margin"][b] < 1e-3).sum())) for b in range(len(res["margin"]))]
        print(f"  {name}: {res['sequences'].shape} passes {shapes} margins < 1e-3 per row {low} "
              f"({time.time() - t0:.1f}s)", flush=True)
    for kw in FALLBACK_CANDIDATES:
        torch.manual_seed(FALLBACK_SEED)
        res, _ = run_case(m, inp, greedy=False, condition_on_prev_tokens=True, **kw)
        ok = mixed_pass(res["passes"], 3)
        print(f"  e: {kw} -> mixed pass {ok} ({time.time() - t0:.1f}s)", flush=True)
        if ok:
            out["e_sequences"] = res["sequences"]
            out["e_segments"] = np.array(json.dumps(res["segments"]))
            out["e_passes"] = np.array(json.dumps(res["passes"]))
            out["e_kwargs"] = np.array(json.dumps({k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}))
            out["e_seed"] = FALLBACK_SEED
            break
    else:
        raise SystemExit("case e: no candidate gave a pass with one conditioned and one fallen-back row")
    np.savez_compressed(os.path.join(GOLD, "prompt_tiny.npz"), **out)
    print(f"prompt_tiny fixtures done in {time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
