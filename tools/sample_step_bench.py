#!/usr/bin/env python
"""Cost of the decoding fallback's step tail and of a fallback attempt on the MI355X (development tool).

1. One decode step's tail at large-v3 shape (B = 32, V = 51866, d = 1280), device time per step from a replayed
   hipGraph: the greedy tails (kw_dec_lm_greedy without timestamps; kw_dec_linear(lm) + kw_greedy_step with) against
   kw_dec_linear(lm) + kw_sample_step at temperature 0 and 0.4, and the token kernels alone.
2. A whole decode of 32 rows (synthetic large-v3, bf16, max_length 128, timestamps): the greedy path, the statistics
   path at temperature 0, and a sampled attempt that re-decodes k of the 32 rows through ``active``.

    python tools/sample_step_bench.py [--reps 100] [--no-decode]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kotoba-whisper_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from kbench import timeit  # noqa: E402
from kwhisper import ops  # noqa: E402
from kwhisper.config import LARGE_V3, generation_constants  # noqa: E402


def tails(reps):
    B, V, K, P = 32, LARGE_V3.vocab_size, LARGE_V3.d_model, 3
    gen = generation_constants(LARGE_V3)
    dev = "cuda"
    W = (torch.randn(V, K, device=dev) / K ** 0.5).bfloat16()
    Wp, cs = ops.pack_weight(W), ops.ln_colsum(W)
    bias = torch.zeros(V, device=dev)
    x = (torch.randn(B, K, device=dev) * 2 + 0.3).bfloat16()
    sup = torch.zeros(V, dtype=torch.uint8, device=dev)
    sup[torch.tensor(gen.suppress_tokens, device=dev)] = 1
    bsup = torch.tensor(gen.begin_suppress_tokens, dtype=torch.int32, device=dev)
    out = {}

    def state():
        ids = torch.zeros((B, 449), dtype=torch.int64, device=dev)
        ids[:, :P] = torch.tensor([50258, 50266, 50360])
        return dict(ids=ids, cur=torch.tensor([P], dtype=torch.int32, device=dev),
                    unf=torch.ones(B, dtype=torch.int32, device=dev), cnt=torch.zeros(1, dtype=torch.int32, device=dev),
                    nun=torch.zeros(1, dtype=torch.int32, device=dev))

    def cfg(rt):
        return dict(return_timestamps=rt, ts_begin=gen.timestamp_begin, no_ts_id=gen.no_timestamps_token_id,
                    eos_id=gen.eos_token_id, pad_id=gen.pad_token_id, max_initial_ts=50 if rt else None, max_length=448,
                    begin_index=P)

    logits = torch.empty((B, V), device=dev)
    lm = ops.DecLinearPlan(x, Wp, B, V, K, ln=(1e-5, cs), bias=bias, C=logits)

    def sample_plan(rt, t):
        s = state()
        return ops.SamplePlan(logits, sup, bsup, s["ids"], s["cur"], s["unf"], s["cnt"], s["nun"],
                              inv_temperature=torch.tensor([1 / t if t else 0.0], device=dev),
                              seed=torch.tensor([7], dtype=torch.int64, device=dev),
                              attempt=torch.tensor([1], dtype=torch.int32, device=dev),
                              sum_logprob=torch.zeros(B, device=dev), n_tokens=torch.zeros(B, dtype=torch.int32, device=dev),
                              workspace=torch.zeros(ops.sample_step_workspace_bytes(B) // 4 + 1, device=dev), **cfg(rt))

    def greedy_plan(rt):
        s = state()
        return ops.SamplerPlan(logits, sup, bsup, s["ids"], s["cur"], s["unf"], s["cnt"], s["nun"],
                               workspace=torch.zeros(ops.greedy_step_workspace_bytes(B) // 4 + 1, device=dev), **cfg(rt))

    s = state()
    fused = ops.LmGreedyPlan(x, Wp, B, V, K, ln=(1e-5, cs), bias=bias, suppress_mask=sup, begin_suppress=bsup,
                             ids=s["ids"], cur_len=s["cur"], unfinished=s["unf"], n_unfinished=s["nun"],
                             eos_id=gen.eos_token_id, pad_id=gen.pad_token_id, max_length=448, begin_index=P,
                             workspace=torch.zeros(ops.lm_greedy_workspace_bytes(B, V) // 4 + 1, device=dev))
    lm()
    torch.cuda.synchronize()
    out["lm_greedy_fused_nots"] = timeit([fused], reps)
    out["lm_head"] = timeit([lm], reps)
    for rt in (False, True):
        tag = "ts" if rt else "nots"
        out[f"lm_head+greedy_{tag}"] = 2 * timeit([lm, greedy_plan(rt)], reps)
        out[f"greedy_{tag}"] = timeit([greedy_plan(rt)], reps)
        for t in (0.0, 0.4):
            out[f"lm_head+sample_{tag}_T{t}"] = 2 * timeit([lm, sample_plan(rt, t)], reps)
            out[f"sample_{tag}_T{t}"] = timeit([sample_plan(rt, t)], reps)
    return {k: round(v, 2) for k, v in out.items()}


def decodes():
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import synthetic_state_dict_torch

    B = 32
    gen = generation_constants(LARGE_V3)
    model = KWhisperForConditionalGeneration.from_state_dict(LARGE_V3, synthetic_state_dict_torch(LARGE_V3, 0),
                                                            dtype=torch.bfloat16, generation_config=gen)
    eng = model.engine
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = torch.randn(B, LARGE_V3.num_mel_bins, LARGE_V3.n_frames, device="cuda", generator=g) * 0.5
    sess = eng.new_session(B, eng.encode(feats))
    prompt = torch.tensor([[gen.decoder_start_token_id, gen.lang_to_id["<|ja|>"], gen.task_to_id["transcribe"]]] * B)
    out = {}

    def run(tag, **kw):
        for i in range(3):  # the first call captures the graphs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ids = sess.generate(prompt, gen, max_length=128, return_timestamps=True, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        out[tag] = dict(ms=round(dt * 1e3, 1), steps=int(sess.last_steps), length=int(ids.shape[1]))

    run("greedy")
    run("stats_T0", sample=dict(temperature=0.0))
    for k in (32, 8, 1):
        active = np.zeros(B, bool)
        active[:k] = True
        run(f"sampled_T0.4_active{k}", sample=dict(temperature=0.4, seed=7, attempt=1, active=active))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--no-decode", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "tails_us_per_step": tails(a.reps)}
    if not a.no_decode:
        res["decode_b32_large_v3"] = decodes()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
