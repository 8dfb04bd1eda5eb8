#!/usr/bin/env python
"""Prompt-conditioning timings on the MI355X at the large-v3 shape, bf16 (profiles/prompt_measure.json
is one run).  Prints one JSON line.

  * prefill self-attention, B = 32, q_len 228, 32 layers' worth of launches over 32 distinct caches: kw_self_attn_step
    (one workgroup per (row, head) walking the queries) against kw_self_attn_step_masked in both forms (one workgroup
    per query position; the MFMA tile kernel), with key_start zero and with half the rows at 160;
  * the whole prefill at that length, unmasked and masked;
  * the graph-replayed decode step of an unmasked session (fused self block) against a masked one (kw_dec_linear(qkv) +
    kw_self_attn_step_masked), at positions 230-250;
  * one long-form batch, 8 clips of 70 s, with and without condition_on_prev_tokens: audio seconds per second.

    python tools/prompt_measure.py [--skip-e2e]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kotoba-whisper_amd")]
from kwhisper import ops  # noqa: E402
from kwhisper.config import PRESETS  # noqa: E402
from kwhisper.feature_extraction import WhisperFeatureExtractor  # noqa: E402
from kwhisper.generation import KWhisperForConditionalGeneration  # noqa: E402
from kwhisper.synthetic import dummy_audio, synthetic_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--skip-e2e", action="store_true")
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda:0")
shape = PRESETS["large-v3"]
B, Q, H, HD, T_MAX, NL = 32, 228, shape.decoder_attention_heads, 64, 448, shape.decoder_layers
out = {"B": B, "q_len": Q, "layers": NL}


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        res.append(e0.elapsed_time(e1))
    return res


# ---- the prefill self-attention kernels --------------------------------------------------------------------------------
d = H * HD
g = torch.Generator(device=dev).manual_seed(0)
qkv = [(torch.randn(B * Q, 3 * d, device=dev, generator=g) * 0.5).bfloat16() for _ in range(4)]
kc = torch.zeros(NL, B, H, T_MAX, HD, device=dev, dtype=torch.bfloat16)
vc = torch.zeros_like(kc)
attn = torch.empty(B * Q, d, device=dev, dtype=torch.bfloat16)
cur = torch.tensor([Q], device=dev, dtype=torch.int32)
ks0 = torch.zeros(B, device=dev, dtype=torch.int32)
ks_half = torch.tensor([160 if b % 2 else 0 for b in range(B)], device=dev, dtype=torch.int32)


def serial():
    for li in range(NL):
        ops.self_attn_step(qkv[li % 4], B, Q, H, HD, kc[li], vc[li], T_MAX, cur, attn)


def masked(ks, per_query=False):
    def run():
        for li in range(NL):
            ops.self_attn_step_masked(qkv[li % 4], B, Q, H, HD, kc[li], vc[li], T_MAX, cur, ks, attn, per_query=per_query)
    return run


out["prefill_self_attn_ms_32_layers"] = {
    "kw_self_attn_step": event_ms(serial, a.reps),
    "per_query_key_start_0": event_ms(masked(ks0, True), a.reps),
    "per_query_half_rows_160": event_ms(masked(ks_half, True), a.reps),
    "mfma_tile_key_start_0": event_ms(masked(ks0), a.reps),
    "mfma_tile_half_rows_160": event_ms(masked(ks_half), a.reps),
    "kw_self_attn_step_again": event_ms(serial, a.reps),
}
ref = torch.empty_like(attn)
ops.self_attn_step(qkv[0], B, Q, H, HD, kc[0], vc[0], T_MAX, cur, ref)
ops.self_attn_step_masked(qkv[0], B, Q, H, HD, kc[0], vc[0], T_MAX, cur, ks0, attn, per_query=True)
out["per_query_key_start_0_bitwise_equal"] = bool(torch.equal(ref, attn))
ops.self_attn_step_masked(qkv[0], B, Q, H, HD, kc[0], vc[0], T_MAX, cur, ks0, attn)
out["mfma_tile_key_start_0_max_abs_diff"] = float((ref.float() - attn.float()).abs().max())
del qkv, kc, vc, attn, ref
print(json.dumps(out), flush=True)

# ---- the whole prefill and the decode step ------------------------------------------------------------------------------
model = KWhisperForConditionalGeneration.from_state_dict(shape, synthetic_state_dict(shape, 0), dtype=torch.bfloat16, device=dev)
gen = model.generation_config
fe = WhisperFeatureExtractor(feature_size=shape.num_mel_bins, device=dev)
feats = fe.extract(torch.from_numpy(np.stack([dummy_audio(i) for i in range(B)])).to(dev))
eng = model.engine
sess = eng.new_session(B, eng.encode(feats))
rng = np.random.default_rng(0)
init = [gen.decoder_start_token_id, gen.lang_to_id["<|ja|>"], gen.task_to_id["transcribe"]]
prompt = np.concatenate([np.full((B, 1), gen.prev_sot_token_id), rng.integers(1000, 30000, (B, Q - 4)),
                         np.tile(init, (B, 1))], 1).astype(np.int64)
padded = prompt.copy()
padded[1::2, :160] = gen.pad_token_id
padded[1::2, 160] = gen.prev_sot_token_id
ks = [160 if b % 2 else 0 for b in range(B)]


def prefill_ms(ids, key_start):
    masked_ = sess._set_key_start(key_start)
    sess.ids.zero_()
    sess.ids[:, :Q].copy_(torch.from_numpy(ids))
    sess.cur_len.fill_(Q)
    seq = sess._step_plans(Q, masked=masked_)
    return event_ms(lambda: sess._run(seq), a.reps)


out["prefill_ms"] = {"unmasked": prefill_ms(prompt, None), "masked_half_rows_160": prefill_ms(padded, ks),
                     "unmasked_again": prefill_ms(prompt, None)}
print(json.dumps(out), flush=True)


def step_ms(ids, key_start):
    sess.generate(torch.from_numpy(ids), gen, max_length=256, return_timestamps=True, key_start=key_start)
    graph, res = sess._graph, []
    for _ in range(a.reps):
        sess.cur_len.fill_(230)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 20)
    return res, bool(sess.fused_last)


out["decode_step_ms"] = {}
for name, ids, k in (("unmasked", prompt, None), ("masked_half_rows_160", padded, ks), ("unmasked_again", prompt, None)):
    ms, fused = step_ms(ids, k)
    out["decode_step_ms"][name] = {"ms": ms, "fused_self_block": fused}
del sess
print(json.dumps(out), flush=True)

# ---- end to end: 8 clips of 70 s --------------------------------------------------------------------------------------
if not a.skip_e2e:
    n, sec = 8, 70
    clips = [np.concatenate([dummy_audio(i + 10 * k) for k in range(3)])[: sec * 16000] for i in range(n)]
    inp = fe(clips, truncation=False, padding="longest", return_attention_mask=True)
    e2e = {}
    for name, kw in (("plain", {}), ("condition_on_prev_tokens", dict(condition_on_prev_tokens=True))):
        ts = []
        for _ in range(2):  # (the first run of a kind captures its graphs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.generate(inp["input_features"], attention_mask=inp["attention_mask"], language="ja",
                           return_timestamps=True, **kw)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        e2e[name] = {"seconds": ts, "audio_s_per_s": [n * sec / t for t in ts], "passes": int(model.stats["passes"]),
                     "pass_P": model.stats["pass_P"],
                     "masked_passes": sum(1 for k in model.stats["pass_key_start"] if k and any(k))}
    out["end_to_end_8x70s"] = e2e
print(json.dumps(out), flush=True)
