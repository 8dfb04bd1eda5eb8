#!/usr/bin/env python
"""sequence_bias / bad_words_ids timings on the MI355X (profiles/seq_bias.txt holds one run).  Prints
one JSON line per part.

  * kw_seq_bias_process alone at R = 32, V = 51866, histories of 100 tokens, with 8 and with 1,024 sequences (2 to 6
    tokens, a quarter of them ending in a token another ends in), beside kw_repeat_process (1.3, 3) in the same run:
    20 launches per captured graph;
  * kw_beam_logprobs_proc against kw_beam_logprobs_rep and kw_beam_logprobs at R = 40 rows (8 items x 5 beams), k = 10,
    with the workspace (the split kernel, what a session runs) and without, both table sizes;
  * the graph-replayed decode step of a large-v3 bf16 session, B = 32, at positions 100-120, without timestamps: off
    on the fused LM-head + greedy launch, off on the two-launch tail (what a table's step takes), and with a
    sequence_bias and a bad_words_ids table -- so the launch the tables lose and the launches they add show apart.

    python tools/seq_bias_measure.py [--skip-session]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kotoba-whisper_amd")]
from kwhisper import _lib as L  # noqa: E402
from kwhisper import ops  # noqa: E402
from kwhisper.config import PRESETS, generation_constants  # noqa: E402
from kwhisper.decode import capture_graph  # noqa: E402
from kwhisper.seq_bias import SeqTable  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--skip-session", action="store_true")
ap.add_argument("--reps", type=int, default=7)
a = ap.parse_args()
dev = torch.device("cuda:0")
shape = PRESETS["large-v3"]
V, HIST, N = shape.vocab_size, 100, 20
REPEAT = (1.3, 3)


def replay_us(graph, reps, per):
    graph.replay()
    torch.cuda.synchronize()
    res = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        res.append(round(e0.elapsed_time(e1) * 1000 / per, 2))
    return res


def history(R, rng):
    ids = np.zeros((R, 449), np.int64)
    for r in range(R):
        cyc = rng.integers(1000, 40000, 12)
        ids[r, :HIST] = np.concatenate([[50258, 50266, 50360], np.tile(cyc, 9)])[:HIST]
    return ids


def entries(n, hist, rng, value):
    """n sequences of 2-6 tokens: every eighth is the tail of a history row (it applies), a quarter share a last
    token with another; ``value(i)`` gives entry i's float."""
    out, lasts = {}, []
    while len(out) < n:
        i = len(out)
        k = int(rng.integers(2, 7))
        if i % 8 == 0:
            pre = [int(t) for t in hist[i % len(hist), HIST - (k - 1): HIST]]
        else:
            pre = [int(t) for t in rng.integers(1000, 40000, k - 1)]
        last = lasts[int(rng.integers(len(lasts)))] if lasts and i % 4 == 1 else int(rng.integers(1000, 40000))
        lasts.append(last)
        out[tuple(pre) + (last,)] = value(i)
    return out


rng = np.random.default_rng(0)
kw = L.load_torch_ops()
gen = generation_constants(shape)
cur = torch.tensor([HIST], dtype=torch.int32, device=dev)

# ---- kw_seq_bias_process alone, beside kw_repeat_process ------------------------------------------------------------------
R = 32
hist = history(R, rng)
ids = torch.from_numpy(hist).to(dev)
scores = torch.randn(R, V, device=dev) * 3
out = {"kw_seq_bias_process_us": {"R": R, "V": V, "history": HIST, "launches_per_graph": N}}
tables = {}
for n in (8, 1024):
    tables[n] = (ops.DeviceSeqTable(SeqTable(entries(n, hist, rng, lambda i: 0.5 * (i % 7 - 3)), V), dev),
                 ops.DeviceSeqTable(SeqTable(entries(n, hist, rng, lambda i: float("-inf")), V), dev))
plans = {"kw_repeat_process": ops.RepeatPlan(scores, ids, cur, penalty=REPEAT[0], ngram=REPEAT[1])}
for n in (8, 1024):
    plans[f"{n}_sequences"] = ops.SeqBiasPlan(scores, ids, cur, tables[n][0])
    out["kw_seq_bias_process_us"][f"{n}_groups"] = tables[n][0].n_groups
graphs = {}
for name, plan in plans.items():
    def many(plan=plan):
        for _ in range(N):
            plan()
    graphs[name] = capture_graph(many, dev)
for rnd in ("", "_again"):
    for name, g in graphs.items():
        out["kw_seq_bias_process_us"][name + rnd] = replay_us(g, a.reps, N)
print(json.dumps(out), flush=True)

# ---- kw_beam_logprobs_proc against _rep and the plain launch at 8 x 5 rows ----------------------------------------------
R, K = 40, 10
sup = torch.zeros(V, dtype=torch.uint8)
sup[torch.tensor(gen.suppress_tokens)] = 1
sup = sup.to(dev)
bsup = torch.tensor(gen.begin_suppress_tokens, dtype=torch.int32, device=dev)
done = torch.zeros(1, dtype=torch.int32, device=dev)
logits = torch.randn(R, V, device=dev) * 3
bids = torch.from_numpy(hist[np.arange(R) % len(hist)]).to(dev)  # (the rows the tables' applying entries were cut from)
cv, ci = torch.empty(R, K, device=dev), torch.empty(R, K, dtype=torch.int32, device=dev)
out = {"R": R, "V": V, "k": K, "history": HIST, "launches_per_graph": N, "beam_logprobs_us": {}}
cfg = [1, gen.timestamp_begin, gen.no_timestamps_token_id, gen.eos_token_id, 50, 3, K]
for split in (True, False):
    ws = torch.zeros(ops.beam_logprobs_workspace_bytes(R) // 4 + 1, device=dev) if split else None
    args = (logits, sup, bsup, bids, cur, cv, ci, done, ws, cfg)
    calls = {"kw_beam_logprobs": lambda: kw.beam_logprobs(*args),
             "kw_beam_logprobs_rep_1.3_3": lambda: kw.beam_logprobs_rep(*args, *REPEAT)}
    for n in (8, 1024):
        sb, bw = tables[n]
        calls[f"kw_beam_logprobs_proc_{n}"] = (lambda sb=sb, bw=bw: kw.beam_logprobs_proc(
            *args, 1.0, 0, sb.tensors, sb.max_len, bw.tensors, bw.max_len))
        calls[f"kw_beam_logprobs_proc_{n}_rep_1.3_3"] = (lambda sb=sb, bw=bw: kw.beam_logprobs_proc(
            *args, *REPEAT, sb.tensors, sb.max_len, bw.tensors, bw.max_len))
    gs = {}
    for name, fn in calls.items():
        def many(fn=fn):
            for _ in range(N):
                fn()
        gs[name] = capture_graph(many, dev)
    res = {}
    for rnd in ("", "_again"):
        for name, g in gs.items():
            res[name + rnd] = replay_us(g, a.reps, N)
    out["beam_logprobs_us"]["split" if split else "one_workgroup"] = res
print(json.dumps(out), flush=True)
if a.skip_session:
    sys.exit(0)

# ---- the decode step of a session ---------------------------------------------------------------------------------------
from kwhisper.feature_extraction import WhisperFeatureExtractor  # noqa: E402
from kwhisper.generation import KWhisperForConditionalGeneration  # noqa: E402
from kwhisper.synthetic import dummy_audio, synthetic_state_dict  # noqa: E402

B = 32
model = KWhisperForConditionalGeneration.from_state_dict(shape, synthetic_state_dict(shape, 0), dtype=torch.bfloat16, device=dev)
g = model.generation_config
fe = WhisperFeatureExtractor(feature_size=shape.num_mel_bins, device=dev)
feats = fe.extract(torch.from_numpy(np.stack([dummy_audio(i) for i in range(B)])).to(dev))
eng = model.engine
sess = eng.new_session(B, eng.encode(feats))
init = [g.decoder_start_token_id, g.lang_to_id["<|ja|>"], g.task_to_id["transcribe"], g.no_timestamps_token_id]
host = {n: (SeqTable(entries(n, hist, rng, lambda i: 0.5 * (i % 7 - 3)), V),
            SeqTable(entries(n, hist, rng, lambda i: float("-inf")), V)) for n in (8, 1024)}


def step_ms(seq_tables, fuse=True):
    eng.fuse_lm_greedy = fuse
    prompt = torch.tensor([init] * B, dtype=torch.int64)
    sess.generate(prompt, g, max_length=256, return_timestamps=False, seq_tables=seq_tables)
    graph, res = sess._graph, []
    for _ in range(a.reps):
        sess.cur_len.fill_(100)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        res.append(round(e0.elapsed_time(e1) / 20, 4))
    return {"ms": res, "fused_lm_greedy": bool(sess.lm_greedy_last)}


out = {"decode_step_ms": {"B": B, "positions": "100-120"}}
runs = [("off_fused", None, True), ("off_two_launches", None, False), ("bias_only_8", (host[8][0], None), True),
        ("both_8", host[8], True), ("both_1024", host[1024], True), ("off_fused_again", None, True),
        ("off_two_launches_again", None, False), ("both_8_again", host[8], True)]
for name, tabs, fuse in runs:
    out["decode_step_ms"][name] = step_ms(tabs, fuse)
eng.fuse_lm_greedy = True
print(json.dumps(out), flush=True)
