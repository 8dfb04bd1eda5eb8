#!/usr/bin/env python
"""repetition_penalty / no_repeat_ngram_size timings on the MI355X (profiles/repeat_processors.md holds
one run).  Prints one JSON line per part.

  * kw_beam_logprobs_rep against kw_beam_logprobs at R = 160 rows (32 items x 5 beams), V = 51866, k = 10, histories of
    100 tokens: 20 launches per captured graph, with the workspace (the split kernel, what a session runs) and without;
  * kw_repeat_process alone at R = 32, V = 51866, the same histories, (1.3, 3): 20 launches per graph;
  * the graph-replayed decode step of a large-v3 bf16 session, B = 32, at positions 100-120: with timestamps, (1.3, 3)
    against off; without timestamps the same two and "off" without the fused LM-head + greedy launch, which the
    processors' step cannot take either -- so the launch they lose and the launch they add show separately.

    python tools/repeat_measure.py [--skip-session]
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
    """Looping histories: a 12-token cycle per row behind a 3-token prompt (every token 8 times, bans at every n)."""
    ids = np.zeros((R, 449), np.int64)
    for r in range(R):
        cyc = rng.integers(1000, 40000, 12)
        ids[r, :HIST] = np.concatenate([[50258, 50266, 50360], np.tile(cyc, 9)])[:HIST]
    return torch.from_numpy(ids).to(dev)


rng = np.random.default_rng(0)
kw = L.load_torch_ops()
gen = generation_constants(shape)
sup = torch.zeros(V, dtype=torch.uint8)
sup[torch.tensor(gen.suppress_tokens)] = 1
sup = sup.to(dev)
bsup = torch.tensor(gen.begin_suppress_tokens, dtype=torch.int32, device=dev)
cur = torch.tensor([HIST], dtype=torch.int32, device=dev)
done = torch.zeros(1, dtype=torch.int32, device=dev)

# ---- kw_beam_logprobs_rep against kw_beam_logprobs ------------------------------------------------------------------
R, K = 160, 10
logits = torch.randn(R, V, device=dev) * 3
ids = history(R, rng)
cv, ci = torch.empty(R, K, device=dev), torch.empty(R, K, dtype=torch.int32, device=dev)
out = {"R": R, "V": V, "k": K, "history": HIST, "launches_per_graph": N, "beam_logprobs_us": {}}
for rt in (False, True):
    cfg = [int(rt), gen.timestamp_begin, gen.no_timestamps_token_id, gen.eos_token_id, 50, 3, K]
    for split in (True, False):
        ws = torch.zeros(ops.beam_logprobs_workspace_bytes(R) // 4 + 1, device=dev) if split else None
        args = (logits, sup, bsup, ids, cur, cv, ci, done, ws, cfg)

        def plain():
            for _ in range(N):
                kw.beam_logprobs(*args)

        def rep():
            for _ in range(N):
                kw.beam_logprobs_rep(*args, *REPEAT)

        gp, gr = capture_graph(plain, dev), capture_graph(rep, dev)
        name = f"{'timestamps' if rt else 'no_timestamps'}_{'split' if split else 'one_workgroup'}"
        # alternating: plain, rep, plain
        out["beam_logprobs_us"][name] = {"kw_beam_logprobs": replay_us(gp, a.reps, N),
                                         "kw_beam_logprobs_rep": replay_us(gr, a.reps, N),
                                         "kw_beam_logprobs_again": replay_us(gp, a.reps, N)}
print(json.dumps(out), flush=True)

# ---- kw_repeat_process alone ---------------------------------------------------------------------------------------------
R = 32
scores = torch.randn(R, V, device=dev) * 3
plan = ops.RepeatPlan(scores, history(R, rng), cur, penalty=REPEAT[0], ngram=REPEAT[1])


def many():
    for _ in range(N):
        plan()


out = {"kw_repeat_process_us": {"R": R, "V": V, "history": HIST, "repeat": REPEAT,
                                "per_launch": replay_us(capture_graph(many, dev), a.reps, N)}}
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
init = [g.decoder_start_token_id, g.lang_to_id["<|ja|>"], g.task_to_id["transcribe"]]


def step_ms(rt, repeat, fuse=True):
    eng.fuse_lm_greedy = fuse
    prompt = torch.tensor([init + ([] if rt else [g.no_timestamps_token_id])] * B, dtype=torch.int64)
    sess.generate(prompt, g, max_length=256, return_timestamps=rt, repeat=repeat)
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


out = {"decode_step_ms": {"B": B, "positions": "100-120", "repeat": REPEAT}}
runs = [("timestamps_off", True, None, True), ("timestamps_on", True, REPEAT, True),
        ("timestamps_off_again", True, None, True),
        ("no_timestamps_off_fused", False, None, True), ("no_timestamps_off_two_launches", False, None, False),
        ("no_timestamps_on", False, REPEAT, True), ("no_timestamps_off_fused_again", False, None, True),
        ("no_timestamps_off_two_launches_again", False, None, False)]
for name, rt, repeat, fuse in runs:
    out["decode_step_ms"][name] = step_ms(rt, repeat, fuse)
eng.fuse_lm_greedy = True
print(json.dumps(out), flush=True)
