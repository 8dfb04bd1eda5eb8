#!/usr/bin/env python
"""Cost of return_token_timestamps under beam search at one shape (large-v3 bf16, B = 8 items x 5 beams = 40 running
rows, up to 128 tokens, 10 alignment pairs, S = 1500): generate() with the flag off / on / off, the beam step graph's
replay time off / on / off (the on graph holds the capture launches and kw_beam_select_parents; a beam session's cross
path is two launches either way), and the post-decode stage (backtrace on the host, table upload,
kw_align_weights_rows, reduce, DTW).  Prints one JSON line.

    python tools/beam_ts_measure.py
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kotoba-whisper_amd")]
from kwhisper.config import PRESETS  # noqa: E402
from kwhisper.decode import beam_backtrace, beam_row_table  # noqa: E402
from kwhisper.feature_extraction import WhisperFeatureExtractor  # noqa: E402
from kwhisper.generation import KWhisperForConditionalGeneration  # noqa: E402
from kwhisper.synthetic import dummy_audio, synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
shape = PRESETS["large-v3"]
model = KWhisperForConditionalGeneration.from_state_dict(shape, synthetic_state_dict(shape, 0), dtype=torch.bfloat16,
                                                         device=dev)
HEADS = [[7, 0], [10, 17], [12, 18], [13, 12], [16, 1], [17, 14], [19, 11], [21, 4], [24, 1], [25, 6]]
model.generation_config.alignment_heads = HEADS
fe = WhisperFeatureExtractor(feature_size=shape.num_mel_bins, device=dev)
B, NB = 8, 5
audio = torch.from_numpy(np.stack([dummy_audio(i) for i in range(B)])).to(dev)
feats = fe.extract(audio)
kw = dict(language="ja", task="transcribe", max_length=128, return_timestamps=False, num_beams=NB)
FLAG = {"return_token_timestamps": True}


def timed(n, **extra):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = model.generate(feats, **kw, **extra)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return r, ts


out = {"B": B, "num_beams": NB}
timed(2)
timed(2, **FLAG)
r0, out["generate_s_plain"] = timed(5)
r1, out["generate_s_flag"] = timed(5, **FLAG)
_, out["generate_s_plain_again"] = timed(5)
assert torch.equal(r0, r1["sequences"])
sess = model._session(B, NB)
align = tuple(tuple(p) for p in HEADS)
model.generate(feats, **kw, **FLAG)  # (the last call above was a plain one: the flagged search's state once more)
st = sess._beam_state
P = int(model.stats["pass_P"][0])  # the prompt length (generate() returns the sequences without it)
out["longest_hypothesis"] = int(st["fin_len"][:, 0].max())
post = []
for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bi = beam_backtrace(st["parent_log"].cpu().numpy(), st["fin_parent"][:, 0].cpu().numpy(),
                        st["fin_len"][:, 0].cpu().numpy(), P)
    table = beam_row_table(bi)
    sess._alignment(align, table.shape[1], None, 7, rows=table)
    torch.cuda.synchronize()
    post.append(time.perf_counter() - t0)
out["post_decode_stage_s"] = post


def step_ms(flag):
    """100 replays of the call's one-step graph from position P + 1 (the search's own state; a search that ends inside
    them leaves only the two beam kernels idle, the decoder forward runs on)."""
    model.generate(feats, **kw, **(FLAG if flag else {}))
    cfg = [c for k, c in sess._greedy_cfg.items() if k[0] == "beam" and ("align" in str(k)) == flag][-1]
    g, s = cfg["graph"], cfg["st"]
    res = []
    for _ in range(3):
        sess.cur_len.fill_(P + 1)
        s["done"].zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 100)
    return res, int(s["done"].item())


out["step_ms_plain"], d0 = step_ms(False)
out["step_ms_flag"], d1 = step_ms(True)
out["step_ms_plain_again"], d2 = step_ms(False)
out["search_ended_inside_replays"] = [d0, d1, d2]
print(json.dumps(out))
