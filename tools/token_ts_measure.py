#!/usr/bin/env python
"""Token-timestamp timings at the config-3 shape (large-v3 bf16, B = 32, 128 new tokens, 10 alignment pairs, S = 1500):
generate() with and without return_token_timestamps, the post-decode alignment stage and its three kernels, the step
graph's replay time with and without the query log, and transformers' CPU DTW of one row on this host.  Prints one
JSON line (profiles/token_ts_measure.json is one run).

    python tools/token_ts_measure.py
"""
import os, sys, time, json
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kotoba-whisper_amd")]
from kwhisper.config import PRESETS
from kwhisper.feature_extraction import WhisperFeatureExtractor
from kwhisper.generation import KWhisperForConditionalGeneration
from kwhisper.synthetic import dummy_audio, synthetic_state_dict

dev = torch.device("cuda:0")
shape = PRESETS["large-v3"]
model = KWhisperForConditionalGeneration.from_state_dict(shape, synthetic_state_dict(shape, 0), dtype=torch.bfloat16, device=dev)
HEADS = [[7, 0], [10, 17], [12, 18], [13, 12], [16, 1], [17, 14], [19, 11], [21, 4], [24, 1], [25, 6]]
model.generation_config.alignment_heads = HEADS
fe = WhisperFeatureExtractor(feature_size=shape.num_mel_bins, device=dev)
B = 32
audio = torch.from_numpy(np.stack([dummy_audio(i) for i in range(B)])).to(dev)
feats = fe.extract(audio)
kw = dict(language="ja", task="transcribe", max_length=128, return_timestamps=False)

def timed(n, **extra):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = model.generate(feats, **kw, **extra)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    return r, ts

out = {}
r0, _ = timed(2)
r0, t_plain = timed(5)
r1, _ = timed(2, return_token_timestamps=True)
r1, t_flag = timed(5, return_token_timestamps=True)
assert torch.equal(r0, r1["sequences"])
out["generate_s_plain"] = t_plain; out["generate_s_flag"] = t_flag
sess = model._session(B)
T = r1["sequences"].shape[1] - 1
align = tuple(tuple(p) for p in HEADS)
st = []
for _ in range(5):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    sess._alignment(align, T, None, 7)
    torch.cuda.synchronize(); st.append(time.perf_counter() - t0)
out["alignment_stage_s"] = st; out["steps_T"] = T
# per-kernel split with events
from kwhisper import ops
log = sess._align_log(align)
w = torch.empty((len(align), B, T, 1500), device=dev); m = torch.empty((B, T, 1500), device=dev)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
for _ in range(2):
    ev[0].record(); ops.align_weights(log, sess.cross, align, T, w, layer_step=2)
    ev[1].record(); ops.align_reduce(w, len(align), B, T, 1500, None, 7, m)
    ev[2].record(); fr = ops.dtw(m)
    ev[3].record(); torch.cuda.synchronize()
out["kernel_ms"] = dict(weights=ev[0].elapsed_time(ev[1]), reduce=ev[1].elapsed_time(ev[2]), dtw=ev[2].elapsed_time(ev[3]))
out["step_overhead_ms"] = (np.median(t_flag) - np.median(st) - np.median(t_plain)) / T * 1e3
# transformers' CPU DTW on this host, one 127 x 1500 row
from transformers.models.whisper.generation_whisper import _dynamic_time_warping
mm = m[0].cpu().double().numpy()
t0 = time.perf_counter(); _dynamic_time_warping(mm); out["hf_cpu_dtw_row_s"] = time.perf_counter() - t0
def step_ms(flag):
    model.generate(feats, **kw, **({"return_token_timestamps": True} if flag else {}))
    g = sess._graph
    res = []
    for _ in range(3):
        sess.cur_len.fill_(5); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(100):
            g.replay()
        e1.record(); torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) / 100)
    return res
out["step_ms_plain"] = step_ms(False); out["step_ms_flag"] = step_ms(True); out["step_ms_plain_again"] = step_ms(False)
out["token_timestamps_row0_head"] = r1["token_timestamps"][0, :12].tolist()
print(json.dumps(out))
