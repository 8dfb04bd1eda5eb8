#!/usr/bin/env python
"""Config 3 (bench.py's workload: large-v3, 32 noise clips, greedy, max_length 128) with the fp8 cross K/V option
off and on, in one process (development tool; bench.py itself measures the default engine only).

Per engine: audio-s/s over ``--steps`` batches as bench.py times them (alternating rounds), the decode step's graph
replay time, the once-per-batch cost of ``cross_kv()`` (projection, and for fp8 the quantisation) by device events, and
``torch.cuda.max_memory_allocated()`` over one batch.  The second engine's peak is taken relative to what was allocated
before it was built (the first engine's weights and buffers, which stay resident for the alternating rounds).

    python tools/fp8_bench.py [--steps 3] [--rounds 3] [--out profiles/fp8_cross_bench_ab.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kotoba-whisper_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--max-length", type=int, default=128)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from kwhisper.config import PRESETS
    from kwhisper.feature_extraction import WhisperFeatureExtractor
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import dummy_audio, synthetic_state_dict

    dev = torch.device("cuda", 0)
    shape = PRESETS[a.model]
    sd = synthetic_state_dict(shape, 0)
    fe = WhisperFeatureExtractor(feature_size=shape.num_mel_bins, device=dev)
    B = a.batch
    audio = torch.from_numpy(np.stack([dummy_audio(i) for i in range(B)])).to(dev)
    kw = dict(language="ja", task="transcribe", max_length=a.max_length, return_timestamps=False)

    models, mem, toks = {}, {}, {}
    for name, opt in (("bf16", None), ("fp8_e4m3", "fp8_e4m3")):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        m = models[name] = KWhisperForConditionalGeneration.from_state_dict(shape, sd, dtype=torch.bfloat16, device=dev,
                                                                            cross_kv_dtype=opt)
        m.generate(fe.extract(audio), **kw)  # warm-up: sessions, graphs
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        toks[name] = m.generate(fe.extract(audio), **kw).cpu().numpy()
        torch.cuda.synchronize()
        sess = m._sessions[(B, 1)]
        mem[name] = {"peak_GB": (torch.cuda.max_memory_allocated(dev) - base) / 1e9,
                     "cross_cache_GB": (sess.cross.numel() * sess.cross.element_size()
                                        + (sess.cross_scale.numel() * 4 if sess.cross_scale is not None else 0)) / 1e9}

    def ev_ms(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    rounds = {k: [] for k in models}
    for _ in range(a.rounds):
        for name, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                m.generate(fe.extract(audio), **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            sess = m._sessions[(B, 1)]
            enc = m.engine.encode(fe.extract(audio))
            rounds[name].append({"audio_s_per_s": B * 30.0 * a.steps / dt, "ms_per_batch": dt / a.steps * 1e3,
                                 "decode_step_ms": ev_ms(sess._graph.replay, 20),
                                 "cross_kv_ms": ev_ms(lambda: sess.set_encoder_output(enc), 3)})
    res = {"workload": f"config 3: {shape.name}, B = {B}, max_length {a.max_length}, {a.steps} batches per round",
           "device": torch.cuda.get_device_name(dev), "rounds": rounds, "memory": mem,
           "tokens_equal_fraction": float((toks["bf16"] == toks["fp8_e4m3"]).mean())
           if toks["bf16"].shape == toks["fp8_e4m3"].shape else None}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
