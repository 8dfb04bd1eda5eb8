#!/usr/bin/env python
"""Accuracy of the fp8 (e4m3) cross K/V option at large-v3 (development tool, not a test).

Builds the numpy-recipe large-v3 (seed 0) twice -- bf16 cross cache and cross_kv_dtype="fp8_e4m3" -- and teacher-forces
both along tests/golden/large_v3_b32_fp32.npz exactly as tests/test_gpu_workloads.py::test_config3_bf16_generate_b32
does.  Writes, for both engines: the top-8 logit error (max / mean) against transformers' fp32, over all 32 rows and on
the rows tests/golden/large_v3_bf16ref.npz covers; the number of safe-margin steps (fp32 margin >= 0.2) whose
processed greedy choice differs from fp32's; and transformers' own bf16 figures from that fixture.

The bar is the project's: no worse than the reference's own bf16 arithmetic (max and mean on the same rows) and no
differing safe-margin step.  To say where the error sits, the tool also reports, per layer, the relative RMS error of
the dequantised K and V against the bf16 K / V they were made from, and the 4 worst (head, dim) channels.

    python tools/fp8_accuracy.py [--out profiles/fp8_cross_kv_accuracy.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "kotoba-whisper_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

MARGIN_FLOOR = 0.2  # tests/test_gpu_workloads.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_cross_kv_accuracy.json"))
    a = ap.parse_args()
    from kwhisper import synthetic as S
    from kwhisper.config import LARGE_V3, generation_constants
    from kwhisper.generation import KWhisperForConditionalGeneration
    from oracle.fixtures import load_fixture
    from oracle.mel import log_mel

    gold = os.path.join(ROOT, "tests", "golden")
    g = load_fixture(os.path.join(gold, "large_v3_b32_fp32.npz"))
    r = load_fixture(os.path.join(gold, "large_v3_bf16ref.npz"))
    rows = [int(x) for x in r["rows"]]
    audio = np.stack([getattr(S, f"{str(c).split(':')[0]}_audio")(int(str(c).split(":")[1])) for c in g["cases"]])
    feats = torch.from_numpy(log_mel(audio, LARGE_V3.num_mel_bins)).cuda()
    sd = S.synthetic_state_dict(LARGE_V3, 0)
    gen = generation_constants(LARGE_V3)
    seq = torch.from_numpy(g["greedy_sequences"])
    idx = torch.from_numpy(g["greedy_logits_top_idx"].astype(np.int64)).cuda()
    val = g["greedy_logits_top_val"]
    n_pos = g["greedy_margin"].shape[1]
    want_tok = g["greedy_sequences"][:, 4: 4 + n_pos]
    safe = g["greedy_margin"] >= MARGIN_FLOOR
    out = {"fixture": "tests/golden/large_v3_b32_fp32.npz (transformers fp32, 32 clips)", "rows_with_hf_bf16": rows,
           "safe_margin": MARGIN_FLOOR, "safe_steps": int(safe.sum()), "engines": {}}
    ref_err = np.abs(r["tf_logits_at_fp32_top8"] - val[rows])
    out["hf_bf16"] = {"rows_max": float(ref_err.max()), "rows_mean": float(ref_err.mean())}
    layer_err = None
    for name, opt in (("bf16", None), ("fp8_e4m3", "fp8_e4m3")):
        model = KWhisperForConditionalGeneration.from_state_dict(LARGE_V3, sd, dtype=torch.bfloat16, generation_config=gen,
                                                                 cross_kv_dtype=opt)
        eng = model.engine
        enc = eng.encode(feats)
        sess = eng.new_session(32, enc)
        lg = sess.teacher_forced_logits(seq[:, :-1], 4)
        got = torch.gather(lg[:, : idx.shape[1]], -1, idx).cpu().numpy()
        err = np.abs(got - val)
        proc = lg[:, :n_pos].clone()
        proc[:, :, torch.tensor(gen.suppress_tokens, device=proc.device)] = -float("inf")
        proc[:, 0, torch.tensor(gen.begin_suppress_tokens, device=proc.device)] = -float("inf")
        choice = proc.argmax(-1).cpu().numpy()
        bad = np.argwhere(safe & (choice != want_tok))
        out["engines"][name] = {"all_max": float(err.max()), "all_mean": float(err.mean()),
                                "rows_max": float(err[rows].max()), "rows_mean": float(err[rows].mean()),
                                "safe_steps_differing": int(len(bad)), "differing": bad[:16].tolist(),
                                "all_steps_agree": float((choice == want_tok).mean())}
        if opt:  # the cache's own error against the bf16 K / V it was made from, per layer (and the worst channels)
            eng.cross_kv_fp8 = False  # (the bf16 projection of the same engine, for this one call)
            ref_kv = eng.cross_kv(enc, 32)
            eng.cross_kv_fp8 = True
            lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().cuda()
            layer_err = []
            for i in range(ref_kv.shape[0]):
                deq = lut[sess.cross[i].int()] * sess.cross_scale[i].unsqueeze(-2)
                x = ref_kv[i].float()
                e2 = ((deq - x) ** 2).sum(dim=(0, 2))  # [H][64]
                x2 = (x ** 2).sum(dim=(0, 2))
                rel = (e2 / x2.clamp_min(1e-30)).sqrt()
                top = torch.topk(rel.flatten(), 4)
                layer_err.append({"layer": i // 2, "kv": "KV"[i % 2], "rel_rms": float((e2.sum() / x2.sum()).sqrt()),
                                  "worst_channels": [[int(j) // 64, int(j) % 64, float(v)] for v, j in
                                                     zip(top.values.cpu(), top.indices.cpu())]})
            del ref_kv
        del model, eng, sess, lg, proc, enc
        torch.cuda.empty_cache()
    f8, hf = out["engines"]["fp8_e4m3"], out["hf_bf16"]
    out["meets_bar"] = bool(f8["rows_max"] <= hf["rows_max"] and f8["rows_mean"] <= hf["rows_mean"]
                            and f8["safe_steps_differing"] == 0)
    out["cache_error_per_layer"] = layer_err
    text = json.dumps(out, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "cache_error_per_layer"}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
