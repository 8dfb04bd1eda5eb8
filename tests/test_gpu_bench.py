"""A plain bench.py run on the GPU (tiny model, so it takes seconds): the lean result line, and --dump-outputs
writing the token ids generate() returned in the last timed step, equal to a direct generate() on the same seeded
model and audio."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "tiny",
           "--batch", "4", "--max-length", "24", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["warmup"] == 1 and r["n_gpus"] == 1 and r["dtype"] == "bf16"
    assert r["higher_is_better"] is True and r["unit"] == "audio-s/s" and r["ms_per_step"] > 0
    assert abs(r["value"] - 4 * 30.0 / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    # nothing beside the headline was measured
    assert not {"roofline", "encoder_mfma", "decode_kernel_us", "decode_step_ms", "cpu_baseline", "inflight"} & set(r)

    assert sorted(os.listdir(tmp_path)) == ["token_ids.npy"]
    got = np.load(tmp_path / "token_ids.npy")
    assert got.dtype == np.float32 and got.shape == (4, r["config"]["new_tokens"])

    from kwhisper.config import PRESETS
    from kwhisper.feature_extraction import WhisperFeatureExtractor
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import dummy_audio, synthetic_state_dict

    shape = PRESETS["tiny"]
    model = KWhisperForConditionalGeneration.from_state_dict(shape, synthetic_state_dict(shape, 0), dtype=torch.bfloat16,
                                                             device="cuda:0")
    fe = WhisperFeatureExtractor(feature_size=shape.num_mel_bins, device="cuda:0")
    audio = torch.from_numpy(np.stack([dummy_audio(i) for i in range(4)])).cuda()
    want = model.generate(fe.extract(audio), language="ja", task="transcribe", max_length=24, return_timestamps=False)
    np.testing.assert_array_equal(got, want.cpu().numpy().astype(np.float32))
