"""tests/golden/forward_tiny.npz: transformers' ``WhisperForConditionalGeneration.forward`` with labels on the seeded
tiny model (CPU, fp32), for tests/test_distill_cpu.py and tests/test_distill_gpu.py.

Three clips; labels [3][24] built the way kotoba-whisper's collator builds them (run_distillation.py:254-270): a full
row ``labels_full`` [25] per clip -- two rows start with a ``<|startofprev|>`` prompt, two rows end in padding -- then
``decoder_input_ids = labels_full[:, :-1]``, ``labels = labels_full[:, 1:]`` with -100 over the padding and over the
prompt.  Stored: the labels and decoder ids, HF's logits as per-position top-8 (indices and values) and log-sum-exp,
HF's ``.loss``, and the float64 distillation loss and per-position divergences (torch's KLDivLoss expression of
``train_step``, :614-622, 652-657) of those logits against the student
``np.random.RandomState(9).standard_normal(shape).astype(np.float32) * 3`` at T = 1 and T = 2.

    python tools/make_forward_fixtures.py            # a few seconds
"""
import os
import sys

import numpy as np
import torch

from make_fixtures import GOLD, ROOT, TINY, features, hf_model

sys.path.insert(0, ROOT)  # the in-repo oracle

CLIPS = [("dummy", 0), ("tone", 1), ("tone", 2)]
T_FULL = 25
STUDENT_SEED, STUDENT_SCALE = 9, 3.0
TEMPS = (1.0, 2.0)


def collate(shape, seed=4):
    """(labels_full, decoder_input_ids, labels) as the reference's collator makes them."""
    from kwhisper.config import generation_constants

    g = generation_constants(shape)
    rng = np.random.RandomState(seed)
    sot, pad = shape.decoder_start_token_id, shape.pad_token_id
    prev = g.prev_sot_token_id
    head = [sot, g.lang_to_id["<|ja|>"], g.task_to_id["transcribe"], g.no_timestamps_token_id]
    text = lambda n: rng.randint(1000, 50000, size=n).tolist()  # noqa: E731
    rows = [[prev] + text(4) + head + text(T_FULL - 10) + [shape.eos_token_id],      # a prompt, no padding
            [prev] + text(2) + head + text(9) + [shape.eos_token_id],                # a prompt and a padded tail
            head + text(12) + [shape.eos_token_id]]                                  # no prompt, a padded tail
    full = np.full((len(rows), T_FULL), pad, np.int64)
    mask = np.zeros((len(rows), T_FULL), bool)
    for r, row in enumerate(rows):
        assert len(row) <= T_FULL
        full[r, : len(row)], mask[r, : len(row)] = row, True
    full, mask = torch.from_numpy(full), torch.from_numpy(mask)
    ids, labels = full[:, :-1], full[:, 1:]
    labels = labels.masked_fill(~mask[:, 1:], -100)
    bos = torch.argmax((labels == sot).long(), dim=1)
    bos = torch.where(bos > 0, bos + 1, bos)
    labels = torch.where(torch.arange(labels.shape[1]) < bos[:, None], -100, labels)
    return full, ids.contiguous(), labels.contiguous()


def kd_f64(teacher, student, labels, T):
    """train_step's expression at float64: (loss, per-position divergence with ignored positions at 0)."""
    t, s = teacher.double(), student.double()
    p = torch.nn.functional.softmax(t / T, dim=-1)
    lq = torch.nn.functional.log_softmax(s / T, dim=-1)
    div = torch.nn.KLDivLoss(reduction="none")(lq, p)
    m = (labels >= 0).unsqueeze(-1)
    div = div * m
    return (div.sum() / m.sum() * T ** 2).item(), div.sum(-1).numpy()


def main():
    m = hf_model(TINY, 0)
    feats = features(TINY.num_mel_bins, CLIPS)
    full, ids, labels = collate(TINY)
    with torch.no_grad():
        out = m(input_features=feats, decoder_input_ids=ids, labels=labels)
        shifted = m(input_features=feats, labels=labels)  # the labels alone: shift_tokens_right inside
    logits = out.logits.float()
    top = logits.topk(8, -1)
    fx = {"cases": np.array([f"{k}:{s}" for k, s in CLIPS]), "labels_full": full.numpy(), "decoder_input_ids": ids.numpy(),
          "labels": labels.numpy(), "top_idx": top.indices.numpy().astype(np.int32),
          "top_val": top.values.numpy().astype(np.float32),
          "lse": torch.logsumexp(logits.double(), -1).numpy(), "loss": np.float64(out.loss.item()),
          "shift_top_val": shifted.logits.float().topk(8, -1).values.numpy().astype(np.float32),
          "shift_lse": torch.logsumexp(shifted.logits.double(), -1).numpy(), "shift_loss": np.float64(shifted.loss.item()),
          "student_seed": STUDENT_SEED, "student_scale": STUDENT_SCALE, "temperatures": np.array(TEMPS)}
    student = torch.from_numpy(
        np.random.RandomState(STUDENT_SEED).standard_normal(tuple(logits.shape)).astype(np.float32) * np.float32(STUDENT_SCALE))
    for T in TEMPS:
        loss, rows = kd_f64(logits, student, labels, T)
        fx[f"kd_loss_T{T:g}"], fx[f"kd_rows_T{T:g}"] = np.float64(loss), rows
        print(f"  T = {T:g}: kd loss {loss:.9f}")
    # the in-repo oracle on the same inputs (the GPU tests' full-tensor yardstick)
    from kwhisper.synthetic import synthetic_state_dict
    from oracle.whisper_np import WhisperNP

    o = WhisperNP(synthetic_state_dict(TINY, 0), TINY)
    lg = o.decode(ids.numpy(), o.new_cache(o.encode(feats.numpy())))
    print(f"  oracle vs transformers: max |logit difference| {np.abs(lg - logits.numpy()).max():.3g}; "
          f"HF loss {out.loss.item():.7f}")
    path = os.path.join(GOLD, "forward_tiny.npz")
    np.savez_compressed(path, **fx)
    print(f"forward_tiny fixture: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
