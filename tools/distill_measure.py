"""The teacher's forward and the distillation loss on one MI355X: large-v3, synthetic bf16 weights.

1. ``DecodeSession.forward_all`` (the decoder's many-row pass; the encoder is not in the timed window) over rows =
   B x T in {64 .. 4096}: the wide plan (kw_layernorm + kw_gemm over row-major weights) against the packed row-chunk
   plan (kw_dec_linear in 32-row chunks, the parent's prefill plan with the LM head on every row).  Rounds alternate the
   two plans; device events around each call; the median of all rounds.  Also the largest logit difference between
   the two plans' outputs at each size.  ``WIDE_MIN_ROWS`` in kwhisper/decode.py is read off this table.
2. ``kwhisper.distill.kd_loss`` forward + backward against the eager expression of run_distillation.py:652-657 (+ its
   backward) on the same tensors, 4,096 x 51,866, bf16 and f32 students: time, achieved bytes per second against the
   kernel's 2-read + 1-write byte count, and ``torch.cuda.max_memory_allocated()`` above the inputs.

    python tools/distill_measure.py --out profiles/distill_forward.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kotoba-whisper_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SWEEP = [(1, 64), (1, 128), (2, 128), (4, 128), (8, 128), (16, 128), (32, 128)]  # (B, T): 64 .. 4096 rows


def _event_ms(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(fns, rounds, calls):
    """name -> sorted times (ms): ``rounds`` rounds, each running every side ``calls`` times, one side after the other."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            for _ in range(calls):
                out[k].append(_event_ms(fn))
    return {k: sorted(v) for k, v in out.items()}


def _med(v):
    return v[len(v) // 2]


def forward_sweep(model, lines, rounds, calls):
    import torch

    eng, s = model.engine, model.engine.shape
    g = torch.Generator(device="cpu").manual_seed(1)
    lines.append("== forward_all, large-v3 bf16, decoder only (ms per call: median [min .. max]) ==")
    lines.append(f"{'B':>3} {'T':>4} {'rows':>5}  {'wide':>24}  {'chunk':>24}  chunk/wide  max |logit diff|")
    for B, T in SWEEP:
        sess = eng.new_session(B)
        enc = (torch.randn((B * s.max_source_positions, s.d_model), generator=g) * 0.5).to(eng.device, eng.dtype)
        sess.set_encoder_output(enc)
        ids = torch.randint(0, 50000, (B, T), generator=g).to(eng.device)
        a = sess.forward_all(ids, plan="wide")  # warm-up of both plans; the outputs are compared
        b = sess.forward_all(ids, plan="chunk")
        diff = float((a - b).abs().max())
        del a, b
        t = _alternate({"wide": lambda: sess.forward_all(ids, plan="wide"),
                        "chunk": lambda: sess.forward_all(ids, plan="chunk")}, rounds, calls)
        fmt = lambda v: f"{_med(v):8.3f} [{v[0]:7.3f} .. {v[-1]:7.3f}]"  # noqa: E731
        lines.append(f"{B:>3} {T:>4} {B * T:>5}  {fmt(t['wide'])}  {fmt(t['chunk'])}  {_med(t['chunk']) / _med(t['wide']):9.2f}"
                     f"  {diff:.4f}")
        print(lines[-1], flush=True)
        del sess, enc
        torch.cuda.empty_cache()


def model_forward(model, lines, rounds, calls):
    """The whole forward (encoder + cross K/V + decoder) at 16 x 128 and 32 x 128, default plan."""
    import torch

    s = model.engine.shape
    g = torch.Generator(device="cpu").manual_seed(2)
    lines.append("== model.forward (encoder + cross K/V + decoder), large-v3 bf16, default plan (ms per call) ==")
    for B, T in ((16, 128), (32, 128)):
        feats = (torch.randn((B, s.num_mel_bins, 3000), generator=g) * 0.5).cuda()
        labels = torch.randint(0, 50000, (B, T), generator=g).cuda()
        model(input_features=feats, labels=labels)
        t = _alternate({"forward": lambda: model(input_features=feats, labels=labels)}, rounds, calls)["forward"]
        lines.append(f"B = {B}, T = {T}: {_med(t):.2f} [{t[0]:.2f} .. {t[-1]:.2f}], plan "
                     f"{model._fwd_sessions[B].forward_plan_last}")
        print(lines[-1], flush=True)
        model._fwd_sessions.clear()
        torch.cuda.empty_cache()


def loss_compare(lines, rounds, calls, N=4096, V=51866):
    import torch

    from kwhisper.distill import kd_loss

    T = 2.0
    g = torch.Generator(device="cpu").manual_seed(3)
    teacher = (torch.randn((N, V), generator=g) * 3).cuda()
    labels = torch.randint(0, V, (N,), generator=g).cuda()
    labels[::7] = -100
    lines.append(f"== kd_loss forward + backward vs the eager expression, {N} x {V}, T = {T} ==")

    def eager(student):
        p = torch.nn.functional.softmax(teacher / T, dim=-1)
        lq = torch.nn.functional.log_softmax(student / T, dim=-1)
        div = torch.nn.KLDivLoss(reduction="none")(lq, p)
        mask = (labels >= 0).unsqueeze(-1)
        return (div * mask).sum() / mask.sum() * T ** 2

    for dt in (torch.bfloat16, torch.float32):
        student = (torch.randn((N, V), generator=g) * 3).cuda().to(dt).requires_grad_(True)
        es = student.element_size()
        nbytes = N * V * (2 * 4 + 2 * es + es)  # both tensors read twice, the gradient written once

        def run(fn):
            student.grad = None
            fn(student).backward()

        sides = {"kernel": lambda: run(lambda s_: kd_loss(s_, teacher, labels, T)), "eager": lambda: run(eager)}
        vals, peak = {}, {}
        for k, fn in sides.items():  # warm-up, values and peak memory above what is resident before the call
            student.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()  # teacher, student, labels and the earlier side's kept gradient
            torch.cuda.reset_peak_memory_stats()
            loss = (kd_loss(student, teacher, labels, T) if k == "kernel" else eager(student))
            loss.backward()
            torch.cuda.synchronize()
            peak[k] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            vals[k] = (float(loss.detach()), student.grad.clone())
            del loss  # (with it goes the graph and what it saved: nothing of this side but vals[k] is left)
            student.grad = None
        gd = float((vals["kernel"][1].float() - vals["eager"][1].float()).abs().max())
        t = _alternate(sides, rounds, calls)
        for k in sides:
            v = t[k]
            lines.append(f"student {str(dt).split('.')[-1]:>8} {k:>6}: {_med(v):8.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]  "
                         f"{nbytes / _med(v) / 1e9:7.2f} TB/s of the 2-read + 1-write count ({nbytes / 1e9:.2f} GB)  "
                         f"peak memory above the inputs {peak[k]:9.1f} MiB  loss {vals[k][0]:.6f}")
            print(lines[-1], flush=True)
        lines.append(f"student {str(dt).split('.')[-1]:>8}: eager / kernel time {_med(t['eager']) / _med(t['kernel']):.2f}, "
                     f"max |gradient difference| {gd:.3g}")
        print(lines[-1], flush=True)
        del student, vals
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: sweep, forward, loss")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "distill_measure needs the MI355X"
    skip = set(filter(None, a.skip.split(",")))
    lines = [f"tools/distill_measure.py --rounds {a.rounds} --calls {a.calls}: {torch.cuda.get_device_name(0)}"]
    if "loss" not in skip:
        loss_compare(lines, a.rounds, a.calls)
    if not {"sweep", "forward"} <= skip:
        from kwhisper.config import LARGE_V3
        from kwhisper.generation import KWhisperForConditionalGeneration
        from kwhisper.synthetic import synthetic_state_dict_torch

        sd = synthetic_state_dict_torch(LARGE_V3, seed=0, device="cuda:0")
        model = KWhisperForConditionalGeneration.from_state_dict(LARGE_V3, sd, dtype=torch.bfloat16, device="cuda:0")
        del sd
        if "sweep" not in skip:
            forward_sweep(model, lines, a.rounds, a.calls)
        if "forward" not in skip:
            model_forward(model, lines, a.rounds, a.calls)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
