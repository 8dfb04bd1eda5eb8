"""Assisted (speculative) generate at batch 1 on one MI355X: large-v3 as the main model, kotoba-whisper-v2.0 (two decoder
layers) as the assistant, synthetic bf16 weights, 128 new tokens.

Measured, device events around hipGraph replays, medians of ``--repeats``:
  * the main model's plain one-token step;
  * one round (K + 1 assistant steps, the K + 1-position verify forward, kw_spec_accept) for K = 3, 5, 7, on an
    unfinished row (re-armed before every timed run, so the accept step does its whole reduction);
  * generate() wall time: plain greedy; with the kotoba assistant (synthetic weights: next to nothing is accepted -- the
    lower bound); with an assistant of the main model's own weights (every draft accepted -- the upper bound on
    acceptance, at the price of full-size drafts).
From the first two follows the break-even acceptance: a round with per-draft acceptance a yields (1 - a^(K+1)) / (1 - a)
tokens, and pays off when that exceeds t_round / t_step.

    python tools/spec_measure.py --out profiles/spec_decode.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "kotoba-whisper_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _replay_ms(graph, n, repeats, before=None):
    import torch

    out = []
    for _ in range(repeats):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            graph.replay()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / n)
    return sorted(out)[len(out) // 2]


def _wall_ms(fn, repeats):
    import torch

    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)[len(out) // 2]


def break_even(ratio, K):
    """The per-draft acceptance a at which (1 - a^(K+1)) / (1 - a) == ratio (bisection); None if even a = 1 loses."""
    if ratio >= K + 1:
        return None
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = (lo + hi) / 2
        tokens = (1 - mid ** (K + 1)) / (1 - mid) if mid < 1 else K + 1
        lo, hi = (mid, hi) if tokens < ratio else (lo, mid)
    return hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from kwhisper.config import KOTOBA_V2, LARGE_V3
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import synthetic_state_dict_torch

    dev = "cuda:0"

    def model(shape, seed):
        sd = synthetic_state_dict_torch(shape, seed=seed, device=dev)
        return KWhisperForConditionalGeneration.from_state_dict(shape, sd, dtype=torch.bfloat16, device=dev)

    main_m, same_m, kotoba = model(LARGE_V3, 0), model(LARGE_V3, 0), model(KOTOBA_V2, 1)
    g = torch.Generator(device="cpu").manual_seed(0)
    feats = (torch.randn((1, LARGE_V3.num_mel_bins, 3000), generator=g) * 0.5).to(dev)
    kw = dict(language="ja", task="transcribe", return_timestamps=False, max_new_tokens=a.tokens)
    res = {"tokens": a.tokens, "repeats": a.repeats, "main": LARGE_V3.name, "assistant": KOTOBA_V2.name}

    plain = main_m.generate(feats, **kw)
    res["generate_plain_ms"] = _wall_ms(lambda: main_m.generate(feats, **kw), a.repeats)
    res["generated"] = int(plain.shape[1])
    res["main_step_ms"] = _replay_ms(main_m._session(1)._graph, 20, a.repeats)
    res["rounds"] = {}
    for K in (3, 5, 7):
        main_m.generate(feats, assistant_model=kotoba, num_assistant_tokens=K, **kw)
        st = dict(main_m.stats["assisted"])
        wall = _wall_ms(lambda: main_m.generate(feats, assistant_model=kotoba, num_assistant_tokens=K, **kw), a.repeats)
        sess = main_m._spec_session(kotoba)
        cfg = next(c for k, c in sess._cfg.items() if k[0] == K)
        # A finished row would make kw_spec_accept return at once, so the row is re-armed before every timed run:
        # unfinished, 30 positions before max_length on the tokens of the call above (the synthetic assistant's drafts
        # are rejected, so ten rounds move it ten positions on and leave room for a whole round), on which every
        # launch of the round does its full work at about the position the plain step above is timed at.
        L0 = cfg["P"] + a.tokens - 30

        def rearm(sess=sess, L0=L0, K=K):
            for s_ in (sess.main, sess.asst):
                s_.cur_len.fill_(L0)
                s_.unfinished.fill_(1)
            sess.main.n_unfinished.fill_(1)
            sess.verify_len.fill_(L0 + K)

        t_round = _replay_ms(cfg["round_graph"], 10, a.repeats, before=rearm)
        assert int(sess.main.n_unfinished.item()) == 1, "the timed rounds ran on a finished row"
        assert L0 < int(sess.main.cur_len.item()) <= L0 + 10 * (K + 1)
        ratio = t_round / res["main_step_ms"]
        res["rounds"][K] = dict(round_ms=t_round, round_over_step=ratio, break_even_acceptance=break_even(ratio, K),
                                generate_kotoba_ms=wall, stats_kotoba=st)
    for K in (3, 5, 7):
        main_m.generate(feats, assistant_model=same_m, num_assistant_tokens=K, **kw)
        res["rounds"][K]["stats_same_weights"] = dict(main_m.stats["assisted"])
        res["rounds"][K]["generate_same_weights_ms"] = _wall_ms(
            lambda: main_m.generate(feats, assistant_model=same_m, num_assistant_tokens=K, **kw), a.repeats)
        # a projection, not a measurement: every draft accepted at the kotoba assistant's round price, the decode
        # loop alone (no encoders, no prefill) -- ceil((tokens - 1) / (K + 1)) rounds
        r = res["rounds"][K]
        r["projected_all_accepted_ms"] = -(-(a.tokens - 1) // (K + 1)) * r["round_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
