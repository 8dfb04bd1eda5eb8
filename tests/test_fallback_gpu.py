"""GPU tests of the decoding fallback: kw_sample_step (csrc/sampling.hip) against kw_greedy_step, the float64
restatement tests/_fallback_ref.py and the pinned processors of oracle.generate.process_logits; then
generate(temperature=..., *_threshold=...) end to end against the transformers fixture tests/golden/fallback_tiny.npz.

Accuracy bound of the running log-probability (the project's bound for reductions, tests/test_token_ts_gpu.py): the
kernel's error against float64 may be at most 4x the error of torch's own float32 CPU computation against the same
float64 values, floor 1e-6 -- both taken as the largest over one case.
"""
import numpy as np
import pytest
import torch

import _fallback_ref as R
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

SEED, ATTEMPT = 0x123456789ABCDEF0, 3
P = 3


def _gen(V):
    """Generation constants (a dict, as oracle.generate takes them) for vocabulary size V; V = 1000 has its own small
    layout: text [0, 880), EOS 880, specials, <|notimestamps|> 899, timestamps [900, 1000)."""
    from kwhisper.config import LARGE_V3, TINY, generation_constants

    if V == 1000:
        return dict(eos_token_id=880, pad_token_id=879, no_timestamps_token_id=899, max_initial_timestamp_index=50,
                    suppress_tokens=[1, 2, 7, 300, 511, 512] + list(range(881, 899)), begin_suppress_tokens=[220, 880])
    return generation_constants({51865: TINY, 51866: LARGE_V3, 65545: LARGE_V3}[V]).to_dict()


def _history(rng, B, n, gd):
    """Row histories of n generated tokens, written directly.  Row kinds by b % 6: 0 text only, 1 ends with a lone
    timestamp, 2 ends with a timestamp pair, 3 text (its logits favour timestamps: the mass rule bans text), 4 already
    finished (EOS then pad), 5 text (the row tests make inactive)."""
    eos, pad, tsb = gd["eos_token_id"], gd["pad_token_id"], gd["no_timestamps_token_id"] + 1
    ok = np.setdiff1d(np.arange(3, eos - 1), np.asarray(gd["suppress_tokens"]))
    ids = np.zeros((B, P + n), np.int64)
    ids[:, :P] = [tsb - 107, tsb - 99, tsb - 6] if tsb > 1000 else [890, 891, 892]
    for b in range(B):
        row = rng.choice(ok, n)
        if n >= 1:
            row[0] = tsb + rng.integers(0, 5)
        kind = b % 6
        if kind == 1 and n >= 2:
            row[-1] = tsb + 20 + b % 7
        elif kind == 2 and n >= 3:
            row[-2:] = tsb + 30 + b % 5
        elif kind == 4 and n >= 3:
            row[2] = eos
            row[3:] = pad
        ids[b, P:] = row
    return ids


class Case:
    """One batch's device state and both step plans over the same logits buffer."""

    def __init__(self, B, V, rt, hist, max_length, *, active=None, noise=False, seed=SEED, attempt=ATTEMPT, inv_t=0.0):
        from kwhisper import ops

        self.B, self.V, self.rt, self.gd = B, V, rt, _gen(V)
        gd = self.gd
        dev = "cuda"
        self.L0 = hist.shape[1]
        width = max(max_length, self.L0) + 2
        self.logits = torch.zeros((B, V), device=dev)
        sup = torch.zeros(V, dtype=torch.uint8)
        sup[torch.tensor(gd["suppress_tokens"])] = 1
        self.sup = sup.to(dev)
        self.bsup = torch.tensor(gd["begin_suppress_tokens"], dtype=torch.int32, device=dev)
        cfg = dict(return_timestamps=rt, ts_begin=gd["no_timestamps_token_id"] + 1, no_ts_id=gd["no_timestamps_token_id"],
                   eos_id=gd["eos_token_id"], pad_id=gd["pad_token_id"],
                   max_initial_ts=gd["max_initial_timestamp_index"] if rt else None, max_length=max_length, begin_index=P)

        def state():
            ids = torch.zeros((B, width), dtype=torch.int64, device=dev)
            ids[:, : self.L0] = torch.from_numpy(hist)
            return dict(ids=ids, cur=torch.tensor([self.L0], dtype=torch.int32, device=dev),
                        unf=torch.ones(B, dtype=torch.int32, device=dev), cnt=torch.zeros(1, dtype=torch.int32, device=dev),
                        nun=torch.zeros(1, dtype=torch.int32, device=dev))

        self.s, self.g = state(), state()
        self.inv_t = torch.tensor([inv_t], dtype=torch.float32, device=dev)
        self.seed = torch.tensor([seed], dtype=torch.int64, device=dev)
        self.attempt = torch.tensor([attempt], dtype=torch.int32, device=dev)
        self.sum_lp = torch.zeros(B, dtype=torch.float32, device=dev)
        self.n_tok = torch.zeros(B, dtype=torch.int32, device=dev)
        self.active = None if active is None else torch.tensor(active, dtype=torch.uint8, device=dev)
        self.noise = torch.full((B, V), float("nan"), device=dev) if noise else None
        self.ws = torch.zeros(ops.sample_step_workspace_bytes(B) // 4 + 1, device=dev)
        self.gws = torch.zeros(ops.greedy_step_workspace_bytes(B) // 4 + 1, device=dev)
        s, g = self.s, self.g
        self.sample = ops.SamplePlan(self.logits, self.sup, self.bsup, s["ids"], s["cur"], s["unf"], s["cnt"], s["nun"],
                                     inv_temperature=self.inv_t, seed=self.seed, attempt=self.attempt,
                                     sum_logprob=self.sum_lp, n_tokens=self.n_tok, workspace=self.ws, active=self.active,
                                     noise_out=self.noise, **cfg)
        self.greedy = ops.SamplerPlan(self.logits, self.sup, self.bsup, g["ids"], g["cur"], g["unf"], g["cnt"], g["nun"],
                                      workspace=self.gws, **cfg)

    def set_logits(self, x):
        self.logits.copy_(torch.from_numpy(x))

    def processed(self, hist, x):
        from oracle.generate import process_logits

        return process_logits(hist, x, self.gd, P, self.rt)


def _logits(rng, B, V, gd, step=0):
    """Random logits with a spread of a few units; rows of kind 3 (b % 6 == 3) favour timestamps enough for the mass
    rule to ban text."""
    x = (rng.standard_normal((B, V)) * 3).astype(np.float32)
    tsb = gd["no_timestamps_token_id"] + 1
    x[3::6, tsb:] += 9.0
    return x


SHAPES = [(1, 51865), (5, 51866), (32, 51865), (32, 51866), (5, 1000), (32, 1000)]


# ---- equality with the greedy step at inv_temperature = 0 ---------------------------------------------------------
@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("scenario", ["first", "mid", "last"])
@pytest.mark.parametrize("B,V", SHAPES)
def test_argmax_equals_greedy_step(B, V, rt, scenario):
    """inv_temperature == 0: ids, unfinished, n_unfinished and cur_len are kw_greedy_step's on the same inputs, over
    three steps: the first step (begin-suppress; with timestamps max_initial_timestamp_index), rows after a lone
    timestamp, after a pair, under the text ban, already finished, and the step that reaches max_length."""
    rng = np.random.default_rng(B * 7 + V + 2 * rt + len(scenario))
    gd = _gen(V)
    n = 0 if scenario == "first" else 6
    hist = _history(rng, B, n, gd)
    max_length = hist.shape[1] + (1 if scenario == "last" else 40)
    c = Case(B, V, rt, hist, max_length)
    for step in range(3):
        c.set_logits(_logits(rng, B, V, gd, step))
        c.sample()
        c.greedy()
        torch.cuda.synchronize()
        for k in ("ids", "unf", "nun", "cur", "cnt"):
            assert torch.equal(c.s[k], c.g[k]), (k, step)
    assert int(c.s["cur"].item()) == hist.shape[1] + 3
    if scenario == "last":
        assert int(c.s["nun"].item()) == 0
    assert not c.ws.view(torch.int32)[B * 64: B * 65].any()  # per-row arrival counters back at zero
    assert c.noise is None


@pytest.mark.parametrize("rt", [False, True])
def test_tail_beyond_the_register_window(rt):
    """V = 65545 (_util.tail_case: the winner of row 0 and the deciding timestamp mass of row 1 lie in the elements a
    slice walks beyond its register-held window) at inv_temperature = 0: the stated tokens, every flag kw_greedy_step's,
    and sum_logprob against the float64 log-softmax of the processed row within test_running_logprob's bound."""
    from _util import TAIL_V, tail_case

    hist, x, want_nots, want_ts = tail_case()
    want = want_ts if rt else want_nots
    B, L = 3, hist.shape[1]
    c = Case(B, TAIL_V, rt, hist, L + 8)
    c.set_logits(x)
    c.sample()
    c.greedy()
    torch.cuda.synchronize()
    for k in ("ids", "unf", "nun", "cur", "cnt"):
        assert torch.equal(c.s[k], c.g[k]), k
    assert c.s["ids"][:, L].tolist() == want and c.s["unf"].tolist() == [1, 1, 1]
    assert (int(c.s["nun"].item()), int(c.s["cur"].item())) == (B, L + 1) and c.n_tok.tolist() == [1, 1, 1]
    s = c.processed(hist, x)
    rows = np.arange(B)
    want64 = R.log_softmax64(s)[rows, want]
    want32 = torch.log_softmax(torch.from_numpy(s), -1).numpy()[rows, want]
    err_gpu = float(np.abs(c.sum_lp.cpu().numpy() - want64).max())
    err_torch = float(np.abs(want32 - want64).max())
    print(f"sum_logprob V={TAIL_V} rt={rt}: err gpu {err_gpu:.3e} torch fp32 {err_torch:.3e}")
    assert err_gpu <= max(4 * err_torch, 1e-6)


# ---- running log-probability ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("inv_t", [0.0, 1.0])
@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("B,V,steps", [(5, 51866, 1), (32, 51865, 2), (5, 51865, 37), (32, 1000, 37), (1, 51866, 2)])
def test_running_logprob(B, V, steps, rt, inv_t):
    """sum_logprob against a float64 log-softmax of the processed scores (oracle.generate.process_logits) at the tokens
    the kernel chose, n_tokens exact, finished and inactive rows at 0."""
    rng = np.random.default_rng(B + V + steps + 5 * rt + int(inv_t))
    gd = _gen(V)
    hist = _history(rng, B, 6, gd)
    eos = gd["eos_token_id"]
    active = [0 if b % 6 == 5 else 1 for b in range(B)]
    c = Case(B, V, rt, hist, hist.shape[1] + steps + (0 if steps == 2 else 3), active=active, inv_t=inv_t)
    xs = []
    for step in range(steps):
        xs.append(_logits(rng, B, V, gd, step))
        c.set_logits(xs[-1])
        c.sample()
    torch.cuda.synchronize()
    ids = c.s["ids"].cpu().numpy()
    got, n_got = c.sum_lp.cpu().numpy(), c.n_tok.cpu().numpy()
    want64, want32, n_want = np.zeros(B), np.zeros(B, np.float32), np.zeros(B, np.int64)
    fin = np.array([(hist[b, P:] == eos).any() or not active[b] for b in range(B)])
    L = hist.shape[1]
    for step in range(steps):
        s = c.processed(ids[:, : L + step], xs[step])
        tok = ids[:, L + step]
        lp64 = R.log_softmax64(s)
        lp32 = torch.log_softmax(torch.from_numpy(s), -1).numpy()
        for b in range(B):
            if fin[b]:
                assert tok[b] == gd["pad_token_id"]
                continue
            assert np.isfinite(s[b, tok[b]]), (b, step)
            want64[b] += lp64[b, tok[b]]
            want32[b] = np.float32(want32[b] + lp32[b, tok[b]])
            n_want[b] += 1
            fin[b] = tok[b] == eos
    np.testing.assert_array_equal(n_got, n_want)
    assert (got[n_want == 0] == 0).all() and (n_want == 0).any() == (B > 4)
    err_gpu = float(np.abs(got - want64).max())
    err_torch = float(np.abs(want32 - want64).max())
    print(f"sum_logprob B={B} V={V} steps={steps} rt={rt} inv_t={inv_t}: err gpu {err_gpu:.3e} torch fp32 {err_torch:.3e}")
    assert err_gpu <= max(4 * err_torch, 1e-6)
    unf = c.s["unf"].cpu().numpy()
    assert int(c.s["nun"].item()) == int(unf.sum()) and not unf[[b for b in range(B) if not active[b]]].any()


# ---- noise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [51865, 51866, 1000])
def test_noise_is_the_documented_philox_stream(V):
    """noise_out: finite everywhere; its 20-bit uniform index, recovered through the documented map, is the numpy
    Philox restatement's for counter (v >> 2, L, row, attempt) and the seed's two halves; the same for the same
    (seed, attempt, row, L, v) at B = 5 and B = 32."""
    rng = np.random.default_rng(V)
    gd = _gen(V)
    out = {}
    for B in (5, 32):
        hist = _history(rng, 32, 6, gd)[:B]
        c = Case(B, V, True, hist, hist.shape[1] + 8, noise=True, inv_t=1.0)
        c.set_logits(_logits(np.random.default_rng(1), 32, V, gd)[:B])
        c.sample()
        torch.cuda.synchronize()
        out[B] = c.noise.cpu().numpy()
        assert np.isfinite(out[B]).all()
        assert out[B].min() >= -2.68 and out[B].max() <= 14.56
    assert np.array_equal(out[5], out[32][:5])
    L = P + 6
    for row in range(5):
        want = R.uniform_index(R.sample_draws(SEED, ATTEMPT, row, L, V))
        np.testing.assert_array_equal(R.index_of_gumbel(out[5][row]), want)
        # and forward: the stored f32 noise is the float64 map of that index within f32 rounding of logf twice
        np.testing.assert_allclose(out[5][row], R.gumbel_of_index(want), rtol=0, atol=4e-6)
    row, L2 = 31, L
    np.testing.assert_array_equal(R.index_of_gumbel(out[32][row]), R.uniform_index(R.sample_draws(SEED, ATTEMPT, row, L2, V)))


# ---- sampled token ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("inv_t", [2.5, 1.0])
@pytest.mark.parametrize("B,V", [(32, 51865), (5, 51866), (32, 1000)])
def test_sampled_token_is_the_perturbed_argmax(B, V, rt, inv_t):
    """The token is the float64 argmax of s * inv_T + noise_out over the finite processed scores (cases whose float64
    top-two gap is below 1e-4 are left out, at most 1 % of them), over 8 steps from the written histories."""
    rng = np.random.default_rng(B + V + 3 * rt + int(10 * inv_t))
    gd = _gen(V)
    hist = _history(rng, B, 6, gd)
    steps = 8
    c = Case(B, V, rt, hist, hist.shape[1] + steps + 2, noise=True, inv_t=inv_t)
    xs, noises = [], []
    for step in range(steps):
        xs.append(_logits(rng, B, V, gd, step))
        c.set_logits(xs[-1])
        c.sample()
        noises.append(c.noise.clone())
    torch.cuda.synchronize()
    ids = c.s["ids"].cpu().numpy()
    eos, L = gd["eos_token_id"], hist.shape[1]
    fin = np.array([(hist[b, P:] == eos).any() for b in range(B)])
    cases = skipped = 0
    for step in range(steps):
        s = c.processed(ids[:, : L + step], xs[step])
        g = noises[step].cpu().numpy()
        for b in range(B):
            if fin[b]:
                continue
            tok, gap = R.perturbed_argmax(s[b], inv_t, g[b])
            cases += 1
            if gap < 1e-4:
                skipped += 1
            else:
                assert ids[b, L + step] == tok, (b, step, gap)
            fin[b] = ids[b, L + step] == eos
    print(f"perturbed argmax B={B} V={V} rt={rt} inv_t={inv_t}: {cases} cases, {skipped} left out")
    assert cases >= steps * B // 2 and skipped <= 0.01 * cases


# ---- distribution -----------------------------------------------------------------------------------------------------
SIX = {100: 2.0, 2000: 1.5, 30000: 1.0, 5: 0.5, 45000: 0.0, 12345: -0.5}


@pytest.mark.parametrize("temperature", [0.4, 1.0])
def test_sampling_distribution(temperature):
    """32 rows with identical logits whose mass sits on six tokens, 64 steps: each token's count within 5 sigma of the
    binomial expectation from softmax(s / T); rows draw from distinct streams; (seed, attempt) reproduces bitwise and
    the next attempt does not."""
    B, V, steps = 32, 51865, 64
    gd = _gen(V)
    x = np.full((B, V), -40.0, np.float32)
    for t, v in SIX.items():
        assert t not in gd["suppress_tokens"] and t < gd["eos_token_id"]
        x[:, t] = v
    hist = np.tile(np.array([[50258, 50266, 50359, 11]], np.int64), (B, 1))  # (one generated token: no begin-suppress)

    def run(attempt):
        c = Case(B, V, False, hist, hist.shape[1] + steps + 1, attempt=attempt, inv_t=1.0 / temperature)
        c.set_logits(x)
        for _ in range(steps):
            c.sample()
        torch.cuda.synchronize()
        assert int(c.s["nun"].item()) == B
        return c.s["ids"].cpu().numpy()[:, hist.shape[1]: hist.shape[1] + steps]

    toks = run(ATTEMPT)
    assert np.isin(toks, list(SIX)).all()
    s = np.array(list(SIX.values()), np.float64) / temperature
    p = np.exp(s - s.max())
    p /= p.sum()
    n = B * steps
    for (t, _), pt in zip(SIX.items(), p):
        cnt, sigma = int((toks == t).sum()), np.sqrt(n * pt * (1 - pt))
        print(f"T={temperature} token {t}: count {cnt}, expected {n * pt:.1f} +- {sigma:.1f}")
        assert abs(cnt - n * pt) <= 5 * sigma
    assert len({tuple(r) for r in toks.tolist()}) == B
    assert np.array_equal(run(ATTEMPT), toks)
    assert not np.array_equal(run(ATTEMPT + 1), toks)


# ---- end to end: generate() against transformers (tests/golden/fallback_tiny.npz, tools/make_fixtures.py) ------------
import json  # noqa: E402

from kwhisper.config import TINY, generation_constants  # noqa: E402

# tools/make_fixtures.py FALLBACK_MODES: name -> (generate kwargs, eos override)
_A = dict(temperature=0.0, logprob_threshold=-1.0, compression_ratio_threshold=2.4, no_speech_threshold=8e-6)
FALLBACK_MODES = {
    "a_nots": (dict(_A, return_timestamps=False), None),
    "a_ts": (dict(_A, return_timestamps=True), None),
    "a_eos": (dict(_A, return_timestamps=False), 7656),
    "b_nots": (dict(return_timestamps=False, temperature=(0.0, 0.4), logprob_threshold=-4.2,
                    compression_ratio_threshold=2.4), None),
    "b_ts": (dict(return_timestamps=True, temperature=(0.0, 0.4), logprob_threshold=-5.0,
                  compression_ratio_threshold=1.45), None),
    "b_eos": (dict(return_timestamps=False, temperature=(0.0, 0.4), logprob_threshold=-4.2,
                   compression_ratio_threshold=1.2, no_speech_threshold=8e-6), 7656),
}
LP_TOL = 2e-3     # avg_logprob: the fp32 logit bar of test_gpu_generate.py (1e-3) on the token's score and on the normaliser
NSP_RTOL = 4e-3   # no_speech_prob: the same bound on its logit and its normaliser, relative


def _model(dtype):
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import synthetic_state_dict

    return KWhisperForConditionalGeneration.from_state_dict(TINY, synthetic_state_dict(TINY, 0), dtype=dtype,
                                                            generation_config=generation_constants(TINY))


@pytest.fixture(scope="module")
def tiny32():
    return _model(torch.float32)


@pytest.fixture(scope="module")
def tiny16():
    return _model(torch.bfloat16)


@pytest.fixture(scope="module")
def clips(gold):
    """The fixture's clips plus one row of digital silence (the last), as oracle log-mel features."""
    from _util import audio_cases
    from oracle.mel import log_mel

    g = gold("fallback_tiny")
    audio = np.concatenate([audio_cases(g["cases"]), np.zeros((1, 480000), np.float32)])
    return log_mel(audio, TINY.num_mel_bins)


@pytest.fixture(scope="module")
def oracle_enc(clips):
    """The numpy oracle and its encoder output of every clip (computed once, read only)."""
    from kwhisper.synthetic import synthetic_state_dict
    from oracle.whisper_np import WhisperNP

    m = WhisperNP(synthetic_state_dict(TINY, 0), TINY)
    return m, m.encode(clips)


def _run(model, feats, mode, g, seed=7):
    kw, eos = FALLBACK_MODES[mode]
    gen = generation_constants(TINY)
    if eos is not None:
        gen.eos_token_id = eos
    model.manual_seed(seed)
    model.record_pass_ids = True
    try:
        res = model.generate(torch.from_numpy(feats).cuda(), language="ja", task="transcribe",
                             max_length=int(g["max_length"]), return_segments=True, generation_config=gen, **kw)
    finally:
        model.record_pass_ids = False
    return res, model.stats, gen


def _segs(res):
    return [[(float(s["start"]), float(s["end"]), [int(t) for t in s["tokens"]]) for s in row] for row in res["segments"]]


def _check_decisions(stats, kw):
    """Every recorded decision follows from the recorded numbers (_need_fallback's rule)."""
    thr = {k: kw.get(k) for k in ("compression_ratio_threshold", "logprob_threshold", "no_speech_threshold")}
    for ps in stats["fallback"]:
        for at in ps:
            for j in range(len(at["rows"])):
                want = R.need_fallback(compression=at["compression_ratio"][j], avg_lp=at["avg_logprob"][j],
                                       no_speech_prob=at["no_speech_prob"][j], **thr)
                assert (at["needs_fallback"][j], at["should_skip"][j]) == want


def _check_attempt(got, want, ns):
    assert got["rows"] == want["rows"] and got["temperature"] == want["temperature"]
    d = np.abs(np.array(got["avg_logprob"]) - np.array(want["avg_logprob"]))
    print(f"   rows {got['rows']}: avg_logprob max diff {d.max():.2e}")
    assert (d <= LP_TOL).all()
    assert got["compression_ratio"] == want["compression_ratio"]
    if ns:
        np.testing.assert_allclose(got["no_speech_prob"], want["no_speech_prob"], rtol=NSP_RTOL, atol=0)
    assert got["needs_fallback"] == want["needs_fallback"] and got["should_skip"] == want["should_skip"]


@pytest.mark.parametrize("mode", ["a_nots", "a_ts", "a_eos"])
def test_thresholds_one_temperature_vs_transformers(gold, tiny32, clips, mode):
    """Mode (a), tiny fp32: one temperature (0.0) with all three thresholds -- the silent row and no other is skipped;
    sequences, segments and skipped rows equal transformers' exactly, the statistics within the fp32 bars."""
    g = gold("fallback_tiny")
    res, stats, _ = _run(tiny32, clips, mode, g)
    np.testing.assert_array_equal(res["sequences"].cpu().numpy(), g[f"{mode}_sequences"])
    want_segs = json.loads(str(g[f"{mode}_segments"]))
    got_segs = _segs(res)
    assert len(got_segs) == len(want_segs)
    for a, b in zip(got_segs, want_segs):
        assert len(a) == len(b)
        for (s0, e0, t0), (s1, e1, t1) in zip(a, b):
            assert t0 == t1 and abs(s0 - s1) < 1e-9 and abs(e0 - e1) < 1e-9
    want = json.loads(str(g[f"{mode}_passes"]))
    assert len(stats["fallback"]) == len(want)
    skipped = set()
    for ps, wp in zip(stats["fallback"], want):
        assert len(ps) == len(wp["attempts"]) == 1
        _check_attempt(ps[0], wp["attempts"][0], True)
        skipped |= {r for r, sk in zip(ps[0]["rows"], ps[0]["should_skip"]) if sk}
    assert skipped == {clips.shape[0] - 1} and got_segs[-1] == []
    _check_decisions(stats, FALLBACK_MODES[mode][0])


def _first_attempts(passes):
    """row -> its first-attempt record (avg_logprob, compression ratio, needs_fallback) of every pass it was in."""
    out = {}
    for ps in passes:
        at = ps[0] if isinstance(ps, list) else ps["attempts"][0]
        for j, r in enumerate(at["rows"]):
            out.setdefault(r, []).append((at["avg_logprob"][j], at["compression_ratio"][j], at["needs_fallback"][j],
                                          at["should_skip"][j]))
    return out


@pytest.mark.parametrize("mode", ["b_nots", "b_ts", "b_eos"])
def test_temperature_schedule_vs_transformers(gold, tiny32, clips, oracle_enc, mode):
    """Mode (b), tiny fp32, temperature (0.0, 0.4): the first attempt's statistics and the rows that fall back equal
    transformers'; rows that fall back in no pass keep transformers' final tokens; rows that did fall back carry the
    engine's own draws, so they are checked against the oracle: every sampled token has a finite processed score,
    the reported avg_logprob is the oracle's on those tokens, and the decision follows from the recorded numbers."""
    from oracle.generate import process_logits

    g = gold("fallback_tiny")
    kw, _ = FALLBACK_MODES[mode]
    res, stats, gen = _run(tiny32, clips, mode, g)
    want = json.loads(str(g[f"{mode}_passes"]))
    _check_attempt(stats["fallback"][0][0], want[0]["attempts"][0], kw.get("no_speech_threshold") is not None)
    fa_got, fa_want = _first_attempts(stats["fallback"]), _first_attempts(want)
    clean = []
    for r in range(clips.shape[0]):
        # a row's k-th pass is comparable while it fell back in no earlier pass on either side
        for k, (a, b) in enumerate(zip(fa_got[r], fa_want[r])):
            assert abs(a[0] - b[0]) <= LP_TOL and a[1:] == b[1:], (r, k, a, b)
            if a[2] or b[2]:
                break
        else:
            if len(fa_got[r]) == len(fa_want[r]):
                clean.append(r)
    fell0 = [r for r, n in zip(stats["fallback"][0][0]["rows"], stats["fallback"][0][0]["needs_fallback"]) if n]
    print(f"{mode}: rows falling back in pass 0 {fell0}; rows that never fall back {clean}")
    assert fell0 and clean
    got_segs, want_segs = _segs(res), json.loads(str(g[f"{mode}_segments"]))
    for r in clean:
        assert [s[2] for s in got_segs[r]] == [s[2] for s in want_segs[r]], r
    _check_decisions(stats, kw)
    # pass 0's sampled rows, teacher-forced through the oracle
    model, enc = oracle_enc
    gd, rt, P = gen.to_dict(), kw["return_timestamps"], 3 if kw["return_timestamps"] else 4
    ids0 = stats["pass_ids"][0]
    last = stats["fallback"][0][-1]
    assert last["temperature"] == 0.4 and last["rows"] == fell0
    for j, r in enumerate(last["rows"]):
        row = ids0[r]
        body = R.strip_padding(row[P:], gen.pad_token_id, gen.eos_token_id)
        seq = row[: P + len(body)][None]
        logits = model.decode(seq[:, :-1], model.new_cache(enc[r: r + 1]))[0, P - 1:]
        total = 0.0
        for t in range(len(body)):
            s = process_logits(seq[:, : P + t], logits[t][None], gd, P, rt)[0]
            assert np.isfinite(s[body[t]]), (r, t)
            total += R.log_softmax64(s)[body[t]]
        print(f"   row {r}: {len(body)} sampled tokens, avg_logprob {last['avg_logprob'][j]:.4f} oracle {total / len(body):.4f}")
        assert abs(last["avg_logprob"][j] - total / len(body)) <= LP_TOL


def test_manual_seed_reproduces_and_default_path_is_unchanged(gold, tiny32, clips):
    """Two runs after manual_seed(7) are identical (tokens and statistics), another seed draws other tokens, and a run
    without any of the new arguments still equals the tiny_fp32 fixture."""
    from _util import TINY_MODES, oracle_features

    g = gold("fallback_tiny")
    a, sa, _ = _run(tiny32, clips, "b_eos", g)
    b, sb, _ = _run(tiny32, clips, "b_eos", g)
    assert torch.equal(a["sequences"], b["sequences"]) and sa["fallback"] == sb["fallback"]
    c, _, _ = _run(tiny32, clips, "b_eos", g, seed=8)
    assert not torch.equal(a["sequences"], c["sequences"])
    g0 = gold("tiny_fp32")
    kw, _ = TINY_MODES["greedy"]
    feats = torch.from_numpy(oracle_features(TINY, g0["cases"])).cuda()
    toks = tiny32.generate(feats, max_length=int(g0["max_length"]), **kw)
    np.testing.assert_array_equal(toks.cpu().numpy(), g0["greedy_tokens"])
    assert "fallback" not in tiny32.stats


def test_argument_errors(tiny32, clips):
    feats = torch.from_numpy(clips[:2]).cuda()
    with pytest.raises(ValueError, match="logprob_threshold"):
        tiny32.generate(feats, language="ja", no_speech_threshold=0.6)
    for bad in (dict(num_beams=2), dict(return_token_timestamps=True), dict(condition_on_prev_tokens=True)):
        with pytest.raises(NotImplementedError):
            tiny32.generate(feats, language="ja", temperature=(0.0, 0.2), logprob_threshold=-1.0, **bad)
    with pytest.raises(NotImplementedError):
        tiny32.generate(feats, language="ja", temperature=0.2, output_scores=True)
    # temperature=None with a threshold is 0.0
    out = tiny32.generate(feats, language="ja", temperature=None, logprob_threshold=-1.0, max_length=12)
    assert tiny32.stats["fallback"][0][0]["temperature"] == 0.0 and out.shape[0] == 2


# ---- bf16 ----------------------------------------------------------------------------------------------------------
def test_bf16_generate_and_session_logprob(gold, tiny16, clips):
    """bf16 engine: the mode (b) call completes, and a session's avg_logprob agrees with a float64 recomputation from
    the logits the same session recorded (record_scores) within the kernel bound."""
    from oracle.generate import process_logits

    g = gold("fallback_tiny")
    res, stats, gen = _run(tiny16, clips, "b_ts", g)
    assert res["sequences"].shape[0] == clips.shape[0] and stats["fallback"]
    _check_decisions(stats, FALLBACK_MODES["b_ts"][0])
    eng = tiny16.engine
    B = clips.shape[0]
    sess = eng.new_session(B, eng.encode(torch.from_numpy(clips).cuda()))
    gen = generation_constants(TINY)
    gen.eos_token_id = 7656
    prompt = torch.tensor([[gen.decoder_start_token_id, gen.lang_to_id["<|ja|>"], gen.task_to_id["transcribe"]]] * B)
    P = prompt.shape[1]
    active = np.array([True, True, False, True, True])
    ids = sess.generate(prompt, gen, max_length=40, return_timestamps=True, record_scores=True,
                        sample=dict(temperature=0.4, seed=7, attempt=1, active=active))
    gd = gen.to_dict()
    want64, want32, n = np.zeros(B), np.zeros(B, np.float32), np.zeros(B, np.int64)
    fin = ~active
    for t in range(ids.shape[1] - P):
        raw = sess.scores[t][0].cpu().numpy()
        s = process_logits(ids[:, : P + t], raw, gd, P, True)
        lp64, lp32 = R.log_softmax64(s), torch.log_softmax(torch.from_numpy(s), -1).numpy()
        for b in range(B):
            if not fin[b]:
                tok = ids[b, P + t]
                want64[b] += lp64[b, tok]
                want32[b] = np.float32(want32[b] + lp32[b, tok])
                n[b] += 1
                fin[b] = tok == gen.eos_token_id
    np.testing.assert_array_equal(sess.n_tokens, n)
    assert n[2] == 0 and (ids[2, P:] == gen.pad_token_id).all()
    got = sess.avg_logprob[active] * n[active]
    err_gpu = float(np.abs(got - want64[active]).max())
    err_torch = float(np.abs(want32[active] - want64[active]).max())
    print(f"bf16 session sum_logprob: err gpu {err_gpu:.3e} torch fp32 {err_torch:.3e}; tokens per row {n.tolist()}")
    assert err_gpu <= max(4 * err_torch, 1e-6)


FB_KW = dict(num_beams=1, temperature=(0.0, 0.4), logprob_threshold=-4.2, compression_ratio_threshold=2.4,
             no_speech_threshold=8e-6)


def test_pipeline_and_pseudo_label_take_the_thresholds(tiny16, clips):
    """The chunked pipeline (generate_kwargs) and the pseudo-labelling loop (gen_kwargs) hand the fallback arguments
    to generate(): one short clip each, bf16."""
    from _util import OracleFeatureExtractor, StubTok
    from kwhisper.pipeline import ASRPipeline
    from kwhisper.pseudo_label import pseudo_label
    from kwhisper.synthetic import dummy_audio

    pipe = ASRPipeline(tiny16, feature_extractor=OracleFeatureExtractor(TINY.num_mel_bins),
                       tokenizer=StubTok(generation_constants(TINY)), chunk_length_s=15, batch_size=2,
                       generate_kwargs=dict(FB_KW, language="ja", task="transcribe", max_new_tokens=12))
    out = pipe({"array": dummy_audio(0)[: 16000 * 20], "sampling_rate": 16000})
    assert isinstance(out["text"], str) and tiny16.stats["fallback"]
    feats = torch.from_numpy(clips[:2]).cuda()
    tiny16.stats = {}
    ids, preds = pseudo_label(tiny16, lambda idx: feats[list(idx)], 2, batch_size=2, pad_token_id=50257,
                              gen_kwargs=dict(FB_KW, language="ja", task="transcribe", max_length=16))
    assert list(ids) == [0, 1] and len(preds) == 2 and tiny16.stats["fallback"]


def test_ctypes_backend_gives_the_same_step():
    """kw_sample_step through the ctypes binding of the C ABI (kw_sample_args filled in Python) == through
    torch.ops.kw.sample_step, bit for bit: tokens, running statistics and the stored noise."""
    from kwhisper import ops

    gd = _gen(51866)
    hist = _history(np.random.default_rng(3), 5, 6, gd)
    xs = [_logits(np.random.default_rng(4 + i), 5, 51866, gd) for i in range(2)]
    outs = []
    for backend in ("torch", "ctypes"):
        old = ops.set_backend(backend)
        try:
            c = Case(5, 51866, True, hist, hist.shape[1] + 4, noise=True, inv_t=2.5, active=[1, 1, 1, 0, 1])
            for x in xs:
                c.set_logits(x)
                c.sample()
            torch.cuda.synchronize()
        finally:
            ops.set_backend(old)
        outs.append([t.cpu() for t in (c.s["ids"], c.s["unf"], c.s["nun"], c.s["cur"], c.sum_lp, c.n_tok, c.noise)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert outs[0][5][3:].tolist() == [0, 0] and (outs[0][5][:3] >= 1).all()  # inactive / finished rows count nothing
