"""GPU tests of ``repetition_penalty`` / ``no_repeat_ngram_size``: kw_repeat_process (csrc/repeat.hip) and
kw_beam_logprobs_rep (csrc/beam.hip) against the numpy restatement tests/_repeat_ref.py (which tests/test_repeat_cpu.py
holds to transformers' own processors bit for bit), and generate() on the tiny model against transformers
(tests/golden/repeat_tiny.npz, tools/make_repeat_fixture.py).

fp32 engine: cases a, b, d equal the fixture up to the first step whose top-2 margin in the fixture is under the fp32
logit bar of tests/test_prompt_gpu.py (1e-3); at most one (case, row) is cut short there.  Case c (beams) is held bit
exact, as tests/test_gpu_generate.py holds its beam fixtures.  Case e: the temperature-0 attempt.  bf16 engine: the
structural property of no_repeat_ngram_size, which no arithmetic can blur."""
import ctypes
import json

import numpy as np
import pytest
import torch

import _beam_ref as BR
import _repeat_ref as RR
from conftest import gpu_available

from kwhisper.config import TINY, generation_constants

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

F32 = np.float32
G = generation_constants(TINY)
LOGIT_BAR = 1e-3  # tests/test_prompt_gpu.py's
LP_TOL = 2e-3     # avg_logprob: tests/test_fallback_gpu.py's bar
LP_RTOL, LP_ATOL = 1e-6, 1e-5  # tests/test_gpu_beam_kernels.py's bound on kw_beam_logprobs' values, kept here
STRIDE = 512
REPEATS = [(p, n) for p in (1.0, 1.3, 0.7) for n in (0, 1, 2, 3, 6)]


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype).contiguous()


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


# ------------------------------------------------------------------------------------------- kw_repeat_process
def _history(V, L, rng):
    """(3, L) histories.  Every token occurs 3-4 times where L allows (a scatter that does not wait for every gather
    penalises such a token twice), tokens 0, 31, 32 and V-1 are among them, one id is out of range, and from L = 12 on
    the row ends with the first five tokens of an earlier 6-gram (so n = 2 .. 6 each ban that window's next token)."""
    rows = []
    for r in range(3):
        if L < 12:
            pair = [(0, V - 1), (31, 32), (V - 1, V + 5)][r]  # (row 2: an id past the vocabulary)
            rows.append([pair[i % 2] for i in range(L)])
            continue
        pool = np.concatenate([[0, 31, 32, V - 1], rng.choice(np.arange(33, V - 1), L // 4, replace=False)])
        seq = np.concatenate([pool] * 4)[: L - 5]
        rng.shuffle(seq)
        seq[7 + r] = -3 if r else V + 5  # out of range, never dereferenced
        k = 20 + 3 * r
        rows.append(np.concatenate([seq, seq[k: k + 5]]).tolist())
    return np.array(rows, np.int64)


def _scores(V, hist, rng):
    """Random scores of both signs with the special values at history tokens: 0.0, -0.0, -inf, +inf, NaN."""
    x = (rng.standard_normal((3, V)) * 4).astype(F32)
    for r, row in enumerate(hist):
        toks = [int(t) for t in dict.fromkeys(row.tolist()) if 0 <= t < V]
        for t, v in zip(toks[1:], [0.0, -0.0, -np.inf, np.inf, np.nan]):
            x[r, t] = v
    return x


def _run_repeat(x, hist, penalty, ngram, backend):
    from kwhisper import ops

    ids = torch.full((3, STRIDE), -77, dtype=torch.int64, device="cuda")  # (past L: a canary no launch may read as a token)
    ids[:, : hist.shape[1]] = cu(hist, torch.int64)
    cur = cu(np.array([hist.shape[1]]), torch.int32)
    s = cu(x, torch.float32)
    old = ops.set_backend(backend)
    try:
        ops.RepeatPlan(s, ids, cur, penalty=penalty, ngram=ngram)()
    finally:
        ops.set_backend(old)
    torch.cuda.synchronize()
    return s.cpu().numpy()


@pytest.mark.parametrize("L", [1, 2, 3, 5, 448])
@pytest.mark.parametrize("V", [1000, 51866])
def test_repeat_process_bitwise(V, L):
    """Every (penalty, n) of {1.0, 1.3, 0.7} x {0, 1, 2, 3, 6}: the whole buffer -- the penalised, the banned and the
    untouched elements -- is bit for bit the restatement's, through the ctypes and the torch.ops backend; (1.0, 0) is
    the identity."""
    rng = np.random.default_rng(V + L)
    hist = _history(V, L, rng)
    x = _scores(V, hist, rng)
    changed = 0
    for penalty, ngram in REPEATS:
        want = RR.repeat_process(hist, x, penalty, ngram)
        got = {be: _run_repeat(x, hist, penalty, ngram, be) for be in ("ctypes", "torch")}
        for be, g in got.items():
            bad = np.nonzero(_bits(g) != _bits(want))
            assert bad[0].size == 0, (be, penalty, ngram, bad[0][:5], bad[1][:5], g[bad][:5], want[bad][:5])
        if (penalty, ngram) == (1.0, 0):
            assert (_bits(got["torch"]) == _bits(x)).all()
        changed += int((_bits(want) != _bits(x)).sum())
        if ngram and L >= max(ngram, 12):
            assert (np.isneginf(want) & ~np.isneginf(x)).any(), (penalty, ngram)  # the case does ban something
    assert changed


def test_repeat_process_many_rows_in_flight():
    """The gather / scatter barrier under load.  With three rows the waves of a workgroup run in step and a scatter
    that does not wait for the other waves' gathers still lands after them; with 4096 rows of V = 51866 in flight
    their loads come back far enough apart that a build without the barrier penalised 75-278 elements twice in each of
    five runs (and none at R = 3 or at V = 1000).  Every token occurs four times at shuffled positions; the history
    tokens are compared bit for bit, and nothing else may differ from the input."""
    from kwhisper import ops

    R, V, L, U = 4096, 51866, 448, 112
    rng = np.random.default_rng(5)
    base = rng.choice(V, U, replace=False)
    pool = (base[None, :] + 97 * np.arange(R)[:, None]) % V             # each row's U distinct tokens
    idx = rng.permuted(np.tile(np.arange(U), (R, 4)), axis=1)           # ... four times each, shuffled per row
    hist = np.take_along_axis(pool, idx, axis=1).astype(np.int64)
    ids = torch.zeros((R, STRIDE), dtype=torch.int64, device="cuda")
    ids[:, :L] = cu(hist, torch.int64)
    x = torch.randn((R, V), device="cuda") * 4
    s = x.clone()
    ops.RepeatPlan(s, ids, cu(np.array([L]), torch.int32), penalty=1.3, ngram=0)()
    torch.cuda.synchronize()
    pool_t = cu(pool, torch.int64)
    org, got = x.gather(1, pool_t).cpu().numpy(), s.gather(1, pool_t).cpu().numpy()
    want = RR.repeat_process(idx, org, 1.3, 0)  # (the same problem over each row's own U tokens)
    wrong = int((_bits(got) != _bits(want)).sum())
    assert wrong == 0, f"{wrong} history tokens are not the once-penalised original"
    assert int((s != x).sum()) == int((_bits(want) != _bits(org)).sum())


def test_repeat_process_rejects_bad_arguments():
    from kwhisper import _lib as L
    from kwhisper import ops

    lib = L.load()
    s = torch.zeros((2, 100), device="cuda")
    ids = torch.zeros((2, STRIDE), dtype=torch.int64, device="cuda")
    cur = torch.ones(1, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(sp, ip, cp, penalty, ngram, stride=STRIDE):
        return lib.kw_repeat_process(sp, 2, 100, ip, stride, cp, penalty, ngram, _s())

    for args in [(None, p(ids), p(cur), 1.3, 2), (p(s), None, p(cur), 1.3, 2), (p(s), p(ids), None, 1.3, 2),
                 (p(s), p(ids), p(cur), 0.0, 2), (p(s), p(ids), p(cur), -1.0, 2), (p(s), p(ids), p(cur), float("inf"), 2),
                 (p(s), p(ids), p(cur), float("nan"), 2), (p(s), p(ids), p(cur), 1.3, -1)]:
        assert call(*args) == L.KW_EINVAL, args
        assert b"kw_repeat_process" in lib.kw_last_error()
    assert call(p(s), p(ids), p(cur), 1.3, 2, stride=5000) == L.KW_EUNSUPPORTED
    for penalty, ngram in [(0.0, 0), (float("nan"), 0), (1.3, -2)]:
        with pytest.raises(ValueError):
            ops.RepeatPlan(s, ids, cur, penalty=penalty, ngram=ngram)
    torch.cuda.synchronize()
    assert (s == 0).all()  # nothing was launched


# ------------------------------------------------------------------------------------------- kw_beam_logprobs_rep
def _lp_case(V, L, rt):
    """R = 4 rows (2 items x 2 beams), k = 4, inputs as test_beam_logprobs_vs_reference builds them
    (tests/test_gpu_beam_kernels.py _lp_inputs: grid logits, k + 2 tied best text tokens and timestamps) with histories
    of length L made of each row's own best tokens: every token three or more times where L allows, and the row ends
    on the first two tokens of an earlier trigram, so both processors hit candidates."""
    from test_gpu_beam_kernels import P0, _lp_inputs

    k = 4
    gen, _, x = _lp_inputs(4, V, k, "begin")
    ts = gen["no_timestamps_token_id"] + 1
    rng = np.random.default_rng(V + L + rt)
    hist = np.zeros((4, L), np.int64)
    hist[:, :P0] = [2, 4, 7]
    for r in range(4):
        best = np.argsort(-x[r, :gen["eos_token_id"]], kind="stable")[:6]  # the tied best text tokens
        if L - P0 == 1:
            hist[r, P0:] = best[0]
            continue
        body = [ts + 1, ts + 1] if rt else []
        pat = [int(best[0]), int(best[1]), int(best[2]), int(best[0]), int(best[3]), int(best[1])]
        while len(body) < L - P0 - 2:
            body.append(pat[len(body) % len(pat)] if rng.random() < 0.8 else int(rng.integers(8, 200)))
        body = body[: L - P0 - 2]
        body[-3:] = [int(best[0]), int(best[1]), int(best[2])]  # ... a b c
        hist[r, P0:] = body + [int(best[0]), int(best[1])]      # ... a b: n = 3 bans c (n = 2: what followed b)
    return gen, hist, x, k


def _run_lp(gen, hist, x, k, rt, split, repeat):
    from kwhisper import _lib as L
    from kwhisper import ops
    from test_gpu_beam_kernels import P0, logprobs_args

    Rn, V = x.shape
    ids = torch.zeros((Rn, 64), dtype=torch.int64, device="cuda")
    ids[:, : hist.shape[1]] = cu(hist, torch.int64)
    sup = np.zeros(V, np.uint8)
    sup[gen["suppress_tokens"]] = 1
    keep = (cu(x, torch.float32), cu(sup, torch.uint8), cu(np.array(gen["begin_suppress_tokens"]), torch.int32), ids,
            cu(np.array([hist.shape[1]]), torch.int32), torch.full((Rn, k), 7.0, device="cuda"),
            torch.full((Rn, k), 7, dtype=torch.int32, device="cuda"), cu(np.array([0]), torch.int32),
            torch.zeros(ops.beam_logprobs_workspace_bytes(Rn) // 4 + 1, device="cuda") if split else None)
    a = logprobs_args(*keep, gen, rt, P0, k)
    lib = L.load()
    for _ in range(2):  # the split kernel's arrival counters re-arm
        if repeat is None:
            L.check(lib.kw_beam_logprobs(ctypes.byref(a), _s()), "kw_beam_logprobs")
        else:
            L.check(lib.kw_beam_logprobs_rep(ctypes.byref(a), repeat[0], repeat[1], _s()), "kw_beam_logprobs_rep")
    torch.cuda.synchronize()
    return keep[5].cpu().numpy(), keep[6].cpu().numpy()


@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("L", [4, 60])
@pytest.mark.parametrize("V", [1000, 51866])
def test_beam_logprobs_rep_vs_reference(V, L, split, rt):
    """cand_idx exact, values within test_gpu_beam_kernels.py's LP_RTOL / LP_ATOL of the restatement whose normaliser
    is summed in float64 (tests/_repeat_ref.py over oracle.generate); (1.0, 0) is bitwise kw_beam_logprobs.  Conditions
    on the inputs, checked here: the reference's k-th and (k+1)-th best are equal or 1e-3 apart (a tie or no question
    of rounding), and the timestamp rule's margin is 1e-3 from zero."""
    gen, hist, x, k = _lp_case(V, L, rt)
    plain = _run_lp(gen, hist, x, k, rt, split, None)
    off = _run_lp(gen, hist, x, k, rt, split, (1.0, 0))
    assert (_bits(off[0]) == _bits(plain[0])).all() and (off[1] == plain[1]).all()
    hit = 0
    for penalty, ngram in [(1.3, 3), (0.7, 2), (1.3, 0), (1.0, 3), (1.3, 1)]:
        want = RR.processed_logprobs_rep(hist, x, gen, 3, rt, penalty, ngram)
        wv, wi = BR.row_candidates(want, k)
        srt = -np.sort(-want, axis=-1)[:, : k + 1]
        gaps = srt[:, :-1] - srt[:, 1:]
        with np.errstate(invalid="ignore"):
            assert ((gaps == 0) | (gaps >= 1e-3) | ~np.isfinite(gaps)).all(), gaps
        if rt:
            margin = RR.timestamp_margin_rep(hist, x, gen, 3, penalty, ngram)
            assert (np.abs(margin) >= 1e-3).all(), margin
        cv, ci = _run_lp(gen, hist, x, k, rt, split, (penalty, ngram))
        fin = np.isfinite(wv) & np.isfinite(cv)
        err = np.abs(cv[fin] - wv[fin])
        print(f"({penalty}, {ngram}) split={split}: max |log-prob - reference| {err.max() if err.size else 0.0:.3g}")
        np.testing.assert_array_equal(ci, wi, err_msg=f"{penalty}, {ngram}")
        np.testing.assert_array_equal(np.isneginf(cv), np.isneginf(wv))
        np.testing.assert_allclose(cv, wv, rtol=LP_RTOL, atol=LP_ATOL)
        hit += int((ci != plain[1]).any())
    assert hit >= 3  # the processors did change the candidates


def test_beam_logprobs_rep_rejects_bad_arguments():
    from kwhisper import _lib as L

    gen, hist, x, k = _lp_case(1000, 4, False)
    lib = L.load()
    from test_gpu_beam_kernels import logprobs_args

    t = (cu(x, torch.float32), torch.zeros(1000, dtype=torch.uint8, device="cuda"),
         cu(np.array(gen["begin_suppress_tokens"]), torch.int32), torch.zeros((4, 64), dtype=torch.int64, device="cuda"),
         cu(np.array([4]), torch.int32), torch.full((4, k), 7.0, device="cuda"),
         torch.full((4, k), 7, dtype=torch.int32, device="cuda"), cu(np.array([0]), torch.int32), None)
    a = logprobs_args(*t, gen, False, 3, k)
    for penalty, ngram in [(0.0, 0), (-1.3, 0), (float("inf"), 0), (float("nan"), 2), (1.3, -1)]:
        assert lib.kw_beam_logprobs_rep(ctypes.byref(a), penalty, ngram, _s()) == L.KW_EINVAL
        assert b"kw_beam_logprobs_rep" in lib.kw_last_error()
    assert lib.kw_beam_logprobs_rep(None, 1.3, 2, _s()) == L.KW_EINVAL
    a.V = 70000
    assert lib.kw_beam_logprobs_rep(ctypes.byref(a), 1.3, 2, _s()) == L.KW_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (t[5] == 7.0).all()


# ------------------------------------------------------------------------------------------- generate()
def _model(dtype, **kw):
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import synthetic_state_dict

    return KWhisperForConditionalGeneration.from_state_dict(TINY, synthetic_state_dict(TINY, 0), dtype=dtype,
                                                            generation_config=generation_constants(TINY), **kw)


@pytest.fixture(scope="module")
def tiny32():
    return _model(torch.float32)


@pytest.fixture(scope="module")
def tiny16():
    return _model(torch.bfloat16)


@pytest.fixture(scope="module")
def feats(gold):
    from _util import oracle_features

    return torch.from_numpy(oracle_features(TINY, gold("repeat_tiny")["cases"])).cuda()


@pytest.fixture(scope="module")
def feats_silent(gold):
    """Case e's input: the clips and one row of digital silence (tools/make_fixtures.py fallback_features)."""
    from _util import audio_cases
    from oracle.mel import log_mel

    audio = np.concatenate([audio_cases(gold("repeat_tiny")["cases"]), np.zeros((1, 480000), np.float32)])
    return torch.from_numpy(log_mel(audio, TINY.num_mel_bins)).cuda()


def _args(g, case):
    return json.loads(str(g["args"]))[case]


CUT = {}  # (case, row) -> the step a comparison stopped at, over the module's fixture cases


def _compare_rows(case, got, want, margin, offset=0):
    """Rows equal up to their first step whose fixture margin is under LOGIT_BAR (``offset``: columns of ``want`` ahead
    of the first step); returns the rows compared in full."""
    full = []
    for b in range(want.shape[0]):
        low = np.nonzero(margin[b] < LOGIT_BAR)[0]
        n = offset + int(low[0]) if low.size else want.shape[1]
        if low.size:
            CUT[(case, b)] = n
        else:
            full.append(b)
        np.testing.assert_array_equal(got[b, :n], want[b, :n], err_msg=f"case {case} row {b}")
    print(f"case {case}: rows compared only up to a low-margin step so far: {CUT}")
    assert len(CUT) <= 1, CUT
    return full


def _check_segments(res, segs, rows):
    for b in rows:
        assert [len(s["tokens"]) for s in res["segments"][b]] == [s[2] for s in segs[b]]
        if segs[b]:
            np.testing.assert_allclose([(s["start"], s["end"]) for s in res["segments"][b]], [s[:2] for s in segs[b]],
                                       atol=1e-9)


def test_case_a_penalty_greedy(gold, tiny32, feats):
    g = gold("repeat_tiny")
    kw = dict(language="ja", task="transcribe", return_timestamps=False, max_length=int(g["max_length"]))
    got = tiny32.generate(feats, **kw, **_args(g, "a")).cpu().numpy()
    want, margin = g["a_tokens"], g["a_margin"]
    full = _compare_rows("a", got, want, margin, offset=want.shape[1] - margin.shape[1])
    assert got.shape == want.shape or len(full) < want.shape[0]
    assert not tiny32._sessions[(4, 1)].lm_greedy_last


def test_case_b_ngram_timestamps(gold, tiny32, feats):
    g = gold("repeat_tiny")
    res = tiny32.generate(feats, language="ja", return_timestamps=True, return_segments=True,
                          max_length=int(g["max_length"]), **_args(g, "b"))
    full = _compare_rows("b", res["sequences"].cpu().numpy(), g["b_sequences"], g["b_margin"])
    _check_segments(res, json.loads(str(g["b_segments"])), full)


def test_case_c_beams(gold, tiny32, feats):
    """Both processors on the beam rows' log-probs (kw_beam_logprobs_rep, each beam's own re-ordered history): bit
    exact tokens, as test_gpu_generate.py::test_tiny_fp32_beam_bitexact holds the plain beam fixtures."""
    g = gold("repeat_tiny")
    toks = tiny32.generate(feats, language="ja", task="transcribe", return_timestamps=True, num_beams=3,
                           max_length=int(g["max_length"]), **_args(g, "c"))
    np.testing.assert_array_equal(toks.cpu().numpy(), g["c_tokens"])


def test_case_d_longform_conditioned(gold, tiny32):
    """Long-form with condition_on_prev_tokens: the previous text behind <|startofprev|> and its left pads are history
    to both processors, in the prefill and in every step of every pass."""
    from _util import longform_inputs

    g = gold("repeat_tiny")
    f, mask, _ = longform_inputs(g["clips"])
    res = tiny32.generate(torch.from_numpy(f).cuda(), attention_mask=torch.from_numpy(mask).cuda(), language="ja",
                          return_timestamps=True, return_segments=True, condition_on_prev_tokens=True, **_args(g, "d"))
    full = _compare_rows("d", res["sequences"].cpu().numpy(), g["d_sequences"], g["d_margin"])
    _check_segments(res, json.loads(str(g["d_segments"])), full)
    if len(full) == 3:
        passes = json.loads(str(g["d_passes"]))
        assert tiny32.stats["pass_P"] == [len(p["ids"][0]) for p in passes]


def _fallback_run(model, feats, g, **over):
    kw = json.loads(str(g["e_kwargs"]))
    kw["temperature"] = tuple(kw["temperature"])
    kw.update(over)
    model.manual_seed(7)
    model.record_pass_ids = True
    try:
        model.generate(feats, language="ja", task="transcribe", max_length=int(g["e_max_length"]),
                       return_segments=True, **kw, **_args(g, "e"))
    finally:
        model.record_pass_ids = False
    return model.stats


def test_case_e_fallback(gold, tiny32, feats_silent):
    """The temperature-0 attempt of the schedule: its statistics and decisions are the fixture's, and -- from a run of
    that temperature alone, which accepts every row's temperature-0 tokens -- its tokens.  The sampled attempt's
    draws are not torch's; its rows are held to the n-gram property."""
    g = gold("repeat_tiny")
    want = json.loads(str(g["e_passes"]))[0]["attempts"][0]
    n = _args(g, "e")["no_repeat_ngram_size"]
    for only_zero in (False, True):
        stats = _fallback_run(tiny32, feats_silent, g, **({"temperature": 0.0} if only_zero else {}))
        at = stats["fallback"][0][0]
        assert at["rows"] == want["rows"] and at["temperature"] == 0.0
        d = np.abs(np.array(at["avg_logprob"]) - np.array(want["avg_logprob"]))
        print(f"temperature-0 attempt: avg_logprob max diff {d.max():.2e}; falls back {at['needs_fallback']}")
        assert (d <= LP_TOL).all()
        assert at["needs_fallback"] == want["needs_fallback"] and at["should_skip"] == want["should_skip"]
        ids, P = stats["pass_ids"][0], stats["pass_P"][0]
        if only_zero:
            from kwhisper.generation import _strip_pass_row

            for r, toks in enumerate(want["tokens"]):
                got = _strip_pass_row(ids[r, P:], G.pad_token_id, G.eos_token_id, keep_eos=True)
                assert got.tolist() == toks, r
        else:
            last = stats["fallback"][0][-1]
            assert last["temperature"] == 0.4 and last["rows"] == [r for r, f in zip(at["rows"], at["needs_fallback"]) if f]
            for r in last["rows"]:
                assert not RR.has_repeated_ngram(RR.upto_first_eos(ids[r], P, G.eos_token_id), n), r


# ---- bf16 engine: what no rounding can blur --------------------------------------------------------------------------
def _pass_rows(model, feats, **kw):
    model.record_pass_ids = True
    try:
        model.generate(feats, language="ja", task="transcribe", max_length=40, **kw)
    finally:
        model.record_pass_ids = False
    return model.stats["pass_ids"][0], model.stats["pass_P"][0]


@pytest.mark.parametrize("mode", ["greedy", "greedy_ts", "beam3", "fp8"])
def test_bf16_no_trigram_twice(tiny16, feats, mode):
    """no_repeat_ngram_size=3: no row's ids -- prompt and generated tokens, up to and including its first EOS -- hold a
    3-gram twice; the same call without the argument does (the tiny random model loops), so the property is the
    processor's doing."""
    model = _model(torch.bfloat16, cross_kv_dtype="fp8_e4m3") if mode == "fp8" else tiny16
    kw = {"greedy": dict(return_timestamps=False), "greedy_ts": dict(return_timestamps=True),
          "beam3": dict(return_timestamps=True, num_beams=3), "fp8": dict(return_timestamps=False)}[mode]
    ids, P = _pass_rows(model, feats, no_repeat_ngram_size=3, **kw)
    for r, row in enumerate(ids):
        assert not RR.has_repeated_ngram(RR.upto_first_eos(row, P, G.eos_token_id), 3), (mode, r)
    base, _ = _pass_rows(model, feats, **kw)
    assert any(RR.has_repeated_ngram(RR.upto_first_eos(row, P, G.eos_token_id), 3) for row in base)


def test_bf16_penalty_first_step_scores(tiny16, feats):
    """repetition_penalty=1.3 on the bf16 engine: the session's recorded first-step logits are the restatement applied
    to the LM head's own logits at the prompt tokens (bit for bit, and nothing else moved), and the processed scores
    kw_greedy_step recorded are those logits wherever the Whisper processors left them finite."""
    eng = tiny16.engine
    sess = eng.new_session(4, eng.encode(feats))
    prompt = torch.tensor([[G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"],
                            G.no_timestamps_token_id]] * 4, dtype=torch.int64)
    ids = sess.generate(prompt, G, max_length=12, return_timestamps=False, record_scores=True, repeat=(1.3, 0))
    assert ids.shape == (4, 12) and len(sess.raw_logits) == len(sess.scores) == 8
    raw = sess.raw_logits[0].cpu().numpy()
    logits, scores = (t.cpu().numpy() for t in sess.scores[0])
    want = RR.repeat_process(prompt.numpy(), raw, 1.3, 0)
    assert (_bits(logits) == _bits(want)).all()
    assert (_bits(want) != _bits(raw)).sum() == 4 * 4  # the four prompt tokens of every row
    keep = np.isfinite(scores)
    assert (_bits(scores)[keep] == _bits(want)[keep]).all() and keep[:, prompt[0].numpy()].any()
    # a later step: the history is the prompt and the tokens generated so far
    t = 5
    want_t = RR.repeat_process(ids[:, : 4 + t], sess.raw_logits[t].cpu().numpy(), 1.3, 0)
    assert (_bits(sess.scores[t][0].cpu().numpy()) == _bits(want_t)).all()


def test_call_without_the_arguments_is_unchanged(tiny16, feats):
    """A call without the arguments after a call with them returns exactly what it returned before (separate plan and
    graph keys), and takes the fused LM-head + greedy launch again; 1.0 / 0 / None are that same call."""
    kw = dict(language="ja", task="transcribe", return_timestamps=False, max_length=40)
    before = tiny16.generate(feats, **kw).cpu()
    sess = tiny16._sessions[(4, 1)]
    fused, n_cfg = sess.lm_greedy_last, len(sess._greedy_cfg)
    assert fused
    with_args = tiny16.generate(feats, repetition_penalty=1.3, no_repeat_ngram_size=3, **kw).cpu()
    assert not sess.lm_greedy_last and len(sess._greedy_cfg) == n_cfg + 1
    assert with_args.shape != before.shape or not torch.equal(with_args, before)
    for off in (dict(), dict(repetition_penalty=1.0, no_repeat_ngram_size=0), dict(repetition_penalty=None)):
        again = tiny16.generate(feats, **off, **kw).cpu()
        assert torch.equal(again, before) and sess.lm_greedy_last and len(sess._greedy_cfg) == n_cfg + 1
    assert torch.equal(tiny16.generate(feats, repetition_penalty=1.3, no_repeat_ngram_size=3, **kw).cpu(), with_args)


def test_token_timestamps_compose(feats):
    """return_token_timestamps=True with no_repeat_ngram_size=3 returns the tokens of the call without the flag."""
    gen = generation_constants(TINY)
    gen.alignment_heads = [[2, 2], [3, 0], [3, 4]]
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import synthetic_state_dict

    model = KWhisperForConditionalGeneration.from_state_dict(TINY, synthetic_state_dict(TINY, 0), dtype=torch.bfloat16,
                                                            generation_config=gen)
    kw = dict(language="ja", task="transcribe", return_timestamps=True, max_length=40, no_repeat_ngram_size=3)
    plain = model.generate(feats, **kw).cpu()
    res = model.generate(feats, return_token_timestamps=True, **kw)
    assert torch.equal(res["sequences"].cpu(), plain)
    assert res["token_timestamps"].shape == plain.shape


def test_pipeline_and_pseudo_label_forward_the_arguments(tiny16, feats):
    """pseudo_label's gen_kwargs hand the two arguments to generate(): the result is the direct call's."""
    from kwhisper.pseudo_label import pseudo_label

    kw = dict(language="ja", task="transcribe", max_length=24, no_repeat_ngram_size=3, repetition_penalty=1.3)
    want = tiny16.generate(feats[:2].contiguous(), **kw).cpu().numpy()
    ids, preds = pseudo_label(tiny16, lambda idx: feats[list(idx)], 2, batch_size=2, pad_token_id=50257, gen_kwargs=kw)
    assert list(ids) == [0, 1]
    for got, w in zip(preds, want):
        assert list(got)[: len(w)] == w.tolist()[: len(list(got))]
