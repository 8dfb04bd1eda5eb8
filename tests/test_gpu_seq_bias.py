"""GPU tests of ``sequence_bias`` / ``bad_words_ids``: kw_seq_bias_process (csrc/seqbias.hip) and
kw_beam_logprobs_proc (csrc/beam.hip) against the numpy restatement tests/_seq_bias_ref.py (which
tests/test_seq_bias_cpu.py holds to transformers' own processors), and generate() on the tiny model against
transformers (tests/golden/seq_bias_tiny.npz, tools/make_seq_bias_fixture.py).

fp32 engine: token ids equal the fixture's in every case (the tool refuses a fixture with a greedy step whose top-2
margin is under 1e-3).  bf16 and fp8-cache engines: every step's recorded logits are the restatement applied to that
step's recorded raw logits, and its token is the argmax of the oracle's Whisper processors over them."""
import ctypes
import json

import numpy as np
import pytest
import torch

import _beam_ref as BR
import _seq_bias_ref as SR
from conftest import gpu_available
from oracle import generate as og

from kwhisper.config import TINY, generation_constants

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

F32 = np.float32
INF = float("inf")
G = generation_constants(TINY)
LP_TOL = 2e-3     # avg_logprob: tests/test_fallback_gpu.py's bar
LP_RTOL, LP_ATOL = 1e-6, 1e-5  # tests/test_gpu_beam_kernels.py's bound on kw_beam_logprobs' values
STRIDE = 448
R = 3


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype).contiguous()


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.int32)


# ------------------------------------------------------------------------------------------- kw_seq_bias_process
def _case(V, L, rng):
    """(3, L) histories over a small pool and a processor with entries of 1, 2, 5 and 16 tokens: per length one cut
    from each row's tail (it applies where it fits) and one that does not; tokens 0 and V-1 as last tokens; several
    entries on one last token (a length-1 among them); -inf, +inf and both on one token; scores with 0.0, -0.0, +-inf
    and NaN at biased tokens."""
    pool = np.concatenate([[0, V - 1], rng.choice(np.arange(1, V - 1), 8, replace=False)])
    hist = rng.choice(pool, (R, L)).astype(np.int64)
    last = [0, V - 1] + [int(t) for t in rng.choice(np.arange(1, V - 1), 10, replace=False)]
    bias, k = {}, 0
    for n in (1, 2, 5, 16):
        for r in range(R):
            tail = [int(t) for t in hist[r, max(0, L - (n - 1)):]]
            tail = [int(t) for t in rng.choice(pool, n - 1 - len(tail))] + tail  # (longer than the row: never applies)
            for pre in (tail, [int(t) for t in rng.choice(pool, n - 1)]):
                bias[tuple(pre) + (last[k % len(last)],)] = float(np.round(rng.standard_normal() * 3, 2))
                k += 1
    t_inf, t_both = last[5], last[6]
    bias[(t_inf,)] = -INF
    bias[(t_both,)] = INF
    if L >= 2:
        bias[(int(hist[0, -1]), t_both)] = -INF  # row 0: +inf + -inf
    x = (rng.standard_normal((R, V)) * 4).astype(F32)
    for r in range(R):
        for t, v in zip(last[:5], [0.0, -0.0, -np.inf, np.inf, np.nan]):
            x[r, t] = v
    return hist, x, bias


def _run_seq_bias(x, hist, entries, backend, launches=1):
    from kwhisper import ops
    from kwhisper.seq_bias import SeqTable

    V = x.shape[1]
    ids = torch.full((R, STRIDE), -77, dtype=torch.int64, device="cuda")  # (past L: no launch may read it as a token)
    ids[:, : hist.shape[1]] = cu(hist, torch.int64)
    cur = cu(np.array([hist.shape[1]]), torch.int32)
    buf = torch.full((R + 1, V), 123.25, device="cuda")  # the canary row past R
    outs = []
    old = ops.set_backend(backend)
    try:
        plan = ops.SeqBiasPlan(buf[:R], ids, cur, ops.DeviceSeqTable(SeqTable(entries, V), "cuda"))
        for _ in range(launches):
            buf[:R] = cu(x, torch.float32)
            plan()
            torch.cuda.synchronize()
            outs.append(buf[:R].cpu().numpy())
    finally:
        ops.set_backend(old)
    assert (buf[R] == 123.25).all(), "the row past R was written"
    return outs


@pytest.mark.parametrize("L", [1, 2, 4, 5, 448])
@pytest.mark.parametrize("V", [97, 51866])
def test_seq_bias_process_vs_restatement(V, L):
    rng = np.random.default_rng(V + L)
    hist, x, bias = _case(V, L, rng)
    assert {len(k) for k in bias} == {1, 2, 5, 16}
    for entries in (bias, SR.bad_words_dict([list(k) for k in bias], [int(hist[0, -1])])):
        want = SR.sequence_bias(hist, x, entries)
        a, b = _run_seq_bias(x, hist, entries, "ctypes", launches=2)
        (c,) = _run_seq_bias(x, hist, entries, "torch")
        bad = np.nonzero(~((a == want) | (np.isnan(a) & np.isnan(want))))
        assert bad[0].size == 0, (bad[0][:5], bad[1][:5], a[bad][:5], want[bad][:5])
        assert (_bits(a) == _bits(b)).all() and (_bits(a) == _bits(c)).all()  # run to run, backend to backend
        free = np.ones(V, bool)
        free[[k[-1] for k in entries]] = False
        assert (_bits(a)[:, free] == _bits(x)[:, free]).all()  # an element of no group is bit-identical
        with np.errstate(invalid="ignore"):
            assert (want != x).sum() > 0
    if L >= 2:
        assert np.isnan(SR.sequence_bias(hist, x, bias)[0]).sum() > np.isnan(x[0]).sum()  # +inf + -inf did occur


def test_seq_bias_process_empty_table_and_bad_arguments():
    from kwhisper import _lib as L
    from kwhisper import ops
    from kwhisper.seq_bias import MAX_LEN, MAX_SEQS, SeqTable

    lib = L.load()
    s = torch.full((2, 100), 1.5, device="cuda")
    ids = torch.zeros((2, STRIDE), dtype=torch.int64, device="cuda")
    cur = torch.ones(1, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dev = ops.DeviceSeqTable(SeqTable({(0,): 1.0, (0, 5): 2.0}, 100), "cuda")

    def call(sp, ip, cp, table, stride=STRIDE):
        return lib.kw_seq_bias_process(sp, 2, 100, ip, stride, cp, table, _s())

    empty = L.SeqBiasTable()  # n_seq == 0: nothing is launched, whatever the pointers
    assert call(p(s), p(ids), p(cur), ctypes.byref(empty)) == L.KW_OK
    for args in [(None, p(ids), p(cur), dev.ref), (p(s), None, p(cur), dev.ref), (p(s), p(ids), None, dev.ref),
                 (p(s), p(ids), p(cur), None)]:
        assert call(*args) == L.KW_EINVAL, args
        assert b"kw_seq_bias_process" in lib.kw_last_error()
    broken = L.SeqBiasTable.from_buffer_copy(dev.c)
    broken.values = None
    assert call(p(s), p(ids), p(cur), ctypes.byref(broken)) == L.KW_EINVAL
    for field, v in (("n_seq", MAX_SEQS + 1), ("max_len", MAX_LEN + 1)):
        big = L.SeqBiasTable.from_buffer_copy(dev.c)
        setattr(big, field, v)
        assert call(p(s), p(ids), p(cur), ctypes.byref(big)) == L.KW_EUNSUPPORTED
        assert b"KW_SEQ_BIAS_MAX" in lib.kw_last_error()
    with pytest.raises(ValueError):
        ops.DeviceSeqTable(SeqTable({}), "cuda")
    torch.cuda.synchronize()
    assert (s == 1.5).all()  # nothing was launched


# ------------------------------------------------------------------------------------------- kw_beam_logprobs_proc
def _lp_tables(hist, x, gen, L):
    """Entries cut from every row's tail and its best tokens (test_gpu_repeat._lp_case: the rows end on their two best
    text tokens; at L = 4 on the best alone): boosts and penalties on a 0.25 grid on candidates, two entries and a
    length-1 entry on one token, a ban reaching into the prompt, a banned timestamp."""
    ts = gen["no_timestamps_token_id"] + 1
    bias, bad = {}, []
    for r in range(hist.shape[0]):
        best = [int(t) for t in np.argsort(-x[r, :gen["eos_token_id"]], kind="stable")[:6]]
        tail = [int(t) for t in hist[r]]
        bias[(tail[-1], best[3])] = 5.25
        bias[(tail[-2], tail[-1], best[4])] = -3.5
        bias[(best[5],)] = 1.5
        bias[(tail[-1], best[5])] = 0.75
        bias[(tail[-1] + 1, best[2])] = 50.0  # (does not apply)
        bad.append([tail[-3], tail[-2], tail[-1], best[0]])  # L = 4: the prefix is the prompt's last two and the row's one
        bad.append([tail[-1], best[1]])
    bad.append([ts + 12])
    return bias, SR.bad_words_dict(bad)


def _run_lp(gen, hist, x, k, rt, split, repeat, tables):
    from kwhisper import _lib as L
    from kwhisper import ops
    from kwhisper.seq_bias import SeqTable
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
    dev = None if tables is None else [ops.DeviceSeqTable(SeqTable(t, V), "cuda") if t else None for t in tables]
    for _ in range(2):  # the split kernel's arrival counters re-arm
        if tables is None:
            L.check(lib.kw_beam_logprobs_rep(ctypes.byref(a), repeat[0], repeat[1], _s()), "kw_beam_logprobs_rep")
        else:
            L.check(lib.kw_beam_logprobs_proc(ctypes.byref(a), repeat[0], repeat[1], dev[0].ref if dev[0] else None,
                                              dev[1].ref if dev[1] else None, _s()), "kw_beam_logprobs_proc")
    torch.cuda.synchronize()
    return keep[5].cpu().numpy(), keep[6].cpu().numpy()


@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("L", [4, 60])
@pytest.mark.parametrize("V", [1000, 51866])
def test_beam_logprobs_proc_vs_reference(V, L, split, rt):
    """cand_idx exact, values within test_gpu_beam_kernels.py's LP_RTOL / LP_ATOL of the restatement whose normaliser
    is summed in float64; with empty tables the launch is kw_beam_logprobs_rep's, bit for bit.  Conditions on the
    inputs, checked here as tests/test_gpu_repeat.py checks them: the reference's k-th and (k+1)-th best are equal or
    1e-3 apart, and the timestamp rule's margin is 1e-3 from zero."""
    from test_gpu_repeat import _lp_case

    gen, hist, x, k = _lp_case(V, L, rt)
    bias, bad = _lp_tables(hist, x, gen, L)
    for repeat in [(1.0, 0), (1.3, 3)]:
        rep = _run_lp(gen, hist, x, k, rt, split, repeat, None)
        off = _run_lp(gen, hist, x, k, rt, split, repeat, (None, None))
        assert (_bits(off[0]) == _bits(rep[0])).all() and (off[1] == rep[1]).all()
    hit = 0
    for repeat, tables in [((1.0, 0), (bias, bad)), ((1.3, 3), (bias, bad)), ((1.0, 0), (bias, None)),
                           ((0.7, 2), (None, bad))]:
        want = SR.processed_logprobs_proc(hist, x, gen, 3, rt, tables[0], tables[1], *repeat)
        wv, wi = BR.row_candidates(want, k)
        srt = -np.sort(-want, axis=-1)[:, : k + 1]
        gaps = srt[:, :-1] - srt[:, 1:]
        with np.errstate(invalid="ignore"):
            assert ((gaps == 0) | (gaps >= 1e-3) | ~np.isfinite(gaps)).all(), gaps
        if rt:
            margin = SR.timestamp_margin_proc(hist, x, gen, 3, tables[0], tables[1], *repeat)
            assert (np.abs(margin) >= 1e-3).all(), margin
        cv, ci = _run_lp(gen, hist, x, k, rt, split, repeat, tables)
        fin = np.isfinite(wv) & np.isfinite(cv)
        err = np.abs(cv[fin] - wv[fin])
        print(f"{repeat} split={split}: max |log-prob - reference| {err.max() if err.size else 0.0:.3g}")
        np.testing.assert_array_equal(ci, wi, err_msg=f"{repeat}")
        np.testing.assert_array_equal(np.isneginf(cv), np.isneginf(wv))
        np.testing.assert_allclose(cv, wv, rtol=LP_RTOL, atol=LP_ATOL)
        plain = _run_lp(gen, hist, x, k, rt, split, repeat, None)
        hit += int((ci != plain[1]).any())
    assert hit >= 3  # the tables did change the candidates


def test_beam_logprobs_proc_rejects_bad_arguments():
    from kwhisper import _lib as L
    from kwhisper import ops
    from kwhisper.seq_bias import SeqTable
    from test_gpu_beam_kernels import logprobs_args
    from test_gpu_repeat import _lp_case

    gen, hist, x, k = _lp_case(1000, 4, False)
    lib = L.load()
    t = (cu(x, torch.float32), torch.zeros(1000, dtype=torch.uint8, device="cuda"),
         cu(np.array(gen["begin_suppress_tokens"]), torch.int32), torch.zeros((4, 64), dtype=torch.int64, device="cuda"),
         cu(np.array([4]), torch.int32), torch.full((4, k), 7.0, device="cuda"),
         torch.full((4, k), 7, dtype=torch.int32, device="cuda"), cu(np.array([0]), torch.int32), None)
    a = logprobs_args(*t, gen, False, 3, k)
    dev = ops.DeviceSeqTable(SeqTable({(9,): 1.0}, 1000), "cuda")
    for penalty, ngram in [(0.0, 0), (float("nan"), 2), (1.3, -1)]:
        assert lib.kw_beam_logprobs_proc(ctypes.byref(a), penalty, ngram, dev.ref, None, _s()) == L.KW_EINVAL
        assert b"kw_beam_logprobs_proc" in lib.kw_last_error()
    assert lib.kw_beam_logprobs_proc(None, 1.3, 2, dev.ref, None, _s()) == L.KW_EINVAL
    big = L.SeqBiasTable.from_buffer_copy(dev.c)
    big.n_seq = 5000
    assert lib.kw_beam_logprobs_proc(ctypes.byref(a), 1.0, 0, None, ctypes.byref(big), _s()) == L.KW_EUNSUPPORTED
    a.V = 65537
    assert lib.kw_beam_logprobs_proc(ctypes.byref(a), 1.0, 0, dev.ref, None, _s()) == L.KW_EUNSUPPORTED
    assert b"65536" in lib.kw_last_error()
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
def feats(gold):
    from _util import oracle_features

    return torch.from_numpy(oracle_features(TINY, gold("seq_bias_tiny")["cases"])).cuda()


@pytest.fixture(scope="module")
def feats_silent(gold):
    """Case e's input: the clips and one row of digital silence (tools/make_fixtures.py fallback_features)."""
    from _util import audio_cases
    from oracle.mel import log_mel

    audio = np.concatenate([audio_cases(gold("seq_bias_tiny")["cases"]), np.zeros((1, 480000), np.float32)])
    return torch.from_numpy(log_mel(audio, TINY.num_mel_bins)).cuda()


def _args(g, case):
    return json.loads(str(g["args"]))[case]


def test_fixture_entries_fired(gold):
    """Every kind of entry applied at least once in the reference run of every case (the three-token ban of case a2
    sits inside the text; only the others' crosses the prompt boundary), and every case differs from its unbiased
    call's output -- the tool asserted both; the counts it stored say so again."""
    g = gold("seq_bias_tiny")
    for case in ("a", "a2", "b", "c", "d", "e", "f"):
        fired = json.loads(str(g[f"{case}_fired"]))
        assert set(fired) == {"len1", "ban2", "ban3", "boost", "shared"} and all(v > 0 for v in fired.values()), case
        args = _args(g, case)
        assert len(args["sequence_bias"]) == 2 and [len(w) for w in args["bad_words_ids"]] == [2, 3]
    assert (g["a_tokens"] != g["a_base_tokens"]).any() and (g["c_tokens"].shape != g["c_base_tokens"].shape
                                                           or (g["c_tokens"] != g["c_base_tokens"]).any())
    for c in "abdf":
        assert not (g[f"{c}_margin"] < 1e-3).any(), c


def _short(model, feats, g, case):
    kw = dict(language="ja", task="transcribe", return_timestamps=False, max_length=int(g["max_length"]))
    return model.generate(feats, **kw, **_args(g, case)).cpu().numpy()


def test_case_a_greedy(gold, tiny32, feats):
    g = gold("seq_bias_tiny")
    np.testing.assert_array_equal(_short(tiny32, feats, g, "a"), g["a_tokens"])
    assert not tiny32._sessions[(4, 1)].lm_greedy_last  # the two-launch tail, not kw_dec_lm_greedy


def test_case_f_with_the_repetition_pair(gold, tiny32, feats):
    """sequence_bias -> repetition_penalty -> no_repeat_ngram_size -> bad_words_ids, in that order."""
    g = gold("seq_bias_tiny")
    assert set(_args(g, "f")) == {"sequence_bias", "bad_words_ids", "repetition_penalty", "no_repeat_ngram_size"}
    np.testing.assert_array_equal(_short(tiny32, feats, g, "f"), g["f_tokens"])


def test_graph_reuse_a_b_a(gold, tiny32, feats):
    """Call A, call B with other values of the same shape, A again: each returns its own fixture row (the tables'
    digests are in the plan / graph key, so B cannot replay A's arrays)."""
    g = gold("seq_bias_tiny")
    sa, sb = _args(g, "a"), _args(g, "a2")
    assert [len(s[0]) for s in sa["sequence_bias"]] == [len(s[0]) for s in sb["sequence_bias"]] and sa != sb
    for case in ("a", "a2", "a", "a2"):
        np.testing.assert_array_equal(_short(tiny32, feats, g, case), g[f"{case}_tokens"], err_msg=case)
    sess = tiny32._sessions[(4, 1)]
    n = len(sess._greedy_cfg)
    _short(tiny32, feats, g, "a")
    assert len(sess._greedy_cfg) == n  # a repeat call replays its own graph: no new plan


def _check_segments(res, segs):
    for b in range(len(segs)):
        assert [len(s["tokens"]) for s in res["segments"][b]] == [s[2] for s in segs[b]]
        if segs[b]:
            np.testing.assert_allclose([(s["start"], s["end"]) for s in res["segments"][b]], [s[:2] for s in segs[b]],
                                       atol=1e-9)


@pytest.mark.parametrize("case", ["b", "d"])
def test_cases_b_d_longform(gold, tiny32, case):
    """Timestamps over more than one seek pass; d: with condition_on_prev_tokens, where the previous text behind
    <|startofprev|> and its left pads are history to both processors."""
    from _util import longform_inputs

    g = gold("seq_bias_tiny")
    f, mask, _ = longform_inputs(g["clips"])
    extra = dict(condition_on_prev_tokens=True) if case == "d" else {}
    res = tiny32.generate(torch.from_numpy(f).cuda(), attention_mask=torch.from_numpy(mask).cuda(), language="ja",
                          return_timestamps=True, return_segments=True, **extra, **_args(g, case))
    np.testing.assert_array_equal(res["sequences"].cpu().numpy(), g[f"{case}_sequences"])
    _check_segments(res, json.loads(str(g[f"{case}_segments"])))
    passes = json.loads(str(g[f"{case}_passes"]))
    assert len(passes) > 1 and tiny32.stats["pass_P"] == [len(p["ids"][0]) for p in passes]


def test_case_c_beams(gold, tiny32, feats):
    g = gold("seq_bias_tiny")
    toks = tiny32.generate(feats, language="ja", task="transcribe", return_timestamps=True, num_beams=3,
                           max_length=int(g["max_length"]), **_args(g, "c"))
    np.testing.assert_array_equal(toks.cpu().numpy(), g["c_tokens"])


def test_case_e_fallback_temperature_0(gold, tiny32, feats_silent):
    """The temperature-0 attempt of the schedule: its statistics and decisions are the fixture's, and -- from a run of
    that temperature alone, which accepts every row's temperature-0 tokens -- its tokens."""
    from kwhisper.generation import _strip_pass_row

    g = gold("seq_bias_tiny")
    want = json.loads(str(g["e_passes"]))[0]["attempts"][0]
    for only_zero in (False, True):
        kw = json.loads(str(g["e_kwargs"]))
        kw["temperature"] = 0.0 if only_zero else tuple(kw["temperature"])
        tiny32.manual_seed(7)
        tiny32.record_pass_ids = True
        try:
            tiny32.generate(feats_silent, language="ja", task="transcribe", max_length=int(g["e_max_length"]),
                            return_segments=True, **kw, **_args(g, "e"))
        finally:
            tiny32.record_pass_ids = False
        stats = tiny32.stats
        at = stats["fallback"][0][0]
        assert at["rows"] == want["rows"] and at["temperature"] == 0.0
        d = np.abs(np.array(at["avg_logprob"]) - np.array(want["avg_logprob"]))
        print(f"temperature-0 attempt: avg_logprob max diff {d.max():.2e}; falls back {at['needs_fallback']}")
        assert (d <= LP_TOL).all()
        assert at["needs_fallback"] == want["needs_fallback"] and at["should_skip"] == want["should_skip"]
        if only_zero:
            ids, P = stats["pass_ids"][0], stats["pass_P"][0]
            for r, toks in enumerate(want["tokens"]):
                got = _strip_pass_row(ids[r, P:], G.pad_token_id, G.eos_token_id, keep_eos=True)
                assert got.tolist() == toks, r


# ---- bf16 and fp8-cache engines: every step against the restatement ---------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_bf16_engines_every_step(gold, feats, mode):
    """With recorded scores: a step's logits are the restatement (sequence_bias, the repetition pair, bad_words_ids)
    applied to that step's raw logits, as floats with NaNs in place; its token is the argmax of the oracle's Whisper
    processors over them."""
    from kwhisper.seq_bias import build_tables

    g = gold("seq_bias_tiny")
    model = _model(torch.bfloat16, **({"cross_kv_dtype": "fp8_e4m3"} if mode == "fp8" else {}))
    eng = model.engine
    args = _args(g, "a")
    # the fixture's entries come from the fp32 reference's text; add ones that apply on any engine's output
    prompt = np.array([[G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"],
                        G.no_timestamps_token_id]] * 4, np.int64)
    P, T = prompt.shape[1], 12
    sess = eng.new_session(4, eng.encode(feats))
    plain = sess.generate(torch.from_numpy(prompt), G, max_length=T, return_timestamps=False)
    bias = {tuple(s[0]): s[1] for s in args["sequence_bias"]}
    bias.update({(int(plain[0, P]), int(plain[1, P + 1])): 30.0, (int(plain[2, P + 2]),): 1.5,
                 (G.no_timestamps_token_id, int(plain[3, P])): -4.0})
    bad = args["bad_words_ids"] + [[int(plain[1, P]), int(plain[1, P + 1])],
                                   [G.no_timestamps_token_id, int(plain[2, P]), int(plain[2, P + 1])]]
    tables = build_tables(dict(bias), bad, G.eos_token_id, TINY.vocab_size)
    ids = sess.generate(torch.from_numpy(prompt), G, max_length=T, return_timestamps=False, record_scores=True,
                        repeat=(1.3, 0), seq_tables=tables)
    assert ids.shape[1] > P + 3 and len(sess.raw_logits) == len(sess.scores) >= ids.shape[1] - P
    assert (ids[:, : plain.shape[1]] != plain[:, : ids.shape[1]]).any()
    gen = G.to_dict()
    bad_d = SR.bad_words_dict(bad, [G.eos_token_id])
    live = np.ones(4, bool)
    changed = 0
    for t in range(ids.shape[1] - P):
        raw = sess.raw_logits[t].cpu().numpy()
        got = sess.scores[t][0].cpu().numpy()
        want = SR.process(ids[:, : P + t], raw, bias, bad_d, 1.3, 0)
        assert SR.same(got, want), t
        with np.errstate(invalid="ignore"):
            changed += int((want != raw).sum())
        tok = og.process_logits(ids[:, : P + t], want, gen, P, False).argmax(-1)
        assert (tok[live] == ids[live, P + t]).all(), t
        live &= ids[:, P + t] != G.eos_token_id
    assert changed


def test_call_without_the_arguments_is_unchanged(gold, feats):
    """A call without the arguments after a call with them returns what it returned before, on the fused LM-head +
    greedy launch again; bad words that the eos filter empties are that same call."""
    g = gold("seq_bias_tiny")
    model = _model(torch.bfloat16)
    kw = dict(language="ja", task="transcribe", return_timestamps=False, max_length=40)
    before = model.generate(feats, **kw).cpu()
    sess = model._sessions[(4, 1)]
    n_cfg = len(sess._greedy_cfg)
    assert sess.lm_greedy_last
    with_args = model.generate(feats, **kw, **_args(g, "a")).cpu()
    assert not sess.lm_greedy_last and len(sess._greedy_cfg) == n_cfg + 1
    for off in (dict(), dict(sequence_bias=None, bad_words_ids=None), dict(bad_words_ids=[[G.eos_token_id]])):
        again = model.generate(feats, **off, **kw).cpu()
        assert torch.equal(again, before) and sess.lm_greedy_last and len(sess._greedy_cfg) == n_cfg + 1
    assert torch.equal(model.generate(feats, **kw, **_args(g, "a")).cpu(), with_args)


def test_token_timestamps_pipeline_and_pseudo_label(gold, feats):
    """return_token_timestamps (greedy and beams) returns the tokens of the call without the flag; pseudo_label's
    gen_kwargs and ASRPipeline's generate_kwargs hand the arguments to generate()."""
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.pipeline import ASRPipeline
    from kwhisper.pseudo_label import pseudo_label
    from kwhisper.synthetic import synthetic_state_dict

    g = gold("seq_bias_tiny")
    gen = generation_constants(TINY)
    gen.alignment_heads = [[2, 2], [3, 0], [3, 4]]
    model = KWhisperForConditionalGeneration.from_state_dict(TINY, synthetic_state_dict(TINY, 0), dtype=torch.bfloat16,
                                                            generation_config=gen)
    args = _args(g, "c")
    for beams in (dict(), dict(num_beams=3)):
        kw = dict(language="ja", task="transcribe", return_timestamps=True, max_length=40, **beams, **args)
        plain = model.generate(feats, **kw).cpu()
        res = model.generate(feats, return_token_timestamps=True, **kw)
        assert torch.equal(res["sequences"].cpu(), plain) and res["token_timestamps"].shape == plain.shape
        base = model.generate(feats, language="ja", task="transcribe", return_timestamps=True, max_length=40, **beams)
        assert base.shape != plain.shape or not torch.equal(base.cpu(), plain)
    kw = dict(language="ja", task="transcribe", max_length=24, **args)
    want = model.generate(feats[:2].contiguous(), **kw).cpu().numpy()
    ids, preds = pseudo_label(model, lambda idx: feats[list(idx)], 2, batch_size=2, pad_token_id=50257, gen_kwargs=kw)
    assert list(ids) == [0, 1]
    for got, w in zip(preds, want):
        assert list(got)[: len(w)] == w.tolist()[: len(list(got))]
    pipe = ASRPipeline(model, generate_kwargs=dict(args, max_length=24, language="ja", task="transcribe"))
    assert pipe.generate_kwargs["bad_words_ids"] == args["bad_words_ids"]
