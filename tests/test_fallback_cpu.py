"""CPU checks of the decoding fallback: the numpy restatement tests/_fallback_ref.py against transformers and against
its own definition (Philox4x32-10, the uniform-to-Gumbel map), generation.py's host logic over a stub session, and the
C layout of kw_sample_args."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import _fallback_ref as R
from conftest import ROOT

from kwhisper.config import TINY, generation_constants


# ---- the restatement against transformers ------------------------------------------------------------------------
def _tf():
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    return gw.WhisperGenerationMixin


@pytest.mark.parametrize("temperature", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("case", ["eos", "max_length", "pad_is_eos"])
def test_avg_logprob_and_compression_ratio_match_transformers(case, temperature):
    """_retrieve_avg_logprobs / _retrieve_compression_ratio on random scores and tokens: a row that ends at EOS (then
    padding), a row that hits max_length, and pad == EOS."""
    mixin = _tf()
    rng = np.random.default_rng(len(case) + int(10 * temperature))
    V, T, eos = 997, 17, 900
    pad = eos if case == "pad_is_eos" else 899
    tokens = rng.integers(0, 890, T)
    if case != "max_length":
        tokens[9] = eos
        tokens[10:] = pad
    scores = (rng.standard_normal((T, V)) * 3).astype(np.float32)
    scores[:, 5] = -np.inf
    kept = R.strip_padding(tokens, pad, eos)
    assert len(kept) == (T if case == "max_length" else 10)
    # what transformers records when sampling is the processed scores divided by the temperature
    rec = scores / temperature if temperature > 0 else scores
    want = float(mixin._retrieve_avg_logprobs([torch.from_numpy(r) for r in rec], torch.from_numpy(kept), temperature))
    got = R.avg_logprob(rec, kept, temperature)
    assert abs(got - want) <= 2e-6 * max(1.0, abs(want))
    # the engine's statistic: the un-warped scores' log-softmax at the tokens, first EOS included, over their number
    lp = R.log_softmax64(scores[: len(kept)])[np.arange(len(kept)), kept]
    assert abs(lp.sum() / len(kept) - want) <= 2e-5 * max(1.0, abs(want))
    from kwhisper.generation import _compression_ratio

    for toks in (kept, np.tile(kept[:3], 9), np.array([7])):
        want_cr = mixin._retrieve_compression_ratio(torch.from_numpy(np.asarray(toks)), 51865)
        assert R.compression_ratio(toks, 51865) == want_cr == _compression_ratio(np.asarray(toks), 51865)


# (no_speech_threshold without logprob_threshold is left out: the reference dies on an unbound local there, and
# generate() raises ValueError -- test_argument_errors_on_the_host)
@pytest.mark.parametrize("cr_t,lp_t,ns_t", [(c, l, n) for c in (None, 1.35) for l in (None, -1.0) for n in (None, 0.6)
                                            if not (n is not None and l is None)])
def test_need_fallback_truth_table(cr_t, lp_t, ns_t):
    """_need_fallback over the three thresholds (set or not) and values on both sides of each: the restatement and
    generation.py's rule equal transformers', including the order -- a skip cancels a fallback."""
    from transformers.generation.logits_process import WhisperNoSpeechDetection

    from kwhisper.generation import _need_fallback

    mixin = _tf()
    tokens = torch.tensor([11, 12, 13, 900])
    rep = torch.tensor([11] * 40 + [900])
    proc = WhisperNoSpeechDetection(no_speech_token=5, begin_index=3)
    cfg = types.SimpleNamespace(compression_ratio_threshold=cr_t, logprob_threshold=lp_t, no_speech_threshold=ns_t)
    this = types.SimpleNamespace(_retrieve_compression_ratio=mixin._retrieve_compression_ratio,
                                 _retrieve_avg_logprobs=mixin._retrieve_avg_logprobs)
    thr = dict(compression_ratio_threshold=cr_t, logprob_threshold=lp_t, no_speech_threshold=ns_t)
    seen = set()
    for seq in (tokens, rep):
        for peak in (8.0, 0.0):  # confident / flat scores: avg_logprob above / below -1
            scores = torch.zeros((len(seq), 997))
            scores[torch.arange(len(seq)), seq] = peak
            for nsp in (0.9, 0.1):
                proc._no_speech_prob = torch.tensor([nsp])
                want = mixin._need_fallback(this, seq, [{"scores": list(scores)}], 0, [proc], cfg, 997, 0.0)
                lp = R.avg_logprob(scores.numpy(), seq.numpy(), 0.0)
                cr = R.compression_ratio(seq.numpy(), 997)
                assert R.need_fallback(compression=cr, avg_lp=lp, no_speech_prob=nsp, **thr) == want
                assert _need_fallback(cr, lp, nsp, thr) == want
                seen.add(want)
    if cr_t is not None and lp_t is not None and ns_t is not None:
        assert seen == {(False, False), (True, False), (False, True)}


# ---- Philox4x32-10 and the noise map -------------------------------------------------------------------------------
def test_philox_known_answers():
    """The three known-answer vectors of the Random123 distribution (counter, key -> output)."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for c, k, want in kat:
        assert tuple(int(x) for x in R.philox4x32_10(np.array(c, np.uint64), np.array(k, np.uint64))) == want


def test_philox_counter_increments_and_bit_balance():
    """Counter increments in any word (and key changes) give distinct blocks, and each of the 32 output bits averages
    0.5 within 5 sigma over 2^16 draws."""
    n = 1 << 14
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = np.arange(n)
    key = np.array([0x9ABCDEF0, 0x12345678], np.uint64)
    out = R.philox4x32_10(ctr, key)
    draws = out.reshape(-1)  # 2^16 words
    assert len({tuple(r) for r in out.tolist()}) == n
    base = tuple(out[0].tolist())
    for w in range(1, 4):
        c = np.zeros(4, np.uint64)
        c[w] = 1
        assert tuple(R.philox4x32_10(c, key).tolist()) != base
    assert tuple(R.philox4x32_10(np.zeros(4, np.uint64), key + np.array([1, 0], np.uint64)).tolist()) != base
    sigma = 0.5 / np.sqrt(draws.size)
    for bit in range(32):
        mean = float(((draws >> np.uint32(bit)) & np.uint32(1)).mean())
        assert abs(mean - 0.5) <= 5 * sigma, (bit, mean)
    # the per-token draw: word v & 3 of the block of counter (v >> 2, L, row, attempt), whatever the vocabulary's size
    a, b = R.sample_draws(7, 2, 3, 11, 1000), R.sample_draws(7, 2, 3, 11, 51865)
    assert np.array_equal(a, b[:1000])
    assert not np.array_equal(a, R.sample_draws(7, 3, 3, 11, 1000))
    assert not np.array_equal(a, R.sample_draws(7, 2, 4, 11, 1000))
    assert not np.array_equal(a, R.sample_draws(7, 2, 3, 12, 1000))
    assert not np.array_equal(a, R.sample_draws(7 + (1 << 32), 2, 3, 11, 1000))


def test_gumbel_map_is_finite_and_recoverable():
    """Every 20-bit index gives a finite g within the documented range, also when the map runs in float32 as on the
    device, and the index comes back from the float32 value."""
    k = np.arange(1 << R.UNIFORM_BITS)
    assert R.uniform_index(np.array([0, 0xFFF, 0x1000, 0xFFFFFFFF], np.uint32)).tolist() == [0, 0, 1, (1 << 20) - 1]
    g = R.gumbel_of_index(k)
    assert np.isfinite(g).all() and -2.679 < g.min() and g.max() < 14.557 and (np.diff(g) > 0).all()
    u32 = ((k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -20)).astype(np.float32)
    assert u32.max() < 1 and u32.min() > 0 and np.array_equal(u32.astype(np.float64), R.uniform_of_index(k))
    g32 = (-np.log(-np.log(u32, dtype=np.float32), dtype=np.float32)).astype(np.float32)
    assert np.isfinite(g32).all()
    assert np.array_equal(R.index_of_gumbel(g32), k)
    # the same with the float32 value off by a few units in the last place (another logf)
    for ulps in (-3, 3):
        bumped = (g32.view(np.int32) + np.where(g32 >= 0, ulps, -ulps).astype(np.int32)).view(np.float32)
        assert np.array_equal(R.index_of_gumbel(bumped), k)


def test_perturbed_argmax():
    s = np.array([0.0, -np.inf, 1.0, 1.0, -2.0])
    assert R.perturbed_argmax(s, 0.0, np.zeros(5)) == (2, 0.0)  # first index on ties
    tok, gap = R.perturbed_argmax(s, 2.0, np.array([0.0, 99.0, 0.0, 0.5, 9.0]))
    assert tok == 4 and gap == pytest.approx(5.0 - 2.5)  # -inf scores never win, whatever their noise


def test_attempt_loop_bookkeeping():
    """Rows leave the fallback set attempt by attempt; the last temperature's result is accepted."""
    needs = {0: [True, True, True], 1: [False], 2: [True, False], 3: [True, True, True]}

    def decide(ai, t, rows):
        return [(needs[r][ai], False) for r in rows]

    accepted, skipped, decoded = R.attempt_loop(4, [0.0, 0.2, 0.4], decide)
    assert decoded == [[0, 1, 2, 3], [0, 2, 3], [0, 3]] and accepted == [2, 0, 1, 2] and not any(skipped)


# ---- generation.py's host logic over a stub session ------------------------------------------------------------------
class _StubSession:
    """Scripted decodes: ``script[call]`` = (ids (B, L) with the prompt, avg_logprob per row)."""

    def __init__(self, script, nsp):
        self.script, self.nsp, self.calls, self.avg_logprob = script, nsp, [], None

    def set_encoder_output(self, enc, key=None):
        pass

    def no_speech_prob(self, sot, token, logits=None):
        return np.asarray(self.nsp[len(self.calls)], np.float64)

    def generate(self, prompt, gen, *, max_length, return_timestamps, sample=None):
        ids, lp = self.script[len(self.calls)]
        self.calls.append(dict(sample, active=np.asarray(sample["active"]).copy(), prompt=prompt.numpy().copy()))
        self.avg_logprob = np.asarray(lp, np.float64)
        ids = np.asarray(ids, np.int64).copy()
        ids[~self.calls[-1]["active"], prompt.shape[1]:] = gen.pad_token_id  # inactive rows: prompt + pad
        return ids


def _stub_model(script, nsp=None):
    from kwhisper.generation import KWhisperForConditionalGeneration

    sess = _StubSession(script, nsp or {})
    eng = types.SimpleNamespace(shape=TINY, device=torch.device("cpu"), dtype=torch.float32,
                                generation_config=generation_constants(TINY),
                                encode=lambda x: torch.zeros(1), new_session=lambda B, beams=1: sess)
    return KWhisperForConditionalGeneration(eng), sess


G = generation_constants(TINY)
TS = G.timestamp_begin
PROMPT_TS = [G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"]]


def _row(body, L=12):
    r = PROMPT_TS + list(body)
    return r + [G.pad_token_id] * (L - len(r))


def test_skip_advances_the_seek_and_contributes_no_segment():
    """Long-form, one row of 45 s: the first window is skipped (low log-probability and a high no-speech probability
    -- which cancels its fallback), so the seek moves on by the window's 3000 frames with no segment, and the second
    window's segment starts at 30 s."""
    eos = G.eos_token_id
    body = [TS, 100, 101, TS + 50, eos]
    script = [([_row(body)], [-2.0]), ([_row(body)], [-0.5])]
    model, sess = _stub_model(script, nsp={0: [0.9], 1: [0.9]})
    res = model.generate(torch.zeros((1, 80, 4500)), language="ja", task="transcribe", return_timestamps=True,
                         temperature=(0.0, 0.4), logprob_threshold=-1.0, compression_ratio_threshold=2.4,
                         no_speech_threshold=0.6, return_segments=True)
    assert len(sess.calls) == 2 and [c["temperature"] for c in sess.calls] == [0.0, 0.0]
    fb = model.stats["fallback"]
    assert fb[0][0]["should_skip"] == [True] and fb[0][0]["needs_fallback"] == [False] and len(fb[0]) == 1
    assert fb[1][0]["should_skip"] == [False] and fb[1][0]["needs_fallback"] == [False]
    assert model.stats["pass_log"] == [([0], [0], [3000]), ([0], [3000], [1500])]
    (seg,) = res["segments"][0]
    assert seg["start"] == pytest.approx(30.0) and seg["end"] == pytest.approx(31.0)
    assert res["sequences"][0].tolist() == [TS, 100, 101, TS + 50]


def test_rows_leave_the_fallback_set_and_the_last_temperature_is_accepted():
    """Three rows over (0.0, 0.2, 0.4): row 1 is accepted at once, row 2 at 0.2, row 0 never passes and keeps its last
    attempt; each attempt decodes only the rows still in the set, and only sampled decodes advance the attempt word."""
    eos = G.eos_token_id
    nots = lambda body: [PROMPT_TS + [G.no_timestamps_token_id] + list(body)  # noqa: E731
                         + [G.pad_token_id] * (8 - len(body))]
    a0 = nots([10, 11, eos])[0], nots([20, 21, 22, eos])[0], nots([30, eos])[0]
    a1 = nots([12, 13, eos])[0], nots([0])[0], nots([31, 32, eos])[0]
    a2 = nots([14, eos])[0], nots([0])[0], nots([0])[0]
    script = [(list(a0), [-2.0, -0.5, -3.0]), (list(a1), [-2.5, np.nan, -0.9]), (list(a2), [-4.0, np.nan, np.nan])]
    model, sess = _stub_model(script)
    model.manual_seed(5)
    out = model.generate(torch.zeros((3, 80, 3000)), language="ja", task="transcribe", return_timestamps=False,
                         temperature=(0.0, 0.2, 0.4), logprob_threshold=-1.0)
    assert [c["active"].tolist() for c in sess.calls] == [[True] * 3, [True, False, True], [True, False, False]]
    assert [c["temperature"] for c in sess.calls] == [0.0, 0.2, 0.4]
    assert [c["attempt"] for c in sess.calls] == [0, 1, 2] and all(c["seed"] == 5 for c in sess.calls)
    (ps,) = model.stats["fallback"]
    assert [at["rows"] for at in ps] == [[0, 1, 2], [0, 2], [0]]
    assert [at["needs_fallback"] for at in ps] == [[True, False, True], [True, False], [True]]
    pad = G.pad_token_id
    assert out.tolist() == [[14, pad, pad], [20, 21, 22], [31, 32, pad]]
    # a second call goes on with the attempt counter; manual_seed restarts it
    sess.calls.clear()
    sess.script = script
    model.generate(torch.zeros((3, 80, 3000)), language="ja", task="transcribe", return_timestamps=False,
                   temperature=(0.0, 0.2, 0.4), logprob_threshold=-1.0)
    assert [c["attempt"] for c in sess.calls] == [2, 3, 4]
    lane = types.SimpleNamespace(_lane=3, _attempts=0)
    assert (lane._lane << 24) | 1 != 1  # lane() handles: the lane index sits above the counter in the attempt word


def test_argument_errors_on_the_host():
    model, _ = _stub_model([])
    f = torch.zeros((1, 80, 3000))
    with pytest.raises(ValueError, match="logprob_threshold"):
        model.generate(f, language="ja", no_speech_threshold=0.6)
    with pytest.raises(ValueError, match="non-empty"):
        model.generate(f, language="ja", temperature=(), logprob_threshold=-1.0)
    for bad in (dict(num_beams=2), dict(return_token_timestamps=True), dict(condition_on_prev_tokens=True),
                dict(output_scores=True), dict(num_return_sequences=2), dict(prompt_ids=torch.tensor([1]))):
        with pytest.raises(NotImplementedError):
            model.generate(f, language="ja", temperature=(0.0, 0.2), logprob_threshold=-1.0, **bad)


def test_temperature_none_with_a_threshold_is_zero():
    eos = G.eos_token_id
    row = PROMPT_TS + [G.no_timestamps_token_id, 10, eos]
    model, sess = _stub_model([([row], [-0.2])])
    model.generate(torch.zeros((1, 80, 3000)), language="ja", task="transcribe", temperature=None, logprob_threshold=-1.0)
    assert sess.calls[0]["temperature"] == 0.0


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_sample_args_layout_matches_c(tmp_path):
    """The ctypes mirror of kw_sample_args has the C header's size and field offsets."""
    from kwhisper import _lib

    cls = _lib.SampleArgs
    fields = [f for f, _ in cls._fields_]
    code = "#include <stdio.h>\n#include <stddef.h>\n#include \"kwhisper.h\"\nint main(){"
    code += 'printf("%zu\\n", sizeof(kw_sample_args));'
    for f in fields:
        code += f'printf("%zu\\n", offsetof(kw_sample_args, {f}));'
    code += "return 0;}"
    src, exe = str(tmp_path / "kw_layout.c"), str(tmp_path / "kw_layout")
    with open(src, "w") as fh:
        fh.write(code)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == ctypes.sizeof(cls)
    for f, off in zip(fields, got[1:]):
        assert getattr(cls, f).offset == off, f
    assert "kw_sample_step" in _lib.EXPORTS and "kw_sample_step_workspace" in _lib.EXPORTS
    assert "sample_step" in _lib.TORCH_OPS
