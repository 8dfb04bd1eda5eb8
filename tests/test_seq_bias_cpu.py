"""CPU tests of ``sequence_bias`` / ``bad_words_ids``: the numpy restatement tests/_seq_bias_ref.py against
transformers' own SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor, the host table of kwhisper/seq_bias.py
against the restatement's, and generate()'s host logic over a stub session (where the two arguments come from, where
they go, what they refuse)."""
import json
import types

import numpy as np
import pytest
import torch

import _seq_bias_ref as SR

from kwhisper import seq_bias as SB
from kwhisper.config import TINY, generation_constants

F32 = np.float32
INF = float("inf")
G = generation_constants(TINY)
TS = G.timestamp_begin
PROMPT_TS = [G.decoder_start_token_id, G.lang_to_id["<|ja|>"], G.task_to_id["transcribe"]]


# ---- the restatement against transformers ---------------------------------------------------------------------------
def _tf_bias(ids, x, sequence_bias):
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor

    return SequenceBiasLogitsProcessor(sequence_bias)(torch.from_numpy(ids), torch.from_numpy(x).clone()).numpy()


def _tf_bad(ids, x, bad_words_ids, eos):
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor

    return NoBadWordsLogitsProcessor(bad_words_ids, eos)(torch.from_numpy(ids), torch.from_numpy(x).clone()).numpy()


def _random_case(rng, V, L, n_seq):
    """Histories over a small pool (so tails do recur), entries cut out of the histories' ends (so they match) and
    random ones (so they do not), lengths 1 .. 6, several entries per last token."""
    pool = np.concatenate([[1, V - 1], rng.choice(np.arange(2, V - 1), 6, replace=False)])
    ids = rng.choice(pool, (4, L)).astype(np.int64)
    bias = {}
    for _ in range(n_seq):
        n = int(rng.integers(1, 7))
        if rng.random() < 0.6 and n - 1 <= L:
            r = int(rng.integers(4))
            seq = tuple(ids[r, L - (n - 1):].tolist()) + (int(rng.choice(pool)),)
        else:
            seq = tuple(int(t) for t in rng.choice(pool, n))
        bias[seq] = float(np.round(rng.standard_normal() * 3, 2))
    x = (rng.standard_normal((4, V)) * 4).astype(F32)
    return ids, x, bias


@pytest.mark.parametrize("L", [1, 2, 4, 5, 40])
def test_restatement_equals_transformers_random(L):
    pytest.importorskip("transformers")
    V, fired = 97, 0
    for seed in range(6):
        ids, x, bias = _random_case(np.random.default_rng(100 * L + seed), V, L, 24)
        want = _tf_bias(ids, x, dict(bias))
        got = SR.sequence_bias(ids, x, bias)
        assert SR.same(got, want), (L, seed)
        fired += int((want != x).sum())
        bad = [list(k) for k in bias]
        assert SR.same(SR.sequence_bias(ids, x, SR.bad_words_dict(bad, [1])), _tf_bad(ids, x, bad, [1]))
    assert fired


V = 97
HIST = np.array([[7, 8, 9, 10, 11], [7, 8, 9, 10, 12], [3, 3, 3, 3, 3]], np.int64)
EDGE = {
    # history shorter than (6 tokens), equal to (5 + 1 is longer; 5-token entry = 4-token prefix) and longer than an entry
    "longer_than_history": {(7, 8, 9, 10, 11, 20): -2.0},
    "prefix_is_whole_history_but_one": {(8, 9, 10, 11, 21): 3.0},
    "as_long_as_history_beside_a_longer_one": {(7, 8, 9, 10, 11, 22): 3.0, (8, 9, 10, 12, 23): 1.0},
    "short_entry": {(11, 24): 1.5, (12, 24): -1.5},
    # "a sequence reaching into the prompt": the first tokens of the row play the prompt
    "into_the_prompt": {(7, 8, 9, 10, 11, 25)[1:]: 2.0},
    "two_entries_one_last_token": {(11, 30): 1.25, (10, 11, 30): 2.5, (9, 10, 12, 30): 4.0},
    "length1_and_longer_on_one_token": {(10, 11, 31): 0.3, (31,): 0.1, (11, 31): 0.2},
    "token_v_minus_1": {(V - 1,): 1.0, (11, V - 1): -INF, (3, 3, V - 1): 2.0},
    "neg_inf": {(11, 40): -INF, (41,): -INF},
    "pos_inf": {(11, 42): INF, (43,): INF},
    "both_on_one_token": {(11, 44): INF, (10, 11, 44): -INF, (45,): INF, (3, 45): -INF},
}


@pytest.mark.parametrize("name", sorted(EDGE))
def test_restatement_equals_transformers_edges(name):
    pytest.importorskip("transformers")
    bias = EDGE[name]
    x = (np.random.default_rng(3).standard_normal((3, V)) * 4).astype(F32)
    for L in (1, 2, 4, 5):
        ids = np.ascontiguousarray(HIST[:, 5 - L:])
        want = _tf_bias(ids, x, dict(bias))
        assert SR.same(SR.sequence_bias(ids, x, bias), want), (name, L)
    want = _tf_bias(HIST, x, dict(bias))
    if name == "both_on_one_token":
        assert np.isnan(want[0, 44]) and np.isnan(want[2, 45]) and want[1, 44] == x[1, 44]
    if name == "longer_than_history":
        assert (want == x).all()
    if name not in ("longer_than_history",):
        assert (want != x).any() or np.isnan(want).any()
    # the list form is the dict form
    as_list = [[list(k), v] for k, v in bias.items()]
    assert SR.same(SR.sequence_bias(HIST, x, SR.as_dict(as_list)), want)
    assert SR.same(_tf_bias(HIST, x, as_list), want)


def test_bad_words_eos_filter_and_plus_inf_then_ban():
    pytest.importorskip("transformers")
    x = (np.random.default_rng(4).standard_normal((3, V)) * 4).astype(F32)
    bad = [[50], [60], [11, 50], [10, 11, 61], [62]]
    for eos in ([50], [50, 62], 60):
        want = _tf_bad(HIST, x, bad, eos)
        ent = SR.bad_words_dict(bad, eos)
        assert SR.same(SR.sequence_bias(HIST, x, ent), want)
        e = [eos] if isinstance(eos, int) else eos
        assert all((k,) not in ent for k in e) and (11, 50) in ent
        assert all(np.isfinite(want[2, k]) for k in e)  # [eos] itself is not banned ...
    assert np.isneginf(_tf_bad(HIST, x, bad, [50])[0, 50])  # ... but a longer entry ending in eos still bans it
    # +inf from sequence_bias, then a ban: NaN, through the whole chain
    got = SR.process(HIST, x, {(11, 61): INF}, SR.bad_words_dict([[10, 11, 61]]), 1.3, 0)
    assert np.isnan(got[0, 61]) and np.isfinite(got[1, 61])


def test_host_table_is_the_restatements():
    """kwhisper.seq_bias.SeqTable: grouped by last token (stable), the length-1 entry first, the rest in dict order."""
    for seed in range(4):
        _, _, bias = _random_case(np.random.default_rng(seed), V, 12, 40)
        bias[(5,)] = 0.5
        bias[(9, 5)] = 0.25
        t = SB.SeqTable(SB.sequence_bias_dict(dict(bias)), V)
        for got, want in zip(t.arrays(), SR.flat_table(bias)):
            assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        assert t.n_seq == len(bias) and t.n_groups == len({k[-1] for k in bias}) and t.max_len == max(map(len, bias))
        assert (np.diff(t.group_tok) > 0).all()
    d = {(3, 5): 1.0, (5,): 2.0, (4, 5): 3.0, (2,): 4.0}
    t = SB.SeqTable(d)
    assert t.group_tok.tolist() == [2, 5] and t.values.tolist() == [4.0, 2.0, 1.0, 3.0]
    assert t.tokens.tolist() == [2, 5, 3, 5, 4, 5] and t.seq_off.tolist() == [0, 1, 2, 4, 6]
    assert t.group_off.tolist() == [0, 1, 4]
    # a digest per content; the same content, the same digest
    assert SB.SeqTable(dict(d)).digest == t.digest != SB.SeqTable({**d, (2,): 4.5}).digest


# ---- argument errors --------------------------------------------------------------------------------------------------
BAD_BIAS = [{}, [], "x", {5: 1.0}, {(): 1.0}, {(5, -1): 1.0}, {(5.0,): 1.0}, {(5,): 1}, [[[5], 1]], [[[0], 1.0]],
            [[[5, -2], 1.0]], [[5, 1.0]]]
BAD_WORDS = [[], "x", [5], [[5], 6], [[5, -1]], [[5.0]]]


@pytest.mark.parametrize("i", range(len(BAD_BIAS)))
def test_sequence_bias_errors_are_the_references(i):
    tf = pytest.importorskip("transformers.generation.logits_process")
    with pytest.raises(ValueError) as want:
        tf.SequenceBiasLogitsProcessor(BAD_BIAS[i])
    with pytest.raises(ValueError) as got:
        SB.sequence_bias_dict(BAD_BIAS[i])
    assert str(got.value) == str(want.value)


@pytest.mark.parametrize("i", range(len(BAD_WORDS)))
def test_bad_words_errors_are_the_references(i):
    tf = pytest.importorskip("transformers.generation.logits_process")
    with pytest.raises(ValueError) as want:
        tf.NoBadWordsLogitsProcessor(BAD_WORDS[i], [1])
    with pytest.raises(ValueError) as got:
        SB.bad_words_dict(BAD_WORDS[i], [1])
    assert str(got.value) == str(want.value)


def test_vocabulary_error_is_the_references():
    tf = pytest.importorskip("transformers.generation.logits_process")
    bias = {(5, 97): 1.0, (200,): 2.0}
    with pytest.raises(ValueError) as want:
        tf.SequenceBiasLogitsProcessor(dict(bias))(torch.zeros((1, 3), dtype=torch.int64), torch.zeros((1, 97)))
    with pytest.raises(ValueError) as got:
        SB.SeqTable(SB.sequence_bias_dict(bias), 97)
    assert str(got.value) == str(want.value) and "[97, 200]" in str(got.value)


def test_caps():
    """include/kwhisper.h states them; no smaller than 1,024 sequences of up to 16 tokens."""
    hdr = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "kwhisper.h")).read()
    assert f"#define KW_SEQ_BIAS_MAX_SEQS {SB.MAX_SEQS}\n" in hdr and f"#define KW_SEQ_BIAS_MAX_LEN {SB.MAX_LEN}\n" in hdr
    assert SB.MAX_SEQS >= 1024 and SB.MAX_LEN >= 16
    ok = {tuple(range(1, 17)) + (i + 20,): 1.0 for i in range(1024)}
    assert len(SB.SeqTable(ok, 2000)) == 1024
    SB.SeqTable({(i + 1,): 1.0 for i in range(SB.MAX_SEQS)})
    SB.SeqTable({tuple(range(1, SB.MAX_LEN + 1)): 1.0})
    with pytest.raises(NotImplementedError, match="at most"):
        SB.SeqTable({(i + 1,): 1.0 for i in range(SB.MAX_SEQS + 1)})
    with pytest.raises(NotImplementedError, match="at most"):
        SB.SeqTable({tuple(range(1, SB.MAX_LEN + 2)): 1.0})


# ---- generate()'s host logic over a stub session -----------------------------------------------------------------------
class _StubSession:
    """Scripted decodes that record the keywords each call was given."""

    def __init__(self, script):
        self.script, self.calls, self.avg_logprob = script, [], None

    def set_encoder_output(self, enc, key=None):
        pass

    def _next(self, kind, kw):
        ids, lp = self.script[len(self.calls) % len(self.script)]
        self.calls.append(dict(kind=kind, kw=dict(kw)))
        self.avg_logprob = np.asarray(lp, np.float64)
        return np.asarray(ids, np.int64).copy()

    def generate(self, prompt, gen, *, max_length, return_timestamps, **kw):
        return self._next("greedy", kw)

    def generate_beam(self, prompt, gen, *, num_beams, max_length, return_timestamps, **kw):
        return self._next("beam", kw)


def _stub_model(script, gen=None):
    from kwhisper.generation import KWhisperForConditionalGeneration

    sess = _StubSession(script)
    eng = types.SimpleNamespace(shape=TINY, device=torch.device("cpu"), dtype=torch.float32,
                                generation_config=gen or generation_constants(TINY),
                                encode=lambda x: torch.zeros(1), new_session=lambda B, beams=1: sess)
    return KWhisperForConditionalGeneration(eng), sess


def _row(body, L=12):
    r = PROMPT_TS + list(body)
    return r + [G.pad_token_id] * (L - len(r))


BODY = [TS, 100, 101, TS + 50, G.eos_token_id]
KW = dict(language="ja", task="transcribe", return_timestamps=True)
X = torch.zeros((1, 80, 3000))
BIAS = {(100,): 1.5, (100, 101): -2.0}
BAD = [[7, 8], [9]]


def test_generate_takes_the_arguments_parent_refuses():
    """On the parent commit both names land in the "not used by the model" ValueError."""
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(X, sequence_bias=dict(BIAS), **KW)
    sb, bw = sess.calls[0]["kw"]["seq_tables"]
    assert bw is None and sb.digest == SB.SeqTable(BIAS).digest
    model.generate(X, bad_words_ids=BAD, **KW)
    sb, bw = sess.calls[1]["kw"]["seq_tables"]
    assert sb is None and bw.digest == SB.SeqTable({(7, 8): -INF, (9,): -INF}).digest
    assert np.isneginf(bw.values).all()
    # the list form is the dict form
    model.generate(X, sequence_bias=[[list(k), v] for k, v in BIAS.items()], bad_words_ids=BAD, **KW)
    sb, bw = sess.calls[2]["kw"]["seq_tables"]
    assert sb.digest == SB.SeqTable(BIAS).digest and bw is not None


def test_tables_reach_every_pass_attempt_and_beam_call():
    d = SB.SeqTable(BIAS).digest
    both = dict(sequence_bias=dict(BIAS), bad_words_ids=BAD)

    def digests(sess):
        return [c["kw"]["seq_tables"][0].digest for c in sess.calls]

    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(torch.zeros((1, 80, 4500)), **both, **KW)  # long-form, 45 s: two passes
    assert len(sess.calls) == 2 and digests(sess) == [d, d] and all(c["kind"] == "greedy" for c in sess.calls)
    model, sess = _stub_model([([_row(BODY)], [-2.0])])
    model.generate(X, **both, repetition_penalty=1.3, temperature=(0.0, 0.2, 0.4), logprob_threshold=-1.0, **KW)
    assert [c["kw"]["sample"]["temperature"] for c in sess.calls] == [0.0, 0.2, 0.4] and digests(sess) == [d, d, d]
    assert all(c["kw"]["repeat"] == (1.3, 0) and c["kw"]["seq_tables"][1] is not None for c in sess.calls)
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(X, num_beams=3, **both, **KW)
    assert [c["kind"] for c in sess.calls] == ["beam"] and digests(sess) == [d]
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(torch.zeros((1, 80, 4500)), condition_on_prev_tokens=True, **both, **KW)
    assert len(sess.calls) == 2 and digests(sess) == [d, d]
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate_multitask(X, [("ja", "transcribe"), ("en", "translate")], return_timestamps=True, **both)
    assert len(sess.calls) == 2 and digests(sess) == [d, d]


def test_values_come_from_the_call_else_the_config():
    gen = generation_constants(TINY)
    assert gen.sequence_bias is None and gen.bad_words_ids is None  # the dataclass carries the fields
    gen.sequence_bias = [[[100], 1.5], [[100, 101], -2.0]]  # (generation_config.json stores the list form)
    gen.bad_words_ids = [[7, 8]]
    model, sess = _stub_model([([_row(BODY)], [-0.5])], gen)
    model.generate(X, **KW)
    model.generate(X, sequence_bias={(5,): 1.0}, **KW)
    model.generate(X, bad_words_ids=[[9]], **KW)
    model.generate(X, generation_config={**generation_constants(TINY).to_dict(), "bad_words_ids": [[3]]}, **KW)
    got = [tuple(None if t is None else t.digest for t in c["kw"]["seq_tables"]) for c in sess.calls]
    dg = lambda d: SB.SeqTable(d).digest  # noqa: E731
    assert got == [(dg(BIAS), dg({(7, 8): -INF})), (dg({(5,): 1.0}), dg({(7, 8): -INF})),
                   (dg(BIAS), dg({(9,): -INF})), (None, dg({(3,): -INF}))]
    # a deep copy / dict round trip of the config keeps tuple keys
    gen.sequence_bias = dict(BIAS)
    model, sess = _stub_model([([_row(BODY)], [-0.5])], gen)
    model.generate(X, **KW)
    assert sess.calls[0]["kw"]["seq_tables"][0].digest == dg(BIAS)


@pytest.mark.parametrize("off", [dict(), dict(sequence_bias=None, bad_words_ids=None),
                                 dict(bad_words_ids=[[G.eos_token_id]])])
def test_call_without_the_arguments_is_todays_call(off):
    """No new keyword reaches the session: not for the plain, the beam, the fallback, the token-timestamp or the
    conditioned call.  Bad words that the eos filter empties are no argument."""
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    model.generate(X, **off, **KW)
    model.generate(X, num_beams=2, **off, **KW)
    model.generate(X, temperature=(0.0, 0.4), logprob_threshold=-1.0, **off, **KW)
    model.generate(torch.zeros((1, 80, 4500)), condition_on_prev_tokens=True, **off, **KW)
    model.generate(X, repetition_penalty=1.3, **off, **KW)
    old = {"key_start", "sample", "repeat", "length_penalty", "early_stopping"}  # the session keywords of these calls
    assert all(set(c["kw"]) <= old for c in sess.calls), [sorted(c["kw"]) for c in sess.calls]
    assert [c["kind"] for c in sess.calls] == ["greedy", "beam", "greedy", "greedy", "greedy", "greedy"]


def test_refusals():
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    with pytest.raises(ValueError, match="not used by the model.*sequence_biass"):
        model.generate(X, sequence_biass={(5,): 1.0}, **KW)
    with pytest.raises(ValueError, match="`sequence_bias` has to be a non-empty dictionary"):
        model.generate(X, sequence_bias={}, **KW)
    with pytest.raises(ValueError, match="`sequence_bias` has to be a dict with floats as values"):
        model.generate(X, sequence_bias={(5,): 1}, **KW)
    with pytest.raises(ValueError, match="`bad_words_ids` has to be a list of lists"):
        model.generate(X, bad_words_ids=[5], **KW)
    with pytest.raises(ValueError, match="`bad_words_ids` has to be a non-empty list"):
        model.generate(X, bad_words_ids=[], **KW)
    V = TINY.vocab_size
    with pytest.raises(ValueError, match=rf"The model vocabulary size is {V}, but the following tokens were being "
                                         rf"biased: \[{V}\]"):
        model.generate(X, sequence_bias={(5, V): 1.0}, **KW)
    with pytest.raises(ValueError, match="vocabulary size"):
        model.generate(X, bad_words_ids=[[V + 3]], **KW)
    with pytest.raises(NotImplementedError, match="at most"):
        model.generate(X, bad_words_ids=[[i + 1] for i in range(SB.MAX_SEQS + 1)], **KW)
    with pytest.raises(NotImplementedError, match="at most"):
        model.generate(X, sequence_bias={tuple(range(1, SB.MAX_LEN + 2)): 1.0}, **KW)
    assert not sess.calls  # refused before any device work


def test_assistant_model_is_refused():
    model, sess = _stub_model([([_row(BODY)], [-0.5])])
    assistant, _ = _stub_model([([_row(BODY)], [-0.5])])
    kw = dict(language="ja", task="transcribe", return_timestamps=False)
    for arg in (dict(sequence_bias={(5,): 1.0}), dict(bad_words_ids=[[5]])):
        with pytest.raises(NotImplementedError, match="`assistant_model` together with `sequence_bias` / `bad_words_ids`"):
            model.generate(X, assistant_model=assistant, **arg, **kw)
    assert not sess.calls


def test_one_digest_for_both_forms():
    """pseudo_label's checkpoint plan digest: a dict with tuple keys is no JSON; both forms of one bias hash alike, in
    any order, and another value hashes differently."""
    from kwhisper.pseudo_label import run_digest

    model = types.SimpleNamespace()
    d1 = run_digest(model, gen_kwargs=dict(language="ja", sequence_bias={(100,): 1.5, (100, 101): -INF}), pad_token_id=1)
    d2 = run_digest(model, gen_kwargs=dict(language="ja", sequence_bias=[[[100, 101], -INF], [[100], 1.5]]),
                    pad_token_id=1)
    d3 = run_digest(model, gen_kwargs=dict(language="ja", sequence_bias={(100,): 1.25, (100, 101): -INF}), pad_token_id=1)
    d4 = run_digest(model, gen_kwargs=dict(language="ja", bad_words_ids=[[7, 8]]), pad_token_id=1)
    assert d1 == d2 and len({d1, d3, d4, run_digest(model, gen_kwargs=dict(language="ja"), pad_token_id=1)}) == 4
    assert json.dumps(SB.canonical_sequence_bias({(2, 1): 1.0, (1,): 2.0})) == "[[[1], 2.0], [[2, 1], 1.0]]"
