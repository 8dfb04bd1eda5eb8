"""Token timestamps under beam search, host side (no GPU): the backtrace from the parent log to the reference's
``beam_indices``, the row table built from them, the step restatement with the parent outputs, and generate()'s
argument checks."""
import types

import numpy as np
import pytest

import _beam_ref as R
import _beam_ts_ref as T
from kwhisper.decode import beam_backtrace, beam_row_table


def _passes(g):
    """(mode, pass index, number of beams) of every committed pass."""
    import json

    for mode in g["modes"].tolist():
        nb = json.loads(str(g[f"{mode}_kw"]))["num_beams"]
        for i in range(int(g[f"{mode}_passes"])):
            yield mode, i, nb


# ---- the backtrace -----------------------------------------------------------------------------------------
def test_backtrace_equals_brute_force_histories():
    """2 items x 3 beams, 6 steps of hand-made parents (every beam switches somewhere); item 0's hypothesis is taken at
    step 2 from a candidate of running row 1, item 1's at the last step from row 5."""
    nb, P, max_length = 3, 4, 12
    parents = [np.array(p) for p in ([0, 0, 0, 3, 3, 3], [0, 0, 1, 4, 3, 3], [1, 0, 2, 3, 3, 5],
                                     [2, 2, 0, 5, 4, 3], [0, 1, 1, 3, 5, 5], [1, 0, 2, 4, 4, 3])]
    plog = np.zeros((max_length, 6), np.int32)
    for t, p in enumerate(parents):
        plog[P + t] = p
    hist = T.brute_histories(parents, nb)
    # a finished hypothesis is a candidate: the parent's history before the step + the parent
    fin = {0: (2, 1), 1: (5, 5)}  # item -> (step, running row the candidate came from)
    want = np.full((2, 6), -1, np.int32)
    for b, (t, r) in fin.items():
        h = (hist[t - 1][r] if t else []) + [r]
        want[b, : len(h)] = h
    fin_parent = np.array([fin[0][1], fin[1][1]])
    fin_len = np.array([fin[0][0] + 1, fin[1][0] + 1])
    got = beam_backtrace(plog, fin_parent, fin_len, P)
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32 and len(set(got[1].tolist())) > 1
    # a hypothesis of a single token, and one that never finished
    got = beam_backtrace(plog, np.array([2, -1]), np.array([1, 0]), P)
    np.testing.assert_array_equal(got, [[2], [-1]])


def test_backtrace_recovers_the_committed_beam_indices(gold):
    g = gold("beam_ts_tiny")
    short = switch = 0
    for mode, i, nb in _passes(g):
        bi, P = g[f"{mode}_p{i}_beam_indices"], int(g[f"{mode}_p{i}_P"])
        plog, fin_par, fin_len = T.parents_from_beam_indices(bi, P, P + bi.shape[1] + 3, len(bi) * nb)
        np.testing.assert_array_equal(beam_backtrace(plog, fin_par, fin_len, P), bi)
        lens = (bi != -1).sum(-1)
        assert lens[0] == lens.max()  # the agreed region of the row-0 rule: the pass's first item is among the longest
        short += int((lens < lens.max()).any())
        switch += int(any(len(set(bi[b, : lens[b]].tolist())) > 1 for b in range(len(bi))))
        assert bi.shape[1] == lens.max() and g[f"{mode}_p{i}_ts"].shape[1] == P + bi.shape[1]
    assert short and switch  # a row shorter than its pass's longest; a beam switch inside a returned hypothesis


# ---- the row table -----------------------------------------------------------------------------------------
def test_row_table_equals_the_reference_lines(gold):
    g = gold("beam_ts_tiny")
    fell_back = 0
    for mode, i, nb in _passes(g):
        bi, P = g[f"{mode}_p{i}_beam_indices"], int(g[f"{mode}_p{i}_P"])
        table = beam_row_table(bi)
        assert table.dtype == np.int32 and table.shape == (len(bi), bi.shape[1] - 1)
        np.testing.assert_array_equal(table, T.reference_row_table(bi, P))
        assert table.min() >= 0 and table.max() < len(bi) * nb
        fell_back += int(((bi[:, 1:] == -1) & (table == 0)).any())
    assert fell_back
    np.testing.assert_array_equal(beam_row_table(np.array([[3, 4, -1, -1], [6, 7, 8, 6]])), [[4, 0, 0], [7, 8, 6]])
    assert beam_row_table(np.array([[2], [5]])).shape == (2, 0)


# ---- the step restatement with the parent outputs ------------------------------------------------------------
@pytest.mark.parametrize("case", [R.CLOSED_LOOP_CASES[i] for i in (0, 7, 14, 22, 31)])
def test_parent_restatement_agrees_with_the_plain_one(case):
    """Closed loop on the toy model: ``BeamParentRef`` goes through the states ``BeamRef`` goes through, and its
    parent outputs, backtraced, are the oracle's own ``beam_idx`` of the best finished hypothesis."""
    gen, table, max_length, kw = R.case_setup(case)
    nb, rt = case[1], case[2]
    plain, trace = R.run_case(case)
    ref = T.BeamParentRef(R.CLOSED_LOOP_PROMPT, nb, max_length, eos=gen["eos_token_id"], fill=gen["pad_token_id"], **kw)
    for want in trace:
        hist = ref.history()
        lp = R.processed_logprobs(hist, table[hist[:, -1]], gen, ref.P, rt).reshape(ref.B, nb, -1)
        L = ref.st["cur_len"]
        ref.step(lp)
        assert R.same_state(ref.st, want)
        np.testing.assert_array_equal(ref.plog[L], ref.st["run_bi"][:, :, L - ref.P].reshape(-1))
    assert not ref.go and np.array_equal(ref.bp, plain.bp)
    st = ref.st
    # every finished slot's parent is the last valid entry of its beam_idx row
    for b in range(ref.B):
        for j in range(nb):
            n = int(st["fin_len"][b, j])
            if st["fin"][b, j]:
                assert ref.fin_par[b, j] == st["beam_idx"][b, j, n - 1]
    fin_len = np.where(st["fin"][:, 0], st["fin_len"][:, 0], 0)
    bi = beam_backtrace(ref.plog, ref.fin_par[:, 0], fin_len, ref.P)
    inside = np.arange(bi.shape[1]) < fin_len[:, None]
    np.testing.assert_array_equal(bi, np.where(inside, st["beam_idx"][:, 0, : bi.shape[1]], -1))


# ---- generate()'s argument checks ----------------------------------------------------------------------------
def _host_model(alignment_heads):
    """generate()'s argument checks run before anything touches the device: a model over a stub engine."""
    from kwhisper.config import TINY, generation_constants
    from kwhisper.generation import KWhisperForConditionalGeneration

    gen = generation_constants(TINY)
    gen.alignment_heads = alignment_heads
    m = object.__new__(KWhisperForConditionalGeneration)
    m.engine = types.SimpleNamespace(shape=TINY, generation_config=gen, device="cpu")
    m.generation_config = gen
    return m


class _ReachedTheDevice(Exception):
    pass


def test_beam_search_with_token_timestamps_is_no_longer_refused():
    """On an engine that declares ``beam_token_ts``, as WhisperEngine does, the combination passes every argument
    check (the stub's first device call is what stops it); with the fallback, a prompt or more than 8 beams it is
    refused as before.  (An engine object that does not declare it is still refused: tests/test_token_ts_cpu.py.)"""
    import torch

    m = _host_model([[3, 0]])
    m.engine.beam_token_ts = True

    def reached(*a, **k):
        raise _ReachedTheDevice

    m._init_tokens = reached
    feats = torch.zeros(1, 80, 3000)
    with pytest.raises(_ReachedTheDevice):
        m.generate(feats, return_token_timestamps=True, num_beams=3)
    for bad in (dict(temperature=(0.0, 0.4)), dict(logprob_threshold=-1.0), dict(prompt_ids=np.array([5, 6])),
                dict(condition_on_prev_tokens=True)):
        with pytest.raises(NotImplementedError):
            m.generate(feats, return_token_timestamps=True, num_beams=3, **bad)
    with pytest.raises(NotImplementedError, match="num_beams > 8"):
        m.generate(feats, return_token_timestamps=True, num_beams=9)
