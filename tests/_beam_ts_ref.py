"""Reference code for token timestamps under beam search (tests only).

``BeamParentRef`` is ``_beam_ref.BeamRef`` -- the step restatement over ``oracle.generate.beam_step`` -- that also
keeps what ``kw_beam_select_parents`` records beside the plain step: the per-step parent log and the finished
slots' parents.  ``brute_histories`` builds beam histories by carrying whole lists through the steps (no backtrace),
``parents_from_beam_indices`` turns a ``beam_indices`` table back into a parent log, and ``reference_row_table``
runs the reference's own torch lines (transformers generation_whisper.py:272-291) on a ``beam_indices`` array."""
import numpy as np

import _beam_ref as R


class BeamParentRef(R.BeamRef):
    """``BeamRef`` with ``plog`` (max_length, B nb) -- row L, written by the step at cur_len = L: the running row
    every next running row continues -- and ``fin_par`` (B, nb): the running row every finished slot's hypothesis
    was taken from, permuted with the slot like the finished scores."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._init_parents()

    def _init_parents(self):
        self.plog = np.zeros((self.max_length, self.B * self.nb), np.int32)
        self.fin_par = np.full((self.B, self.nb), -1, np.int32)

    @classmethod
    def from_state(cls, st, bp, nb, max_length, begin_index, fin_par=None, **kw):
        ref = super().from_state(st, bp, nb, max_length, begin_index, **kw)
        ref._init_parents()
        if fin_par is not None:
            ref.fin_par = np.array(fin_par, np.int32)
        return ref

    def step(self, lp):
        L = self.st["cur_len"]
        info = super().step(lp)
        rows = info["parent"] + np.arange(self.B)[:, None] * self.nb  # (B, 2 nb): the continuations' running rows
        self.plog[L] = np.take_along_axis(rows, info["run_pick"], axis=1).reshape(-1)
        merged = np.concatenate([self.fin_par, rows.astype(np.int32)], axis=1)
        self.fin_par = np.take_along_axis(merged, info["fin_pick"], axis=1)
        return info


def brute_histories(parents, nb):
    """``parents``: a list over steps of (R,) arrays, entry r = the running row that next running row r continues.
    Returns a list over steps of the rows' histories after that step: history[r] = the running rows whose logits
    gave each of row r's tokens, carried along as whole lists."""
    R_ = len(parents[0])
    hist = [[] for _ in range(R_)]
    out = []
    for par in parents:
        hist = [hist[int(par[r])] + [int(par[r])] for r in range(R_)]
        out.append(hist)
    return out


def parents_from_beam_indices(bi, P, max_length, R_):
    """A parent log and the returned hypotheses' parents that a search with these ``beam_indices`` (B, W; -1 padded)
    would have recorded (entries no returned hypothesis went through stay 0)."""
    bi = np.asarray(bi)
    plog = np.zeros((max_length, R_), np.int32)
    fin_par = np.full(len(bi), -1, np.int32)
    fin_len = (bi != -1).sum(-1).astype(np.int32)
    for b, n in enumerate(fin_len):
        if n == 0:
            continue
        fin_par[b] = bi[b, n - 1]
        for k in range(1, n):
            plog[P + k - 1, bi[b, k]] = bi[b, k - 1]
    return plog, fin_par, fin_len


def reference_row_table(beam_indices, num_input_ids):
    """transformers generation_whisper.py:272-291 on a ``beam_indices`` array (torch, as there), then the cut of the
    prompt positions (:333): for every returned row, the running row each DTW step's weights are taken from."""
    import torch

    beam_indices = torch.from_numpy(np.asarray(beam_indices).astype(np.int64))
    weight_length = (beam_indices != -1).sum(-1).max()
    beam_indices = beam_indices[:, :weight_length]
    if num_input_ids is not None and num_input_ids > 1:
        weight_length += num_input_ids - 1
        beam_indices_first_step_unrolled = (
            torch.ones(beam_indices.shape[0], num_input_ids - 1, dtype=torch.long) * (beam_indices[:, 0:1]))
        unrolled_beam_indices = torch.cat([beam_indices_first_step_unrolled, beam_indices], dim=-1)
    else:
        unrolled_beam_indices = beam_indices
    unrolled_beam_indices = unrolled_beam_indices.masked_fill(unrolled_beam_indices == -1, 0)
    return unrolled_beam_indices[:, num_input_ids:].numpy()
