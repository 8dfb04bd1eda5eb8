"""Step-wise reference for the beam-search kernels (tests only).  Everything numeric is ``oracle.generate``:
``beam_step`` is the loop body of the ``beam_search`` that ``test_oracle_golden.py`` pins to transformers, and
``process_logits`` / ``_log_softmax`` are the processors on log-probs.  On top of that this module keeps what the
device keeps and the oracle does not (the slot table of ``kw_beam_select``), restates the kernels' two-stage
selection (per-row candidates, then the flat top-k over them), holds a stateless toy "model" for closed-loop
runs, and counts the events a run went through."""
import collections

import numpy as np

from oracle import generate as og

NEG = np.float32(-1.0e9)


# ---- a toy vocabulary with Whisper's layout: text < eos < specials < no_timestamps < timestamps -----------------
def toy_gen(V, nb=2, *, mostly_suppressed=False):
    """The generation constants ``process_logits`` reads, for a V-token vocabulary.  ``max_initial_timestamp_index``
    leaves the first step at least 2 nb timestamps (the one live row must fill the top 2 nb alone there)."""
    eos, ts_begin = V * 5 // 8, V * 3 // 4
    sup = list(range(eos + 1, ts_begin - 1)) + [1, 5]
    if mostly_suppressed:
        sup += [t for t in range(8, eos) if t % 8]
    return {"suppress_tokens": sorted(set(sup)), "begin_suppress_tokens": [3, eos], "eos_token_id": eos,
            "pad_token_id": eos, "no_timestamps_token_id": ts_begin - 1,
            "max_initial_timestamp_index": min(V - ts_begin - 1, max(2 * nb - 1, (V - ts_begin) // 2))}


def grid_table(V, seed, *, eos_boost=0.0, ts_boost=0.0, scale=2.0):
    """A V x V f32 table on a 0.5 grid (equal logits give bit-equal log-probs, unequal ones differ by >= 0.5 before
    the normaliser): the toy model's logits of a row are ``table[last token of the row]``."""
    rng = np.random.default_rng(seed)
    g = toy_gen(V)
    t = np.round(rng.standard_normal((V, V)) * scale * 2) / 2
    t[:, g["eos_token_id"]] += eos_boost
    t[:, g["no_timestamps_token_id"] + 1:] += ts_boost
    t[rng.random((V, V)) < 0.02] = -0.0
    return t.astype(np.float32)


class ToyModel:
    """The table as a model for ``oracle.generate.beam_search`` (no cache: ``reorder`` has nothing to move)."""

    def __init__(self, table):
        self.table = table

    def new_cache(self, enc):
        return None

    def decode(self, ids, cache):
        return self.table[np.asarray(ids)]

    def reorder(self, cache, idx):
        pass


# ---- the processed log-probs and the candidates kw_beam_logprobs hands on ---------------------------------------
def processed_logprobs(hist, logits, gen, begin_index, return_timestamps):
    """``process_logits(history, log_softmax(logits))``: (R, V) f32, the normaliser summed in float64."""
    return og.process_logits(np.asarray(hist), og._log_softmax(np.asarray(logits)), gen, begin_index, return_timestamps)


def timestamp_margin(hist, logits, gen, begin_index):
    """Per row, WhisperTimeStamp's decision variable in float64: logsumexp(log-probs of the timestamps) minus the
    best text log-prob, on the scores the earlier rules left (text is banned when this is positive)."""
    ts = gen["no_timestamps_token_id"] + 1
    lp = og._log_softmax(np.asarray(logits))
    post = og.process_logits(np.asarray(hist), lp, gen, begin_index, True)
    no_ts = lp.copy()
    no_ts[:, ts:] = -np.inf  # without timestamp mass the rule never fires: the text scores before it
    pre = og.process_logits(np.asarray(hist), no_ts, gen, begin_index, True)
    pre[:, ts:] = post[:, ts:]
    pre = pre.astype(np.float64)
    out = np.empty(len(pre))
    with np.errstate(invalid="ignore", divide="ignore"):
        for r, s in enumerate(pre):
            m = s.max()
            logp = s - (m + np.log(np.exp(s - m).sum()))
            mt = logp[ts:].max()
            ts_lp = mt + np.log(np.exp(logp[ts:] - mt).sum()) if np.isfinite(mt) else -np.inf
            tx = logp[:ts].max()
            out[r] = np.inf if not np.isfinite(tx) else (-np.inf if not np.isfinite(ts_lp) else ts_lp - tx)
    return out


def row_candidates(lp, k):
    """Stage one: every row's k best by (log-prob descending, token ascending) -> (values, tokens), shape (..., k).
    A place past the row's finite scores holds -inf and the lowest tokens that are -inf, in order."""
    idx = og._topk(lp, k)
    return np.take_along_axis(lp, idx, axis=-1).astype(np.float32), idx.astype(np.int32)


def scatter_candidates(cand_val, cand_idx, V):
    """The candidates as a (..., V) log-prob array that is -inf elsewhere.  The flat top-k of ``beam_step`` over it
    is stage two: by (candidate + row score descending, flat index ascending).  (A -inf place can only be taken
    when the item holds fewer than 2 nb finite candidates, and then from the first row, all of whose finite scores
    are candidates: its -inf tokens are the same set in both arrays.)"""
    out = np.full(cand_val.shape[:-1] + (V,), -np.inf, np.float32)
    finite = np.isfinite(cand_val)
    lead = np.nonzero(finite)[:-1]
    out[lead + (cand_idx[finite],)] = cand_val[finite]
    return out


def two_stage(lp, nb):
    """(B, nb, V) processed log-probs -> what the two kernels' formulation keeps of them."""
    cv, ci = row_candidates(lp, 2 * nb)
    return scatter_candidates(cv, ci, lp.shape[-1])


# ---- the search state, one step at a time ------------------------------------------------------------------------
STATE_KEYS = ("running", "run_scores", "sequences", "beam_scores", "fin", "fin_len", "unsat", "cur_len")


class BeamRef:
    """``beam_step`` with the slot table ``kw_beam_select`` keeps beside it -- not the oracle's ``beam_indices``:
    ``bp_new[j] = bp_old[parent(j)][:L] + [r0 + j]``, ``bp[r][p] = r`` before the first step -- and event counters."""

    def __init__(self, prompt, nb, max_length, *, eos, fill, length_penalty=1.0, early_stopping=False):
        prompt = np.asarray(prompt, np.int64)
        self.B, self.P = prompt.shape
        self.nb, self.max_length = nb, max_length
        self.kw = dict(eos=eos, max_length=max_length, begin_index=self.P, length_penalty=length_penalty,
                       early_stopping=early_stopping)
        self.st = og.beam_init(prompt, nb, max_length, fill)
        self.bp = np.tile(np.arange(self.B * nb, dtype=np.int32)[:, None], (1, max_length))
        self.go = True
        self.events = collections.Counter()
        self.info = None

    @classmethod
    def from_state(cls, st, bp, nb, max_length, begin_index, **kw):
        """Continue from a hand-built state (``mid_state``)."""
        ref = cls(np.zeros((st["running"].shape[0], begin_index), np.int64), nb, max_length, **kw)
        ref.st, ref.bp = st, np.array(bp, np.int32)
        return ref

    def history(self):
        """The running rows' tokens so far, (B nb, cur_len)."""
        return self.st["running"].reshape(self.B * self.nb, -1)[:, : self.st["cur_len"]]

    def step(self, lp):
        prev, nb = self.st, self.nb
        lp = np.asarray(lp, np.float32).reshape(self.B, nb, -1)
        st, info = og.beam_step(lp, prev, **self.kw)
        L = prev["cur_len"]
        parent = np.take_along_axis(info["parent"], info["run_pick"], axis=1)  # (B, nb) beam each new row continues
        rows = (parent + np.arange(self.B)[:, None] * nb).reshape(-1)
        bp = self.bp.copy()
        bp[:, :L] = self.bp[rows, :L]
        bp[:, L] = np.arange(self.B * nb)
        self._count(lp, prev, st, info)
        self.st, self.bp, self.go, self.info = st, bp, info["go"], info
        return info

    def _count(self, lp, prev, st, info):
        ev, nb, es = self.events, self.nb, self.kw["early_stopping"]
        ev["steps"] += 1
        eos_top = (info["tok"][:, :nb] == self.kw["eos"]) & np.isfinite(info["topk_lp"][:, :nb])
        ev["finish_in_top_nb"] += int(eos_top.sum())
        kept = info["topk_lp"]
        ev["tie_among_kept"] += int((np.isfinite(kept[:, 1:]) & (kept[:, 1:] == kept[:, :-1])).any())
        for b in range(self.B):
            gone = [j for j in range(nb) if prev["fin"][b, j] and j not in info["fin_pick"][b]]
            ev["finished_displaced"] += len(gone)
        stopped = prev["unsat"][:, 0] & ~st["unsat"][:, 0]
        ev["item_stops_improving_alone"] += int(stopped.any() and st["unsat"].any())
        ev["row_short_of_candidates"] += int((np.isfinite(lp).sum(-1) < 2 * nb).any())
        if not info["go"]:
            clauses = {"stop_no_improve": not st["unsat"].any(), "stop_all_fin": bool(st["fin"].all() and es is True),
                       "stop_all_hit": bool(info["hits"].all())}
            for k, v in clauses.items():
                ev[k] += int(v)
                ev[k + "_alone"] += int(v and sum(clauses.values()) == 1)


def closed_loop(table, prompt, nb, max_length, gen, return_timestamps, *, length_penalty=1.0, early_stopping=False,
                selection=None):
    """Run the toy model under ``BeamRef`` until the loop condition fails; ``selection`` maps the processed
    log-probs (B, nb, V) of a step to the ones the step sees (``two_stage``, or None for the reference's own).
    Returns the BeamRef and the list of per-step states."""
    ref = BeamRef(prompt, nb, max_length, eos=gen["eos_token_id"], fill=gen["pad_token_id"],
                  length_penalty=length_penalty, early_stopping=early_stopping)
    trace = []
    while ref.go:
        hist = ref.history()
        lp = processed_logprobs(hist, table[hist[:, -1]], gen, ref.P, return_timestamps)
        lp = lp.reshape(ref.B, nb, -1)
        ref.step(selection(lp, nb) if selection else lp)
        trace.append(ref.st)
    return ref, trace


def mid_state(rng, B, nb, V, P, L, max_length, fill, *, n_dead=0, n_fin=None, unsat=None):
    """A hand-built state in the middle of a search -> (state, slot table).  Histories are random and distinct,
    running scores sit on a 0.5 grid in descending order (ties between beams), the last ``n_dead`` rows of every
    item at -1e9; item b holds ``n_fin[b]`` finished sequences (random when None) with descending grid scores;
    ``unsat``: per item (all True when None).  The slot table names a random row of the same item per position."""
    st = og.beam_init(rng.integers(0, 8, (B, P)), nb, max_length, fill)
    st["running"][:, :, P:L] = rng.integers(0, V, (B, nb, L - P))
    st["cur_len"] = L
    sc = (-np.sort(rng.integers(0, 6, (B, nb)), axis=1) * 0.5).astype(np.float32)
    if n_dead:
        sc[:, nb - n_dead:] = NEG
    st["run_scores"] = sc
    n_fin = rng.integers(0, nb + 1, B) if n_fin is None else np.broadcast_to(n_fin, (B,))
    for b in range(B):
        n = int(n_fin[b])
        st["fin"][b, :n] = True
        st["beam_scores"][b, :n] = (-np.sort(rng.integers(2, 12, n)) * 0.25).astype(np.float32)
        for j in range(n):
            ln = int(rng.integers(1, L - P + 1)) if L > P else 0
            st["fin_len"][b, j] = ln
            st["sequences"][b, j, P:P + ln] = rng.integers(0, V, ln)
    if unsat is not None:
        st["unsat"] = np.asarray(unsat, bool).reshape(B, 1)
    bp = np.tile(np.arange(B * nb, dtype=np.int32)[:, None], (1, max_length))
    bp[:, :L] = (rng.integers(0, nb, (B * nb, L)) + (np.arange(B * nb) // nb * nb)[:, None]).astype(np.int32)
    return st, bp


# The closed-loop cases of the GPU test: (V, nb, return_timestamps, early_stopping, length_penalty, seed, new
# tokens).  tests/test_beam_cpu.py asserts that their union holds every event counted above.
CLOSED_LOOP_PROMPT = np.array([[2, 4, 7], [2, 4, 9], [2, 4, 12]])
CLOSED_LOOP_CASES = [
    (V, nb, rt, es, (1.0, 0.5, 2.0, 0.0, -0.5)[i % 5], i, 12 + i % 5)
    for i, (V, nb, rt, es) in enumerate((V, nb, rt, es) for V in (64, 200) for nb in (2, 5, 8)
                                        for rt in (False, True) for es in (False, True, "never"))]


def case_setup(case):
    """-> (gen, table, max_length, keyword arguments of the search) of a closed-loop case."""
    V, nb, rt, es, lpn, seed, n_new = case
    gen = toy_gen(V, nb, mostly_suppressed=(seed % 3 == 2))
    table = grid_table(V, seed, eos_boost=(seed % 3) * 1.5, ts_boost=1.0 if rt else 0.0)
    return gen, table, CLOSED_LOOP_PROMPT.shape[1] + n_new, dict(length_penalty=lpn, early_stopping=es)


def run_case(case):
    gen, table, max_length, kw = case_setup(case)
    return closed_loop(table, CLOSED_LOOP_PROMPT, case[1], max_length, gen, case[2], **kw)


def same_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in STATE_KEYS)
