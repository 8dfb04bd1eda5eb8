"""numpy f32 restatements of GenerationMixin's two anti-repetition processors (tests only):
RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor (TF/generation/logits_process.py:406-413,
1121-1139), which lead the processor list (TF/generation/utils.py:1174-1183).  tests/test_repeat_cpu.py holds both to
transformers' own classes bit for bit; the GPU tests hold kw_repeat_process and kw_beam_logprobs_rep to these."""
import numpy as np

from oracle import generate as og

F32 = np.float32


def repetition_penalty(ids, scores, penalty):
    """(R, L) history, (R, V) f32 scores: gather the history tokens' original scores, penalise, scatter.  Ids outside
    [0, V) are skipped (the device never dereferences them; torch would raise)."""
    s = np.array(scores, dtype=F32)
    V, p = s.shape[1], F32(penalty)
    for r, row in enumerate(np.asarray(ids)):
        t = np.unique(row[(row >= 0) & (row < V)])
        g = s[r, t]
        with np.errstate(invalid="ignore"):
            s[r, t] = np.where(g < 0, g * p, g / p)
    return s


def no_repeat_ngram(ids, scores, n):
    """Every window ids[i : i+n] (i + n <= L) whose first n-1 tokens are the row's last n-1 bans its last token."""
    s = np.array(scores, dtype=F32)
    ids = np.asarray(ids)
    L, V = ids.shape[1], s.shape[1]
    if n <= 0 or L < n:
        return s
    for r, row in enumerate(ids):
        tail = row[L - (n - 1):].tolist() if n > 1 else []
        for i in range(L - n + 1):
            t = int(row[i + n - 1])
            if row[i: i + n - 1].tolist() == tail and 0 <= t < V:
                s[r, t] = -np.inf
    return s


def repeat_process(ids, scores, penalty=1.0, ngram=0):
    """Both, in the reference's order; (1.0, 0) returns the scores unchanged."""
    s = np.array(scores, dtype=F32)
    if penalty != 1.0:
        s = repetition_penalty(ids, s, penalty)
    if ngram:
        s = no_repeat_ngram(ids, s, ngram)
    return s


def has_repeated_ngram(row, n):
    """Whether any n-gram occurs twice in ``row`` (the property no_repeat_ngram_size=n rules out)."""
    row = [int(t) for t in row]
    grams = [tuple(row[i: i + n]) for i in range(len(row) - n + 1)]
    return len(grams) != len(set(grams))


def upto_first_eos(row, P, eos):
    """``row`` up to and including its first EOS after the prompt (the tokens the processors acted on)."""
    hit = np.nonzero(np.asarray(row[P:]) == eos)[0]
    return row[: P + int(hit[0]) + 1] if hit.size else row


# ---- the beam entry point: the two processors on log_softmax(logits), then tests/_beam_ref.py's processor step -------
def rep_logprobs(hist, logits, penalty, ngram):
    """log_softmax (normaliser in float64, oracle.generate._log_softmax) -> the two processors, not renormalised
    (TF/generation/utils.py:3380-3381)."""
    return repeat_process(hist, og._log_softmax(np.asarray(logits)), penalty, ngram)


def processed_logprobs_rep(hist, logits, gen, begin_index, return_timestamps, penalty, ngram):
    """_beam_ref.processed_logprobs with the two processors ahead of the Whisper ones."""
    return og.process_logits(np.asarray(hist), rep_logprobs(hist, logits, penalty, ngram), gen, begin_index,
                             return_timestamps)


def timestamp_margin_rep(hist, logits, gen, begin_index, penalty, ngram):
    """_beam_ref.timestamp_margin on the penalised log-probs: per row, logsumexp(timestamps) - max(text) in float64 of
    the scores the earlier rules left (text is banned when positive)."""
    ts = gen["no_timestamps_token_id"] + 1
    lp = rep_logprobs(hist, logits, penalty, ngram)
    post = og.process_logits(np.asarray(hist), lp, gen, begin_index, True)
    no_ts = lp.copy()
    no_ts[:, ts:] = -np.inf
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
