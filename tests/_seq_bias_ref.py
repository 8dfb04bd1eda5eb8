"""numpy f32 restatements of GenerationMixin's SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor (tests only;
TF/generation/logits_process.py:1288-1319, 1450-1467), as plain loops: the table (entries grouped by last token, the
length-1 entry first, the others in dict order), the matching against the tail of the history, the ordered f32 sums.
tests/test_seq_bias_cpu.py holds both to transformers' own classes; the GPU tests hold kw_seq_bias_process and
kw_beam_logprobs_proc to these.  Nothing here imports the package: the table below is built on its own and compared to
kwhisper.seq_bias.SeqTable's arrays by the CPU test."""
import numpy as np

import _repeat_ref as RR
from oracle import generate as og

F32 = np.float32


def as_dict(sequence_bias):
    """The dict the processor keeps (:1388-1392): the list form ``[[ids], value]`` becomes ``{tuple(ids): value}``."""
    if isinstance(sequence_bias, list):
        return {tuple(ids): v for ids, v in sequence_bias}
    return dict(sequence_bias)


def bad_words_dict(bad_words_ids, eos_ids=()):
    """NoBadWords' dict (:1454-1466): entries equal to ``[eos]`` dropped, every value -inf."""
    eos = [eos_ids] if isinstance(eos_ids, (int, np.integer)) else list(eos_ids or ())
    return {tuple(w): float("-inf") for w in bad_words_ids if all(list(w) != [e] for e in eos)}


def table(entries):
    """-> list of groups ``(token, [(ids, value), ...])``, ascending by token; inside a group the length-1 entry, then
    the longer ones in dict order."""
    groups = {}
    for ids, v in entries.items():
        groups.setdefault(int(ids[-1]), []).append((tuple(int(t) for t in ids), v))
    out = []
    for tok in sorted(groups):
        g = groups[tok]
        out.append((tok, [e for e in g if len(e[0]) == 1] + [e for e in g if len(e[0]) > 1]))
    return out


def flat_table(entries):
    """The groups as the five arrays of kw_seq_bias_table: tokens, seq_off, values, group_off, group_tok."""
    tokens, seq_off, values, group_off, group_tok = [], [0], [], [0], []
    for tok, g in table(entries):
        group_tok.append(tok)
        for ids, v in g:
            tokens += list(ids)
            seq_off.append(len(tokens))
            values.append(v)
        group_off.append(len(values))
    with np.errstate(over="ignore"):
        return (np.array(tokens, np.int32), np.array(seq_off, np.int32), np.array(values, np.float64).astype(F32),
                np.array(group_off, np.int32), np.array(group_tok, np.int32))


def applies(ids, row):
    """Whether an entry applies to the history ``row``: it fits (:1303), and its first n-1 tokens are the row's last
    n-1 (:1307-1310); a length-1 entry always does."""
    n, L = len(ids), len(row)
    if n > L:
        return False
    return n == 1 or [int(t) for t in row[L - (n - 1):]] == list(ids[:-1])


def row_bias(entries, row):
    """{token: f32 bias} of the groups with an applying entry, and the per-kind firing counts of this row."""
    out = {}
    for tok, g in table(entries):
        b, hit = F32(0.0), False
        for ids, v in g:
            if applies(ids, row):
                with np.errstate(invalid="ignore", over="ignore"):
                    b = F32(b + F32(v))
                hit = True
        if hit:
            out[tok] = b
    return out


def sequence_bias(ids, scores, entries):
    """(R, L) history, (R, V) f32 scores -> scores + bias (:1318).  A token of no group is not touched; a token whose
    group has no applying entry gets the reference's + 0.0."""
    s = np.array(scores, dtype=F32)
    for r, row in enumerate(np.asarray(ids)):
        for tok, _ in table(entries):
            with np.errstate(invalid="ignore"):
                s[r, tok] = s[r, tok] + F32(0.0)
        for tok, b in row_bias(entries, row).items():
            with np.errstate(invalid="ignore"):
                s[r, tok] = F32(scores[r][tok]) + b
    return s


def process(ids, scores, bias=None, bad=None, penalty=1.0, ngram=0):
    """The reference's order (TF/generation/utils.py:1154-1213): SequenceBias, RepetitionPenalty, NoRepeatNGram,
    NoBadWords.  ``bias`` / ``bad``: entry dicts or None."""
    s = np.array(scores, dtype=F32)
    if bias:
        s = sequence_bias(ids, s, bias)
    s = RR.repeat_process(ids, s, penalty, ngram)
    if bad:
        s = sequence_bias(ids, s, bad)
    return s


def same(a, b):
    """Equal as floats, NaNs in the same places (0.0 == -0.0: the reference adds a +0.0 bias to every element)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ---- the beam entry point: the processors on log_softmax(logits), then the Whisper processors --------------------------
def proc_logprobs(hist, logits, bias, bad, penalty, ngram):
    """log_softmax (normaliser in float64) -> bias -> the repetition pair -> bans, not renormalised.  A ban is -inf
    whatever came before (kw_beam_logprobs_proc's bitset), which is the reference's sum unless the score is +inf / NaN."""
    lp = process(hist, og._log_softmax(np.asarray(logits)), bias, None, penalty, ngram)
    if bad:
        for r, row in enumerate(np.asarray(hist)):
            for tok in row_bias(bad, row):
                lp[r, tok] = -np.inf
    return lp


def processed_logprobs_proc(hist, logits, gen, begin_index, return_timestamps, bias, bad, penalty=1.0, ngram=0):
    return og.process_logits(np.asarray(hist), proc_logprobs(hist, logits, bias, bad, penalty, ngram), gen, begin_index,
                             return_timestamps)


def timestamp_margin_proc(hist, logits, gen, begin_index, bias, bad, penalty=1.0, ngram=0):
    """_beam_ref.timestamp_margin on the processed log-probs (as _repeat_ref.timestamp_margin_rep)."""
    ts = gen["no_timestamps_token_id"] + 1
    lp = proc_logprobs(hist, logits, bias, bad, penalty, ngram)
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
