"""``sequence_bias`` / ``bad_words_ids``: the host side (numpy only; no device, no torch).

SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor (TF/generation/logits_process.py:1276-1392, 1450-1481) as
the kernels read them: a processor is flattened into a ``SeqTable`` -- tokens, offsets and values per entry, the
entries grouped by their last token with a stable sort, a group's length-1 entry first and the others in the
processor's (the dict's) order -- so one reader that walks a group forms the reference's f32 sum
(:1294-1318: ``bias = 0; bias += length_1_bias; bias[last] += value`` per applying longer entry, in dict order).
``kw_seq_bias_process`` (csrc/seqbias.hip) and ``kw_beam_logprobs_proc`` (csrc/beam.hip) take the table's arrays.

The argument checks raise the reference's ``ValueError``s, the vocabulary check its vocabulary-size error
(:1324-1334, raised there at the first call; here before any launch).
"""
from __future__ import annotations

import hashlib

import numpy as np

# include/kwhisper.h: KW_SEQ_BIAS_MAX_SEQS entries of at most KW_SEQ_BIAS_MAX_LEN tokens
MAX_SEQS = 4096
MAX_LEN = 32

_INT = (int, np.integer)


def validate_sequence_bias(sequence_bias):
    """``SequenceBiasLogitsProcessor._validate_arguments`` (:1351-1386), message for message."""
    if not isinstance(sequence_bias, dict) and not isinstance(sequence_bias, list) or len(sequence_bias) == 0:
        raise ValueError(
            f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sequence_bias}.")
    if isinstance(sequence_bias, dict) and any(not isinstance(ids, tuple) for ids in sequence_bias):
        raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sequence_bias}.")
    if isinstance(sequence_bias, dict) and any(
            any((not isinstance(t, _INT) or t < 0) for t in ids) or len(ids) == 0 for ids in sequence_bias):
        raise ValueError(
            f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sequence_bias}.")

    def pair_ok(seq):
        return (isinstance(seq[0], list) and all(isinstance(t, _INT) and t > 0 for t in seq[0])
                and isinstance(seq[1], float))

    if isinstance(sequence_bias, list) and any(
            len(seq) == 0 or not pair_ok(seq) for seq in sequence_bias):
        raise ValueError(
            f"Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and float, but is "
            f"{sequence_bias}.")
    if isinstance(sequence_bias, dict) and any(not isinstance(b, float) for b in sequence_bias.values()):
        raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sequence_bias}.")


def validate_bad_words_ids(bad_words_ids):
    """``NoBadWordsLogitsProcessor._validate_arguments`` (:1469-1481)."""
    if not isinstance(bad_words_ids, list) or len(bad_words_ids) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad_words_ids}.")
    if any(not isinstance(w, list) for w in bad_words_ids):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad_words_ids}.")
    if any(any((not isinstance(t, _INT) or t < 0) for t in w) for w in bad_words_ids):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad_words_ids}.")


def sequence_bias_dict(sequence_bias) -> dict:
    """The checked argument as the dict the processor keeps (``_convert_list_arguments_into_dict``, :1388-1392: in the
    list form a later entry of the same tokens replaces an earlier one's value and keeps its place)."""
    validate_sequence_bias(sequence_bias)
    if isinstance(sequence_bias, list):
        return {tuple(int(t) for t in ids): float(b) for ids, b in sequence_bias}
    return {tuple(int(t) for t in ids): float(b) for ids, b in sequence_bias.items()}


def bad_words_dict(bad_words_ids, eos_token_ids) -> dict:
    """The checked argument as the -inf bias dict (:1454-1467): entries equal to ``[eos]`` for an eos id of the
    generation config are dropped first.  A zero-length entry passes the reference's checks and then breaks its call
    (``sequence_ids[-1]``); it is refused here."""
    validate_bad_words_ids(bad_words_ids)
    if any(len(w) == 0 for w in bad_words_ids):
        raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists, but is {bad_words_ids}.")
    if eos_token_ids is None:
        eos = []
    elif isinstance(eos_token_ids, _INT):
        eos = [int(eos_token_ids)]
    else:
        eos = [int(e) for e in eos_token_ids]
    kept = [w for w in bad_words_ids if all(list(w) != [e] for e in eos)]
    return {tuple(int(t) for t in w): float("-inf") for w in kept}


def canonical_sequence_bias(sequence_bias) -> list:
    """One JSON-able form for the dict and the list form of one bias: ``[[ids], value]`` sorted by ids (the sums the
    processor forms are over one token's entries, whose order a sort by ids changes only between entries of different
    length or content -- a plan digest wants one spelling, not an order)."""
    d = sequence_bias_dict(sequence_bias)
    return [[list(k), d[k]] for k in sorted(d)]


class SeqTable:
    """A processor's entries as the arrays of ``kw_seq_bias_table`` (numpy, host).  ``digest`` names the content: a
    captured graph holds the device arrays' addresses, so sessions key their plans and graphs by it."""

    def __init__(self, entries: dict, vocab_size: int | None = None):
        if vocab_size is not None:
            bad = [t for ids in entries for t in ids if t >= vocab_size]
            if bad:  # (:1330-1334)
                raise ValueError(f"The model vocabulary size is {vocab_size}, but the following tokens were being "
                                 f"biased: {bad}")
        seqs = [(tuple(int(t) for t in ids), float(v)) for ids, v in entries.items()]
        if any(len(ids) == 0 or min(ids) < 0 for ids, _ in seqs):
            raise ValueError("a sequence table entry must be a non-empty tuple of non-negative token ids")
        self.max_len = max((len(ids) for ids, _ in seqs), default=0)
        if len(seqs) > MAX_SEQS or self.max_len > MAX_LEN:
            raise NotImplementedError(
                f"sequence_bias / bad_words_ids tables hold at most {MAX_SEQS} sequences of at most {MAX_LEN} tokens on "
                f"the MI355X engine (got {len(seqs)} sequences, the longest of {self.max_len} tokens)")
        # groups by last token (ascending); inside a group the length-1 entry first, the others in dict order: a
        # stable sort on (last token, length > 1)
        order = sorted(range(len(seqs)), key=lambda i: (seqs[i][0][-1], len(seqs[i][0]) > 1))
        seqs = [seqs[i] for i in order]
        self.n_seq = len(seqs)
        self.tokens = np.array([t for ids, _ in seqs for t in ids], dtype=np.int32)
        self.seq_off = np.zeros(self.n_seq + 1, dtype=np.int32)
        self.seq_off[1:] = np.cumsum([len(ids) for ids, _ in seqs])
        with np.errstate(over="ignore"):
            self.values = np.array([v for _, v in seqs], dtype=np.float64).astype(np.float32)  # (torch.tensor(float))
        last = np.array([ids[-1] for ids, _ in seqs], dtype=np.int32)
        starts = np.flatnonzero(np.r_[True, last[1:] != last[:-1]]) if self.n_seq else np.zeros(0, np.int64)
        self.group_tok = last[starts].astype(np.int32)
        self.n_groups = len(starts)
        self.group_off = np.r_[starts, self.n_seq].astype(np.int32)
        h = hashlib.sha256()
        for a in (self.tokens, self.seq_off, self.values, self.group_off):
            h.update(a.tobytes())
            h.update(b"|")
        self.digest = h.hexdigest()[:32]

    def arrays(self):
        """(tokens, seq_off, values, group_off, group_tok), the order the bindings take them in."""
        return self.tokens, self.seq_off, self.values, self.group_off, self.group_tok

    def __len__(self):
        return self.n_seq


def build_tables(sequence_bias, bad_words_ids, eos_token_ids, vocab_size):
    """(sequence_bias table or None, bad_words_ids table or None) of the two arguments (None = not given).  A table
    that ends empty -- every bad word was ``[eos]`` -- is the same as no argument."""
    sb = bw = None
    if sequence_bias is not None:
        sb = SeqTable(sequence_bias_dict(sequence_bias), vocab_size)
    if bad_words_ids is not None:
        bw = SeqTable(bad_words_dict(bad_words_ids, eos_token_ids), vocab_size)
        if len(bw) == 0:
            bw = None
    return sb, bw
