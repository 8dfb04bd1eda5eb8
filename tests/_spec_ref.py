"""A numpy restatement of speculative decoding's accept step (kw_spec_accept, include/kwhisper.h) on top of the pinned
processors ``oracle.generate.process_logits``, and of the round loop around it.  The tests compare the kernel and the
paired session with this; nothing here is used by the engine."""
import numpy as np

from oracle.generate import process_logits


def greedy_token(history, logits_row, gd, begin_index, rt):
    """The token one greedy step chooses after ``history`` (1-D, prompt included): the processed arg-max, first index
    on ties (np.argmax)."""
    s = process_logits(np.asarray(history, np.int64)[None], np.asarray(logits_row, np.float32)[None], gd, begin_index, rt)
    return int(s[0].argmax())


def position_tokens(ids, L, K, logits, gd, begin_index, rt, max_length):
    """t_j for j = 0 .. K: the greedy token at length L + j with the drafts ids[L, L + j) in place (None at or beyond
    ``max_length``)."""
    return [greedy_token(ids[: L + j], logits[j], gd, begin_index, rt) if L + j < max_length else None
            for j in range(K + 1)]


def accept(ids, L, K, tokens, gd, max_length):
    """The accept walk over the per-position tokens.  ``ids``: the row (1-D, drafts at [L, L + K)); returns a dict with
    the new row, the new length, the number of accepted drafts and whether the row finished."""
    ids = np.asarray(ids, np.int64).copy()
    eos, pad = gd["eos_token_id"], gd["pad_token_id"]
    n, new_len, done = 0, L, False
    for q in range(K + 1):
        p = L + q
        if p >= max_length:
            done = True
            break
        tok = tokens[q]
        match = q < K and ids[p] == tok
        if not match:
            ids[p] = tok
        new_len = p + 1
        n += int(match)
        if tok == eos or new_len >= max_length:
            done = True
            break
        if not match:
            break
    if done:
        ids[new_len: min(L + K + 1, max_length)] = pad
    return dict(ids=ids, new_len=new_len, n=n, done=done)


def assisted_decode(main_logits, draft_logits, prompt, K, gd, rt, max_length, t_max=448):
    """The whole paired loop on two logits functions ``f(history) -> [V]``: the first token from the main model, rounds
    of K drafts + accept while a whole round fits (L + K + 1 <= max_length and L + 2K + 1 <= t_max), plain main steps
    for the rest.  Returns (ids with the prompt, stats)."""
    P = len(prompt)
    eos = gd["eos_token_id"]
    ids = np.zeros(max(max_length, t_max) + 1, np.int64)
    ids[:P] = prompt
    stats = dict(rounds=0, drafted=0, accepted=0, steps=0)
    ids[P] = greedy_token(ids[:P], main_logits(ids[:P]), gd, P, rt)
    L = P + 1
    done = ids[P] == eos or L >= max_length
    while not done and L + K + 1 <= max_length and L + 2 * K + 1 <= t_max:
        for j in range(K):  # the assistant: the same processors, its own logits
            ids[L + j] = greedy_token(ids[: L + j], draft_logits(ids[: L + j]), gd, P, rt)
        logits = np.stack([main_logits(ids[: L + j]) for j in range(K + 1)])
        toks = position_tokens(ids, L, K, logits, gd, P, rt, max_length)
        r = accept(ids, L, K, toks, gd, max_length)
        ids, L, done = r["ids"], r["new_len"], r["done"]
        stats["rounds"] += 1
        stats["drafted"] += K
        stats["accepted"] += r["n"]
    while not done:
        ids[L] = greedy_token(ids[:L], main_logits(ids[:L]), gd, P, rt)
        L += 1
        stats["steps"] += 1
        done = ids[L - 1] == eos or L >= max_length
    return ids[:L].copy(), stats


def plain_greedy(main_logits, prompt, gd, rt, max_length):
    P = len(prompt)
    ids = list(prompt)
    while True:
        ids.append(greedy_token(ids, main_logits(np.asarray(ids)), gd, P, rt))
        if ids[-1] == gd["eos_token_id"] or len(ids) >= max_length:
            return np.asarray(ids, np.int64)
