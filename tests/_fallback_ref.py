"""Numpy restatement of the decoding fallback (tests only): the statistics and the decision of Whisper's
``generate_with_fallback`` (transformers 5.15.0, models/whisper/generation_whisper.py:970-1116, 1243-1287, 1949-1974),
and the device sampler's noise: Philox4x32-10, the uniform-to-Gumbel map and the perturbed argmax of
``kw_sample_step`` (include/kwhisper.h).  Written from the algorithms' definitions, not from the kernel."""
import zlib

import numpy as np

# ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) -----------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: (..., 4) and key: (..., 2) unsigned 32-bit words (broadcast against each other) -> (..., 4) uint32.
    One round: (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)); the key is
    bumped by (W0, W1) between rounds; ten rounds."""
    c = np.asarray(counter).astype(np.uint64) & _M32
    k = np.asarray(key).astype(np.uint64) & _M32
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for r in range(10):
        p0 = np.uint64(PHILOX_M0) * c0
        p1 = np.uint64(PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & _M32, \
            p0 & _M32
        k0 = (k0 + np.uint64(PHILOX_W0)) & _M32
        k1 = (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def sample_draws(seed, attempt, row, L, V):
    """The 32-bit draw of every token v < V of one (row, position): counter (v >> 2, L, row, attempt), key = the
    halves of the 64-bit seed, output word v & 3."""
    n4 = (V + 3) // 4
    ctr = np.zeros((n4, 4), np.uint64)
    ctr[:, 0] = np.arange(n4)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = L, row, attempt
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    out = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
    return out.reshape(-1)[:V]


UNIFORM_BITS = 20  # the top bits of a draw the uniform takes


def uniform_index(draw):
    return np.asarray(draw, np.uint32) >> np.uint32(32 - UNIFORM_BITS)


def uniform_of_index(k):
    """u = (k + 0.5) * 2^-20, in [2^-21, 1 - 2^-21]."""
    return (np.asarray(k, np.float64) + 0.5) * 2.0 ** -UNIFORM_BITS


def gumbel_of_index(k):
    """g = -log(-log(u)) in float64: within [-2.679, 14.557] for every index."""
    return -np.log(-np.log(uniform_of_index(k)))


def index_of_gumbel(g):
    """The inverse map, from a stored (float32) g back to the 20-bit index: u = exp(-exp(-g))."""
    u = np.exp(-np.exp(-np.asarray(g, np.float64)))
    return np.rint(u * 2.0 ** UNIFORM_BITS - 0.5).astype(np.int64)


def perturbed_argmax(scores, inv_t, noise):
    """argmax over the finite processed scores of s * inv_T + g in float64 (first index on ties), and the gap between
    the best and the second best value.  inv_t == 0: the plain argmax."""
    s = np.asarray(scores, np.float64)
    p = s * inv_t + np.asarray(noise, np.float64) if inv_t != 0 else s.copy()
    p[~np.isfinite(s)] = -np.inf
    tok = int(np.argmax(p))
    rest = np.delete(p, tok)
    gap = p[tok] - rest.max() if rest.size else np.inf
    return tok, float(gap)


# ---- statistics ------------------------------------------------------------------------------------------------
def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def strip_padding(tokens, pad, eos):
    """The row's generated tokens as ``_need_fallback`` sees them (:1063-1071): the padding removed, the EOS kept."""
    tokens = np.asarray(tokens)
    if tokens.size and tokens[-1] == pad:
        n = int((tokens == pad).sum())
        if pad == eos:
            n -= 1
        if n != 0:
            tokens = tokens[:-n]
    return tokens


def avg_logprob(scores, tokens, temperature=0.0):
    """``_retrieve_avg_logprobs`` (:1958-1974) for one row: ``scores`` (T, V) the recorded scores of every step (the
    processed scores, divided by the temperature when sampling), ``tokens`` the row's tokens from ``strip_padding``
    (the first EOS included).  The scores are cut to the tokens' length, multiplied by the temperature when it is
    above 0 (which undoes the warp), log-softmaxed and gathered at the tokens; the mean over all of them."""
    scores = np.asarray(scores, np.float64)
    tokens = np.asarray(tokens)
    if scores.shape[0] > tokens.shape[0]:
        scores = scores[: tokens.shape[0]]
    else:
        tokens = tokens[-scores.shape[0]:]
    rescale = temperature if temperature > 0.0 else 1
    lp = log_softmax64(scores * rescale)
    return float(lp[np.arange(len(tokens)), tokens].sum() / len(tokens))


def compression_ratio(tokens, vocab_size):
    """``_retrieve_compression_ratio`` (:1949-1955)."""
    length = int(np.log2(vocab_size) / 8) + 1
    tb = b"".join(int(t).to_bytes(length, "little") for t in np.asarray(tokens).tolist())
    return len(tb) / len(zlib.compress(tb))


def need_fallback(*, compression, avg_lp, no_speech_prob, compression_ratio_threshold, logprob_threshold,
                  no_speech_threshold):
    """``_need_fallback`` (:1243-1287) on its numbers: (needs_fallback, should_skip).  A skip cancels a fallback."""
    needs_fallback = should_skip = False
    if compression_ratio_threshold is not None and compression > compression_ratio_threshold:
        needs_fallback = True
    if logprob_threshold is not None and avg_lp < logprob_threshold:
        needs_fallback = True
    if no_speech_threshold is not None:
        if avg_lp < logprob_threshold and no_speech_prob > no_speech_threshold:
            needs_fallback = False
            should_skip = True
    return needs_fallback, should_skip


def attempt_loop(n_rows, temperatures, decide):
    """The row bookkeeping of ``generate_with_fallback`` (:1001-1116): ``decide(attempt, temperature, rows)`` returns
    (needs_fallback, should_skip) per row of ``rows`` (original indices).  Returns (accepted attempt per row, skipped
    flag per row, the rows decoded at every attempt)."""
    accepted = [None] * n_rows
    skipped = [False] * n_rows
    rows = list(range(n_rows))
    decoded = []
    for ai, t in enumerate(temperatures):
        decoded.append(list(rows))
        nxt = []
        for r, (nf, sk) in zip(rows, decide(ai, t, rows)):
            last = ai == len(temperatures) - 1
            accepted[r] = ai
            skipped[r] = bool(sk)
            if nf and not last:
                nxt.append(r)
        rows = nxt
        if not rows:
            break
    return accepted, skipped, decoded
