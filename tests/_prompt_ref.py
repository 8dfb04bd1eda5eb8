"""A plain restatement of one seek pass's decoder input under ``prompt_ids`` / ``condition_on_prev_tokens``
(transformers 5.15.0 generation_whisper.py ``_prepare_decoder_input_ids`` :1853-1918 and ``_pad_to_max_length``
:126-235), on Python lists, for tests/test_prompt_cpu.py and tests/test_prompt_gpu.py.  It shares no code with
kwhisper.generation.build_pass_input; both are checked against tests/golden/prompt_tiny.npz."""
import json

import numpy as np


def pass_input(init, segments, rows, do_condition, prompt_ids, *, pad, prev_sot, ts_begin, max_target=448,
               all_segments=False):
    """-> (ids: list of rows, key_start: list or None).  ``segments[a]``: audio a's token lists so far."""
    init = [int(t) for t in init]
    if any(do_condition) and len(segments[0]) > 0:
        head = [int(t) for t in prompt_ids] if (prompt_ids is not None and all_segments) else [prev_sot]
        prev = []
        for a in rows:
            if not do_condition[a] or not segments[a]:
                prev.append(list(head))
                continue
            text = []
            for seg in segments[a]:
                seg = [int(t) for t in seg]
                if len(seg) > 2 and seg[-2] >= ts_begin:
                    seg = seg[:-1]
                text += seg
            text = text[-(max_target // 2 - 1):]
            prev.append(head + text)
        width = max(len(p) for p in prev)
        ids = [[pad] * (width - len(p)) + p + init for p in prev]
        key_start = []
        for row in ids:
            n = 0
            while n < len(row) and row[n] == pad:
                n += 1
            key_start.append(n)
        return ids, key_start
    if prompt_ids is not None:
        return [[int(t) for t in prompt_ids] + init for _ in rows], None
    return [list(init) for _ in rows], None


def fixture_case(g, name):
    """One case of prompt_tiny.npz: sequences, segments (start, end, count), passes, and per audio its segments'
    token lists (the sequences cut by the recorded counts)."""
    seqs = g[f"{name}_sequences"]
    segs = json.loads(str(g[f"{name}_segments"]))
    passes = json.loads(str(g[f"{name}_passes"]))
    toks = []
    for b, row in enumerate(segs):
        out, at = [], 0
        for _, _, n in row:
            out.append([int(t) for t in seqs[b, at: at + n]])
            at += n
        toks.append(out)
    return seqs, segs, passes, toks


CASE_KWARGS = {  # tools/make_prompt_fixture.py's cases (prompt_ids: the fixture's "prompt_ids")
    "a": dict(condition_on_prev_tokens=True),
    "b": dict(prompt_ids=True),
    "c": dict(prompt_ids=True, prompt_condition_type="all-segments", condition_on_prev_tokens=True),
    "d": dict(prompt_ids=True, prompt_condition_type="first-segment", condition_on_prev_tokens=True),
    "f": dict(condition_on_prev_tokens=True),
}


def segments_before(case, p, toks, prompt_ids, prev_sot):
    """Per audio, the segments ``_prepare_decoder_input_ids`` saw at pass ``p``: the first ``nsegs`` of its final
    segments -- with "first-segment" behind the seeded prompt text, which the result no longer carries."""
    kw = CASE_KWARGS.get(case, {})
    seeded = bool(kw.get("prompt_ids")) and kw.get("prompt_condition_type", "first-segment") == "first-segment"
    out = []
    for a, n in enumerate(p["nsegs"]):
        if seeded:
            pt = [int(t) for t in prompt_ids]
            seed = pt[1:] if pt[0] == prev_sot else pt
            out.append([seed] + toks[a][: n - 1])
        else:
            out.append(toks[a][:n])
    return out


def key_start_of(mask):
    return None if mask is None else [int(len(r) - np.count_nonzero(r)) for r in mask]
