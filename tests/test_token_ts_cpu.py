"""Token-level timestamps, the parts that need no GPU: the numpy restatement (tests/_token_ts_ref.py) is pinned to
transformers' own functions and to the HF fixture, and generate()'s host logic (errors, per-pass assembly) is
checked against the fixture's per-pass times."""
import types

import numpy as np
import pytest

import _token_ts_ref as R
from _token_ts_ref import dtw_inputs


def _hf_dtw_frames(matrix):
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    with np.errstate(invalid="ignore"):
        text, time = gw._dynamic_time_warping(matrix.astype(np.float64))
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    return time[jumps].astype(np.int32)


@pytest.mark.parametrize("kind", ["random", "constant", "integer", "nan"])
@pytest.mark.parametrize("shape", [(1, 4), (3, 2), (7, 33), (12, 50)])
def test_restated_dtw_equals_transformers(kind, shape):
    m = dtw_inputs(kind, *shape)
    np.testing.assert_array_equal(R.dtw_frames(m), _hf_dtw_frames(m))


def test_restated_median_filter_equals_transformers():
    torch = pytest.importorskip("torch")
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    rng = np.random.default_rng(3)
    for frames in (1, 3, 4, 7, 40):
        x = rng.standard_normal((2, 5, frames)).astype(np.float32)
        x[0, 1, frames // 2] = np.nan
        want = gw._median_filter(torch.from_numpy(x), 7).numpy()
        np.testing.assert_array_equal(R.median_filter(x, 7), want)


def test_restatement_reproduces_the_fixture_row(gold):
    """The full-weights case (B = 1, 2 heads, 11 steps): weights -> matrix -> DTW -> times equals HF exactly."""
    g = gold("token_ts_tiny")
    w = g["pin_weights"]
    assert w.shape[0] == 2 and w.shape[1] <= 12
    frames = R.dtw_frames(R.dtw_matrix(w.astype(np.float64), int(g["pin_num_frames"]) // 2))
    np.testing.assert_array_equal(R.pass_timestamps(frames, int(g["pin_P"])), g["pin_ts"])
    # and torch's own float32 arithmetic, restated in float32, lands on the same path
    frames32 = R.dtw_frames(R.dtw_matrix(w, int(g["pin_num_frames"]) // 2))
    np.testing.assert_array_equal(frames32, frames)


# ---- host logic ------------------------------------------------------------------------------------------
def _host_model(alignment_heads=None):
    """generate()'s argument checks run before anything touches the device: a model over a stub engine."""
    from kwhisper.config import TINY, generation_constants
    from kwhisper.generation import KWhisperForConditionalGeneration

    gen = generation_constants(TINY)
    gen.alignment_heads = alignment_heads
    m = object.__new__(KWhisperForConditionalGeneration)
    m.engine = types.SimpleNamespace(shape=TINY, generation_config=gen, device="cpu")
    m.generation_config = gen
    return m


def test_missing_alignment_heads_raises_hf_error():
    import torch

    with pytest.raises(ValueError, match="Model generation config has no `alignment_heads`, token-level timestamps "
                                         "not available"):
        _host_model().generate(torch.zeros(1, 80, 3000), return_token_timestamps=True)


def test_beam_search_with_token_timestamps_is_refused():
    import torch

    with pytest.raises(NotImplementedError, match="num_beams"):
        _host_model([[3, 0]]).generate(torch.zeros(1, 80, 3000), return_token_timestamps=True, num_beams=2)


def test_generation_constants_carry_alignment_heads():
    from kwhisper.config import TINY, generation_constants

    gen = generation_constants(TINY)
    assert gen.alignment_heads is None and TINY.median_filter_width == 7
    gen.alignment_heads = [[2, 2], [3, 0]]
    assert gen.copy().alignment_heads == [[2, 2], [3, 0]] and gen.to_dict()["alignment_heads"] == [[2, 2], [3, 0]]


@pytest.mark.parametrize("mode", ["ts", "nots"])
def test_per_pass_assembly_matches_fixture(gold, mode):
    """Fed the fixture's per-pass frame indices, the host assembly (prompt zeros, duplicated last time, time_offset,
    segment slices, padding) gives HF's segments' and top-level token timestamps exactly."""
    from kwhisper.config import TINY, generation_constants
    from kwhisper.generation import (_pad_token_timestamps, _pass_token_timestamps, _retrieve_segment,
                                     _strip_pass_row)

    g = gold("token_ts_tiny")
    gen = generation_constants(TINY)
    B = len(g["cases"])
    seek, max_frames = np.zeros(B, np.int64), np.full(B, 3000)
    segments = [[] for _ in range(B)]
    for i in range(int(g[f"{mode}_passes"])):
        rows, P, ids, ts = g[f"{mode}_p{i}_rows"], int(g[f"{mode}_p{i}_P"]), g[f"{mode}_p{i}_sequences"], g[f"{mode}_p{i}_ts"]
        # back to what the device hands over (frame indices), then through the engine's own formatting
        T = ids.shape[1] - P - 1
        frames = np.rint(ts[:, P: P + T].astype(np.float64) / 0.02).astype(np.int32)
        pass_ts = _pass_token_timestamps(frames, P, ids.shape[1])
        np.testing.assert_array_equal(pass_ts, ts)
        time_offset = seek.astype(np.float64) * 0.02 / 2
        seek_num = np.minimum(max_frames - seek, 3000)
        for r, p in enumerate(rows):
            seq = _strip_pass_row(ids[r, P:], gen.pad_token_id, gen.eos_token_id)
            segs, off = _retrieve_segment(seq, gen.timestamp_begin, int(seek_num[p]), float(time_offset[p]),
                                          token_ts=(pass_ts[r], ids[r], P))
            seek[p] += off
            segments[p] += segs
    for b in range(B):
        np.testing.assert_array_equal(np.array([len(s["tokens"]) for s in segments[b]]), g[f"{mode}_seg_len_{b}"])
        got = np.concatenate([s["token_timestamps"] for s in segments[b]]) if segments[b] else np.zeros(0, np.float32)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, g[f"{mode}_seg_tts_{b}"])
    want = g[f"{mode}_token_timestamps"]
    np.testing.assert_array_equal(_pad_token_timestamps(segments, want.shape[1]), want)
