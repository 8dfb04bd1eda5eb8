"""numpy restatement of the token-timestamp arithmetic of transformers 5.15.0
(models/whisper/generation_whisper.py: _median_filter :43-61, _dynamic_time_warping :64-115,
_extract_token_timestamps :341-379), the reference the device kernels are held to.

``dtw_matrix`` works in the dtype it is given (float64 for the references of the accuracy tests, float32 to
restate torch's own path); ``dtw_frames`` keeps the reference's float32 cost and its tie rule exactly.
"""
import numpy as np


def median_filter(x: np.ndarray, width: int) -> np.ndarray:
    """Median of ``width`` along the last axis with reflect padding; the input itself when it has <= width // 2
    frames.  NaN sorts last, as in torch.sort."""
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]  # np.sort places NaN last too


def dtw_matrix(weights: np.ndarray, frames: int | None = None, width: int = 7) -> np.ndarray:
    """weights [heads][steps][S] of one row -> the matrix handed to DTW, [steps][frames]: crop, z-score over steps
    (population std), median filter over frames, mean over heads, negate."""
    w = weights if frames is None else weights[..., :frames]
    with np.errstate(invalid="ignore", divide="ignore"):
        std = w.std(axis=-2, keepdims=True)
        mean = w.mean(axis=-2, keepdims=True)
        z = (w - mean) / std
    return -median_filter(z, width).mean(axis=0)


def dtw_frames(matrix: np.ndarray) -> np.ndarray:
    """int32 [steps]: the frame index at which the DTW path first reaches each step (the reference's
    ``time_indices[jumps]``)."""
    T, F = matrix.shape
    cost = np.full((T + 1, F + 1), np.inf, dtype=np.float32)
    trace = np.full((T + 1, F + 1), -1, dtype=np.int8)
    cost[0, 0] = 0
    m64 = matrix.astype(np.float64)
    with np.errstate(invalid="ignore"):
        for j in range(1, F + 1):
            for i in range(1, T + 1):
                c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
                if c0 < c1 and c0 < c2:
                    c, t = c0, 0
                elif c1 < c0 and c1 < c2:
                    c, t = c1, 1
                else:
                    c, t = c2, 2
                cost[i, j] = m64[i - 1, j - 1] + c
                trace[i, j] = t
    trace[0, :] = 2
    trace[:, 0] = 1
    i, j = T, F
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    text = np.array(text)[::-1]
    time = np.array(time)[::-1]
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    return time[jumps].astype(np.int32)


def pass_timestamps(frames_idx: np.ndarray, num_input_ids: int) -> np.ndarray:
    """float32 [num_input_ids + steps + 1]: zeros for the prompt, ``frame * 0.02``, the last time once more."""
    jt = np.asarray(frames_idx, dtype=np.int64) * 0.02
    return np.concatenate([np.zeros(num_input_ids), jt, jt[-1:]]).astype(np.float32)


def dtw_inputs(kind, T, F, seed=0):
    """Test matrices (T, F) for the DTW checks: "random", "constant", "integer" (tie-heavy) or all-NaN."""
    rng = np.random.default_rng(seed + 1000 * T + F)
    if kind == "random":
        return rng.standard_normal((T, F)).astype(np.float32)
    if kind == "constant":
        return np.full((T, F), -0.25, np.float32)
    if kind == "integer":  # small integers: ties on every branch of the rule
        return rng.integers(-2, 3, (T, F)).astype(np.float32)
    return np.full((T, F), np.nan, np.float32)
