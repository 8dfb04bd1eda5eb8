"""Token-level timestamps on the MI355X: the four kernels of csrc/token_ts.hip against the numpy restatement
(tests/_token_ts_ref.py, itself pinned to transformers on the CPU) and generate(return_token_timestamps=True) end to
end against the HF fixture tests/golden/token_ts_tiny.npz.

Accuracy bounds (kw_align_reduce, kw_align_weights): the kernel's error against a float64 reference may be at most
4x the error of torch's own float32 CPU path against that reference on the same inputs, floor 1e-6 -- both errors
taken as the largest over one case (all its rows).  The factor covers a different reduction order over <= 444 terms.
"""
import json

import numpy as np
import pytest
import torch

import _token_ts_ref as R
from _token_ts_ref import dtw_inputs

pytestmark = pytest.mark.gpu

from kwhisper.config import TINY, generation_constants  # noqa: E402
from kwhisper.synthetic import synthetic_state_dict  # noqa: E402

from _util import oracle_features  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---- kw_dtw --------------------------------------------------------------------------------------------------
# (T, [S' per row]) per launch: the issue's shapes, then rows of different S' in one launch
DTW_LAUNCHES = [(1, [4, 1500]), (3, [2]), (7, [96]), (63, [1500]), (444, [1500]), (7, [96, 4, 1500, 33, 1])]


@pytest.mark.parametrize("kind", ["random", "constant", "integer", "nan"])
def test_dtw_equals_restatement(kind):
    from kwhisper import ops

    for T, widths in DTW_LAUNCHES:
        S = max(widths)
        m = np.full((len(widths), T, S), np.nan, np.float32)  # columns past a row's S' must never be read
        for b, F in enumerate(widths):
            m[b, :, :F] = dtw_inputs(kind, T, F, seed=b)
        frames = torch.tensor(widths, dtype=torch.int32, device="cuda")
        got = ops.dtw(torch.from_numpy(m).cuda(), frames).cpu().numpy()
        for b, F in enumerate(widths):
            np.testing.assert_array_equal(got[b], R.dtw_frames(m[b, :, :F]), err_msg=f"{kind} T={T} S'={F}")
    # frames=None: every row uses all S columns
    m = dtw_inputs(kind, 5, 40)
    got = ops.dtw(torch.from_numpy(m[None]).cuda()).cpu().numpy()[0]
    np.testing.assert_array_equal(got, R.dtw_frames(m))


# ---- kw_align_reduce -----------------------------------------------------------------------------------------
REDUCE_FRAMES = [3, 4, 7, 96, 1500]


def _torch_matrix(w, F, width=7):
    """transformers' float32 arithmetic for one row (generation_whisper.py:354-363)."""
    from transformers.models.whisper.generation_whisper import _median_filter

    x = torch.from_numpy(w)[..., :F]
    std = torch.std(x, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(x, dim=-2, keepdim=True)
    return (-_median_filter((x - mean) / std, width).mean(dim=0)).numpy()


@pytest.mark.parametrize("heads", [1, 6])
@pytest.mark.parametrize("steps", [1, 2, 23])
def test_align_reduce_against_float64(heads, steps):
    from kwhisper import ops

    rng = np.random.default_rng(100 * heads + steps)
    B, S = len(REDUCE_FRAMES), 1500
    # attention-like weights: positive, a few orders of magnitude apart
    w = np.exp(3 * rng.standard_normal((heads, B, steps, S))).astype(np.float32)
    w /= w.sum(-1, keepdims=True)
    frames = torch.tensor(REDUCE_FRAMES, dtype=torch.int32, device="cuda")
    out = torch.full((B, steps, S), 7.0, device="cuda")
    ops.align_reduce(torch.from_numpy(w).cuda(), heads, B, steps, S, frames, 7, out)
    got = out.cpu().numpy()
    err_gpu = err_torch = 0.0
    for b, F in enumerate(REDUCE_FRAMES):
        ref = R.dtw_matrix(w[:, b].astype(np.float64), F)
        t32 = _torch_matrix(w[:, b], F)
        g = got[b, :, :F]
        assert (got[b, :, F:] == 0).all()
        if steps == 1:  # std 0: 0 / 0 = NaN everywhere, as torch gives
            assert np.isnan(ref).all() and np.isnan(t32).all() and np.isnan(g).all()
            continue
        assert not np.isnan(g).any()
        err_gpu = max(err_gpu, float(np.abs(g - ref).max()))
        err_torch = max(err_torch, float(np.abs(t32 - ref).max()))
    print(f"align_reduce heads={heads} steps={steps}: err gpu {err_gpu:.3e} torch fp32 {err_torch:.3e}")
    assert err_gpu <= max(4 * err_torch, 1e-6)


def test_align_reduce_chunks_of_pairs():
    """Pairs fed in two chunks (first / last) give the one-launch result up to the order of the head sum."""
    from kwhisper import ops

    rng = np.random.default_rng(5)
    A, B, T, S = 6, 2, 9, 200
    w = torch.from_numpy(rng.random((A, B, T, S)).astype(np.float32)).cuda()
    one = torch.empty((B, T, S), device="cuda")
    two = torch.empty((B, T, S), device="cuda")
    ops.align_reduce(w, A, B, T, S, None, 7, one)
    ops.align_reduce(w[:4].contiguous(), 4, B, T, S, None, 7, two, a_total=A, first=True, last=False)
    ops.align_reduce(w[4:].contiguous(), 2, B, T, S, None, 7, two, a_total=A, first=False, last=True)
    ref = np.stack([R.dtw_matrix(w[:, b].cpu().numpy().astype(np.float64)) for b in range(B)])
    assert np.abs(one.cpu().numpy() - ref).max() < 1e-5 and np.abs(two.cpu().numpy() - ref).max() < 1e-5
    assert torch.equal(one, two)  # the same sequential sum over the pairs


# ---- kw_align_weights ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("steps", [1, 5, 130])
def test_align_weights_against_float64(dtype, steps):
    from kwhisper import ops

    rng = np.random.default_rng(steps)
    B, H, S, t_log = 2, 6, 1500, 130
    pairs = [(0, 0), (0, 5)]
    q = torch.from_numpy((0.6 * rng.standard_normal((len(pairs), B, t_log, 64))).astype(np.float32)).to(dtype)
    k = torch.from_numpy(rng.standard_normal((1, B, H, S, 64)).astype(np.float32)).to(dtype)
    out = torch.full((len(pairs), B, steps, S), -1.0, device="cuda")
    ops.align_weights(q.cuda(), k.cuda(), pairs, steps, out)
    got = out.cpu().numpy().astype(np.float64)
    err_gpu = err_torch = 0.0
    for a, (_, h) in enumerate(pairs):
        for b in range(B):
            q32, k32 = q[a, b, :steps].float(), k[0, b, h].float()  # the rounded inputs
            ref = torch.softmax(q32.double() @ k32.double().T, -1).numpy()
            t32 = torch.softmax(q32 @ k32.T, -1).numpy().astype(np.float64)
            scale = ref.max(-1)
            err_gpu = max(err_gpu, float((np.abs(got[a, b] - ref).max(-1) / scale).max()))
            err_torch = max(err_torch, float((np.abs(t32 - ref).max(-1) / scale).max()))
    print(f"align_weights {dtype} steps={steps}: err gpu {err_gpu:.3e} torch fp32 {err_torch:.3e}")
    assert err_gpu <= max(4 * err_torch, 1e-6)


# ---- kw_align_capture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_align_capture_graph_replay_bitwise(dtype):
    """A captured step (new queries, capture, position + 1) replayed 5 times: the log holds exactly the queries'
    head slices of the steps whose position lies in the log's range, and nothing else is written."""
    from kwhisper import ops
    from kwhisper.decode import capture_graph

    B, d, t_log, P = 3, 384, 3, 4
    heads, slots = [2, 5], [1, 0]
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.standard_normal((6, B, d)).astype(np.float32)).to(dtype).cuda()
    q = torch.zeros((B, d), dtype=dtype, device="cuda")
    step = torch.zeros((1,), dtype=torch.int64, device="cuda")
    cur_len = torch.full((1,), P, dtype=torch.int32, device="cuda")  # first replay: t = -1, outside the log
    log = torch.full((2, B, t_log, 64), 9.0, dtype=dtype, device="cuda")
    plan = ops.AlignCapturePlan(q, heads, slots, cur_len, P, log)

    def one():
        q.copy_(src.index_select(0, step)[0])
        plan()
        step.add_(1)
        cur_len.add_(1)

    g = capture_graph(one, "cuda")
    for _ in range(5):  # t = -1, 0, 1, 2, 3: the first and the last fall outside [0, t_log)
        g.replay()
    torch.cuda.synchronize()
    want = torch.full_like(log, 9.0)
    for t in range(t_log):
        for h, s in zip(heads, slots):
            want[s, :, t] = src[t + 1, :, 64 * h: 64 * h + 64]
    assert torch.equal(log.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


# ---- end to end ----------------------------------------------------------------------------------------------
def _model(dtype, heads):
    from kwhisper.generation import KWhisperForConditionalGeneration

    gen = generation_constants(TINY)
    gen.alignment_heads = [list(map(int, p)) for p in heads]
    m = KWhisperForConditionalGeneration.from_state_dict(TINY, synthetic_state_dict(TINY, 0), dtype=dtype,
                                                         generation_config=gen)
    m.record_alignment = True
    return m


@pytest.fixture(scope="module")
def tiny32(gold):
    return _model(torch.float32, gold("token_ts_tiny")["alignment_heads"])


@pytest.fixture(scope="module")
def tiny16(gold):
    return _model(torch.bfloat16, gold("token_ts_tiny")["alignment_heads"])


@pytest.fixture(scope="module")
def inputs(gold):
    g = gold("token_ts_tiny")
    feats = torch.from_numpy(oracle_features(TINY, g["cases"])).cuda()
    mask = (torch.arange(feats.shape[-1])[None, :] < torch.from_numpy(g["attention_frames"])[:, None]).long()
    return g, feats, mask


def _run(model, feats, mask, kw, flag):
    res = model.generate(feats, attention_mask=mask, language="ja", task="transcribe", return_segments=True,
                         return_token_timestamps=flag, **kw)
    return res, (model.stats["alignment"] if flag else None)


def _check_composition(align):
    """The exported DTW matrix, fed to the restatement, gives exactly the engine's frame indices."""
    for p in align:
        for r in range(len(p["rows"]) if p["T"] else 0):
            F = p["matrix"].shape[2] if p["num_frames"] is None else int(p["num_frames"][r])
            np.testing.assert_array_equal(R.dtw_frames(p["matrix"][r, :, :F]), p["frames"][r])


@pytest.mark.parametrize("mode", ["ts", "nots"])
def test_end_to_end_fp32(inputs, tiny32, mode):
    from kwhisper.generation import _pass_token_timestamps

    g, feats, mask = inputs
    kw = json.loads(str(g[f"{mode}_kw"]))
    model = tiny32
    plain, _ = _run(model, feats, mask, kw, False)
    res, align = _run(model, feats, mask, kw, True)
    assert torch.equal(res["sequences"], plain["sequences"])  # the flag does not change the tokens
    np.testing.assert_array_equal(res["sequences"].cpu().numpy(), g[f"{mode}_sequences"])
    assert len(align) == int(g[f"{mode}_passes"])
    _check_composition(align)
    ts, st = g["tstride"], g["sstride"]
    unstable_diff = unstable = 0
    row_stable = np.ones(len(g["cases"]), bool)
    failures = []
    for i, p in enumerate(align):
        assert p["rows"] == g[f"{mode}_p{i}_rows"].tolist() and p["num_input_ids"] == int(g[f"{mode}_p{i}_P"])
        shape = g[f"{mode}_p{i}_shape"]  # per row: (steps, the reference's crop n // 2, a Python slice bound)
        assert p["T"] == int(shape[0][0])
        assert p["num_frames"].tolist() == [len(range(1500)[: int(n)]) for n in shape[:, 1]]
        # raw weights against the fixture's float64 sample: [A][B][T][S] -> [B][A][::ts][::st]
        w = p["weights"].transpose(1, 0, 2, 3)[:, :, ::ts, ::st].astype(np.float64)
        w64, eps = g[f"{mode}_p{i}_w64"], float(g[f"{mode}_p{i}_eps_ref"])
        err = float((np.abs(w - w64).max(-1) / w64.max(-1)).max())
        print(f"{mode} pass {i}: weights err {err:.3e} vs 8 eps_ref {8 * eps:.3e}")
        if err > 8 * eps:
            failures.append(f"pass {i}: weights err {err:.3e} > {8 * eps:.3e}")
        got = _pass_token_timestamps(p["frames"], p["num_input_ids"], g[f"{mode}_p{i}_ts"].shape[1])
        for r, b in enumerate(p["rows"]):
            same = np.array_equal(got[r], g[f"{mode}_p{i}_ts"][r])
            if g[f"{mode}_p{i}_stable"][r]:
                if not same:
                    failures.append(f"pass {i} row {b} (stable): timestamps differ from HF")
            else:
                row_stable[b] = False
                unstable += 1
                unstable_diff += not same
    print(f"{mode}: {unstable_diff} of {unstable} unstable (pass, row) cases differ from HF (not gated)")
    tts = res["token_timestamps"].cpu().numpy()
    assert tts.dtype == np.float32 and tts.shape == g[f"{mode}_token_timestamps"].shape
    for b in np.nonzero(row_stable)[0]:
        if not np.array_equal(tts[b], g[f"{mode}_token_timestamps"][b]):
            failures.append(f"row {b}: top-level token_timestamps differ from HF")
        seg = np.concatenate([s["token_timestamps"] for s in res["segments"][b]]) if res["segments"][b] else \
            np.zeros(0, np.float32)
        if not np.array_equal(seg, g[f"{mode}_seg_tts_{b}"]):
            failures.append(f"row {b}: segments' token_timestamps differ from HF")
    assert not failures, failures


def test_end_to_end_bf16(inputs, tiny16):
    g, feats, mask = inputs
    model = tiny16
    for mode in ("ts", "nots"):
        kw = json.loads(str(g[f"{mode}_kw"]))
        plain, _ = _run(model, feats, mask, kw, False)
        res, align = _run(model, feats, mask, kw, True)
        assert torch.equal(res["sequences"], plain["sequences"])
        _check_composition(align)
        tts, want = res["token_timestamps"].cpu().numpy(), g[f"{mode}_token_timestamps"]
        n = min(tts.shape[1], want.shape[1])
        d = np.abs(tts[:, :n].astype(np.float64) - want[:, :n])
        print(f"bf16 {mode}: tokens within 0.02 s of HF fp32: {np.mean(d <= 0.02 + 1e-6):.3f}, within 0.1 s: "
              f"{np.mean(d <= 0.1 + 1e-6):.3f} ({d.size} tokens; sequences equal: "
              f"{tts.shape == want.shape and np.array_equal(res['sequences'].cpu().numpy(), g[f'{mode}_sequences'])})")
        assert np.isfinite(tts).all()


def test_dict_output_single_pass(inputs, tiny32):
    """return_dict_in_generate without timestamps: sequences with the prompt and the pass's timestamps (P zeros first)."""
    g, feats, mask = inputs
    model = tiny32
    kw = json.loads(str(g["nots_kw"]))
    res = model.generate(feats, attention_mask=mask, language="ja", task="transcribe", return_dict_in_generate=True,
                         return_token_timestamps=True, **kw)
    np.testing.assert_array_equal(res["sequences"].cpu().numpy(), g["nots_p0_sequences"])
    st = g["nots_p0_stable"]
    np.testing.assert_array_equal(res["token_timestamps"].cpu().numpy()[st], g["nots_p0_ts"][st])


def test_generate_multitask_with_token_timestamps(inputs, tiny32):
    """generate_multitask (one encoder pass shared by the prompts) returns what generate returns per task."""
    g, feats, mask = inputs
    kw = dict(json.loads(str(g["ts_kw"])), attention_mask=mask, return_token_timestamps=True)
    tasks = [("ja", "transcribe"), ("en", "translate")]
    multi = tiny32.generate_multitask(feats, tasks, **kw)
    for (lang, task), got in zip(tasks, multi):
        one = tiny32.generate(feats, language=lang, task=task, **kw)
        assert torch.equal(got["sequences"], one["sequences"])
        assert torch.equal(got["token_timestamps"], one["token_timestamps"])
    np.testing.assert_array_equal(multi[0]["sequences"].cpu().numpy(), g["ts_sequences"])
