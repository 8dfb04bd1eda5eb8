"""generate(return_token_timestamps=True, num_beams > 1) on the MI355X against transformers' beam search with token
timestamps (tests/golden/beam_ts_tiny.npz, tools/make_fixtures.py --only beam_ts): tokens, the reconstructed
``beam_indices``, the gathered alignment weights and the timestamps.

Bounds: the raw weights may differ from the fixture's float64 sample by at most 8 x eps_ref relative to the row
maximum (eps_ref: torch's own float32 error on that sample; the bound of tests/test_token_ts_gpu.py).  Timestamps are
compared exactly on the (pass, row) cases the fixture marks stable -- those whose timestamps survive a relative
perturbation of 32 eps_ref of every weight.  The bf16 engine is compared, bitwise, with a recomputation from its own
query log; no tolerance against the reference is claimed for it."""
import json

import numpy as np
import pytest
import torch

import _token_ts_ref as R

pytestmark = pytest.mark.gpu

from kwhisper.config import TINY, generation_constants  # noqa: E402
from kwhisper.synthetic import synthetic_state_dict  # noqa: E402

from _util import oracle_features  # noqa: E402

MODES = ["b3", "b3_ts", "b4_lp_es", "b2"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


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
    return _model(torch.float32, gold("beam_ts_tiny")["alignment_heads"])


@pytest.fixture(scope="module")
def tiny16(gold):
    return _model(torch.bfloat16, gold("beam_ts_tiny")["alignment_heads"])


@pytest.fixture(scope="module")
def inputs(gold):
    g = gold("beam_ts_tiny")
    assert g["modes"].tolist() == MODES
    feats = torch.from_numpy(oracle_features(TINY, g["cases"])).cuda()
    mask = (torch.arange(feats.shape[-1])[None, :] < torch.from_numpy(g["attention_frames"])[:, None]).long()
    return g, feats, mask


def _run(model, g, feats, mask, mode, flag=True):
    gen = model.generation_config.copy()
    if int(g[f"{mode}_eos"]) >= 0:
        gen.eos_token_id = int(g[f"{mode}_eos"])
    kw = json.loads(str(g[f"{mode}_kw"]))
    res = model.generate(feats, generation_config=gen, attention_mask=mask, language="ja", task="transcribe",
                         return_segments=True, return_token_timestamps=flag, **kw)
    return res, (model.stats["alignment"] if flag else None), kw


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_fp32(inputs, tiny32, mode):
    from kwhisper.generation import _pass_token_timestamps

    g, feats, mask = inputs
    res, align, kw = _run(tiny32, g, feats, mask, mode)
    np.testing.assert_array_equal(res["sequences"].cpu().numpy(), g[f"{mode}_sequences"])
    assert len(align) == int(g[f"{mode}_passes"])
    ts, st = int(g["tstride"]), int(g["sstride"])
    failures = []
    compared = cases = 0
    row_stable = np.ones(len(g["cases"]), bool)
    for i, p in enumerate(align):
        assert p["rows"] == g[f"{mode}_p{i}_rows"].tolist() and p["num_input_ids"] == int(g[f"{mode}_p{i}_P"])
        bi = g[f"{mode}_p{i}_beam_indices"]
        np.testing.assert_array_equal(p["beam_indices"], bi, err_msg=f"pass {i}")
        assert p["T"] == bi.shape[1] - 1 and p["frames"].shape == (len(p["rows"]), p["T"])
        assert p["num_frames"].tolist() == [len(range(1500)[: int(n) // 2]) for n in g[f"{mode}_p{i}_num_frames"]]
        # the exported DTW matrix, fed to the restatement, gives exactly the engine's frame indices
        for r in range(len(p["rows"])):
            np.testing.assert_array_equal(R.dtw_frames(p["matrix"][r, :, : int(p["num_frames"][r])]), p["frames"][r])
        # raw weights against the fixture's float64 sample: [A][B][T][S] -> [B][A][::ts][::st]
        w = p["weights"].transpose(1, 0, 2, 3)[:, :, ::ts, ::st].astype(np.float64)
        w64, eps = g[f"{mode}_p{i}_w64"], float(g[f"{mode}_p{i}_eps_ref"])
        assert w.shape == w64.shape
        err = float((np.abs(w - w64).max(-1) / w64.max(-1)).max())
        print(f"{mode} pass {i}: weights err {err:.3e} vs 8 eps_ref {8 * eps:.3e}")
        if err > 8 * eps:
            failures.append(f"pass {i}: weights err {err:.3e} > {8 * eps:.3e}")
        want = g[f"{mode}_p{i}_ts"]
        got = _pass_token_timestamps(p["frames"], p["num_input_ids"], want.shape[1])
        for r, b in enumerate(p["rows"]):
            cases += 1
            if not g[f"{mode}_p{i}_stable"][r]:
                row_stable[b] = False
                continue
            compared += 1
            if not np.array_equal(got[r], want[r]):
                failures.append(f"pass {i} row {b} (stable): timestamps differ from the reference")
    assert 4 * compared >= 3 * cases, (compared, cases)
    tts = res["token_timestamps"].cpu().numpy()
    assert tts.dtype == np.float32 and tts.shape == g[f"{mode}_token_timestamps"].shape
    assert 4 * int(row_stable.sum()) >= 3 * len(row_stable)
    for b in np.nonzero(row_stable)[0]:
        if not np.array_equal(tts[b], g[f"{mode}_token_timestamps"][b]):
            failures.append(f"row {b}: top-level token_timestamps differ from the reference")
        segs = res["segments"][b]
        assert [len(s["tokens"]) for s in segs] == g[f"{mode}_seg_len_{b}"].tolist()
        seg = np.concatenate([s["token_timestamps"] for s in segs]) if segs else np.zeros(0, np.float32)
        if not np.array_equal(seg, g[f"{mode}_seg_tts_{b}"]):
            failures.append(f"row {b}: segments' token_timestamps differ from the reference")
    assert not failures, failures


def test_the_flag_changes_no_token_and_no_plain_graph(inputs, tiny32):
    """With and without the flag the tokens are the same, and a plain beam call after a flagged one replays the plan
    and graphs it had before (its configuration key has no alignment part)."""
    g, feats, mask = inputs
    plain, _, kw = _run(tiny32, g, feats, mask, "b3", flag=False)
    sess = tiny32._session(len(g["cases"]), kw["num_beams"])

    def plain_keys():
        return [k for k in sess._greedy_cfg if k[0] == "beam" and "align" not in str(k)]

    keys = plain_keys()
    graphs = {k: sess._greedy_cfg[k]["graph"] for k in keys}
    assert keys and all(v is not None for v in graphs.values())
    res, _, _ = _run(tiny32, g, feats, mask, "b3")
    assert torch.equal(res["sequences"], plain["sequences"])
    assert sum("align" in str(k) for k in sess._greedy_cfg) >= 1
    again, _, _ = _run(tiny32, g, feats, mask, "b3", flag=False)
    assert torch.equal(again["sequences"], plain["sequences"])
    assert plain_keys() == keys and all(sess._greedy_cfg[k]["graph"] is graphs[k] for k in keys)


def test_dict_output_single_pass(inputs, tiny32):
    """return_dict_in_generate without timestamps: sequences with the prompt, the pass's times (P zeros first)."""
    g, feats, mask = inputs
    gen = tiny32.generation_config.copy()
    gen.eos_token_id = int(g["b3_eos"])
    res = tiny32.generate(feats, generation_config=gen, attention_mask=mask, language="ja", task="transcribe",
                          return_dict_in_generate=True, return_token_timestamps=True, **json.loads(str(g["b3_kw"])))
    np.testing.assert_array_equal(res["sequences"].cpu().numpy(), g["b3_p0_sequences"])
    st = g["b3_p0_stable"]
    assert st.sum() * 4 >= 3 * len(st)
    np.testing.assert_array_equal(res["token_timestamps"].cpu().numpy()[st], g["b3_p0_ts"][st])


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_bf16(inputs, tiny16, mode):
    """The same calls complete on the bf16 engine, and the last pass's frames equal a recomputation from the session's
    query log with the existing kernels in the reference's order: kw_align_weights of every running row (over its own
    item's keys), the gather on the host by the reported beam_indices, kw_align_reduce, kw_dtw: bitwise weights, equal
    frames."""
    from kwhisper import ops
    from kwhisper.decode import beam_row_table

    g, feats, mask = inputs
    res, align, kw = _run(tiny16, g, feats, mask, mode)
    tts = res["token_timestamps"].cpu().numpy()
    assert np.isfinite(tts).all() and tts.shape == tuple(res["sequences"].shape)
    for p in align:
        bi = p["beam_indices"]
        lens = (bi != -1).sum(-1)
        assert bi.shape[1] == lens.max() and p["T"] == bi.shape[1] - 1
        for b in range(len(bi)):  # a hypothesis stays inside its item's running rows
            own = bi[b, : lens[b]]
            assert ((own >= b * kw["num_beams"]) & (own < (b + 1) * kw["num_beams"])).all()
    p = align[-1]
    if p["T"] == 0:
        return
    B, T_ = len(p["rows"]), p["T"]
    sess = tiny16._session(B, kw["num_beams"])
    pairs = tuple((int(l), int(h)) for l, h in tiny16.generation_config.alignment_heads)
    log = sess._align_log(pairs)  # [A][R][448][64], the last pass's queries
    table = beam_row_table(p["beam_indices"])
    S, nb = sess.T, kw["num_beams"]
    full = torch.empty((len(pairs), B * nb, T_, S), device="cuda")
    ops.align_weights(log, sess.cross.repeat_interleave(nb, dim=1).contiguous(), pairs, T_, full, layer_step=2)
    w = torch.stack([torch.stack([full[:, int(table[b, t]), t] for t in range(T_)], 1) for b in range(B)], 1).contiguous()
    assert np.array_equal(w.cpu().numpy().view(np.int32), p["weights"].view(np.int32))
    frames = torch.from_numpy(p["num_frames"].astype(np.int32)).cuda()
    matrix = torch.empty((B, T_, S), device="cuda")
    ops.align_reduce(w, len(pairs), B, T_, S, frames, TINY.median_filter_width, matrix)
    np.testing.assert_array_equal(ops.dtw(matrix, frames).cpu().numpy(), p["frames"])
