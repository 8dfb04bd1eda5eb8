"""The opt-in fp8 (e4m3) cross K/V cache on the GPU: the quantisation kernel against the format's CPU restatement
(bit for bit), the fp8 cross-attention step against fp32 arithmetic on the dequantised cache, the fused query
projection + step against its two launches (bit for bit), and a tiny bf16 engine with cross_kv_dtype="fp8_e4m3"
against the numpy oracle running on that engine's own cache."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kwhisper import ops  # noqa: E402
from kwhisper.config import TINY, generation_constants  # noqa: E402
from kwhisper.synthetic import synthetic_state_dict  # noqa: E402

import _fp8_ref as R  # noqa: E402
from _util import oracle_features  # noqa: E402

EPS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _quant(x):
    """kw_cross_kv_quant on a bf16 device tensor [..., S, 64] -> (codes uint8, scales f32)."""
    codes = torch.empty(x.shape, device="cuda", dtype=torch.uint8)
    scales = torch.empty(x.shape[:-2] + x.shape[-1:], device="cuda", dtype=torch.float32)
    ops.cross_kv_quant(x, codes, scales)
    return codes, scales


_LUT = None


def _dequant(codes, scales):
    """float(code) * scale on the device (a 256-entry table of the CPU decode: reference arithmetic only)."""
    global _LUT
    if _LUT is None:
        _LUT = torch.from_numpy(R.decode(np.arange(256, dtype=np.uint8))).cuda()
    return _LUT[codes.int()] * scales.unsqueeze(-2)


# ---- kw_cross_kv_quant ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["random", "exact"])
@pytest.mark.parametrize("n,S", [(2 * 2 * 3, 1500), (3, 77), (3, 1)])
def test_quant_matches_reference(kind, n, S):
    """Codes and scales bit for bit the CPU restatement's: random bf16 tiles (with a channel of zeros and a channel
    whose maximum is negative planted in one tile), and tiles the format holds exactly (codes with one +-448 per
    channel times a power-of-two scale: the kernel must give back those codes and scales)."""
    rng = np.random.default_rng(n * 10000 + S)
    if kind == "exact":
        x, want_c, want_s = R.exact_case(rng, n, S)
        xb = torch.from_numpy(x).bfloat16()
        assert torch.equal(xb.float(), torch.from_numpy(x))
    else:
        # channels spread over 12 octaves, so the scales differ and small channels reach fp8's subnormals
        x = rng.standard_normal((n, S, 64)).astype(np.float32) * np.exp2(rng.integers(-6, 6, size=(n, 1, 64))).astype(np.float32)
        xb = torch.from_numpy(x).bfloat16()
        xb[1, :, 5] = 0.0
        xb[1, :, 9] = -xb[1, :, 9].abs() - 1.0
        want_c, want_s = R.quantize(xb)
        assert want_s[1, 5] == 0 and not want_c[1, :, 5].any()
    codes, scales = _quant(xb.cuda())
    ref_c, ref_s = R.quantize(xb)
    assert np.array_equal(scales.cpu().numpy(), ref_s)
    bad = np.argwhere(codes.cpu().numpy() != ref_c)
    assert bad.size == 0, (len(bad), bad[:4])
    if kind == "exact":
        assert np.array_equal(ref_c, want_c) and np.array_equal(ref_s, want_s)


# ---- kw_cross_attn_step_fp8 -------------------------------------------------------------------------------------

def _fp8_case(B, H, q_len, S, seed):
    """bf16 K / V with channel c scaled by 2^((c % 7) - 3) -- so a scale applied to the wrong dim, or K's scales to V,
    is an error of several octaves -- quantised by kw_cross_kv_quant (held bit-exact above); a bf16 query."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    chan = torch.exp2((torch.arange(64, device="cuda") % 7 - 3).float())
    k = (torch.randn(B, H, S, 64, device="cuda", generator=g) * chan).bfloat16()
    v = (torch.randn(B, H, S, 64, device="cuda", generator=g) * chan.flip(0)).bfloat16()
    q = (torch.randn(B * q_len, H * 64, device="cuda", generator=g) * 0.3).bfloat16()
    kc, ks = _quant(k)
    vc, vs = _quant(v)
    return q, kc, ks, vc, vs


def _step(q, B, q_len, H, kc, ks, vc, vs, S):
    out = torch.full((B * q_len, H * 64), 7.0, device="cuda", dtype=torch.bfloat16)
    ops.cross_attn_step_fp8(q, B, q_len, H, 64, kc, vc, ks, vs, S, out)
    return out


@pytest.mark.parametrize("B,H,q_len,S", [(2, 6, 1, 1500), (3, 4, 4, 1500), (2, 6, 1, 1399), (2, 6, 1, 1536),
                                         (32, 20, 1, 1500)])
def test_step_fp8_close_to_fp32(B, H, q_len, S):
    """The unfused op vs fp32 softmax(q K^T) V over the DEQUANTISED cache (K^ = codes * scale), atol = rtol = 2e-2:
    the tolerance test_cross_attn_step gives the bf16 kernels against the same kind of reference -- the kernel does
    f32 arithmetic on exactly those values; what differs is the bf16 query, exp2 and the bf16 store, as for bf16 K/V.
    Tiny's 12 pairs; the prefill mapping (a row reads its own item's K/V); chunks of 234 / 229 keys; 6 x 256; the
    bench's 640 pairs.  Two launches on the same buffers are equal."""
    q, kc, ks, vc, vs = _fp8_case(B, H, q_len, S, seed=B * 1000 + S + q_len)
    out = _step(q, B, q_len, H, kc, ks, vc, vs, S)
    assert torch.equal(_step(q, B, q_len, H, kc, ks, vc, vs, S), out)
    assert not bool(torch.isnan(out.float()).any())
    qq = q.float().view(B, q_len, H, 64).permute(0, 2, 1, 3)
    kh, vh = _dequant(kc, ks), _dequant(vc, vs)
    ref = (torch.softmax(qq @ kh.transpose(-1, -2), -1) @ vh).permute(0, 2, 1, 3).reshape(B * q_len, H * 64)
    err = (out.float() - ref).abs()
    print(f"fp8 step B={B} H={H} q_len={q_len} S={S}: max abs err {err.max().item():.3g} (|ref| max {ref.abs().max().item():.3g})")
    torch.testing.assert_close(out.float(), ref, atol=2e-2, rtol=2e-2)


def test_step_fp8_rejects():
    """S that does not give six chunks each reaching the last key group (1349: a last chunk of 224; 77: one chunk) and
    head_dim 32 are KW_EUNSUPPORTED with a message, on both backends; nothing is launched (out keeps its canary)."""
    from kwhisper._lib import KWError

    B, H = 2, 6
    old = ops.backend()
    try:
        for be in ("torch", "ctypes"):
            ops.set_backend(be)
            for S, hd, msg in ((1349, 64, "6 chunks"), (77, 64, "6 chunks"), (1500, 32, "head_dim")):
                q = torch.zeros(B, H * hd, device="cuda", dtype=torch.bfloat16)
                kc = torch.zeros(B, H, S, hd, device="cuda", dtype=torch.uint8)
                sc = torch.ones(B, H, hd, device="cuda")
                out = torch.full((B, H * hd), 7.0, device="cuda", dtype=torch.bfloat16)
                with pytest.raises((KWError, RuntimeError), match=msg):
                    ops.cross_attn_step_fp8(q, B, 1, H, hd, kc, kc, sc, sc, S, out)
                torch.cuda.synchronize()
                assert bool((out == 7.0).all())
    finally:
        ops.set_backend(old)
    assert not ops.xq_cross_fp8_supported(2, 384, 6, 1349) and not ops.xq_cross_fp8_supported(2, 384, 6, 77)
    assert ops.xq_cross_fp8_supported(2, 384, 6, 1500) and ops.xq_cross_fp8_supported(32, 1280, 20, 1399)


def test_step_fp8_batch_invariant():
    """One grid at every batch size: rows 5 and 6 of a B = 32, H = 20 launch are bitwise the same two items as B = 2."""
    B, H, S = 32, 20, 1500
    q, kc, ks, vc, vs = _fp8_case(B, H, 1, S, seed=77)
    big = _step(q, B, 1, H, kc, ks, vc, vs, S)
    sl = slice(5, 7)
    small = _step(q[sl].contiguous(), 2, 1, H, kc[sl].contiguous(), ks[sl].contiguous(), vc[sl].contiguous(),
                  vs[sl].contiguous(), S)
    assert torch.equal(small, big[sl])


# ---- kw_dec_xq_cross_fp8 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("M,d,H", [(2, 384, 6), (32, 1280, 20)])
def test_xq_cross_fp8_fused_matches_two_launches(M, d, H, tiled):
    """The fused block is bitwise kw_dec_linear(xq) followed by kw_cross_attn_step_fp8, row-major and KW_LD_TILED
    (hb in, attn out), for two different inputs launched on ONE workspace (the second launch reads nothing of the
    first: re-armed), and the workspace is left all zero -- as the bf16 block leaves it."""
    S = 1500
    assert ops.xq_cross_fp8_supported(M, d, H, S)
    g = torch.Generator(device="cuda").manual_seed(M * 10 + int(tiled))
    W = (torch.randn(d, d, device="cuda", generator=g) / d ** 0.5).bfloat16()
    packed, colsum = ops.pack_weight(W), ops.ln_colsum(W)
    bias = torch.randn(d, device="cuda", generator=g) * 0.1
    ws = torch.zeros(ops.xq_cross_workspace_bytes(M, d, H, S) // 4 + 1, device="cuda")
    lin_ws = torch.zeros(ops.dec_linear_workspace_bytes(d, d) // 4 + 1, device="cuda")
    rows = 16 * ((M + 15) // 16)
    outs = []
    for rep in range(2):
        _, kc, ks, vc, vs = _fp8_case(M, H, 1, S, seed=M * 100 + rep)
        hb = torch.randn(M, d, device="cuda", generator=g).bfloat16()
        x = ops.act_tile(hb) if tiled else hb
        ldx = ops.KW_LD_TILED if tiled else None
        qx = torch.empty(M, d, device="cuda", dtype=torch.bfloat16)
        ops.DecLinearPlan(x, packed, M, d, d, ln=(EPS, colsum), bias=bias, C=qx, scale=0.125, scale_cols=d,
                          workspace=lin_ws, ldx=ldx)()
        want = _step(qx, M, 1, H, kc, ks, vc, vs, S)
        out = torch.full((rows, d), 7.0, device="cuda", dtype=torch.bfloat16)
        ops.XqCrossFp8Plan(x, packed, M, d, H, ln=(EPS, colsum), bias=bias, scale=0.125, k=kc, v=vc, k_scale=ks,
                           v_scale=vs, S=S, out=out, workspace=ws, ldx=ldx)()
        torch.cuda.synchronize()
        got = ops.act_untile(out.view(-1), M, d) if tiled else out[:M]
        assert not bool(torch.isnan(got.float()).any())
        assert torch.equal(got, want), (rep, (got.float() - want.float()).abs().max().item())
        assert int(ws.view(torch.int32).abs().sum()) == 0, "workspace not re-armed / status word set"
        outs.append(got)
    assert not torch.equal(outs[0], outs[1])  # (the inputs do differ)


# ---- the engine option ------------------------------------------------------------------------------------------

def _model(cross_kv_dtype, dtype=torch.bfloat16):
    from kwhisper.generation import KWhisperForConditionalGeneration

    return KWhisperForConditionalGeneration.from_state_dict(
        TINY, synthetic_state_dict(TINY, 0), dtype=dtype, generation_config=generation_constants(TINY),
        cross_kv_dtype=cross_kv_dtype)


@pytest.fixture(scope="module")
def tiny_fp8():
    return _model("fp8_e4m3")


def test_fp8_default_untouched(tiny_fp8):
    """cross_kv_dtype=None is today's engine: a bf16 cross cache, XqCrossPlan in the step plan and no fp8 plan; the
    fp8 engine holds uint8 codes + f32 scales and plans the fp8 block instead.  lane() handles inherit the option."""
    m = _model(None)
    sess = m.engine.new_session(2)
    assert sess.cross.dtype == torch.bfloat16 and sess.cross_scale is None
    kinds = {type(p).__name__ for p in sess._step_plans(1)}
    assert "XqCrossPlan" in kinds and "XqCrossFp8Plan" not in kinds
    s8 = tiny_fp8.engine.new_session(2)
    assert s8.cross.dtype == torch.uint8 and s8.cross.shape == sess.cross.shape
    assert s8.cross_scale.dtype == torch.float32 and tuple(s8.cross_scale.shape) == (8, 2, 6, 64)
    kinds = {type(p).__name__ for p in s8._step_plans(1)}
    assert "XqCrossFp8Plan" in kinds and "XqCrossPlan" not in kinds
    assert tiny_fp8.lane().engine.cross_kv_dtype == "fp8_e4m3" and m.lane().engine.cross_kv_dtype is None


def test_tiny_fp8_engine_against_its_own_cache(gold, tiny_fp8):
    """Engine and oracle on the SAME K/V: the session's codes and scales are read back, dequantised and put into the
    numpy oracle's cache["cross"]; both are teacher-forced along the fixture's greedy sequences (2 rows x 32 steps).
    They then differ by the engine's bf16 arithmetic only, so the bar is the tiny bf16 engine's: top-8 logits within
    max 0.25 / mean 0.03 (test_tiny_bf16_logits_and_tokens)."""
    from oracle.whisper_np import WhisperNP

    g = gold("tiny_fp32")
    rows, steps, P = 2, 32, 4
    feats = torch.from_numpy(oracle_features(TINY, g["cases"][:rows])).cuda()
    eng = tiny_fp8.engine
    sess = eng.new_session(rows, eng.encode(feats))
    seq = g["greedy_sequences"][:rows, : P + steps - 1]
    lg = sess.teacher_forced_logits(torch.from_numpy(seq), P).cpu().numpy()
    assert lg.shape[1] == steps
    kv = R.dequantize(sess.cross.cpu().numpy(), sess.cross_scale.cpu().numpy())  # [2L][B][H][S][64]
    m = WhisperNP(synthetic_state_dict(TINY, 0), TINY)
    cache = {"cross": [(kv[2 * i], kv[2 * i + 1]) for i in range(TINY.decoder_layers)],
             "self": [None] * TINY.decoder_layers, "len": 0}
    want = m.decode(seq, cache)[:, P - 1:]
    idx = g["greedy_logits_top_idx"][:rows, :steps].astype(np.int64)
    err = np.abs(np.take_along_axis(lg, idx, -1) - np.take_along_axis(want, idx, -1))
    print("tiny fp8 engine vs the oracle on its own cache: top-8 logit err max %.4f mean %.4f" % (err.max(), err.mean()))
    assert err.max() < 0.25 and err.mean() < 0.03


def test_tiny_fp8_generate(gold, tiny_fp8):
    """Greedy generate() on the fp8 engine: tokens equal transformers' fp32 up to each row's first step with fp32 margin
    < 0.1 (the gate of test_tiny_bf16_logits_and_tokens); with timestamps it runs and its segments are well formed
    (ordered times, tokens);
    the ctypes and torch.ops backends give identical tokens; beams and token timestamps are refused."""
    g = gold("tiny_fp32")
    feats = torch.from_numpy(oracle_features(TINY, g["cases"])).cuda()
    kw = dict(language="ja", task="transcribe", max_length=128)
    toks = tiny_fp8.generate(feats, **kw).cpu().numpy()
    want, margin = g["greedy_tokens"], g["greedy_margin"]
    compared = 0
    for b in range(want.shape[0]):
        unsafe = np.nonzero(margin[b] < 0.1)[0]
        upto = unsafe[0] if unsafe.size else want.shape[1]
        np.testing.assert_array_equal(toks[b, :upto], want[b, :upto])
        compared += int(upto)
    assert compared > 4 * want.shape[0]
    sess = tiny_fp8._session(feats.shape[0])
    assert sess.fp8 and "kw_dec_xq_cross_fp8" in {n for n, _, _ in sess.status_words()}
    # timestamps: runs, and the segment structure is sound
    res = tiny_fp8.generate(feats, return_timestamps=True, return_segments=True, **kw)
    seqs = res["sequences"].cpu().numpy()
    assert seqs.shape[0] == feats.shape[0] and len(res["segments"]) == feats.shape[0]
    for row in res["segments"]:
        for s in row:  # (times carry the seek loop's offset: a later pass's segments lie past its window's start)
            assert 0.0 <= float(s["start"]) <= float(s["end"])
            assert len(s["tokens"]) > 0
    # backends
    res2 = {}
    old = ops.backend()
    try:
        for be in ("torch", "ctypes"):
            ops.set_backend(be)
            m = _model("fp8_e4m3")
            res2[be] = m.generate(feats, language="ja", task="transcribe", max_length=64).cpu()
            del m
    finally:
        ops.set_backend(old)
    assert torch.equal(res2["torch"], res2["ctypes"])
    assert np.array_equal(res2["torch"].numpy(), toks[:, :64][:, : res2["torch"].shape[1]])
    with pytest.raises(NotImplementedError, match="num_beams"):
        tiny_fp8.generate(feats, num_beams=2, **kw)
    with pytest.raises(NotImplementedError, match="return_token_timestamps"):
        tiny_fp8.generate(feats, return_token_timestamps=True, return_timestamps=True, **kw)


def test_handoff_timeout_raises_fp8(gold, tiny_fp8):
    """test_handoff_timeout_raises for the fused fp8 block: its fault-injection word makes one launch's first
    projection workgroup skip its publish, that launch's consumers time out (NaN rows + status word), generate()
    raises KWError naming kw_dec_xq_cross_fp8, the session re-arms, and the next call returns undisturbed tokens."""
    from kwhisper._lib import KWError

    g = gold("tiny_fp32")
    feats = torch.from_numpy(oracle_features(TINY, g["cases"][:2])).cuda()
    kw = dict(language="ja", task="transcribe", max_length=24)
    want = tiny_fp8.generate(feats, **kw).cpu().numpy()
    sess = tiny_fp8._session(2)
    words = {name: (ws, off) for name, ws, off in sess.status_words()}
    assert {"kw_dec_qkv_self", "kw_dec_xq_cross_fp8"} <= set(words) and "kw_dec_xq_cross" not in words
    ws, off = words["kw_dec_xq_cross_fp8"]
    ws.view(torch.int32)[off // 4 + 1] = 1  # arm the fault-injection word
    with pytest.raises(KWError, match="kw_dec_xq_cross_fp8"):
        tiny_fp8.generate(feats, **kw)
    assert int(ws.view(torch.int32)[off // 4 + 1]) == 0  # consumed by exactly one launch
    assert all(int(w.view(torch.int32)[o // 4]) == 0 for _, w, o in sess.status_words())  # re-armed
    np.testing.assert_array_equal(tiny_fp8.generate(feats, **kw).cpu().numpy(), want)
