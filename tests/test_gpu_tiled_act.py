"""Fragment-major bf16 activations on the GPU (KW_LD_TILED, include/kwhisper.h): every kernel that reads a tiled
operand gives, bit for bit, what it gives from the same rows stored row-major -- the same fragments reach the same
MFMAs in the same order."""
import pytest
import torch

from kwhisper import ops

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _tiled_with_nan_padding(x):
    """act_tile(x) with the padding rows M .. 16 T - 1 holding NaN (they feed discarded outputs only)."""
    M, K = x.shape
    T = (M + 15) // 16
    p = torch.full((16 * T, K), float("nan"), device=x.device, dtype=x.dtype)
    p[:M] = x
    return ops.act_tile(p)


def _linear(x, ldx, packed, colsum, bias, h0, M, N, K, mode, ws):
    """One kw_dec_linear call in ``mode``; returns its outputs."""
    if mode == "resid":
        h, hb = h0.clone(), torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
        ops.DecLinearPlan(x, packed, M, N, K, ldx=ldx, bias=bias, resid=(h, hb, N, 0), workspace=ws)()
        return h, hb
    C = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    kw = {"ln": (EPS, colsum)} if mode in ("ln", "gelu_bf16") else {}
    ops.DecLinearPlan(x, packed, M, N, K, ldx=ldx, bias=bias, C=C, gelu=mode == "gelu_bf16", workspace=ws, **kw)()
    return (C,)


@pytest.mark.parametrize("N,K,mode", [(48, 96, "store"), (1152, 384, "ln"), (384, 1536, "resid"),
                                      (1280, 5120, "resid"), (5120, 1280, "gelu_bf16")])
def test_dec_linear_tiled_input_is_bitwise_row_major(N, K, mode):
    """kw_dec_linear from a tiled x == from row-major x: M = 1, 5, 16 (one row tile), 17, 32 (two: the row split's
    16-row chunks where the grid takes it, both halves of a 32-row tile where it does not); the padding rows hold
    NaN; (1280, 5120) takes the split-K seam (its workspace holds partial slabs) and runs twice on one workspace."""
    torch.manual_seed(N + K)
    W = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    packed, colsum = ops.pack_weight(W), ops.ln_colsum(W)
    bias = torch.randn(N, device="cuda") * 0.1
    need = ops.dec_linear_workspace_bytes(N, K)
    seam = need > 4096 * 4  # more than the arrival counters: K-split partial slabs
    assert seam == ((N, K) == (1280, 5120))
    ws = torch.zeros(need // 4 + 1, device="cuda")
    for M in (1, 5, 16, 17, 32):
        x = torch.randn(M, K, device="cuda").bfloat16()
        h0 = torch.randn(M, N, device="cuda")
        want = _linear(x, None, packed, colsum, bias, h0, M, N, K, mode, ws)
        xt = _tiled_with_nan_padding(x)
        assert torch.equal(ops.act_untile(xt, M, K), x)
        for rep in range(2 if seam else 1):
            got = _linear(xt, ops.KW_LD_TILED, packed, colsum, bias, h0, M, N, K, mode, ws)
            torch.cuda.synchronize()
            for g, w in zip(got, want):
                assert not bool(torch.isnan(g.float()).any()), (M, rep)
                assert torch.equal(g, w), (M, rep, (g.float() - w.float()).abs().max().item())
    if seam:
        assert int(ws.view(torch.int32)[:4096].abs().sum()) == 0  # the arrival counters re-armed (slabs keep partials)


def test_tiled_input_rejected_where_no_kernel_reads_it():
    """A tiled x with a shape no tiled reader covers is KW_EINVAL (ValueError), never a wrong read: more than 32
    rows, and an LM head shape its persistent kernel does not cover (more than 8 column groups per workgroup)."""
    W = ops.pack_weight(torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16))
    x = torch.zeros(4096, device="cuda", dtype=torch.bfloat16)
    C = torch.zeros(33, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.DecLinearPlan(x, W, 33, 64, 64, ldx=ops.KW_LD_TILED, C=C)()
    V, K = 80000, 64
    assert not ops.lm_greedy_supported(4, V, K)
    Wl = ops.pack_weight(torch.zeros(V, K, device="cuda", dtype=torch.bfloat16))
    logits = torch.zeros(4, V, device="cuda")
    with pytest.raises(ValueError):
        ops.DecLinearPlan(x, Wl, 4, V, K, ldx=ops.KW_LD_TILED, ln=(EPS, torch.zeros(V, device="cuda")), C=logits)()


@pytest.mark.parametrize("M", [1, 17, 32])
@pytest.mark.parametrize("L", [1, 16, 129])
def test_qkv_self_tiled_input_is_bitwise_row_major(M, L):
    """kw_dec_qkv_self tiled (hb in, attn out) == row-major: out after act_untile, the appended K / V cache rows and
    the status word; rows >= M of the tiled out are never written."""
    d, H, t_max = 384, 6, 448
    torch.manual_seed(M * 100 + L)
    hb = torch.randn(M, d, device="cuda").bfloat16()
    W = (torch.randn(3 * d, d, device="cuda") / d ** 0.5).bfloat16()
    packed, colsum = ops.pack_weight(W), ops.ln_colsum(W)
    bias = torch.randn(3 * d, device="cuda") * 0.1
    kc = torch.randn(M, H, t_max, 64, device="cuda").bfloat16()
    vc = torch.randn(M, H, t_max, 64, device="cuda").bfloat16()
    cur = torch.tensor([L], dtype=torch.int32, device="cuda")
    res = []
    for x, ldx in ((hb, None), (_tiled_with_nan_padding(hb), ops.KW_LD_TILED)):
        qws = torch.zeros(ops.qkv_self_workspace_bytes(M, d) // 4 + 1, device="cuda")
        kc2, vc2 = kc.clone(), vc.clone()
        out = torch.full((16 * ((M + 15) // 16), d), 7.0, device="cuda", dtype=torch.bfloat16)
        ops.QkvSelfPlan(x, packed, M, d, H, ln=(EPS, colsum), bias=bias, scale=0.125, k_cache=kc2, v_cache=vc2,
                        t_max=t_max, cur_len=cur, out=out, workspace=qws, ldx=ldx)()
        torch.cuda.synchronize()
        assert int(qws.view(torch.int32).abs().sum()) == 0, "granules not re-armed / status word set"
        if ldx is not None:
            assert bool((ops.act_untile(out.view(-1), out.shape[0], d)[M:] == 7.0).all())
            out = ops.act_untile(out.view(-1), M, d)
        res.append((out[:M], kc2, vc2))
    assert not bool(torch.isnan(res[0][0].float()).any()) and not bool((res[0][0] == 7.0).all())
    for g, w in zip(res[1], res[0]):
        assert torch.equal(g, w)
    assert not torch.equal(res[0][1][:, :, L - 1], kc[:, :, L - 1])  # (the row at L - 1 was appended)


@pytest.mark.parametrize("M,d,H", [(1, 384, 6), (17, 384, 6), (32, 384, 6), (32, 1280, 20)])
def test_xq_cross_tiled_input_is_bitwise_row_major(M, d, H):
    """kw_dec_xq_cross tiled (hb in, attn out) == row-major: out after act_untile and the status word (S = 1500); the
    large-v3 shape runs the one-workgroup-per-pair kernel (cross_attn_row_kernel), the small ones xq_cross_kernel."""
    S = 1500
    assert ops.cross_attn_pair_kernel(M * H, S, fused=True) == (d == 1280)
    torch.manual_seed(M)
    hb = torch.randn(M, d, device="cuda").bfloat16()
    W = (torch.randn(d, d, device="cuda") / d ** 0.5).bfloat16()
    packed, colsum = ops.pack_weight(W), ops.ln_colsum(W)
    bias = torch.randn(d, device="cuda") * 0.1
    k = torch.randn(M, H, S, 64, device="cuda").bfloat16()
    v = torch.randn(M, H, S, 64, device="cuda").bfloat16()
    res = []
    for x, ldx in ((hb, None), (_tiled_with_nan_padding(hb), ops.KW_LD_TILED)):
        ws = torch.zeros(ops.xq_cross_workspace_bytes(M, d, H, S) // 4 + 1, device="cuda")
        out = torch.full((16 * ((M + 15) // 16), d), 7.0, device="cuda", dtype=torch.bfloat16)
        ops.XqCrossPlan(x, packed, M, d, H, ln=(EPS, colsum), bias=bias, scale=0.125, k=k, v=v, S=S, out=out,
                        workspace=ws, ldx=ldx)()
        torch.cuda.synchronize()
        assert int(ws.view(torch.int32).abs().sum()) == 0, "granules not re-armed / status word set"
        if ldx is not None:
            assert bool((ops.act_untile(out.view(-1), out.shape[0], d)[M:] == 7.0).all())
            out = ops.act_untile(out.view(-1), M, d)
        res.append(out[:M])
    assert not bool(torch.isnan(res[0].float()).any()) and not bool((res[0] == 7.0).all())
    assert torch.equal(res[1], res[0])


@pytest.mark.parametrize("N,K", [(384, 1536), (1280, 5120), (1280, 1280)])
def test_resid_writes_tiled_mirror_bitwise(N, K):
    """RESID with KW_EPI_HB_TILED (tiled x in, tiled hb out): act_untile(hb) == the row-major hb and h bit for bit;
    rows >= M of the tiled hb are never written (they keep the canary); M as above, so the spread epilogue's 16 x 16
    blocks (one row tile), the row split's chunks and the split-K seam's wave-0 epilogue (1280 x 5120) all write it."""
    torch.manual_seed(N * 3 + K)
    W = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
    packed = ops.pack_weight(W)
    bias = torch.randn(N, device="cuda") * 0.1
    ws = torch.zeros(ops.dec_linear_workspace_bytes(N, K) // 4 + 1, device="cuda")
    for M in (1, 5, 16, 17, 32):
        x = torch.randn(M, K, device="cuda").bfloat16()
        h0 = torch.randn(M, N, device="cuda")
        h1, hb1 = _linear(x, None, packed, None, bias, h0, M, N, K, "resid", ws)
        T = (M + 15) // 16
        h2 = h0.clone()
        hbt = torch.full((16 * T * N,), 3.0, device="cuda", dtype=torch.bfloat16)  # canary
        ops.DecLinearPlan(_tiled_with_nan_padding(x), packed, M, N, K, ldx=ops.KW_LD_TILED, bias=bias,
                          resid=(h2, hbt, N, 0), workspace=ws, hb_tiled=True)()
        torch.cuda.synchronize()
        assert torch.equal(h2, h1), M
        assert torch.equal(ops.act_untile(hbt, M, N), hb1), M
        pad = ops.act_untile(hbt, 16 * T, N)[M:]
        assert bool((pad == 3.0).all()), M


def test_tiled_mirror_rejected_where_not_covered():
    W = ops.pack_weight(torch.zeros(48, 64, device="cuda", dtype=torch.bfloat16))
    x = torch.zeros(4, 64, device="cuda", dtype=torch.bfloat16)
    h, hb = torch.zeros(4, 48, device="cuda"), torch.zeros(16 * 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):  # N % 32 != 0: not a whole k-tile of the next linear
        ops.DecLinearPlan(x, W, 4, 48, 64, resid=(h, hb, 48, 0), hb_tiled=True)()
    with pytest.raises(ValueError):  # no RESID epilogue
        ops.DecLinearPlan(x, W, 4, 48, 64, C=torch.zeros(4, 48, device="cuda"), hb_tiled=True)


@pytest.mark.parametrize("B,d", [(3, 384), (32, 384), (3, 1280), (32, 1280)])
def test_embed_writes_tiled_mirror_bitwise(B, d):
    V = 1000
    torch.manual_seed(B + d)
    tok = torch.randn(V, d, device="cuda").bfloat16()
    pos = torch.randn(448, d, device="cuda").bfloat16()
    ids = torch.randint(0, V, (B, 449), device="cuda")
    cur = torch.tensor([7], dtype=torch.int32, device="cuda")
    h1, hb1 = torch.empty(B, d, device="cuda"), torch.empty(B, d, device="cuda", dtype=torch.bfloat16)
    ops.embed(ids, B, 1, cur, tok, pos, h1, hb1)
    T = (B + 15) // 16
    h2 = torch.empty(B, d, device="cuda")
    hbt = torch.full((16 * T * d,), 3.0, device="cuda", dtype=torch.bfloat16)
    ops.embed(ids, B, 1, cur, tok, pos, h2, hbt, hb_tiled=True)
    torch.cuda.synchronize()
    assert torch.equal(h2, h1)
    assert torch.equal(ops.act_untile(hbt, B, d), hb1)
    assert bool((ops.act_untile(hbt, 16 * T, d)[B:] == 3.0).all())
    with pytest.raises(ValueError):  # q_len 2: rows are not one per item
        ops.embed(ids, B, 2, cur, tok, pos, torch.empty(2 * B, d, device="cuda"), hbt, hb_tiled=True)


@pytest.mark.parametrize("B,V,K", [(5, 8192, 384), (32, 8192, 1280)])
def test_lm_head_and_lm_greedy_tiled_input_bitwise(B, V, K):
    """The LM head (kw_dec_linear's persistent kernel) and kw_dec_lm_greedy from a tiled hb: logits and tokens bit for
    bit those from row-major hb."""
    torch.manual_seed(B + K)
    P, eos, pad = 3, 7000, 6999
    W = (torch.randn(V, K, device="cuda") / K ** 0.5).bfloat16()
    Wp, cs = ops.pack_weight(W), ops.ln_colsum(W)
    bias = 0.1 * torch.randn(V, device="cuda")
    sup = torch.zeros(V, dtype=torch.uint8, device="cuda")
    sup[torch.randint(0, V, (400,), device="cuda")] = 1
    bsup = torch.tensor([220, eos], dtype=torch.int32, device="cuda")
    x = (torch.randn(B, K, device="cuda") * 2 + 0.3).bfloat16()
    assert ops.lm_greedy_supported(B, V, K)
    res = []
    for xin, ldx in ((x, None), (_tiled_with_nan_padding(x), ops.KW_LD_TILED)):
        head = torch.full((B, V), float("nan"), device="cuda")
        ops.DecLinearPlan(xin, Wp, B, V, K, ldx=ldx, ln=(EPS, cs), bias=bias, C=head)()
        ids = torch.zeros((B, 64), dtype=torch.int64, device="cuda")
        ids[:, :P] = torch.tensor([50258, 50266, 50360])
        cur = torch.tensor([P], dtype=torch.int32, device="cuda")
        unf = torch.ones(B, dtype=torch.int32, device="cuda")
        nun = torch.zeros(1, dtype=torch.int32, device="cuda")
        logits = torch.full((B, V), float("nan"), device="cuda")
        ws = torch.zeros(ops.lm_greedy_workspace_bytes(B, V) // 4 + 1, device="cuda")
        ops.LmGreedyPlan(xin, Wp, B, V, K, ln=(EPS, cs), bias=bias, suppress_mask=sup, begin_suppress=bsup, ids=ids,
                         cur_len=cur, unfinished=unf, n_unfinished=nun, eos_id=eos, pad_id=pad, max_length=P + 4,
                         begin_index=P, workspace=ws, logits=logits, ldx=ldx)()
        torch.cuda.synchronize()
        res.append((head, logits, ids, unf))
    assert not bool(torch.isnan(res[0][0]).any())
    for g, w in zip(res[1], res[0]):
        assert torch.equal(g, w)
    assert torch.equal(res[0][0], res[0][1])  # (the two LM heads agree, as test_lm_greedy_equals_lm_head_then_sampler)


def test_decode_session_tiled_plan_tokens_identical(gold):
    """The tiny model's greedy generate with the tiled step plan (the default) and with it forced off
    (tiled_act=False): identical token ids; the tiled plan really ran (its hb holds whole 16-row tiles, its linears
    carry KW_LD_TILED); a session of more than 32 rows falls back to the row-major plan and matches too."""
    from kwhisper.config import TINY, generation_constants
    from kwhisper.engine import WhisperEngine
    from kwhisper.generation import KWhisperForConditionalGeneration
    from kwhisper.synthetic import synthetic_state_dict

    from _util import oracle_features

    g = gold("tiny_fp32")
    feats = torch.from_numpy(oracle_features(TINY, g["cases"])).cuda()
    sd = synthetic_state_dict(TINY, 0)

    def mk(tiled):
        return KWhisperForConditionalGeneration(WhisperEngine(TINY, sd, dtype=torch.bfloat16,
                                                              generation_config=generation_constants(TINY),
                                                              tiled_act=tiled))

    on, off = mk(True), mk(False)
    for ts in (False, True):  # (kw_dec_lm_greedy tail; LM head + sampler tail)
        a = on.generate(feats, language="ja", task="transcribe", max_length=48, return_timestamps=ts).cpu()
        b = off.generate(feats, language="ja", task="transcribe", max_length=48, return_timestamps=ts).cpu()
        assert torch.equal(a, b), ts
    s_on, s_off = on._sessions[(4, 1)], off._sessions[(4, 1)]
    assert s_on.tiled_ok and not s_off.tiled_ok
    assert s_on._buffers(1)["hb"].shape[0] == 16 and s_off._buffers(1)["hb"].shape[0] == 4
    lins = [p for p in s_on._step_plans(1, fused=s_on.fused_last)
            if getattr(p, "tag", None) in ("fc1", "o", "xo", "qkv_self", "xq_cross")]
    assert len(lins) == 5 * TINY.decoder_layers
    assert all((p.args if hasattr(p, "args") else p._a).ldx == ops.KW_LD_TILED for p in lins)
    assert not any((p.args if hasattr(p, "args") else p._a).ldx == ops.KW_LD_TILED
                   for p in s_off._step_plans(1, fused=s_off.fused_last) if not isinstance(p, tuple))
    big = feats.repeat(9, 1, 1)  # 36 rows: more than two row tiles
    a = on.generate(big, language="ja", task="transcribe", max_length=24).cpu()
    b = off.generate(big, language="ja", task="transcribe", max_length=24).cpu()
    assert not on._sessions[(36, 1)].tiled_ok
    assert torch.equal(a, b)
