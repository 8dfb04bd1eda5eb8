"""kw_self_attn_step_masked: the decoder self-attention step with a per-row first key (left-padded prompts).

Row b attends key positions key_start[b] <= k <= own position.  Checked here: key_start zero is bitwise
kw_self_attn_step; a float64 restatement with the explicit mask, at test_gpu_kernels.test_self_attn_step's
tolerances; pad queries give exact zeros; the appended K/V are the unmasked kernel's bits; whatever sits below
key_start (NaN here) reaches no valid output bit; a beam slot table together with key_start; and a row's output
does not depend on the other rows of the batch.  Shapes: B 3, H 2, head dim 64, t_max 448; the step at 2, 200 and
300 keys (300 crosses the 256-key chunk seam), the prefill at 5, 33 and 70 positions (one, two and three rounds
of attend_rows' 32 key slots).
"""
import pytest
import torch

from kwhisper import ops

pytestmark = pytest.mark.gpu

B, H, HD, T_MAX = 3, 2, 64, 448
D = H * HD
DTYPES = [torch.float32, torch.bfloat16]
TOL = {torch.float32: 1e-5, torch.bfloat16: 2e-2}  # test_gpu_kernels.test_self_attn_step's


def _key_starts(q_len, L):
    """Rows drawn from {0, 1, q_len - 4, q_len - 1} (the step: {0, 1, L - 2}), as rotations over the 3 rows."""
    vals = [0, 1, L - 2] if q_len == 1 else [0, 1, q_len - 4, q_len - 1]
    vals = [max(v, 0) for v in vals]
    return [[vals[(i + r) % len(vals)] for i in range(B)] for r in range(len(vals))]


# (q_len, L): the step at three lengths, the prefill from an empty cache and one on top of 10 cached positions
# (70: five 16-query tiles, the last of 6, and three 32-key tiles; 40 on 300: the tile kernel's keys from the cache)
SHAPES = [(1, 2), (1, 200), (1, 300), (5, 5), (33, 33), (70, 70), (5, 15), (40, 340)]
CASES = [(q, L, tuple(ks)) for q, L in SHAPES for ks in _key_starts(q, L)]
CASES.append((1, 2, (2, 0, 1)))  # a step whose row 0 is still a pad: no key at all


def _inputs(dtype, q_len, L, seed=0, rows=B):
    g = torch.Generator(device="cuda").manual_seed(1000 * q_len + L + seed)
    past = L - q_len
    kc = torch.zeros(rows, H, T_MAX, HD, device="cuda", dtype=dtype)
    vc = torch.zeros_like(kc)
    kc[:, :, :past] = torch.randn(rows, H, past, HD, device="cuda", generator=g).to(dtype)
    vc[:, :, :past] = torch.randn(rows, H, past, HD, device="cuda", generator=g).to(dtype)
    qkv = torch.randn(rows * q_len, 3 * D, device="cuda", generator=g).to(dtype)
    return qkv, kc, vc


def _ws(rows=B):
    return torch.zeros(ops.self_attn_workspace_bytes(rows, H, T_MAX) // 4 + 1, device="cuda")


def _i32(x):
    return torch.tensor(x, device="cuda", dtype=torch.int32)


def _masked(qkv, kc, vc, q_len, L, ks, bp=None, rows=B, twice=True, per_query=False):
    kc, vc = kc.clone(), vc.clone()
    out = torch.full((rows * q_len, D), float("nan"), device="cuda", dtype=qkv.dtype)
    ws = _ws(rows)
    for _ in range(2 if twice else 1):  # the arrival counters must come back to zero
        ops.self_attn_step_masked(qkv, rows, q_len, H, HD, kc, vc, T_MAX, _i32([L]), _i32(list(ks)), out, ws, bp=bp,
                                  per_query=per_query)
    return out, kc, vc


def _unmasked(qkv, kc, vc, q_len, L, bp=None):
    kc, vc = kc.clone(), vc.clone()
    out = torch.full((B * q_len, D), float("nan"), device="cuda", dtype=qkv.dtype)
    ops.self_attn_step(qkv, B, q_len, H, HD, kc, vc, T_MAX, _i32([L]), out, _ws(), bp=bp)
    return out, kc, vc


def _reference(qkv, kc, vc, q_len, L, ks, table=None):
    """float64, the explicit mask: key k of row b is attended by query position p iff ks[b] <= k <= p; a query with
    no key gives zeros.  ``table``: position k < L - 1 of row b is read from cache row table[b][k]."""
    past = L - q_len
    x = qkv.double().view(B, q_len, 3, H, HD)
    kcd, vcd = kc.double(), vc.double()
    if table is not None:
        idx = table[:, :past].long()  # [B][past]
        kcd = torch.stack([kcd[idx[b], :, torch.arange(past, device="cuda")].permute(1, 0, 2) for b in range(B)])
        vcd = torch.stack([vcd[idx[b], :, torch.arange(past, device="cuda")].permute(1, 0, 2) for b in range(B)])
    k_all = torch.cat([kcd[:, :, :past], x[:, :, 1].permute(0, 2, 1, 3)], 2)
    v_all = torch.cat([vcd[:, :, :past], x[:, :, 2].permute(0, 2, 1, 3)], 2)
    q = x[:, :, 0].permute(0, 2, 1, 3)
    s = q @ k_all.transpose(-1, -2)  # [B][H][q_len][L]
    kpos = torch.arange(L, device="cuda")[None, None, :]
    qpos = (torch.arange(q_len, device="cuda") + past)[None, :, None]
    keep = (kpos <= qpos) & (kpos >= _i32(list(ks)).long()[:, None, None])  # [B][q_len][L]
    s = s.masked_fill(~keep[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(keep.any(-1)[:, None, :, None], p, torch.zeros_like(p))  # (a row of -inf: softmax gives NaN)
    ref = (p @ v_all).permute(0, 2, 1, 3).reshape(B * q_len, D)
    return ref, keep.any(-1).reshape(B * q_len)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q_len,L", SHAPES)
def test_zero_key_start_is_the_unmasked_kernel(dtype, q_len, L):
    """key_start all zero: bitwise kw_self_attn_step -- the f32 engine (parity mode) at every q_len, bf16 at q_len 1
    and, with the per-query form selected (KW_SELF_ATTN_PER_QUERY), in the prefill.  The bf16 prefill's default, the
    MFMA tile kernel, sums in another order: within the dtype's tolerance of kw_self_attn_step, caches bitwise."""
    qkv, kc, vc = _inputs(dtype, q_len, L)
    o0, k0, v0 = _unmasked(qkv, kc, vc, q_len, L)
    o1, k1, v1 = _masked(qkv, kc, vc, q_len, L, [0] * B, per_query=True)
    assert torch.equal(o1.view(torch.uint8), o0.view(torch.uint8))
    assert torch.equal(k1, k0) and torch.equal(v1, v0)
    o2, k2, v2 = _masked(qkv, kc, vc, q_len, L, [0] * B)
    assert torch.equal(k2, k0) and torch.equal(v2, v0)
    if dtype == torch.bfloat16 and q_len > 1:
        torch.testing.assert_close(o2.float(), o0.float(), atol=TOL[dtype], rtol=TOL[dtype])
    else:
        assert torch.equal(o2.view(torch.uint8), o0.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q_len,L,ks", CASES)
def test_against_float64_mask(dtype, q_len, L, ks):
    qkv, kc, vc = _inputs(dtype, q_len, L)
    out, k1, v1 = _masked(qkv, kc, vc, q_len, L, ks)
    ref, has_key = _reference(qkv, kc, vc, q_len, L, ks)
    assert torch.isfinite(out.float()).all()
    torch.testing.assert_close(out.double(), ref, atol=TOL[dtype], rtol=TOL[dtype])
    # pad queries: exactly zero (never NaN)
    assert (out[~has_key] == 0).all()
    assert int((~has_key).sum()) == sum(min(max(s - (L - q_len), 0), q_len) for s in ks)
    # the appended K/V: the unmasked kernel's bits, for every row (pads included)
    _, k0, v0 = _unmasked(qkv, kc, vc, q_len, L)
    assert torch.equal(k1, k0) and torch.equal(v1, v0)
    # whatever sits below key_start is not read: NaN there (cached rows, and the new rows' q / k / v of a prefill)
    past = L - q_len
    kc2, vc2, qkv2 = kc.clone(), vc.clone(), qkv.clone().view(B, q_len, 3 * D)
    for b, s in enumerate(ks):
        kc2[b, :, :min(s, past)] = float("nan")
        vc2[b, :, :min(s, past)] = float("nan")
        if s > past:
            qkv2[b, :min(s - past, q_len)] = float("nan")
    out2, _, _ = _masked(qkv2.view(B * q_len, 3 * D), kc2, vc2, q_len, L, ks)
    assert torch.equal(out2.view(torch.uint8), out.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [2, 200, 300])
def test_slot_table_with_key_start(dtype, L):
    """bp and key_start together (q_len 1): rows 0 and 1 are the two beams of one item and read their cached
    positions from each other's cache rows in turn; row 2 reads its own."""
    qkv, kc, vc = _inputs(dtype, 1, L, seed=5)
    table = torch.arange(B, device="cuda", dtype=torch.int32)[:, None].repeat(1, T_MAX).contiguous()
    pos = torch.arange(T_MAX, device="cuda")
    table[0] = (pos % 2).int()
    table[1] = ((pos // 3) % 2).int()
    for ks in _key_starts(1, L):
        out, _, _ = _masked(qkv, kc, vc, 1, L, ks, bp=table)
        ref, _ = _reference(qkv, kc, vc, 1, L, ks, table=table)
        torch.testing.assert_close(out.double(), ref, atol=TOL[dtype], rtol=TOL[dtype])
    o1, _, _ = _masked(qkv, kc, vc, 1, L, [0] * B, bp=table)
    o0, _, _ = _unmasked(qkv, kc, vc, 1, L, bp=table)
    assert torch.equal(o1.view(torch.uint8), o0.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q_len,L", [(1, 300), (33, 33), (70, 70)])
def test_batch_invariance(dtype, q_len, L):
    """A row's output with B = 3 is its output alone, bit for bit."""
    qkv, kc, vc = _inputs(dtype, q_len, L, seed=9)
    ks = _key_starts(q_len, L)[1]
    out, _, _ = _masked(qkv, kc, vc, q_len, L, ks)
    for b in range(B):
        o1, _, _ = _masked(qkv[b * q_len:(b + 1) * q_len].contiguous(), kc[b:b + 1], vc[b:b + 1], q_len, L, [ks[b]],
                           rows=1)
        assert torch.equal(o1.view(torch.uint8), out[b * q_len:(b + 1) * q_len].view(torch.uint8)), b


def test_rejects_bad_arguments():
    qkv, kc, vc = _inputs(torch.float32, 2, 2)
    out = torch.empty(B * 2, D, device="cuda")
    table = torch.zeros(B, T_MAX, device="cuda", dtype=torch.int32)
    with pytest.raises(ValueError):  # a slot table needs q_len == 1
        ops.self_attn_step_masked(qkv, B, 2, H, HD, kc, vc, T_MAX, _i32([2]), _i32([0] * B), out, _ws(), bp=table)
    with pytest.raises(ValueError):  # key_start: int32, one per row
        ops.self_attn_step_masked(qkv, B, 2, H, HD, kc, vc, T_MAX, _i32([2]), _i32([0]), out, _ws())
