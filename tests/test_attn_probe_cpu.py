"""The per-key weight probe (tests/_attn_probe.py) on the CPU, over a plain torch attention written here: chunked,
merged with an online softmax, with optional bf16 rounding of P and of the output -- the structure of the decode
kernels.  The probe must reproduce float64 softmax within its bound, and must fail for each planted fault; the check
the suite had before (softmax(Q K^T) V against a reference at atol = rtol = 2e-2) passes one of them.
"""
import pytest
import torch

import _attn_probe as P


def _bf16(x):
    return x.bfloat16().double()


def chunked_attention(q, k, v, chunk=256, mask=None, round_p=False, round_out=False, fault=None, fault_chunk=0):
    """q [R][64], k / v [R][T][64] (each row's own keys: a slot table is resolved by the caller), mask [R][T] -> out
    [R][64].  float64 arithmetic with the explicit bf16 roundings.  Per chunk (m, l, o), merged in chunk order.
    ``fault`` (in chunk ``fault_chunk``): "drop_last" -- its last key is left out; "seam_twice" -- the next chunk's
    first key is counted here as well; "no_rescale" -- the chunk is merged without the exp(m - M) factors (a later
    chunk: the first has none); "admit_masked" -- the mask is ignored."""
    R, T, _ = k.shape
    q, k, v = q.double(), k.double(), v.double()
    s_all = torch.einsum("rd,rtd->rt", q, k)
    if mask is not None and fault != "admit_masked":
        s_all = s_all.masked_fill(~mask, float("-inf"))
    M = torch.full((R,), float("-inf"), dtype=torch.float64)
    Lr = torch.zeros(R, dtype=torch.float64)
    A = torch.zeros(R, 64, dtype=torch.float64)
    for c, k0 in enumerate(range(0, T, chunk)):
        k1 = min(T, k0 + chunk)
        hit = fault is not None and c == fault_chunk
        if hit and fault == "seam_twice":
            k1 = min(T, k1 + 1)
        s = s_all[:, k0:k1].clone()
        if hit and fault == "drop_last":
            s[:, -1] = float("-inf")
        m = s.max(-1).values
        safe = torch.where(torch.isfinite(m), m, torch.zeros_like(m))  # a chunk without a key: p = 0
        p = torch.exp(s - safe[:, None])
        l = p.sum(-1)
        o = torch.einsum("rt,rtd->rd", _bf16(p) if round_p else p, v[:, k0:k1])
        Mn = torch.maximum(M, m)
        ref = torch.where(torch.isfinite(Mn), Mn, torch.zeros_like(Mn))
        f0, f1 = torch.exp(M - ref), torch.exp(m - ref)
        if hit and fault == "no_rescale":
            f0, f1 = torch.ones_like(f0), torch.ones_like(f1)
        Lr = Lr * f0 + l * f1
        A = A * f0[:, None] + o * f1[:, None]
        M = Mn
    out = torch.where(Lr[:, None] > 0, A / Lr.clamp_min(1e-300)[:, None], torch.zeros_like(A))
    return out.bfloat16() if round_out else out


def _inputs(R, T, seed, spike=()):
    """The decode kernels' base set: K ~ N(0, 1), Q ~ N(0, 0.25^2), both bf16; ``spike``: keys with a score of 12."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(R, 64, generator=g) * 0.25
    k = torch.randn(R, T, 64, generator=g)
    for pos in spike:
        if 0 <= pos < T:
            k[:, pos] = P.plant_spike(q)
    return q.bfloat16().float(), k.bfloat16().float()


def _probe(q, k, T, **kw):
    R = q.shape[0]
    return P.probe_weights(lambda v: chunked_attention(q, k, v[None].expand(R, -1, -1), **kw), T)


@pytest.mark.parametrize("round_p,round_out", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("spike", [False, True])
@pytest.mark.parametrize("T", [1, 77, 300, 448, 1500])
def test_probe_reads_float64_softmax(T, spike, round_p, round_out):
    """The correct attention is within (n + 1) 2^-8 for n bf16 roundings, per key, at every length and with the
    weight on the structural positions (first and last key, both sides of the chunk seam)."""
    q, k = _inputs(4, T, 100 + T, spike=(0, 255, 256, T - 1) if spike else ())
    p_hat, same = _probe(q, k, T, round_p=round_p, round_out=round_out)
    n = int(round_p) + int(round_out)
    got = P.check_weights(p_hat, _ref(q, k), P.bf16_rtol(n) if n else 1e-9, repeatable=same)
    assert got <= (n * 2.0 ** -8 * 1.01 if n else 1e-9)  # the roundings alone: the bound's extra 2^-8 is unused here


def _ref(q, k, mask=None):
    """reference_weights for per-row keys k [R][T][64]: row r's weights over its own keys, [R][T]."""
    m = None if mask is None else mask[:, None, :]
    return P.reference_weights(q[:, None, :], k, m)[:, 0, :]


def test_masks_and_cache_tail():
    """A causal / key_start mask and a cache longer than the sequence: excluded keys read back as exact zeros, a row
    without a key sums to zero, and the ones in V past T (this block's cache slots) reach no column."""
    T, t_total, R = 70, 128, 5
    q, k = _inputs(R, T, 7)
    starts = torch.tensor([0, 1, 69, 70, 33])  # row 3 has no key
    mask = torch.arange(T)[None, :] >= starts[:, None]
    kc = torch.cat([k, torch.full((R, t_total - T, 64), float("nan"))], 1)

    def run(v, fault=None):
        assert v.shape == (t_total, 64)
        return chunked_attention(q, kc[:, :T], v[None, :T].expand(R, -1, -1), chunk=32, mask=mask, round_out=True,
                                 fault=fault)

    p_hat, same = P.probe_weights(run, T, t_total)
    assert p_hat.shape == (R, 128)
    P.check_weights(p_hat, _ref(q, k, mask), P.bf16_rtol(1), mask=mask, repeatable=same)
    assert (p_hat[3] == 0).all() and (P.unit_values(T, 1, t_total)[T:] == 1).all()
    # a kernel that reads one slot past T: the ones of that slot land in every column of the last block
    def past_end(v):
        vv = v[None, :T + 1].expand(R, -1, -1)
        kk = torch.cat([k, k[:, :1]], 1)
        mm = torch.cat([mask, mask[:, :1]], 1)
        return chunked_attention(q, kk, vv, chunk=32, mask=mm, round_out=True)

    p_bad, same = P.probe_weights(past_end, T, t_total)
    with pytest.raises(AssertionError):
        P.check_weights(p_bad, _ref(q, k, mask), P.bf16_rtol(1), mask=mask, repeatable=same)


FAULTS = ["drop_last", "seam_twice", "no_rescale", "admit_masked"]


@pytest.mark.parametrize("spike", [False, True])
@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_fail_the_probe(fault, spike):
    """Each fault at the seam of a 300-key row (chunks of 256, the self-attention step's; the faults of a chunk's end
    in chunk 0, the merge without rescale in chunk 1), MFMA-style roundings (n = 2): the probe fails, whether the
    weight sits on the seam or anywhere else."""
    T, R = 300, 3
    # (two equal spikes on both sides of the seam give both chunks one maximum: nothing to rescale, so that fault
    # gets the spike on one side only)
    q, k = _inputs(R, T, 11, spike=((255,) if fault == "no_rescale" else (255, 256)) if spike else ())
    mask = torch.ones(R, T, dtype=torch.bool)
    mask[:, :2] = False  # key_start 2
    ref = _ref(q, k, mask)
    kw = dict(mask=mask, round_p=True, round_out=True)
    p_ok, same = _probe(q, k, T, **kw)
    P.check_weights(p_ok, ref, P.bf16_rtol(2), mask=mask, repeatable=same)
    p_bad, same = _probe(q, k, T, fault=fault, fault_chunk=1 if fault == "no_rescale" else 0, **kw)
    assert same
    with pytest.raises(AssertionError):
        P.check_weights(p_bad, ref, P.bf16_rtol(2), mask=mask, repeatable=same)


def test_wrong_slot_table_row_fails_the_probe():
    """A beam row reads position t from cache row table[b][t].  Cache rows hold different K, and the unit vectors
    of V sit only in the cache row the table names: a kernel that takes V of one position from its own row instead
    reads a zero there and the probe fails (K from the wrong row changes the weight itself)."""
    T, B = 300, 3
    g = torch.Generator().manual_seed(5)
    q = (torch.randn(B, 64, generator=g) * 0.25).bfloat16().float()
    kc = torch.randn(B, T, 64, generator=g).bfloat16().float()
    pos = torch.arange(T)
    table = torch.arange(B)[:, None].repeat(1, T)
    table[0], table[1] = pos % 2, (pos // 3) % 2
    k_rows = kc[table, pos[None, :]]  # [B][T][64]

    def run(v, wrong_at=None):
        vc = torch.zeros(B, T, 64)
        for b in range(B):
            vc[table[b], pos] = v
        t2 = table.clone()
        if wrong_at is not None:
            t2[0, wrong_at] = 0  # row 0 takes V of that position from its own cache row (the table says row 1)
        return chunked_attention(q, k_rows, vc[t2, pos[None, :]], round_out=True)

    ref = _ref(q, k_rows)
    p_hat, same = P.probe_weights(run, T)
    P.check_weights(p_hat, ref, P.bf16_rtol(1), repeatable=same)
    assert int(table[0, 257]) == 1
    p_bad, same = P.probe_weights(lambda v: run(v, wrong_at=257), T)
    with pytest.raises(AssertionError, match="key 257 in row 0"):
        P.check_weights(p_bad, ref, P.bf16_rtol(1), repeatable=same)


def test_unrepeatable_launch_fails_the_probe():
    q, k = _inputs(2, 100, 3)
    calls = []

    def run(v):
        calls.append(1)
        out = chunked_attention(q, k, v[None].expand(2, -1, -1), round_out=True)
        return out if len(calls) < 3 else (out.float() * (1 + 2.0 ** -7)).bfloat16()  # a stale workspace, say

    p_hat, same = P.probe_weights(run, 100)
    assert len(calls) == 3 and not same  # ceil(100 / 64) + 1 launches
    with pytest.raises(AssertionError, match="bit-identical"):
        P.check_weights(p_hat, _ref(q, k), P.bf16_rtol(1), repeatable=same)


def test_mixed_sum_check_misses_what_the_probe_finds():
    """test_cross_attn_step's bf16 inputs at S = 1500 (B 3, H 4: 12 rows; K, V ~ N(0, 1), Q ~ N(0, 0.3^2); six
    250-key chunks), the last key of chunk 3 (key 999) dropped from every row.  The check that test makes --
    softmax(Q K^T) V against the float64 reference at atol = rtol = 2e-2 -- passes; the probe fails.  With these
    inputs the loss of a key is noticed by that check (in any of the 12 rows) for 14 % of the 1500 key positions."""
    S, R, chunk = 1500, 12, 250
    g = torch.Generator().manual_seed(0)
    k = torch.randn(R, S, 64, generator=g).bfloat16().float()
    v = torch.randn(R, S, 64, generator=g).bfloat16().float()
    q = (torch.randn(R, 64, generator=g) * 0.3).bfloat16().float()
    ref_p = _ref(q, k)
    ref_out = torch.einsum("rt,rtd->rd", ref_p, v.double())
    good = chunked_attention(q, k, v, chunk=chunk, round_out=True)
    bad = chunked_attention(q, k, v, chunk=chunk, round_out=True, fault="drop_last", fault_chunk=3)
    assert P.is_close_mixed(good, ref_out, 2e-2)
    assert not torch.equal(good, bad)
    assert P.is_close_mixed(bad, ref_out, 2e-2), "the mixed-sum check was expected to miss the dropped key"
    run = lambda fault: P.probe_weights(  # noqa: E731
        lambda u: chunked_attention(q, k, u[None].expand(R, -1, -1), chunk=chunk, round_out=True, fault=fault,
                                    fault_chunk=3), S)
    p_hat, same = run(None)
    P.check_weights(p_hat, ref_p, P.bf16_rtol(1), repeatable=same)
    p_hat, same = run("drop_last")
    with pytest.raises(AssertionError, match="weight of key 999 in row 0 is 0,"):
        P.check_weights(p_hat, ref_p, P.bf16_rtol(1), repeatable=same)
    # every key position in turn removed from the float64 reference and renormalised, under the same mixed-sum check
    without = (ref_out[:, None, :] - ref_p[:, :, None] * v.double()) / (1 - ref_p)[:, :, None]  # [R][S][64]
    err = (without - ref_out[:, None, :]).abs()
    noticed = (err > 2e-2 + 2e-2 * ref_out[:, None, :].abs()).any(-1).any(0)  # per key position, over all rows
    assert 0.10 < float(noticed.double().mean()) < 0.20  # 0.144 with this seed
