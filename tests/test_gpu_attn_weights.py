"""Every attention kernel's softmax weights, key by key, against float64 softmax (the probe of tests/_attn_probe.py).

The other attention tests compare softmax(Q K^T) V on random inputs at atol = rtol = 2e-2: a mixture of keys in which,
at the decoder's real lengths, nine keys in ten weigh less than the tolerance (tests/test_attn_probe_cpu.py records
it).  Here V holds unit vectors, so each launch returns the weights of 64 keys, one per output column, and every key
of every row is checked on its own: relative error within the kernel's bound, exact zeros on excluded keys (causal
and key_start masks, cache slots past the sequence -- K is NaN there and V holds ones), row sums, and a repeated first
launch that must be bit-identical on the shared, once-zeroed workspace.

Inputs (seeded): the base set K ~ N(0, 1), Q ~ N(0, 0.25^2) for the decode kernels (the encoder keeps its 0.5 scales);
the spike set plants keys with a score of 12 on the structural positions of each kernel (first and last key, both
sides of a chunk / tile seam, the last valid key of a ragged tile); the ramp set scales key t by 1 + a t / T so that
the running maximum moves in most tiles.  For the bf16 encoder kernels a = 2 keeps every weight a normal number and
a = 20 spreads the scores over hundreds, checked above the probe's underflow floor.  The f32 kernel gets a = 0.5: the
relative error of an f32 weight is the absolute error of its exponent s - m, which is a handful of roundings of half
an ulp each -- ulp 2^-20 while |s| < 16 and 2^-19 while |s - m| < 32, which is where 1e-5 can hold, and where the
base and spike sets (|s| <= 12, s - m >= -20) and a score deviation of 2 (1 + 0.5) over 1500 x 1500 scores stay.
(At a = 2, scores to +-37, attn_fwd_f32 measured 1.14e-5: f32 arithmetic, not a fault -- profiles/attn_key_weights.md.)

Dispatch notes (kw_cross_attn_step, no code changed for them):
  * KW_CROSS_MFMA_MIN_Q is 5, so the cross_attn_multi_kernel<bf16, 8> branch is unreachable in the default build:
    q_len 2..4 run cross_attn_multi_kernel<bf16, 4>, q_len >= 5 cross_attn_mfma_kernel;
  * the f32 path takes cross_attn_kernel<float> for every q_len;
  * no case here needs a build flag or an environment switch: the KW_CROSS_ROW=0 form of the pair-kernel shapes
    (the chunk grid at >= one pair per CU) is left out for that reason;
  * S = 1345 splits into chunks of 225 with a last chunk of 220 keys, which neither row_groups_ok() nor dma_ok()
    accepts: at the pair kernel's row count it runs cross_attn_kernel<bf16> and is tested as that.  The pair kernel's
    shortest chunks (225 keys, one key in group ROW_JV) are S = 1350.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kwhisper import _lib as L  # noqa: E402
from kwhisper import ops  # noqa: E402

import _attn_probe as P  # noqa: E402
import _fp8_ref as R  # noqa: E402

# ------------------------------------------------------------------------------------------------
# The bound of every kernel: n = the values rounded to bf16 between a score and the output (rtol = (n + 1) 2^-8),
# with the place of each rounding in kotoba-whisper_amd/csrc; f32 kernels: the project's 1e-5.
# ------------------------------------------------------------------------------------------------
F32_RTOL = 1e-5
N_BF16 = {
    # encoder
    "attn_fwd_bf16": 2,  # attention.hip attn_fwd_bf16: pf[i][s][e] = (__bf16)p; os[..] = f2bf(o * inv_l)
    "attn_fwd_l2": 2,  # attention.hip attn_fwd_l2: pf[i][s][e] = (__bf16)p; os[..] = f2bf(o * inv_l)
    # decoder self-attention
    "self_attn_step1<bf16,false>": 1,  # attend_chunk keeps p f32; TypeIO<bf16_t>::st(o / l) (publish_and_combine)
    "self_attn_step1<bf16,true>": 1,  # the same body, rows through the slot table
    "self_attn_step<bf16>": 1,  # attend_rows keeps p f32 in LDS; TypeIO<T>::st(out, o / l)
    "self_attn_step1_masked<bf16>": 1,  # self_attn_step1's body from key_start: TypeIO<T>::st(orow, o / l)
    "self_attn_prefill_masked<bf16>": 1,  # attend_rows; TypeIO<T>::st(orow + tid, o / l)
    "self_attn_prefill_masked_mfma": 2,  # pf[j] = (__bf16)p[..]; orow[..] = f2bf(o[dt][r] * inv)
    # decoder cross-attention
    "cross_attn_kernel<bf16>": 1,  # attend_chunk (wave_row_bf16: p f32); publish_and_combine's TypeIO<T>::st
    "cross_attn_dma_kernel": 1,  # wave_row_bf16; wave_partials_combine's TypeIO<bf16_t>::st(out_el, o / l)
    "cross_attn_row_kernel<false,6>": 1,  # wave_values_bf16 / row_fold f32; TypeIO<bf16_t>::st(p.out, o / l)
    "cross_attn_multi_kernel<bf16,4>": 1,  # wave_row_bf16; TypeIO<T>::st(orow + dd, ot / lt)
    "cross_attn_mfma_kernel": 2,  # pf[i][s][e] = (__bf16)p; orow[e] = f2bf(ot * inv)
    "cross_attn_row_fp8_kernel": 1,  # codes decode exactly, scales multiply in f32; st(o * vs / l)
}
F32_KERNELS = ["attn_fwd_f32", "self_attn_step1<float,false>", "self_attn_step1<float,true>", "self_attn_step<float>",
               "self_attn_step1_masked<float>", "self_attn_prefill_masked<float>", "cross_attn_kernel<float>"]


def rtol_of(kernel):
    return P.bf16_rtol(N_BF16[kernel]) if kernel in N_BF16 else F32_RTOL


assert not set(N_BF16) & set(F32_KERNELS)

HD = 64
BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF16]
_MEASURED = {}  # kernel -> [max relative error, cases]


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    yield
    lines = ["| kernel | n | bound | measured max relative error | cases |", "|---|---|---|---|---|"]
    for kernel in list(N_BF16) + F32_KERNELS:
        if kernel in _MEASURED:
            worst, cases = _MEASURED[kernel]
            lines.append(f"| `{kernel}` | {N_BF16.get(kernel, '-')} | {rtol_of(kernel):.3g} | {worst:.3g} | {cases} |")
    print("\n".join(lines))
    path = os.environ.get("KW_ATTN_WEIGHTS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


def _i32(x):
    return torch.tensor(x, device="cuda", dtype=torch.int32)


def _tname(dtype):
    return "float" if dtype == F32 else "bf16"


def _verify(kernel, case, run, T, p_ref, mask=None, t_total=None, floor=0.0):
    """Probe, print the figures, then assert (the figures of a failing case are in the output)."""
    p_hat, same = P.probe_weights(run, T, t_total, device="cuda")
    p_ref = p_ref.reshape(-1, T)
    mask = None if mask is None else mask.reshape(-1, T)
    max_rel, bad_zero, sum_err, empty, under = P.weight_errors(p_hat, p_ref, mask, floor)
    rtol = rtol_of(kernel)
    print(f"{kernel} {case}: rows {p_ref.shape[0]} keys {T} max rel {max_rel:.3g} (bound {rtol:.3g}) nonzero-excluded "
          f"{bad_zero} row-sum err {sum_err:.3g} empty-row sum {empty:.3g} repeatable {same}")
    rec = _MEASURED.setdefault(kernel, [0.0, 0])
    rec[0], rec[1] = max(rec[0], max_rel), rec[1] + 1
    P.check_weights(p_hat, p_ref, rtol, mask=mask, repeatable=same, floor=floor, what=f"{kernel} {case}")


# ------------------------------------------------------------------------------------------------ encoder
ENC_T = [1, 63, 64, 65, 128, 129, 200]
# the ramps of each variant (module docstring: an f32 kernel's bound of 1e-5 holds only while scores stay small)
ENC_RAMPS = {"bf16": ["ramp2", "ramp20"], "q_log2": ["ramp2", "ramp20"], "f32": ["ramp0.5"]}
ENC_CASES = [(v, 2, 2, T, kind) for v in ENC_RAMPS for T in ENC_T for kind in ["base", "spike"] + ENC_RAMPS[v]]
ENC_CASES += [(v, 1, 1, 1500, kind) for v in ENC_RAMPS for kind in ["spike"] + ENC_RAMPS[v]]  # 24 key, 12 query tiles


@pytest.mark.parametrize("variant,B,H,T,kind", ENC_CASES)
def test_attention(variant, B, H, T, kind):
    """ops.attention -> attn_fwd_bf16 / attn_fwd_l2 / attn_fwd_f32: AK = 64 key tiles and AQ = 128 query tiles with
    the ragged last tile of each (T = 63, 65, 129, 200), one key, and 1500 keys once.  Spikes on keys 0, 63, 64, T - 1
    (each for a query of its own)."""
    kernel = {"bf16": "attn_fwd_bf16", "q_log2": "attn_fwd_l2", "f32": "attn_fwd_f32"}[variant]
    dtype = F32 if variant == "f32" else BF16
    g = _gen(1000 * T + B)
    q = _randn(g, B, H, T, HD) * 0.5
    k = _randn(g, B, H, T, HD) * 0.5
    if kind == "spike":
        for pos in sorted({0, 63, 64, T - 1}):
            if pos < T:
                k[:, :, pos] = P.plant_spike(q[:, :, (7 * pos + 3) % T])
    if kind.startswith("ramp"):
        k *= P.ramp(T, float(kind[4:]), device="cuda")
    if variant == "q_log2":
        q = q * P.LOG2E
    qkv = torch.stack([q, k, torch.zeros_like(k)]).to(dtype).contiguous()
    out = torch.full((B, T, H * HD), float("nan"), device="cuda", dtype=dtype)

    def run(v):
        qkv[2] = v[:T].to(dtype)
        ops.attention(qkv, B, H, T, HD, out, q_log2=variant == "q_log2")
        return out.view(B, T, H, HD).permute(0, 2, 1, 3).reshape(-1, HD)

    ref = P.reference_weights(qkv[0], qkv[1], q_log2=variant == "q_log2")
    _verify(kernel, f"T={T} {kind}", run, T, ref, floor=P.UNDERFLOW_FLOOR if kind == "ramp20" else 0.0)


# ------------------------------------------------------------------------------------------------ self-attention
def _self_inputs(g, B, H, q_len, L, dtype, spikes):
    """Q [B][H][q_len][64] ~ N(0, 0.25^2) and K of positions 0 .. L - 1 [B][H][L][64] ~ N(0, 1), in ``dtype``.
    ``spikes``: (b or None, key position, query index) -- that key scores 12 against that query."""
    q = _randn(g, B, H, q_len, HD) * 0.25
    k = _randn(g, B, H, L, HD)
    for b, pos, qi in spikes:
        if 0 <= pos < L:
            rows = slice(None) if b is None else slice(b, b + 1)
            k[rows, :, pos] = P.plant_spike(q[rows, :, qi])
    return q.to(dtype), k.to(dtype)


class _SelfCase:
    """The buffers of one self-attention case: qkv rows [B q_len][3 d] (q, k of the new positions), the K cache (the
    past positions; NaN from the first new position on -- the kernel appends the new rows, whatever lies past L stays
    NaN) and the V cache / qkv V rows that each launch fills from the probe's values."""

    def __init__(self, q, k_all, t_max, table=None, k_cache_rows=None):
        self.B, self.H, self.q_len, _ = q.shape
        self.L, self.t_max, self.dtype = k_all.shape[2], t_max, q.dtype
        B, H, q_len, L = self.B, self.H, self.q_len, self.L
        self.past, self.d = L - q_len, H * HD
        self.table = table
        self.qkv = torch.zeros(B * q_len, 3 * self.d, device="cuda", dtype=self.dtype)
        v5 = self.qkv.view(B, q_len, 3, H, HD)
        v5[:, :, 0] = q.permute(0, 2, 1, 3)
        v5[:, :, 1] = k_all[:, :, self.past:].permute(0, 2, 1, 3)
        self.kc = torch.full((B, H, t_max, HD), float("nan"), device="cuda", dtype=self.dtype)
        self.kc[:, :, :self.past] = k_all[:, :, :self.past] if k_cache_rows is None else k_cache_rows[:, :, :self.past]
        self.vc = torch.zeros_like(self.kc)
        self.out = torch.full((B * q_len, self.d), float("nan"), device="cuda", dtype=self.dtype)
        self.ws = torch.zeros(ops.self_attn_workspace_bytes(B, H, t_max) // 4 + 1, device="cuda")
        self.cur = _i32([L])

    def fill_values(self, v):
        """v [t_max][64]: the cache rows (through the slot table: only the cache row it names holds position k's
        values, the others zeros) and the new positions' rows of qkv."""
        vd = v.to(self.dtype)
        if self.table is None:
            self.vc[:] = vd
        else:
            self.vc.zero_()
            pos = torch.arange(self.t_max, device="cuda")
            for b in range(self.B):
                self.vc[self.table[b].long(), :, pos] = vd[:, None, :]
        self.qkv.view(self.B, self.q_len, 3, self.H, HD)[:, :, 2] = vd[self.past:self.L][None, :, None, :]

    def rows(self):
        return self.out.view(self.B, self.q_len, self.H, HD).reshape(-1, HD)


def _rows_bqh(p):
    """[B][H][q_len][T] -> the kernels' output row order (b, query, head)."""
    return p.permute(0, 2, 1, 3).reshape(-1, p.shape[-1])


STEP1_LENGTHS = [(448, 1), (448, 2), (448, 255), (448, 256), (448, 257), (448, 300), (448, 448), (512, 512)]


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("t_max,L", STEP1_LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_self_attn_step1(dtype, t_max, L, kind):
    """ops.self_attn_step, q_len 1 -> self_attn_step1<T, false>: one and two 256-key chunks, the seam, the appended
    key (L - 1, read from the qkv row), t_max = L = 512 (the documented limit).  Spikes on 0, 255, 256, L - 2, L - 1."""
    B, H = 2, 2
    spikes = [(None, pos, 0) for pos in (0, 255, 256, L - 2, L - 1)] if kind == "spike" else []
    q, k_all = _self_inputs(_gen(10 * L + 1), B, H, 1, L, dtype, spikes)
    c = _SelfCase(q, k_all, t_max)

    def run(v):
        c.fill_values(v)
        ops.self_attn_step(c.qkv, B, 1, H, HD, c.kc, c.vc, t_max, c.cur, c.out, c.ws)
        return c.rows()

    _verify(f"self_attn_step1<{_tname(dtype)},false>", f"t_max={t_max} L={L} {kind}", run, L,
            _rows_bqh(P.reference_weights(q, k_all)), t_total=t_max)
    assert torch.equal(c.kc[:, :, L - 1], k_all[:, :, L - 1]) and not torch.isfinite(c.kc[:, :, L:].float()).any()


def _slot_table(B, t_max):
    """tests/test_gpu_self_attn_masked.py::test_slot_table_with_key_start's: rows 0 and 1 read their cached positions
    from each other's cache rows in turn, row 2 reads its own."""
    table = torch.arange(B, device="cuda", dtype=torch.int32)[:, None].repeat(1, t_max).contiguous()
    pos = torch.arange(t_max, device="cuda")
    table[0] = (pos % 2).int()
    table[1] = ((pos // 3) % 2).int()
    return table


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("L", [2, 257, 300])
@pytest.mark.parametrize("dtype", DTYPES)
def test_self_attn_step1_slot_table(dtype, L, kind):
    """The same with a beam slot table -> self_attn_step1<T, true>.  Cache rows hold different K; the unit vectors of
    V sit only in the cache row the table names, so a value taken from another row reads back as a zero weight."""
    B, H, t_max = 3, 2, 448
    table = _slot_table(B, t_max)
    g = _gen(20 * L + 3)
    q, k_new = _self_inputs(g, B, H, 1, L, dtype, [])
    k_cache = _randn(g, B, H, t_max, HD)
    if kind == "spike":
        for b in range(B):
            for pos in (255, 256):
                if pos < L - 1:
                    k_cache[int(table[b, pos]), :, pos] = P.plant_spike(q[b, :, 0].float())
    k_cache = k_cache.to(dtype)
    pos = torch.arange(L - 1, device="cuda")
    k_all = torch.stack([k_cache[table[b, :L - 1].long(), :, pos].permute(1, 0, 2) for b in range(B)])  # [B][H][L-1][64]
    k_all = torch.cat([k_all, k_new[:, :, L - 1:]], 2)
    c = _SelfCase(q, k_all, t_max, table=table, k_cache_rows=k_cache)

    def run(v):
        c.fill_values(v)
        ops.self_attn_step(c.qkv, B, 1, H, HD, c.kc, c.vc, t_max, c.cur, c.out, c.ws, bp=table)
        return c.rows()

    _verify(f"self_attn_step1<{_tname(dtype)},true>", f"L={L} {kind}", run, L,
            _rows_bqh(P.reference_weights(q, k_all)), t_total=t_max)


PREFILL = [(2, 0), (5, 10), (33, 0), (70, 0), (40, 300)]  # (q_len, past)


def _prefill_spikes(q_len, past):
    """Each query's own position; keys 31 and 32 (attend_rows' 32 key slots) for the last query."""
    return [(None, past + qi, qi) for qi in range(q_len)] + [(None, 31, q_len - 1), (None, 32, q_len - 1)]


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("q_len,past", PREFILL)
@pytest.mark.parametrize("dtype", DTYPES)
def test_self_attn_prefill(dtype, q_len, past, kind):
    """ops.self_attn_step, q_len > 1 -> self_attn_step<T>: attend_rows' rounds of 32 key slots x 4, the causal edge
    of every query (the later new positions hold unit vectors and must read back as exact zeros)."""
    B, H, t_max, L = 2, 2, 448, past + q_len
    q, k_all = _self_inputs(_gen(30 * L + q_len), B, H, q_len, L, dtype,
                            _prefill_spikes(q_len, past) if kind == "spike" else [])
    c = _SelfCase(q, k_all, t_max)

    def run(v):
        c.fill_values(v)
        ops.self_attn_step(c.qkv, B, q_len, H, HD, c.kc, c.vc, t_max, c.cur, c.out)
        return c.rows()

    mask = (torch.arange(L, device="cuda")[None, :] <= past + torch.arange(q_len, device="cuda")[:, None])[None, None]
    mask = mask.expand(B, H, q_len, L)
    _verify(f"self_attn_step<{_tname(dtype)}>", f"q_len={q_len} past={past} {kind}", run, L,
            _rows_bqh(P.reference_weights(q, k_all, mask)), mask=_rows_bqh(mask), t_total=t_max)


def _key_starts(q_len, L, B=3):
    """tests/test_gpu_self_attn_masked.py::_key_starts: rows drawn from {0, 1, q_len - 4, q_len - 1} (the step: {0, 1,
    L - 2}), as rotations over the 3 rows."""
    vals = [0, 1, L - 2] if q_len == 1 else [0, 1, q_len - 4, q_len - 1]
    vals = [max(v, 0) for v in vals]
    return [[vals[(i + r) % len(vals)] for i in range(B)] for r in range(len(vals))]


MASKED_SHAPES = [(1, 2), (1, 200), (1, 300), (2, 2), (5, 15), (33, 33), (70, 70), (40, 340)]  # (q_len, L)
MASKED_CASES = [(q, L_, tuple(ks)) for q, L_ in MASKED_SHAPES for ks in _key_starts(q, L_)]
MASKED_CASES += [(1, 2, (2, 0, 1)), (5, 15, (15, 12, 0))]  # rows that are still all pad: no key at all
# (KW_SELF_ATTN_PER_QUERY selects among the prefill kernels only: no per-query variant of the step)
MASKED_CASES = [(v, *c) for v in ("f32", "bf16", "bf16_per_query") for c in MASKED_CASES
                if not (v == "bf16_per_query" and c[0] == 1)]


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("variant,q_len,L,ks", MASKED_CASES)
def test_self_attn_masked(variant, q_len, L, ks, kind):
    """ops.self_attn_step_masked: the step (self_attn_step1_masked, chunks that start at key_start), the per-query
    prefill (self_attn_prefill_masked) and the bf16 MFMA prefill (16-query / 32-key tiles from key_start).  Row b
    attends [key_start[b], own position]: the keys below (K is NaN there in the cache) and the later new positions
    read back as exact zeros, a query without a key as a zero row.  Spikes on key_start[b], key_start[b] + 1 (for
    the last query) and on every query's own position."""
    dtype = F32 if variant == "f32" else BF16
    per_query = variant == "bf16_per_query"
    B, H, t_max, past = 3, 2, 448, L - q_len
    if q_len == 1:
        kernel = f"self_attn_step1_masked<{_tname(dtype)}>"
    elif dtype == BF16 and not per_query:
        kernel = "self_attn_prefill_masked_mfma"
    else:
        kernel = f"self_attn_prefill_masked<{_tname(dtype)}>"
    spikes = []
    if kind == "spike":
        spikes = [(None, past + qi, qi) for qi in range(q_len)]
        for b, s in enumerate(ks):
            spikes += [(b, s, q_len - 1), (b, s + 1, q_len - 1)]
    q, k_all = _self_inputs(_gen(40 * L + q_len + sum(ks)), B, H, q_len, L, dtype, spikes)
    c = _SelfCase(q, k_all, t_max)
    for b, s in enumerate(ks):
        c.kc[b, :, :min(s, past)] = float("nan")  # below key_start: never read
    key_start = _i32(list(ks))

    def run(v):
        c.fill_values(v)
        ops.self_attn_step_masked(c.qkv, B, q_len, H, HD, c.kc, c.vc, t_max, c.cur, key_start, c.out, c.ws,
                                  per_query=per_query)
        return c.rows()

    kpos = torch.arange(L, device="cuda")[None, None, None, :]
    qpos = (past + torch.arange(q_len, device="cuda"))[None, None, :, None]
    mask = ((kpos <= qpos) & (kpos >= key_start.long()[:, None, None, None])).expand(B, H, q_len, L)
    _verify(kernel, f"q_len={q_len} L={L} ks={ks} {kind}", run, L, _rows_bqh(P.reference_weights(q, k_all, mask)),
            mask=_rows_bqh(mask), t_total=t_max)


# ------------------------------------------------------------------------------------------------ cross-attention
class CrossGeo:
    """attention.hip's CrossGeo restated: ns = ceil(S / 256) chunks of chunk = ceil(S / ns) keys, the last of `last`."""
    ROW_JV, ROW_NS = 7, 6

    def __init__(self, S):
        self.S = S
        self.ns = max(-(-S // 256), 1)
        self.chunk = -(-S // self.ns)
        self.last = S - (self.ns - 1) * self.chunk

    def dma_ok(self):  # the chunk grid issues all 8 key groups of a chunk: the last group must hold a valid key
        return 224 < self.chunk <= 256 and self.last > 224

    def row_groups_ok(self):  # the pair kernel checks only key group ROW_JV against the chunk end
        return self.chunk > 32 * self.ROW_JV and self.last > 32 * self.ROW_JV

    def seams(self):
        """Every chunk's first and last key, and S - 1."""
        s = set()
        for c in range(self.ns):
            s |= {c * self.chunk, min((c + 1) * self.chunk, self.S) - 1}
        return sorted(s | {self.S - 1})


DMA_S = [225, 256, 1399, 1500, 1536, 2048]  # dma_ok(): cross_attn_dma_kernel
REG_S = [1, 77, 224, 257, 600]  # not dma_ok(): cross_attn_kernel<bf16>


def test_cross_geo_names_the_kernels():
    assert all(CrossGeo(S).dma_ok() for S in DMA_S) and not any(CrossGeo(S).dma_ok() for S in REG_S)
    g = CrossGeo(1345)
    assert (g.ns, g.chunk, g.last) == (6, 225, 220) and not g.row_groups_ok() and not g.dma_ok()
    g = CrossGeo(1350)
    assert (g.ns, g.chunk, g.last) == (6, 225, 225) and g.row_groups_ok()
    assert CrossGeo(1500).row_groups_ok() and CrossGeo(1500).chunk == 250


def _pair_rows():
    """The smallest B with B H >= CUs at H = 20: the pair kernel's lower row limit."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return -(-cus // 20), 20


class _CrossCase:
    def __init__(self, g, B, q_len, H, S, dtype, spike_pos, kq_dtype=None):
        self.B, self.q_len, self.H, self.S, self.dtype = B, q_len, H, S, dtype
        q = _randn(g, B, H, q_len, HD) * 0.25
        k = _randn(g, B, H, S, HD)
        for i, pos in enumerate(spike_pos):
            if 0 <= pos < S:
                k[:, :, pos] = P.plant_spike(q[:, :, i % q_len])
        self.q, self.k = q.to(dtype), k.to(dtype).contiguous()
        self.qrows = self.q.permute(0, 2, 1, 3).reshape(B * q_len, H * HD).contiguous()
        self.v = torch.zeros_like(self.k)
        self.out = torch.full((B * q_len, H * HD), float("nan"), device="cuda", dtype=dtype)
        self.ws = torch.zeros(ops.cross_attn_workspace_bytes(B, q_len, H, HD, S) // 4 + 1, device="cuda")

    def run(self, v):
        self.v[:] = v[:self.S].to(self.dtype)
        ops.cross_attn_step(self.qrows, self.B, self.q_len, self.H, HD, self.k, self.v, self.S, self.out, self.ws)
        return self.out.view(-1, HD)

    def verify(self, kernel, case):
        _verify(kernel, case, self.run, self.S, _rows_bqh(P.reference_weights(self.q, self.k)))
        if kernel in ("cross_attn_dma_kernel", "cross_attn_row_kernel<false,6>"):  # granules re-armed / untouched
            assert int(self.ws.view(torch.int32).abs().sum()) == 0, "the workspace is not left zero"


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("q_len,S", [(1, 1), (1, 77), (1, 256), (1, 257), (1, 1500), (1, 2048), (3, 257)])
def test_cross_attn_f32(q_len, S, kind):
    """ops.cross_attn_step, f32 -> cross_attn_kernel<float>: one chunk, ragged chunks, eight chunks (the limit); once
    with three query rows per item, which the f32 path gives to the same kernel."""
    geo = CrossGeo(S)
    spikes = [0, geo.chunk - 1, geo.chunk, S - 1] if kind == "spike" else []
    _CrossCase(_gen(50 + S + q_len), 2, q_len, 2, S, F32, spikes).verify("cross_attn_kernel<float>",
                                                                          f"q_len={q_len} S={S} {kind}")


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("S", DMA_S + REG_S)
def test_cross_attn_bf16_chunk_grid(S, kind):
    """q_len 1, bf16, fewer pairs than CUs: cross_attn_dma_kernel where every chunk fills its 8 key groups, else
    cross_attn_kernel<bf16>.  Spikes on every chunk's first and last key."""
    geo = CrossGeo(S)
    assert not ops.cross_attn_pair_kernel(2 * 2, S)
    kernel = "cross_attn_dma_kernel" if geo.dma_ok() else "cross_attn_kernel<bf16>"
    _CrossCase(_gen(60 + S), 2, 1, 2, S, BF16, geo.seams() if kind == "spike" else []).verify(kernel, f"S={S} {kind}")


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("S", [1500, 1350])
def test_cross_attn_bf16_pair_kernel(S, kind):
    """q_len 1, bf16, one pair per CU or more -> cross_attn_row_kernel<false, 6>, every row probed: six chunks of 250
    keys, and of 225 (one key in group ROW_JV, the only group checked against the chunk end).  Spikes on both sides of
    the first seam, the last key, and the first and last key of group ROW_JV of chunk 2."""
    B, H = _pair_rows()
    geo = CrossGeo(S)
    assert ops.cross_attn_pair_kernel(B * H, S)
    spikes = [geo.chunk - 1, geo.chunk, S - 1, 2 * geo.chunk + 32 * geo.ROW_JV, 3 * geo.chunk - 1]
    _CrossCase(_gen(70 + S), B, 1, H, S, BF16, spikes if kind == "spike" else []).verify(
        "cross_attn_row_kernel<false,6>", f"S={S} rows={B * H} {kind}")


def test_cross_attn_bf16_1345_at_pair_rows():
    """S = 1345 at the pair kernel's row count: its last chunk of 220 keys fits neither the pair kernel nor the DMA
    chunk grid (module docstring), so the dispatch must fall to cross_attn_kernel<bf16>."""
    B, H = _pair_rows()
    geo = CrossGeo(1345)
    assert not ops.cross_attn_pair_kernel(B * H, 1345) and not geo.dma_ok()
    _CrossCase(_gen(71), B, 1, H, 1345, BF16, geo.seams()).verify("cross_attn_kernel<bf16>", f"S=1345 rows={B * H} spike")


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("S", [77, 1500])
@pytest.mark.parametrize("q_len", [2, 3, 4])
def test_cross_attn_bf16_multi(q_len, S, kind):
    """q_len 2 .. 4 -> cross_attn_multi_kernel<bf16, 4>: the rows of an item share one K / V pass."""
    geo = CrossGeo(S)
    _CrossCase(_gen(80 + S + q_len), 2, q_len, 2, S, BF16, geo.seams() if kind == "spike" else []).verify(
        "cross_attn_multi_kernel<bf16,4>", f"q_len={q_len} S={S} {kind}")


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("S", [64, 65, 300, 1500])
@pytest.mark.parametrize("q_len", [5, 32, 33])
def test_cross_attn_bf16_mfma(q_len, S, kind):
    """q_len >= 5 -> cross_attn_mfma_kernel: 64-key wave tiles, 4 waves per chunk (waves without a key at S = 64, 65),
    32-row groups with a ragged second group (33)."""
    geo = CrossGeo(S)
    spikes = [63, 64, geo.chunk - 1, geo.chunk, S - 1] if kind == "spike" else []
    _CrossCase(_gen(90 + S + q_len), 2, q_len, 2, S, BF16, spikes).verify(
        "cross_attn_mfma_kernel", f"q_len={q_len} S={S} {kind}")


@pytest.mark.parametrize("kind", ["base", "spike"])
@pytest.mark.parametrize("B,H,q_len,S", [(2, 6, 1, 1500), (3, 4, 4, 1500), (2, 6, 1, 1399), (2, 6, 1, 1536)])
def test_cross_attn_fp8(B, H, q_len, S, kind):
    """ops.cross_attn_step_fp8 -> cross_attn_row_fp8_kernel.  K: the dequantised codes the kernel reads.  V: the unit
    vectors go through ops.cross_kv_quant (code 448 times scale 1 / 448; all-zero channels get scale 0)."""
    geo = CrossGeo(S)
    g = _gen(100 + S + q_len)
    q = _randn(g, B, H, q_len, HD) * 0.25
    k = _randn(g, B, H, S, HD)
    if kind == "spike":
        for i, pos in enumerate([geo.chunk - 1, geo.chunk, S - 1, 2 * geo.chunk + 32 * geo.ROW_JV, 3 * geo.chunk - 1]):
            k[:, :, pos] = P.plant_spike(q[:, :, i % q_len])
    q, k = q.bfloat16(), k.bfloat16().contiguous()
    kcodes = torch.empty(B, H, S, HD, device="cuda", dtype=torch.uint8)
    kscale = torch.empty(B, H, HD, device="cuda")
    ops.cross_kv_quant(k, kcodes, kscale)
    k_read = torch.from_numpy(np.ascontiguousarray(R.dequantize(kcodes.cpu().numpy(), kscale.cpu().numpy()))).cuda()
    qrows = q.permute(0, 2, 1, 3).reshape(B * q_len, H * HD).contiguous()
    vb = torch.zeros(B, H, S, HD, device="cuda", dtype=BF16)
    vcodes, vscale = torch.empty_like(kcodes), torch.empty_like(kscale)
    out = torch.full((B * q_len, H * HD), float("nan"), device="cuda", dtype=BF16)

    def run(v):
        vb[:] = v[:S].bfloat16()
        ops.cross_kv_quant(vb, vcodes, vscale)
        ops.cross_attn_step_fp8(qrows, B, q_len, H, HD, kcodes, vcodes, kscale, vscale, S, out)
        return out.view(-1, HD)

    _verify("cross_attn_row_fp8_kernel", f"B={B} H={H} q_len={q_len} S={S} {kind}", run, S,
            _rows_bqh(P.reference_weights(q, k_read)))
    assert set(vcodes.unique().tolist()) <= {0, 0x7E}
    assert set(vscale.unique().tolist()) <= {0.0, float(np.float32(1) / np.float32(448))}
