"""The exact-arithmetic GEMM reference (tests/_gemm_ref.py) checked on the host: the float64 restatement against a
plain triple loop, the recipe's exactness bound and GELU-input share at every K the GPU file uses, the guarded
buffer's checker against planted stray elements, and the GELU acceptance bound against numpy-f32 emulations of both
GELU forms of csrc/kw_common.h."""
import math

import numpy as np
import pytest
import torch

import _gemm_ref as R


def _loop_reference(abuf, al, W, bias, M, N, K, *, epilogue, gelu, scale, scale_cols, row_add, period, cl, cbuf):
    """kw_gemm as three nested loops over Python floats, writing into the flat list ``cbuf``."""
    a_rpb = al.rpb if al.rpb > 0 else M
    c_rpb = cl.rpb if cl.rpb > 0 else M
    for m in range(M):
        a0 = al.front + (m // a_rpb) * al.bs + (m % a_rpb) * al.lda
        for n in range(N):
            v = 0.0
            for k in range(K):
                v += float(abuf[a0 + k]) * float(W[n][k])
            if bias is not None:
                v += float(bias[n])
            if epilogue == R.HEADSPLIT:
                width = cl.heads * cl.hd
                part, rem = divmod(n, width)
                h, d = divmod(rem, cl.hd)
                b, t = divmod(m, cl.seq)
                off = cl.front + ((((part * (M // cl.seq) + b) * cl.heads + h) * cl.seq + t) * cl.hd + d)
            else:
                off = cl.front + (m // c_rpb) * cl.bs + (m % c_rpb) * cl.ldc + n
            if epilogue == R.RESID:
                cbuf[off] += v
                continue
            if gelu:
                v = 0.5 * v * (1.0 + math.erf(v / math.sqrt(2.0)))
            if n < scale_cols:
                v *= scale
            if row_add is not None:
                v += float(row_add[m % period][n])
            cbuf[off] = v


CASES = [
    # M, N, K, A layout, C layout, epilogue, gelu, scale_cols, period
    (5, 6, 4, R.ALayout(4), R.CLayout(ldc=6, front=3, back=2), R.STORE, False, 0, 0),
    (7, 6, 4, R.ALayout(6, front=2), R.CLayout(ldc=9, rpb=3, bs=31, front=1), R.STORE, True, 4, 3),
    (6, 4, 6, R.ALayout(4, rpb=3, bs=14), R.CLayout(ldc=4), R.RESID, False, 0, 0),  # stride-2 conv row map, d = 2
    (6, 12, 4, R.ALayout(4), R.CLayout(seq=3, heads=2, hd=3, front=5), R.HEADSPLIT, False, 6, 0),
    (4, 8, 4, R.ALayout(4), R.CLayout(seq=1, heads=1, hd=2, front=0), R.HEADSPLIT, False, 0, 2),  # 4 parts
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_restatement_equals_triple_loop(case):
    M, N, K, al, cl, epilogue, gelu, scale_cols, period = CASES[case]
    rng = np.random.default_rng(case)
    abuf = torch.from_numpy(R.recipe_a(rng, al.span(M, K) + 3))
    W = torch.from_numpy(R.recipe_w(rng, (N, K)))
    bias = torch.from_numpy(R.recipe_g(rng, N)) if case != 0 else None
    row_add = torch.from_numpy(R.recipe_g(rng, (period, N))) if period else None
    idx, total = R.element_offsets(cl, M, N)
    base = torch.from_numpy(R.recipe_g(rng, (M, N)))
    A = R.gather_rows(abuf, al, M, K)
    assert A.shape == (M, K)
    pre, val = R.reference(A.double() @ W.double().t(), bias=bias, epilogue=epilogue, gelu=gelu, scale=0.125,
                           scale_cols=scale_cols, row_add=row_add, row_add_period=period, base=base)
    cbuf = [float("nan")] * total
    if epilogue == R.RESID:
        for m in range(M):
            for n in range(N):
                cbuf[int(idx[m, n])] = float(base[m, n])
    _loop_reference(abuf.tolist(), al, W.tolist(), None if bias is None else bias.tolist(), M, N, K, epilogue=epilogue,
                    gelu=gelu, scale=0.125, scale_cols=scale_cols, row_add=None if row_add is None else row_add.tolist(),
                    period=period, cl=cl, cbuf=cbuf)
    want = torch.full((total,), float("nan"), dtype=torch.float64)
    want[idx.reshape(-1)] = val.reshape(-1)
    got = torch.tensor(cbuf, dtype=torch.float64)
    assert torch.equal(torch.isnan(got), torch.isnan(want))  # the same places written
    if gelu:
        torch.testing.assert_close(got[idx], val, atol=1e-14, rtol=1e-14)
    else:
        assert torch.equal(got[idx], val)  # exact inputs: bitwise, whatever the summation order


def test_expected_bits_round_to_nearest_even():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -20), 0.0, -0.0, 2.0 ** -130],
                     dtype=torch.float64)
    bits = R.expected_bits(v, torch.bfloat16)
    assert bits.tolist() == [0x3F80, 0x3F80, 0x3F82, 0xBF81, 0x0000, 0x8000, 0x0008]  # ties to even, both ways
    assert torch.equal(bits, R.bits_of(v.float().bfloat16()))
    assert R.expected_bits(v, torch.float32).tolist() == R.bits_of(v.float()).tolist()
    with pytest.raises(AssertionError):
        R.expected_bits(torch.tensor([1.0 + 2.0 ** -30], dtype=torch.float64), torch.float32)


# every K tests/test_gpu_gemm_exact.py uses, bf16 and f32 kernels alike (384 = 3 x 128: the conv1 layout case), and
# the engine's largest (fc2 of large-v3: 5120)
K_USED = [16, 48, 64, 128, 192, 256, 320, 384, 1280, 5120]


@pytest.mark.parametrize("K", K_USED)
def test_recipe_is_exact_and_gelu_inputs_are_curved(K):
    rng = np.random.default_rng(K)
    M, N = 256, 128
    A = torch.from_numpy(R.recipe_a(rng, (M, K)))
    W = torch.from_numpy(R.recipe_w(rng, (N, K)))
    bias = torch.from_numpy(R.recipe_g(rng, N))
    units = R.assert_exact(A, W)
    assert units <= 4 * K + 6 * R.GRID  # sum |a| |w| <= K / 8 = 4 K grid units
    # bf16 holds every input exactly (the bf16 kernels see the same numbers as the reference)
    for t in (A, W, bias):
        assert torch.equal(R.to_device(t.numpy(), torch.bfloat16, "cpu").float(), t)
    acc = A.double() @ W.double().t()
    f = A @ W.t()  # float32 accumulation, another order: the same numbers
    assert torch.equal(f.double(), acc)
    pre, _ = R.reference(acc, bias=bias)
    share = R.assert_gelu_share(pre)
    print(f"K={K}: {units} grid units, pre-activation std {float(pre.std()):.2f}, share inside (-4, 4) {share:.2f}")


def test_recipe_guards_fire():
    A = torch.full((2, 2 ** 13), 1024.0)  # 2^25 grid units
    W = torch.full((1, 2 ** 13), 0.125)
    with pytest.raises(AssertionError):
        R.assert_exact(A, W)
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([[0.3]]), torch.tensor([[0.125]]))
    with pytest.raises(AssertionError):
        R.assert_gelu_share(torch.full((4, 4), 9.0, dtype=torch.float64))


LAYOUTS = [
    (10, 8, R.CLayout(ldc=12, rpb=4, bs=60, front=5, back=7)),
    (6, 12, R.CLayout(seq=3, heads=2, hd=3, front=5, back=7)),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", range(len(LAYOUTS)))
def test_guarded_buffer_catches_one_stray_element(which, dtype):
    M, N, lay = LAYOUTS[which]
    idx, total = R.element_offsets(lay, M, N)
    val = torch.from_numpy(R.recipe_g(np.random.default_rng(0), (M, N))).double()
    want = R.expected_bits(val, dtype)

    def fresh():
        buf = R.guarded(total, dtype, "cpu")
        assert bool((R.bits_of(buf) == R.SENTINEL[dtype]).all()) and bool(torch.isnan(buf.float()).all())
        R.plant(buf, idx, val)
        return buf

    stray, wrong = R.check_guarded(fresh(), idx, want)
    assert stray.numel() == 0 and wrong.shape[0] == 0
    if lay.seq > 0:
        one_part = (M // lay.seq) * lay.heads * lay.seq * lay.hd
        regions = {"before": lay.front - 1, "extra part": lay.front + (N // (lay.heads * lay.hd)) * one_part + 4,
                   "after": total - 1}
    else:
        regions = {"before": lay.front - 1, "right of column N": lay.front + N, "between batches": lay.front + 4 * lay.ldc + 1,
                   "after": total - 1}
    inside = set(idx.reshape(-1).tolist())
    for name, off in regions.items():
        assert off not in inside, name
        buf = fresh()
        buf[off] = 0.0  # a plausible result, planted where nothing may be written
        stray, wrong = R.check_guarded(buf, idx, want)
        assert stray.tolist() == [off] and wrong.shape[0] == 0, name
    buf = fresh()
    buf[int(idx[M - 1, N - 1])] = 3.0  # and a wrong value inside an image is a value error, not a guard error
    stray, wrong = R.check_guarded(buf, idx, want)
    assert stray.numel() == 0 and wrong.tolist() == [[M - 1, N - 1]]
    assert "1 image elements differ" in R.describe(stray, wrong)


# ---------------------------------------------------------------------------------------- GELU bound
_POLY = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def _gelu_bf16out_np(x, poly=_POLY):
    """numpy-f32 emulation of gelu_bf16out (csrc/kw_common.h), operation by operation (fmaf through float64: one
    rounding; rcp and exp2 correctly rounded here, within an ulp on the device)."""
    f = np.float32
    x = x.astype(f)
    t =(1.0 / (np.abs(x).astype(np.float64) * np.float64(f(f(0.3275911) * f(0.70710678118654752440))) + 1.0).astype(f).astype(
        np.float64)).astype(f)
    p = f(poly[4])
    for c in (poly[3], poly[2], poly[1], poly[0]):
        p = (f(c) + t * p).astype(f)
    p = (t * p).astype(f)
    xx = ((x * x).astype(f) * f(-0.72134752044448170368)).astype(f)
    ex = np.exp2(xx.astype(np.float64)).astype(f)
    e = (-(p.astype(np.float64)) * ex.astype(np.float64) + 1.0).astype(f)
    h = (f(0.5) * x).astype(f)
    return (np.abs(h).astype(np.float64) * e.astype(np.float64) + h.astype(np.float64)).astype(f)


def _gelu_erff_np(x):
    """numpy-f32 emulation of gelu_erf: 0.5 x (1 + erff(x / sqrt 2)) with a correctly rounded erff."""
    f = np.float32
    x = x.astype(f)
    arg = (x * f(0.70710678118654752440)).astype(f)
    er = torch.erf(torch.from_numpy(arg.astype(np.float64))).numpy().astype(f)
    return ((f(0.5) * x).astype(f) * (f(1.0) + er).astype(f)).astype(f)


def _accepts(y32, x):
    x64 = torch.from_numpy(x.astype(np.float64))
    ref = R.gelu64(x64)
    got = torch.from_numpy(y32).bfloat16().double()  # the store's RNE rounding
    return (got - ref).abs() <= R.gelu_bf16_bound(ref, x64)


def test_gelu_bound_accepts_both_forms_and_rejects_a_moved_coefficient():
    x = (np.arange(-64 * R.GRID, 64 * R.GRID + 1) / float(R.GRID)).astype(np.float32)
    x64 = torch.from_numpy(x.astype(np.float64))
    ref = R.gelu64(x64)
    for name, y in (("gelu_bf16out", _gelu_bf16out_np(x)), ("gelu_erf", _gelu_erff_np(x))):
        rel = R.gelu_rel_err(torch.from_numpy(y.astype(np.float64)), ref, x64)
        print(f"{name}: worst f32 error {float(rel.max()):.3g} x max(1, |x|)")
        assert float(rel.max()) < 1e-6 / 4  # the emulation sits well inside the bound's second term
        assert bool(_accepts(y, x).all()), name
    for i in range(5):
        moved = list(_POLY)
        moved[i] += 1e-4
        ok = _accepts(_gelu_bf16out_np(x, tuple(moved)), x)
        assert not bool(ok.all()), f"coefficient {i} moved by 1e-4 passes the bound"


def test_walk256_reaches_two_ragged_tiles_in_a_row():
    """M = 1025, N = 16384 on 256 CUs: 5 x 64 tiles, 40 per XCD, 32 workgroups per XCD.  The last 64 tiles (row tile
    4) are ragged; XCD 7's run is all ragged and its workgroups 0..7 take two tiles each."""
    walk = R.walk256(1025, 16384, 256)
    assert len(walk) == 256 and sum(len(w) for w in walk) == 320
    two_ragged = [w for w in walk if len(w) == 2 and w[0][0] == 4 and w[1][0] == 4]
    assert len(two_ragged) == 8
    assert R.ragged_handoffs(1025, 16384, 256) == (8, 56)
    # one tile per workgroup: no hand-off at all
    assert R.ragged_handoffs(1279, 768, 256) == (0, 0)
