"""The decode linears' exact-arithmetic reference (tests/_declin_ref.py) checked on the host: the two fragment-major
layouts are bijections and agree with the package's own permutations, every shape of the GPU file's table keeps the
recipe exact, the derived LayerNorm bound accepts a float32 emulation of the kernel's operation sequence and refuses
five corruptions of it, and the bitwise checker reports three corruptions of an expected image."""
import functools

import numpy as np
import pytest
import torch

import _declin_ref as D
from kwhisper import ops

ROWS = (1, 16, 17, 32, 33, 70)
# name -> (N, K, rows): the table of tests/test_gpu_declin_exact.py (one shape per path of choose() / launch_one())
SHAPES = {
    "n40_k160": (40, 160, ROWS),
    "n48_k384": (48, 384, ROWS),
    "n48_k2592": (48, 2592, ROWS + (257,)),
    "n64_k2560": (64, 2560, ROWS),
    "n4112_k2560": (4112, 2560, ROWS),
    "n5120_k384": (5120, 384, ROWS),
    "n5120_k512": (5120, 512, ROWS),
    "n8192_k384": (8192, 384, ROWS),
    "lm_n8200_k256": (8200, 256, (1, 32, 33, 40, 129, 300, 321)),
}
LN_SHAPES = [s for s in SHAPES if s != "n48_k2592"]  # (the K-split shape takes no fused LayerNorm)
EPS = (1e-5, 2.0 ** -6)
NCOL = 200  # columns of each shape the LayerNorm checks run on (statistics are per row, cs and bias per column)


# ---------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32])
def test_tiled_offsets_is_a_bijection_and_agrees_with_act_tile(M):
    K = 96
    off = D.tiled_offsets(M, K)
    T = (M + 15) // 16
    assert off.shape == (16 * T, K) and D.tiled_elems(M, K) == (K // 32) * T * 512
    assert sorted(off.reshape(-1).tolist()) == list(range((K // 32) * T * 512))
    x = torch.arange(1, M * K + 1, dtype=torch.float32).view(M, K)  # distinct, none zero
    tiled = ops.act_tile(x)
    assert torch.equal(tiled[off[:M]], x)
    assert bool((tiled[off[M:]] == 0).all())
    assert torch.equal(ops.act_untile(tiled, M, K), tiled[off[:M]])
    xb = D.to_device(D.recipe_a(np.random.default_rng(M), (M, K)), torch.bfloat16, "cpu")
    mine = D.tile_x(xb)
    assert torch.equal(D.untile_hb(mine, M, K), xb) and torch.equal(ops.act_untile(mine, M, K), xb)
    assert bool((D.bits_of(mine[off[M:]]) == D.POISON).all()) and bool(torch.isnan(mine[off[M:]].float()).all())


@pytest.mark.parametrize("N,K", [(40, 160), (48, 64), (64, 32), (1, 32), (33, 96)])
def test_packed_offsets_is_a_bijection_with_zero_padding(N, K):
    off = D.packed_offsets(N, K)
    Np = (N + 31) // 32 * 32
    assert off.shape == (Np, K)
    assert sorted(off.reshape(-1).tolist()) == list(range(Np * K))
    W = torch.arange(1, N * K + 1, dtype=torch.float32).view(N, K)
    # the package's inverse permutation, on the host (unpack_weight itself takes device tensors): [cb][kt][4][16][8]
    flat = torch.zeros(Np * K)
    flat[off[:N].reshape(-1)] = W.reshape(-1)
    back = flat.view(Np // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(Np, K)
    assert torch.equal(back[:N], W) and bool((back[N:] == 0).all())
    Wb = D.to_device(D.recipe_w(np.random.default_rng(N), (N, K)) + 0.125, torch.bfloat16, "cpu")
    img = D.packed_image(Wb)
    assert torch.equal(img[off[:N]], D.bits_of(Wb)) and bool((img[off[N:]] == 0).all())
    # the header's words: lane l of fragment (cb, kt) holds k = 32 kt + 8 (l / 16) .. of row 16 cb + l % 16
    cb, kt, lane = (N - 1) // 16, K // 32 - 1, 37
    n, k = 16 * cb + lane % 16, 32 * kt + 8 * (lane // 16)
    if n < Np:
        assert off[n, k:k + 8].tolist() == [((cb * (K // 32) + kt) * 64 + lane) * 8 + e for e in range(8)]


# ---------------------------------------------------------------------------------------------- the recipe
@functools.lru_cache(maxsize=None)
def _weights(name):
    N, K, _ = SHAPES[name]
    rng = np.random.default_rng([sum(name.encode()), N, K])
    return torch.from_numpy(D.recipe_w(rng, (N, K))), torch.from_numpy(D.recipe_g(rng, N)), rng


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_keeps_the_recipe_exact(name):
    N, K, rows = SHAPES[name]
    W, bias, rng = _weights(name)
    M = max(rows)
    x = torch.from_numpy(D.recipe_a(rng, (M, K)))
    units = D.assert_exact(x, W)
    xl = torch.from_numpy(D.ln_rows(rng, M, K))
    ln_units = D.assert_ln_exact(xl, W)
    assert ln_units <= 64 * K < 2 ** 24 and units <= 4 * K + 6 * D.GRID
    for t in (x, xl, W, bias):  # bf16 holds every input exactly
        assert torch.equal(D.to_device(t.numpy(), torch.bfloat16, "cpu").float(), t)
    cs = W.double().sum(dim=1)
    assert torch.equal(cs.float().double(), cs)  # ln_colsum is an exact float32
    acc = xl.double() @ W.double().t()
    assert torch.equal((xl @ W.t()).double(), acc)  # float32 accumulation in another order: the same numbers
    print(f"{name}: {units} grid units, LayerNorm rows {ln_units}")


# ---------------------------------------------------------------------------------------------- the LayerNorm bound
@functools.lru_cache(maxsize=None)
def _ln_case(name, M):
    N, K, _ = SHAPES[name]
    W, bias, _ = _weights(name)
    cols = torch.cat([torch.arange(min(N, NCOL) - 8), torch.arange(N - 8, N)])  # (the partial last block with them)
    W, bias = W[cols], bias[cols]
    x = torch.from_numpy(D.ln_rows(np.random.default_rng([7, M, K]), M, K))
    acc = x.double() @ W.double().t()
    return x, W.double().sum(dim=1), bias, acc


def _ratio(v32, case, eps, dtype):
    x, cs, bias, acc = case
    ref = D.ln_reference(acc, x.double(), cs, bias.double(), eps)
    bound = D.ln_bound(acc, x.double(), cs, bias.double(), eps, dtype)
    err = (D.store_as(v32, dtype) - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # (0 / 0 where the result is an exact 0)
    return torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)  # a NaN result: off the bound


def _emulate(case, eps, **kw):
    x, cs, bias, acc = case
    return D.emulate_ln_f32(acc.numpy(), x.numpy(), cs.numpy(), bias.numpy(), eps, **kw)


@pytest.mark.parametrize("name", LN_SHAPES)
def test_emulation_stays_inside_ln_bound(name):
    """A condition on the bound: the kernel's operation sequence in numpy float32 must pass it everywhere, the
    constant row (variance 0, the reference is the bias) included."""
    worst = {torch.float32: 0.0, torch.bfloat16: 0.0}
    for M in SHAPES[name][2]:
        case = _ln_case(name, M)
        for eps in EPS:
            for dtype in (torch.float32, torch.bfloat16):
                r = _ratio(_emulate(case, eps), case, eps, dtype)
                assert bool(torch.isfinite(r).all()) and float(r.max()) <= 1.0, (name, M, eps, dtype, float(r.max()))
                worst[dtype] = max(worst[dtype], float(r.max()))
            if M >= 2:  # the constant row: finite and the bias within the bound
                v = _emulate(case, eps)[M - 1]
                assert np.isfinite(v).all()
                assert float(_ratio(_emulate(case, eps), case, eps, torch.float32)[M - 1].max()) <= 1.0
    # (a bf16 C's figure is dominated by the store's own half ulp, which the bound grants whole)
    print(f"{name}: worst emulation / bound f32 C {worst[torch.float32]:.3f}, bf16 C {worst[torch.bfloat16]:.3f}")


CORRUPTIONS = {
    "mean * cs dropped": dict(drop_mean_cs=True),
    "one k-tile left out of the sums": dict(skip_ktile=1),
    "divided by K - 1": dict(k_minus_1=True),
    "neighbouring row's statistics": dict(neighbour_stats=True),
}


@pytest.mark.parametrize("what", list(CORRUPTIONS) + ["eps dropped at 2^-6"])
@pytest.mark.parametrize("name", LN_SHAPES)
def test_ln_bound_has_teeth(name, what):
    """Each corruption of the emulation leaves the bound on at least one element of every LayerNorm case (every row
    count, both eps, f32 and bf16 C).  A neighbour's statistics need a neighbour: M >= 2."""
    for M in SHAPES[name][2]:
        if what.startswith("neighbour") and M < 2:
            continue
        case = _ln_case(name, M)
        for eps in (EPS[1],) if what.startswith("eps") else EPS:
            kw = dict(drop_eps=True) if what.startswith("eps") else CORRUPTIONS[what]
            for dtype in (torch.float32, torch.bfloat16):
                r = _ratio(_emulate(case, eps, **kw), case, eps, dtype)
                assert float(r.max()) > 1.0, f"{name} M={M} eps={eps} {dtype}: '{what}' passes the bound"


# ---------------------------------------------------------------------------------------------- the bitwise checker
@pytest.mark.parametrize("epilogue", [D.STORE, D.RESID])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bitwise_checker_has_teeth(epilogue, dtype):
    """A kernel that drops one x element, swaps two rows or shifts the bias by a column writes an image that
    ``check_guarded`` reports against the expected bits (RESID's bf16 image is hb)."""
    M, N, K = 17, 40, 160
    rng = np.random.default_rng(3)
    x = torch.from_numpy(D.recipe_a(rng, (M, K))).double()
    W = torch.from_numpy(D.recipe_w(rng, (N, K))).double()
    bias = torch.from_numpy(D.recipe_g(rng, N)).double()
    base = torch.from_numpy(D.recipe_g(rng, (M, N))).double()
    idx, total = D.element_offsets(D.CLayout(ldc=N + 8), M, N)

    def image(x=x, bias=bias, perm=None):
        _, val = D.reference(x @ W.t(), bias=bias, epilogue=epilogue, base=base)
        return val if perm is None else val[perm]

    want = D.expected_bits(image(), dtype)

    def report(val):
        buf = D.guarded(total, dtype, "cpu")
        D.plant(buf, idx, val)
        return D.check_guarded(buf, idx, want)

    stray, wrong = report(image())
    assert stray.numel() == 0 and wrong.shape[0] == 0
    m, k = 5, 77
    dropped = x.clone()
    dropped[m, k] = 0.0 if float(x[m, k]) != 0.0 else 0.25
    _, wrong = report(image(x=dropped))
    hit = (W[:, k] != 0).nonzero().reshape(-1)
    assert wrong.shape[0] > 0 and set(wrong[:, 0].tolist()) == {m}  # row m only, where w[n][k] != 0
    if dtype == torch.float32:
        assert wrong[:, 1].tolist() == hit.tolist()
    perm = torch.arange(M)
    perm[3], perm[11] = 11, 3
    _, wrong = report(image(perm=perm))
    assert set(wrong[:, 0].tolist()) == {3, 11}
    _, wrong = report(image(bias=torch.roll(bias, 1)))
    assert wrong.shape[0] > 0 and len(set(wrong[:, 0].tolist())) == M  # every row
