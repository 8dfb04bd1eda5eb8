"""Exact-arithmetic reference for the decode linears, ``kw_pack_weight`` and ``kw_dec_linear``
(tests/test_gpu_declin_exact.py, tests/test_declin_ref_cpu.py).

The dyadic recipe, the float64 epilogue restatement, the guarded buffers and the GELU bounds are those of
tests/_gemm_ref.py (imported, not copied).  Added here: the two fragment-major layouts written from their
definitions in include/kwhisper.h (not from ``ops.act_tile`` / ``ops.unpack_weight``), and the fused LayerNorm's
float64 reference with a derived elementwise acceptance bound.  Torch and numpy on whatever device the tensors live
on; nothing here launches a kernel.
"""
from __future__ import annotations

import numpy as np
import torch

from _gemm_ref import (GRID, RESID, SENTINEL, STORE, CLayout, assert_exact, assert_gelu_share, bf16_bits_np,  # noqa: F401
                       bits_of, check_guarded, describe, element_offsets, exact_bound_units, expected_bits, gelu64,
                       gelu_bf16_bound, gelu_rel_err, guarded, plant, recipe_a, recipe_g, recipe_w, reference,
                       to_device, ulp_bf16)

POISON = 0x7FC3  # bf16 quiet NaN with a payload: what x holds wherever the kernel must not look
LN_OFFSETS = (-1.0, -0.5, 0.0, 0.5, 1.0)  # row m of a LayerNorm case is the recipe plus LN_OFFSETS[m % 5]
LN_CONST = 0.75  # the constant last row of a LayerNorm case (variance 0)
U = 2.0 ** -24  # half an ulp of float32, relative


# ------------------------------------------------------------------------------------------------ layouts
def tiled_offsets(M: int, K: int) -> torch.Tensor:
    """[16 T, K] flat element offsets of a ``KW_LD_TILED`` buffer of T = ceil(M / 16) row tiles (kwhisper.h): element
    (m, k) is element k % 8 of 16-B piece ((k / 32) * T + m / 16) * 64 + m % 16 + 16 * ((k % 32) / 8).  All 16 T rows
    are given (the buffer holds them); rows >= M are the ones "never written" / that "may hold anything"."""
    assert 1 <= M <= 32 and K % 32 == 0
    T = (M + 15) // 16
    m = torch.arange(16 * T, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    piece = ((k // 32) * T + m // 16) * 64 + m % 16 + 16 * ((k % 32) // 8)
    return piece * 8 + k % 8


def tiled_elems(M: int, K: int) -> int:
    return (K // 32) * ((M + 15) // 16) * 512


def tile_x(x: torch.Tensor, poison: int = POISON) -> torch.Tensor:
    """x [M, K] bf16 -> the flat fragment-major buffer, rows M .. 16 T - 1 holding the NaN pattern ``poison``."""
    M, K = x.shape
    off = tiled_offsets(M, K)[:M].to(x.device)
    buf = torch.full((tiled_elems(M, K),), poison, dtype=torch.int16, device=x.device).view(torch.bfloat16)
    buf[off.reshape(-1)] = x.reshape(-1)
    return buf


def untile_hb(buf: torch.Tensor, M: int, N: int) -> torch.Tensor:
    """The [M, N] rows of a fragment-major hb."""
    return buf[tiled_offsets(M, N)[:M].to(buf.device)]


def packed_offsets(N: int, K: int) -> torch.Tensor:
    """[Np, K] flat element offsets of kw_pack_weight's output, Np = ceil(N / 32) * 32: fragment (column block
    cb = n / 16, k-tile kt = k / 32) is 64 lanes of 8 elements, fragments ordered [cb][kt]; lane l holds the elements
    k = 32 kt + 8 (l / 16) .. + 7 of row 16 cb + l % 16.  Rows >= N hold zeros."""
    assert K % 32 == 0
    Np, nkt = (N + 31) // 32 * 32, K // 32
    n = torch.arange(Np, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None, :]
    lane = n % 16 + 16 * ((k % 32) // 8)
    return (((n // 16) * nkt + k // 32) * 64 + lane) * 8 + k % 8


def packed_image(W: torch.Tensor) -> torch.Tensor:
    """The bit patterns (int64) kw_pack_weight must write for W [N, K] bf16: W's bits at ``packed_offsets``, zero bits
    in the padding columns."""
    N, K = W.shape
    off = packed_offsets(N, K).to(W.device)
    out = torch.zeros(off.numel(), dtype=torch.int64, device=W.device)
    out[off[:N].reshape(-1)] = bits_of(W).reshape(-1)
    return out


def poisoned_rows(x: torch.Tensor, ldx: int, front: int = 64, back: int = 64, poison: int = POISON):
    """x [M, K] bf16 inside a flat buffer of NaNs: ``front`` elements, M rows ``ldx`` apart, ``back`` elements."""
    M, K = x.shape
    assert ldx >= K
    buf = torch.full((front + M * ldx + back,), poison, dtype=torch.int16, device=x.device).view(torch.bfloat16)
    buf[front:front + M * ldx].view(M, ldx)[:, :K] = x
    return buf


# ------------------------------------------------------------------------------------------------ LayerNorm inputs
def ln_rows(rng, M: int, K: int) -> np.ndarray:
    """The x of a LayerNorm case: the recipe plus LN_OFFSETS[m % 5] per row (the mean is as large as the spread, so
    mean * colsum is as large as the result), and with M >= 2 a constant last row (variance exactly 0).  Multiples
    of 1/4 in [-2, 2]: exact in bf16; sum x (1/4 grid, <= 2 K), sum x^2 (1/16 grid, <= 4 K) and the accumulator
    (1/32 grid, <= K / 4) are exact in float32 in any order for K < 2^18."""
    x = recipe_a(rng, (M, K)) + np.asarray(LN_OFFSETS, dtype=np.float32)[np.arange(M) % 5][:, None]
    if M >= 2:
        x[M - 1] = LN_CONST
    return x.astype(np.float32)


def assert_ln_exact(x: torch.Tensor, W: torch.Tensor) -> int:
    """``assert_exact`` for a LayerNorm case, plus its two statistics: |x| <= 2 on the 1/4 grid, so sum x^2 counts at
    most 64 K units of 1/16 and the accumulator at most 8 K units of 1/32."""
    assert float(x.double().abs().max()) <= 2.0
    units = assert_exact(x, W)
    sq_units = int((x.double() * 4).round().to(torch.int64).pow(2).sum(dim=1).max())
    assert sq_units < 2 ** 24, f"sum of squares left float32: {sq_units} units"
    return max(units, sq_units)


# ------------------------------------------------------------------------------------------------ LayerNorm reference
def _stats64(x64: torch.Tensor):
    K = x64.shape[1]
    mean = x64.sum(dim=1) / K
    msq = (x64 * x64).sum(dim=1) / K
    return mean, msq, msq - mean * mean


def ln_reference(acc64, x64, colsum64, bias64, eps) -> torch.Tensor:
    """float64: (acc - mean * cs) / sqrt(var + eps) + bias, mean and biased variance of each row of x64; ``eps`` is
    taken as the float32 the argument block carries."""
    eps = float(np.float32(eps))
    mean, _, var = _stats64(x64)
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    out = (acc64 - mean[:, None] * colsum64[None, :]) * rstd[:, None]
    return out + (bias64[None, :] if bias64 is not None else 0.0)


def ln_bound(acc64, x64, colsum64, bias64, eps, c_dtype=torch.float32) -> torch.Tensor:
    """Elementwise acceptance bound of the fused LayerNorm's result against ``ln_reference``, from the operation
    sequence of ln_finish_row / ln_rstd / ln_fold (csrc/declin_tile.h) and epi_value (declin.hip).

    With the dyadic inputs sx = sum x, sq = sum x^2, the accumulator acc and colsum cs are exact float32 numbers
    whatever the order of summation.  What follows them is eleven rounded float32 operations; each is charged half an
    ulp (relative u = 2^-24), rsqrtf one ulp (2 u: the HIP programming guide lists rsqrtf at 1 ulp and the ISA
    documents v_rsq_f32 at 1 ulp; neither promises correct rounding).  g(n) = n u / (1 - n u) bounds n compounded
    roundings.  mu, S = sq / K, var = S - mu^2, E = var + eps, R = E^-1/2, s = acc - mu cs are the true values:

      inv  = fl(1 / K)                  (1 / K) (1 + d1)
      mean = fl(sx inv)                 |mean - mu|      <= g(2) |mu|
      a    = fl(sq inv)                 |a - S|          <= g(2) S
      b    = fl(mean mean)              |b - mu^2|       <= g(5) mu^2
      d    = fl(a - b)                  |d - var|        <= g(5) (S + mu^2) + u (1 + g(5)) (S + mu^2) <= g(7) (S + mu^2)
      fmaxf(d, 0)                       var >= 0: clamping cannot move d away from var
      e    = fl(d + eps)                |e - E|          <= g(7) (S + mu^2) (1 + u) + u E
                                        rel(e) = g(8) (S + mu^2) / E + u          -- the first cancellation
      rstd = rsqrtf(e)                  (1 + r)^-1/2 - 1 is within |r| / 2 + r^2 for |r| <= 0.1 (asserted), so
                                        rel(rstd) = rel(e) / 2 + rel(e)^2 + 2 u (1 + rel(e))
      t    = fl(mean cs)                |t - mu cs|      <= g(3) |mu cs|
      w    = fl(acc - t)                |w - s|          <= g(3) |mu cs| + u (|acc| + (1 + g(3)) |mu cs|)
                                                         <= u (|acc| + |mu cs|) + g(4) |mu cs|   -- the second
      p    = fl(rstd w)                 |p - R s|        <= R [ |s| (rel(rstd) + u (1 + rel(rstd)))
                                                               + |w - s| (1 + rel(rstd)) (1 + u) ]   =: dp
      out  = fl(p + bias)               |out - ref|      <= dp + u (|ref| + dp)

    A compiler that contracts a - b or acc - t into one fma drops a rounding and stays inside.  The second
    cancellation is carried in absolute terms, R (|acc| + |mu cs|): where the row's mean is as large as its spread
    the two terms cancel to a result much smaller than either.  For a constant row var = 0, R = eps^-1/2 and acc =
    mu cs exactly, so the reference is the bias itself and the bound is what R makes of the rounding of mean cs.
    For a bf16 C half a bf16 ulp of the true value is added (the store's rounding, as ``gelu_bf16_bound``)."""
    def g(n):
        return n * U / (1.0 - n * U)

    eps = float(np.float32(eps))
    mean, msq, var = _stats64(x64)
    var = var.clamp_min(0.0)
    E = var + eps
    R = 1.0 / torch.sqrt(E)
    rel_e = g(8) * (msq + mean * mean) / E + U
    assert float(rel_e.max()) <= 0.1, f"rel(e) = {float(rel_e.max()):.3g}: the rsqrt expansion needs <= 0.1"
    rel_r = (rel_e / 2 + rel_e * rel_e + 2 * U * (1 + rel_e))[:, None]
    mcs = (mean[:, None] * colsum64[None, :]).abs()
    s = acc64 - mean[:, None] * colsum64[None, :]
    dw = U * (acc64.abs() + mcs) + g(4) * mcs
    dp = R[:, None] * (s.abs() * (rel_r + U * (1 + rel_r)) + dw * (1 + rel_r) * (1 + U))
    ref = s * R[:, None] + (bias64[None, :] if bias64 is not None else 0.0)
    bound = dp + U * (ref.abs() + dp)
    if c_dtype == torch.bfloat16:
        bound = bound + ulp_bf16(ref) / 2
    return bound


# ------------------------------------------------------------------------------------------------ f32 emulation
def emulate_ln_f32(acc, x, colsum, bias, eps, *, drop_mean_cs=False, skip_ktile=None, k_minus_1=False, drop_eps=False,
                   neighbour_stats=False) -> np.ndarray:
    """ln_finish_row / ln_rstd / ln_fold / epi_value in numpy float32, operation by operation (1 / np.sqrt in float32
    for rsqrtf), on numpy inputs: acc [M, N], x [M, K], colsum [N], bias [N] or None.  The keyword switches are the
    corruptions the CPU tests expect ``ln_bound`` to refuse."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    M, K = x.shape
    xs = x
    if skip_ktile is not None:
        keep = np.ones(K, dtype=bool)
        keep[32 * skip_ktile:32 * skip_ktile + 32] = False
        xs = x[:, keep]
    sx = xs.astype(np.float64).sum(axis=1).astype(f)  # exact: the order does not matter
    sq = (xs.astype(np.float64) ** 2).sum(axis=1).astype(f)
    assert np.array_equal(sx.astype(np.float64), xs.astype(np.float64).sum(axis=1))
    inv = f(1.0) / f(K - 1 if k_minus_1 else K)
    mean = (sx * inv).astype(f)
    d = np.maximum(((sq * inv).astype(f) - (mean * mean).astype(f)).astype(f), f(0.0))
    e = d if drop_eps else (d + f(eps)).astype(f)
    with np.errstate(divide="ignore"):
        rstd = (f(1.0) / np.sqrt(e, dtype=f)).astype(f)
    if neighbour_stats:
        mean, rstd = np.roll(mean, 1), np.roll(rstd, 1)
    acc = np.asarray(acc, dtype=f)
    cs = np.asarray(colsum, dtype=f)
    t = np.zeros_like(acc) if drop_mean_cs else (mean[:, None] * cs[None, :]).astype(f)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (rstd[:, None] * (acc - t).astype(f)).astype(f)
        if bias is not None:
            v = (v + np.asarray(bias, dtype=f)[None, :]).astype(f)
    return v


def store_as(v32: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    """What a float32 result reads back as (float64) after the store to ``dtype`` (bf16: round to nearest even)."""
    t = torch.from_numpy(np.ascontiguousarray(v32, dtype=np.float32))
    return (t.bfloat16() if dtype == torch.bfloat16 else t).double()
