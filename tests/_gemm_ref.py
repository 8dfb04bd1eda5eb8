"""Exact-arithmetic reference for ``kw_gemm`` (tests/test_gpu_gemm_exact.py, tests/test_gemm_ref_cpu.py).

Inputs come from small dyadic grids, so every product and every partial sum of A . W^T + bias (+ row_add, + the
residual base), in any order, is a float32 number: a result without GELU has exactly one right f32 value and one
right bf16 value (round to nearest even), and a test compares bits.

    a in {-4 .. 4} / 4,  w in {-1, 0, 1} / 8,  bias / row_add / residual base in {-64 .. 64} / 32,  scale 2^-k

Everything lives on the 1/32 grid (1/256 after the column scale); ``assert_exact`` bounds the largest intermediate
below 2^24 grid units on the host.  The reference is float64 and restates ``epi_one`` (csrc/gemm_common.h).
Everything here is torch on whatever device the tensors live on: the CPU tests run it on the host, the GPU tests
on the device.  Nothing here launches a kernel.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

GRID = 32  # every input is a multiple of 1 / GRID
# guard pattern: NaNs with a payload no arithmetic produces, compared as integers
SENTINEL = {torch.float32: 0x7FA5A5A5, torch.bfloat16: 0x7FA5}
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


# ------------------------------------------------------------------------------------------------ bits
def bf16_bits_np(a) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even (no NaN among the recipe's values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_device(values: np.ndarray, dtype: torch.dtype, device) -> torch.Tensor:
    """float32 values -> a tensor of ``dtype``; bf16 by bit manipulation (exact for the recipe's values)."""
    if dtype == torch.float32:
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(device)
    return torch.from_numpy(bf16_bits_np(values).view(np.int16)).to(device).view(torch.bfloat16)


def expected_bits(ref64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The bit patterns (as int64) of ``ref64`` stored as ``dtype``: f32 bits, or the RNE bf16 bits of the f32
    value.  ``ref64`` must be exactly representable in f32 (the exact cases are: ``assert_exact``)."""
    f = ref64.to(torch.float32)
    assert bool((f.double() == ref64).all()), "reference is not exactly representable in float32"
    u = f.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if dtype == torch.float32:
        return u
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def bits_of(t: torch.Tensor) -> torch.Tensor:
    """A float32 / bfloat16 tensor's bit patterns as non-negative int64."""
    mask = 0xFFFFFFFF if t.dtype == torch.float32 else 0xFFFF
    return t.contiguous().view(_INT[t.dtype]).to(torch.int64) & mask


# ------------------------------------------------------------------------------------------------ recipe
def recipe_a(rng, shape) -> np.ndarray:
    return (rng.integers(-4, 5, size=shape) / 4.0).astype(np.float32)


def recipe_w(rng, shape) -> np.ndarray:
    return (rng.integers(-1, 2, size=shape) / 8.0).astype(np.float32)


def recipe_g(rng, shape) -> np.ndarray:
    """bias, row_add and the residual base: multiples of 1/32 in [-2, 2]."""
    return (rng.integers(-2 * GRID, 2 * GRID + 1, size=shape) / float(GRID)).astype(np.float32)


def exact_bound_units(A: torch.Tensor, W: torch.Tensor, extra: float = 6.0) -> int:
    """An upper bound, in 1/32 grid units and integer arithmetic, of every intermediate of A . W^T + bias + row_add
    (+ residual base): max_m sum_k |4 a| * max |8 w|  +  32 * ``extra`` (|bias| + |row_add| + |base| <= 2 each)."""
    a4 = (A.double().abs() * 4).round().to(torch.int64)
    w8 = (W.double().abs() * 8).round().to(torch.int64)
    assert bool((a4.double() == A.double().abs() * 4).all()) and bool((w8.double() == W.double().abs() * 8).all()), \
        "inputs left the dyadic grid"
    return int(a4.sum(dim=1).max()) * int(w8.max()) + int(GRID * extra)


def assert_exact(A: torch.Tensor, W: torch.Tensor) -> int:
    """The exactness property of the recipe: no intermediate reaches 2^24 grid units (so f32 holds all of them; the
    column scale 2^-k only moves the exponent)."""
    units = exact_bound_units(A, W)
    assert units < 2 ** 24, f"recipe lost exactness: {units} grid units >= 2^24"
    return units


def assert_gelu_share(pre64: torch.Tensor) -> float:
    """At least a quarter of the GELU inputs lie where GELU is curved, (-4, 4)."""
    share = float((pre64.abs() < 4).double().mean())
    assert share >= 0.25, f"only {share:.3f} of the pre-activations inside (-4, 4)"
    return share


# ------------------------------------------------------------------------------------------------ geometry
STORE, RESID, HEADSPLIT = 0, 1, 2  # KW_EPI_*


@dataclass
class ALayout:
    """Rows of A inside a flat buffer: row m starts ``front + (m // rpb) * bs + (m % rpb) * lda`` (kw_gemm's
    lda / a_rows_per_batch / a_batch_stride / a_offset; rpb 0 = one batch)."""
    lda: int
    rpb: int = 0
    bs: int = 0
    front: int = 0

    def offsets(self, M: int) -> torch.Tensor:
        m = torch.arange(M, dtype=torch.int64)
        rpb = self.rpb if self.rpb > 0 else max(M, 1)
        return self.front + (m // rpb) * self.bs + (m % rpb) * self.lda

    def span(self, M: int, K: int) -> int:
        return (int(self.offsets(M).max()) if M else 0) + K


@dataclass
class CLayout:
    """Where C's elements go.  STORE / RESID: row m at ``front + (m // rpb) * bs + (m % rpb) * ldc`` (ldc /
    c_rows_per_batch / c_batch_stride / c_offset).  HEADSPLIT (seq > 0): [part][batch][head][seq][hd] from ``front``.
    ``back`` elements of slack follow the last image (HEADSPLIT: one whole extra part as well)."""
    ldc: int = 0
    rpb: int = 0
    bs: int = 0
    front: int = 64
    back: int = 64
    seq: int = 0
    heads: int = 0
    hd: int = 0

    def parts(self, M: int, N: int):
        """(row part [M], column part [N], buffer elements): element (m, n) lives at row[m] + col[n]."""
        m = torch.arange(M, dtype=torch.int64)
        n = torch.arange(N, dtype=torch.int64)
        if self.seq > 0:
            width = self.heads * self.hd
            assert M % self.seq == 0 and N % width == 0
            nb = M // self.seq
            part, rem = n // width, n % width
            h, d = rem // self.hd, rem % self.hd
            col = (part * nb * self.heads + h) * self.seq * self.hd + d
            row = (m // self.seq) * (self.heads * self.seq * self.hd) + (m % self.seq) * self.hd
            one_part = nb * self.heads * self.seq * self.hd
            total = self.front + (N // width + 1) * one_part + self.back
            return self.front + row, col, total
        rpb = self.rpb if self.rpb > 0 else max(M, 1)
        row = self.front + (m // rpb) * self.bs + (m % rpb) * self.ldc
        total = (int(row.max()) if M else self.front) + max(self.ldc, N) + self.back
        return row, n, total


def element_offsets(lay: CLayout, M: int, N: int, device="cpu"):
    """(flat offsets [M, N], buffer elements); asserts that no two elements share a place."""
    row, col, total = lay.parts(M, N)
    idx = (row.to(device)[:, None] + col.to(device)[None, :])
    if idx.numel():
        assert int(idx.min()) >= 0 and int(idx.max()) < total
        assert int(torch.unique(idx.reshape(-1)).numel()) == idx.numel(), "C images overlap"
    return idx, total


# ------------------------------------------------------------------------------------------------ reference
def gelu64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gather_rows(abuf: torch.Tensor, lay: ALayout, M: int, K: int) -> torch.Tensor:
    """The M x K matrix kw_gemm reads out of the flat buffer ``abuf`` (rows may overlap: the conv row maps)."""
    off = lay.offsets(M).to(abuf.device)
    return abuf[off[:, None] + torch.arange(K, device=abuf.device)[None, :]]


def reference(acc64: torch.Tensor, *, bias=None, epilogue=STORE, gelu=False, scale=1.0, scale_cols=0,
              row_add=None, row_add_period=0, base=None):
    """float64 restatement of ``epi_one`` over acc64 = A . W^T [M, N]: returns (pre-activation, result).
    RESID: result = base + (acc + bias) with ``base`` [M, N] the values C held.  Otherwise bias, GELU, column scale
    for n < scale_cols, row_add[m % period]; where the element goes is the layout's business (``CLayout``)."""
    M, N = acc64.shape
    pre = acc64 + (bias.double()[None, :] if bias is not None else 0.0)
    if epilogue == RESID:
        return pre, base.double() + pre
    v = gelu64(pre) if gelu else pre.clone()
    if scale_cols > 0:
        v[:, :scale_cols] *= scale
    if row_add is not None:
        period = row_add_period if row_add_period > 0 else 1
        v = v + row_add.double()[torch.arange(M, device=acc64.device) % period]
    return pre, v


# ------------------------------------------------------------------------------------------------ guarded buffer
def guarded(total: int, dtype: torch.dtype, device) -> torch.Tensor:
    """``total`` elements of ``dtype``, every one the sentinel bit pattern."""
    return torch.full((total,), SENTINEL[dtype], dtype=_INT[dtype], device=device).view(dtype)


def plant(buf: torch.Tensor, idx: torch.Tensor, values64: torch.Tensor) -> None:
    """Write exactly representable values into the images of a guarded buffer (the residual base)."""
    buf[idx.reshape(-1)] = values64.reshape(-1).to(buf.dtype)


def check_guarded(buf: torch.Tensor, idx: torch.Tensor, want_bits: torch.Tensor | None = None):
    """(stray, wrong): ``stray`` lists the flat offsets outside the images that no longer hold the sentinel,
    ``wrong`` the (m, n) of image elements whose bits differ from ``want_bits`` [M, N] (None: images not compared).
    Both empty means the launch wrote what it should and nothing else."""
    got = bits_of(buf)
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device=buf.device)
    inside[idx.reshape(-1)] = True
    stray = torch.nonzero((got != SENTINEL[buf.dtype]) & ~inside).reshape(-1)
    if want_bits is None:
        return stray, torch.zeros((0, 2), dtype=torch.int64)
    wrong = torch.nonzero(got[idx] != want_bits)
    return stray, wrong


def describe(stray: torch.Tensor, wrong: torch.Tensor) -> str:
    s = f"{stray.numel()} guard elements overwritten" + (f" (first offset {int(stray[0])})" if stray.numel() else "")
    w = f"{wrong.shape[0]} image elements differ" + (f" (first (m, n) = {tuple(wrong[0].tolist())})" if wrong.shape[0] else "")
    return s + "; " + w


# ------------------------------------------------------------------------------------------------ GELU bounds
def ulp_bf16(v: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 numbers around v (float64): 2^(floor(log2 |v|) - 7), the subnormal spacing 2^-133 at least."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=v.device), e - 7).clamp_min(2.0 ** -133)


def gelu_bf16_bound(ref64: torch.Tensor, x64: torch.Tensor) -> torch.Tensor:
    """Acceptance bound of a GELU result stored as bf16: half a bf16 ulp of the true value (the store's rounding)
    plus 1e-6 max(1, |x|) for the f32 evaluation (A&S 7.1.26's 1.5e-7, one ulp each for rcp and exp2, three f32
    roundings, all times |x| / 2), x the exact pre-activation."""
    return ulp_bf16(ref64) / 2 + 1e-6 * x64.abs().clamp_min(1.0)


def gelu_rel_err(got64: torch.Tensor, ref64: torch.Tensor, x64: torch.Tensor) -> torch.Tensor:
    """|got - ref| relative to max(1, |x|): the measure of the f32 GELU bound."""
    return (got64 - ref64).abs() / x64.abs().clamp_min(1.0)


# ------------------------------------------------------------------------------------------------ gemm256's tile walk
def walk256(M: int, N: int, cus: int, gm: int = 4):
    """gemm256_kernel's persistent walk restated: for each workgroup the list of (row tile, column tile) it takes,
    in order (8 contiguous runs, one per XCD; KW_GEMM_GM row tiles walk the columns together)."""
    tiles_n, tiles_m = N // 256, (M + 255) // 256
    nwg = tiles_m * tiles_n
    G = min(nwg, cus)
    q8, r8 = nwg >> 3, nwg & 7
    out = []
    for bid in range(G):
        xcd, loc = bid & 7, bid >> 3
        run0 = xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8
        run_len = q8 + (1 if xcd < r8 else 0)
        per = (G >> 3) + (1 if xcd < (G & 7) else 0)
        tiles = []
        for pos in range(loc, run_len, per):
            wg = run0 + pos
            gidx = wg // (gm * tiles_n)
            first_m = gidx * gm
            g = min(gm, tiles_m - first_m)
            rr = wg - gidx * gm * tiles_n
            tiles.append((first_m + rr % g, rr // g))
        out.append(tiles)
    return out


def ragged_handoffs(M: int, N: int, cus: int):
    """(ragged -> next tile, full -> next tile) hand-off counts of the walk; every tile is taken exactly once."""
    walk = walk256(M, N, cus)
    seen = sorted(t for w in walk for t in w)
    tiles_n, tiles_m = N // 256, (M + 255) // 256
    assert seen == [(i, j) for i in range(tiles_m) for j in range(tiles_n)]
    last = tiles_m - 1 if M % 256 else -1
    ragged = sum(1 for w in walk for t in w[:-1] if t[0] == last)
    full = sum(1 for w in walk for t in w[:-1] if t[0] != last)
    return ragged, full
