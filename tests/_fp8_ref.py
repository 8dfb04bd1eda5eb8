"""The fp8 cross K/V format of include/kwhisper.h ("fp8 cross K/V") restated on the CPU with torch: quantise,
dequantise and the scales, bit for bit what kw_cross_kv_quant must write.

Per channel (one head dim of one [S][64] tile), from the bf16 values x:
  a = max_s |x|;  scale = a / 448;  inv = 448 / a  (f32, one correctly rounded division);  a == 0: scale = inv = 0 and
  every code 0;  code = e4m3fn_rne(x * inv)  (one f32 multiply; a product that passes 448 by rounding is 448).
Dequantised value: float(code) * scale.
"""
from __future__ import annotations

import numpy as np
import torch

E4M3_MAX = 448.0


def quantize(x) -> tuple[np.ndarray, np.ndarray]:
    """x [..., S, D] (bf16 tensor, or any array of bf16-representable values) -> (codes uint8 [..., S, D], scales f32 [..., D]).
    The divisions and the multiply are numpy float32 operations (IEEE, correctly rounded: ``scalar / tensor`` in torch
    is a reciprocal and a multiply, two roundings); torch only casts the products to e4m3fn (round to nearest even)."""
    x = x.detach().cpu().float().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float32)
    a = np.abs(x).max(axis=-2)
    scale = (a / np.float32(E4M3_MAX)).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(a > 0, np.float32(E4M3_MAX) / a, np.float32(0)).astype(np.float32)
    y = np.clip(x * inv[..., None, :], -E4M3_MAX, E4M3_MAX).astype(np.float32)
    codes = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return np.where((a > 0)[..., None, :], codes, np.uint8(0)).astype(np.uint8), scale


def decode(codes) -> np.ndarray:
    """e4m3fn codes (uint8) -> their f32 values."""
    return torch.as_tensor(np.ascontiguousarray(codes)).view(torch.float8_e4m3fn).float().numpy()


def dequantize(codes, scales) -> np.ndarray:
    """(codes [..., S, D], scales [..., D]) -> f32 [..., S, D]: float(code) * scale, one f32 multiply."""
    return decode(codes) * np.asarray(scales, dtype=np.float32)[..., None, :]


def fake_quant(x) -> np.ndarray:
    """Round to bf16, quantise and dequantise: the values an fp8 cache stands for."""
    xb = torch.as_tensor(np.asarray(x, dtype=np.float32)).bfloat16()
    return dequantize(*quantize(xb))


def exact_case(rng: np.random.Generator, n: int, S: int, D: int = 64):
    """A tile set that the format represents exactly: per channel, random finite e4m3 codes with one +-448 planted,
    times a power-of-two channel scale (every product is exact in bf16).  Returns (x f32 [n][S][D], codes uint8,
    scales f32 [n][D]); quantising x must give back exactly these codes and scales.  Zero codes are drawn as +0."""
    codes = rng.integers(0, 256, size=(n, S, D), dtype=np.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0x38  # NaN patterns -> 1.0
    codes[codes == 0x80] = 0  # -0 -> +0
    peak = rng.integers(0, S, size=(n, D))
    sign = rng.integers(0, 2, size=(n, D)).astype(np.uint8) << 7
    np.put_along_axis(codes, peak[:, None, :], (0x7E | sign)[:, None, :], axis=1)  # 0x7E = 448
    exp = rng.integers(-6, 7, size=(n, D))
    scales = np.ldexp(np.float32(1.0), exp).astype(np.float32)
    x = decode(codes) * scales[:, None, :]
    return x.astype(np.float32), codes, scales
