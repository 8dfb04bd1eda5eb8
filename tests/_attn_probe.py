"""Read back every key's softmax weight from an attention kernel, and compare it with float64 softmax.

The attention output is linear in V.  With Q and K fixed, a launch whose V holds the unit vector e_i in row 64 c + i
(block c of the key range, all other rows zero) returns, in output column i, the softmax weight of key 64 c + i and
nothing else: no column ever sums two keys, so the kernel's accumulation adds no error of its own.  ceil(T / 64)
launches return the kernel's whole weight matrix P^ [rows][T]; the first launch is repeated last, on the same
workspace, and must be bit-identical.  Plain torch, device-agnostic: the CPU tests run it over a torch attention with
planted faults (tests/test_attn_probe_cpu.py), the GPU tests over every attention kernel
(tests/test_gpu_attn_weights.py).

Checks (``check_weights``), all per (row, key):
  * relative error: |P^ - P| <= rtol * P wherever the mask admits the key -- no absolute term, a dropped or doubled key
    is a 100 % error whatever its weight;
  * exact zeros: P^ == 0 wherever the mask excludes the key, and in the columns past T of the last block (their V rows
    hold ones when the kernel's cache is longer than T);
  * row sums: |sum_k P^ - 1| <= rtol; a row with no key sums to exactly 0;
  * repeatability: the repeated first launch equals the first one bit for bit.

The bf16 bound: bf16 has unit roundoff 2^-8, a kernel that rounds n values to bf16 on the way from a score to the output
is off by about n 2^-8 at most, and one more 2^-8 covers its f32 terms: rtol = (n + 1) 2^-8 (``bf16_rtol``).
"""
from __future__ import annotations

import torch

BLOCK = 64  # keys per launch = the head dim: one output column per key
LOG2E = 1.4426950408889634
# A weight below 2^-100 may underflow inside a kernel (f32 and bf16 both end at 2^-126; every intermediate of an online
# softmax is at least the final weight, so from 2^-100 up all of them are normal numbers with 26 binades to spare).
# Only input sets that are MEANT to reach below it (the K ramp, whose scores spread over hundreds) pass this floor:
# under it the relative check gives way to P^ <= 2 floor.
UNDERFLOW_FLOOR = 2.0 ** -100


def bf16_rtol(n: int) -> float:
    """The bound of a bf16 kernel that rounds ``n`` values to bf16 between a score and the output."""
    return (n + 1) * 2.0 ** -8


def n_blocks(T: int) -> int:
    return -(-T // BLOCK)


def unit_values(T: int, c: int, t_total: int | None = None, device="cpu") -> torch.Tensor:
    """V of launch c, f32 [t_total][64]: row 64 c + i = e_i for the keys of block c below T; the block's rows from T
    on (slots of a cache longer than T) hold ones, so a kernel that admits one of them shows it in every column;
    every other row is zero."""
    t_total = T if t_total is None else t_total
    v = torch.zeros(t_total, BLOCK, device=device)
    lo, hi = c * BLOCK, min((c + 1) * BLOCK, t_total)
    n_unit = max(min(hi, T) - lo, 0)
    idx = torch.arange(n_unit, device=device)
    v[lo + idx, idx] = 1.0
    if hi > max(T, lo):
        v[max(T, lo):hi] = 1.0
    return v


def probe_weights(run, T: int, t_total: int | None = None, device="cpu"):
    """``run(V) -> out``: one launch of the kernel with the values V (``unit_values``; how they reach the kernel's
    rows, heads and caches is the caller's) returning its output as [rows][64] (any dtype).  All launches must share
    one workspace.  Returns (P^ float64 [rows][64 ceil(T / 64)], repeatable): the weights of all keys, the columns
    past T included, and whether the first block's launch, repeated as the last launch, gave the same bits."""
    cols, first = [], None
    for c in range(n_blocks(T)):
        out = run(unit_values(T, c, t_total, device)).detach().clone()
        if c == 0:
            first = out
        cols.append(out.double().reshape(-1, BLOCK))
    again = run(unit_values(T, 0, t_total, device)).detach().clone()
    same = first.dtype == again.dtype and first.shape == again.shape and torch.equal(
        first.contiguous().view(torch.uint8), again.contiguous().view(torch.uint8))
    return torch.cat(cols, 1), same


def reference_weights(q: torch.Tensor, k: torch.Tensor, mask: torch.Tensor | None = None,
                      q_log2: bool = False) -> torch.Tensor:
    """float64 P = softmax(mask(q k^T)) of the values the kernel is given: ``q`` [..., R, 64] and ``k`` [..., T, 64]
    as the kernel reads them (already cast to its dtype; fp8 keys dequantised), ``mask`` [..., R, T] bool (True: the
    key is admitted).  ``q_log2``: q carries log2 e and is divided back.  A row with no key gives zeros."""
    qd = q.double()
    if q_log2:
        qd = qd / LOG2E
    s = qd @ k.double().transpose(-1, -2)
    if mask is None:
        return torch.softmax(s, -1)
    s = s.masked_fill(~mask, float("-inf"))
    any_key = mask.any(-1, keepdim=True)
    p = torch.softmax(torch.where(any_key, s, torch.zeros_like(s)), -1)
    return torch.where(mask, p, torch.zeros_like(p))


def weight_errors(p_hat: torch.Tensor, p: torch.Tensor, mask: torch.Tensor | None = None, floor: float = 0.0):
    """The figures ``check_weights`` asserts on: (max relative error over admitted keys with P >= floor, number of
    non-zero weights on excluded keys, max |row sum - 1| over rows with a key, max row sum of rows without one, max P^
    over admitted keys under the floor)."""
    rows, T = p.shape
    if mask is None:
        mask = torch.ones(rows, T, dtype=torch.bool, device=p.device)
    full = torch.zeros(rows, p_hat.shape[1], dtype=torch.bool, device=p.device)
    full[:, :T] = mask
    pf = torch.zeros(rows, p_hat.shape[1], dtype=torch.float64, device=p.device)
    pf[:, :T] = p
    checked = full & (pf >= floor)
    under = full & ~checked
    rel = ((p_hat - pf).abs() / pf.clamp_min(1e-300))
    rel = torch.where(torch.isfinite(p_hat), rel, torch.full_like(rel, float("inf")))
    max_rel = float(rel[checked].max()) if checked.any() else 0.0
    bad_zero = int((p_hat[~full] != 0).sum())  # (NaN != 0: counted)
    has_key = mask.any(-1)
    sums = p_hat.sum(-1)
    sum_err = float((sums[has_key] - 1).abs().max()) if has_key.any() else 0.0
    if has_key.any() and not torch.isfinite(sums[has_key]).all():
        sum_err = float("inf")
    empty = float(sums[~has_key].abs().max()) if (~has_key).any() else 0.0
    if (~has_key).any() and not torch.isfinite(sums[~has_key]).all():
        empty = float("inf")
    max_under = float(p_hat[under].abs().max()) if under.any() else 0.0
    if under.any() and not torch.isfinite(p_hat[under]).all():
        max_under = float("inf")
    return max_rel, bad_zero, sum_err, empty, max_under


def check_weights(p_hat: torch.Tensor, p: torch.Tensor, rtol: float, mask: torch.Tensor | None = None,
                  repeatable: bool = True, floor: float = 0.0, what: str = "") -> float:
    """Assert the four properties of the module docstring on P^ [rows][>= T] against P [rows][T] (``mask`` [rows][T],
    None: every key admitted).  ``floor``: 0, or UNDERFLOW_FLOOR for input sets whose weights reach below it.
    Returns the maximum relative error, for the record."""
    max_rel, bad_zero, sum_err, empty, max_under = weight_errors(p_hat, p, mask, floor)
    if max_rel > rtol:
        rows, T = p.shape
        rel = (p_hat[:, :T] - p).abs() / p.clamp_min(1e-300)
        if mask is not None:
            rel = torch.where(mask, rel, torch.zeros_like(rel))
        rel = torch.where(p >= floor, rel, torch.zeros_like(rel))
        rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
        r, kk = divmod(int(rel.argmax()), T)
        raise AssertionError(f"{what}: weight of key {kk} in row {r} is {float(p_hat[r, kk]):.6g}, float64 softmax "
                             f"{float(p[r, kk]):.6g}: relative error {max_rel:.3g} > {rtol:.3g}")
    assert bad_zero == 0, f"{what}: {bad_zero} excluded keys carry a non-zero weight"
    assert sum_err <= rtol, f"{what}: a row's weights sum to 1 +- {sum_err:.3g} > {rtol:.3g}"
    assert empty == 0.0, f"{what}: a row without a key has weights summing to {empty:.3g}"
    assert max_under <= 2 * floor, f"{what}: a weight under the underflow floor reads {max_under:.3g}"
    assert repeatable, f"{what}: the repeated first launch is not bit-identical"
    return max_rel


def plant_spike(q_row: torch.Tensor, score: float = 12.0) -> torch.Tensor:
    """The key whose score against ``q_row`` [..., 64] is ``score``: q score / |q|^2."""
    return q_row * (score / (q_row * q_row).sum(-1, keepdim=True))


def ramp(T: int, amount: float, device="cpu") -> torch.Tensor:
    """The K ramp of test_attention_bf16_q_log2_reference_moves, [T][1]: key t is scaled by 1 + amount t / T, so
    that scores grow along the sequence and the running maximum moves in most tiles."""
    return (1.0 + amount * torch.arange(T, device=device, dtype=torch.float32) / T)[:, None]


def is_close_mixed(out: torch.Tensor, ref: torch.Tensor, tol: float) -> bool:
    """The check the suite had before: assert_close(out, ref, atol = rtol = tol) on softmax(Q K^T) V, as a bool."""
    return bool(((out.double() - ref.double()).abs() <= tol + tol * ref.double().abs()).all())
