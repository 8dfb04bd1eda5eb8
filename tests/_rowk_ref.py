"""Reference, derived acceptance bound and float32 emulation for the stand-alone row kernels of csrc/norm.hip:
``kw_layernorm`` (f32 residual stream) and ``kw_layernorm_bf16res`` (bf16 residual stream)
(tests/test_rowk_ref_cpu.py, tests/test_gpu_layernorm_bound.py).

The inputs follow the dyadic idea of tests/_declin_ref.py: values on a coarse power-of-two grid, so that the sum of a
row is a float32 number in whatever order it is taken and the bound on the mean is one rounding wide.  Plain numpy
(float64 for the reference and the bound, float32 for the emulation); nothing here launches a kernel.
"""
from __future__ import annotations

import numpy as np

from _declin_ref import LN_OFFSETS, U
from _gemm_ref import bf16_bits_np, recipe_a, recipe_g

F32, BF16 = "f32", "bf16"  # the residual stream (the kernel) and the output type
DIMS = {F32: (4, 8, 252, 256, 260, 384, 1280, 2044, 2048), BF16: (8, 16, 384, 504, 512, 520, 1280, 2040, 2048)}
EPS = (1e-5, 2.0 ** -6)
ROW_COUNTS = (1, 3, 4, 5, 9)  # both sides of the four-waves-per-workgroup seam, and the waves that return early
FAMILIES = ("recipe", "offset", "const", "small", "onehot")
CONST = 0.75
# offset: 1024 on the f32 stream; on the bf16 stream 32, the largest power of two P for which every P + v (v on the
# 1/4 grid, |v| <= 4 with delta) is a bf16 number: [32, 64) is spaced 1/4, [64, 128) 1/2
OFFSET = {F32: 1024.0, BF16: 32.0}
ONEHOT_COLS = (0, 3, 4, 7, 8, 255, 256, -8, -4, -1)  # negative: counted from dim


# ------------------------------------------------------------------------------------------------ bf16
def rne_bf16(a) -> np.ndarray:
    """float32 values rounded to bf16 (nearest, ties to even), as float32."""
    return (bf16_bits_np(a).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(a))


def trunc_bf16(a) -> np.ndarray:
    """float32 values cut to bf16 (the low 16 bits dropped), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(a))


def is_bf16(a) -> bool:
    a = np.asarray(a, dtype=np.float32)
    return bool(np.array_equal(rne_bf16(a), a))


def ulp_bf16(v) -> np.ndarray:
    """Spacing of the bf16 numbers around |v| (float64): 2^(floor(log2 |v|) - 7), at least the subnormal 2^-133."""
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -126))  # |v| = m 2^e, m in [1/2, 1)
    return np.ldexp(1.0, e - 8)


# ------------------------------------------------------------------------------------------------ inputs
def onehot_cols(dim: int):
    return sorted({c for c in (c + dim if c < 0 else c for c in ONEHOT_COLS) if 0 <= c < dim})


def ln_inputs(stream: str, dim: int, with_delta: bool) -> dict:
    """The rows of every family for one (stream, dim): x [R, dim] and delta [R, dim] (or None) as float32 values,
    gamma, beta [dim], ``family`` [R] (the name of each row's family) and ``post`` [R, dim] float64, the value x must
    hold after the launch (x + delta, rounded to bf16 on the bf16 stream; x itself without delta).

      recipe  five rows, the 1/4 grid in [-2, 2] plus LN_OFFSETS[m]: the mean is as large as the spread.  delta: the
              1/4 grid on the f32 stream; multiples of 1/512 in (-1/2, 1/2) on the bf16 stream, so that x + delta
              needs up to eleven significand bits and is rounded (ties included)
      offset  the grid + OFFSET[stream]: E[x^2] - mean^2 cancels seven (bf16: three) decimal digits, sum (x - mean)^2
              none.  delta: the 1/4 grid (the sums stay bf16 numbers)
      const   post is 0.75 everywhere (x = 0.75 - delta): variance 0, the result is beta
      small   f32: post = 0.5 + 2^-10 grid; bf16: post = 2^-4 + 2^-11 j, j = 0 .. 16 (bf16 numbers: [2^-4, 2^-3) is
              spaced 2^-11); variance 1.6e-6 / 5.7e-6, below either eps.  delta: f32 x = post - delta on the 1/4
              grid; bf16 delta = 2^-12 m, m = -8 .. 8 (odd m: the sum is a tie or needs rounding)
      onehot  post is zero but for a single 2.0 at column c, one row per c of ONEHOT_COLS inside the row
    gamma: multiples of 1/32 in [-2, 2], the first 4-group fixed to (1.5, 0, -0.75, 0.5); beta: multiples of 2^-10 in
    [-2, 2] (eleven significand bits: not bf16 numbers, so a bf16 store of beta rounds)."""
    rng = np.random.default_rng([2024, int(stream == BF16), dim, int(with_delta)])
    f = np.float32

    def grid(n=1):
        return recipe_a(rng, (n, dim))

    fams, xs, ds = [], [], []

    def add(name, x, d):
        for m in range(x.shape[0]):
            fams.append(name)
        xs.append(x.astype(f))
        ds.append(d.astype(f))

    fine = (rng.integers(-255, 256, size=(5, dim)) / 512.0).astype(f) if stream == BF16 else grid(5)
    add("recipe", grid(5) + np.asarray(LN_OFFSETS, dtype=f)[:, None], fine)
    add("offset", grid() + f(OFFSET[stream]), grid())
    d = grid()
    add("const", np.full((1, dim), CONST, dtype=f) - (d if with_delta else 0), d)
    if stream == F32:
        d = grid()
        add("small", f(0.5) + f(2.0 ** -10) * grid() - (d if with_delta else 0), d)
    else:
        add("small", f(2.0 ** -4) + f(2.0 ** -11) * (4 * grid() + 8), f(2.0 ** -12) * rng.integers(-8, 9, size=(1, dim)))
    cols = onehot_cols(dim)
    hot = np.zeros((len(cols), dim), dtype=f)
    hot[np.arange(len(cols)), cols] = 2.0
    d = grid(len(cols))
    add("onehot", hot - (d if with_delta else 0), d)

    x = np.concatenate(xs)
    delta = np.concatenate(ds) if with_delta else None
    gamma = recipe_g(rng, (dim,))
    gamma[:4] = (1.5, 0.0, -0.75, 0.5)
    beta = (rng.integers(-2048, 2049, size=(dim,)) / 1024.0).astype(f)
    assert (gamma < 0).any() and (gamma == 0).any() and len(set(gamma[:4])) == 4

    if stream == BF16:
        assert is_bf16(x) and (delta is None or is_bf16(delta)), "the bf16 stream's inputs must be bf16 numbers"
    if delta is None:
        post = x.astype(np.float64)
    else:
        assert is_bf16(delta)
        s32 = (x + delta).astype(f)
        assert np.array_equal(s32.astype(np.float64), x.astype(np.float64) + delta.astype(np.float64)), \
            "x + delta must be exact in float32"
        post = (rne_bf16(s32) if stream == BF16 else s32).astype(np.float64)
        if stream == BF16:
            rounded = (post != s32)[np.asarray(fams) == "recipe"]
            assert rounded.mean() > 0.25, "the bf16 stream's recipe sums must need rounding"
    fam = np.asarray(fams)
    assert np.all(post[fam == "const"] == CONST)
    assert np.array_equal(post[fam == "onehot"], hot)
    return dict(x=x, delta=delta, gamma=gamma, beta=beta, family=fam, post=post)


def row_windows(n_rows: int):
    """The launches of one case: for each count of ROW_COUNTS the pool rows it takes (consecutive, wrapping), so that
    every row of a pool of up to sum(ROW_COUNTS) rows is launched at least once."""
    out, at = [], 0
    for r in ROW_COUNTS:
        out.append([(at + i) % n_rows for i in range(r)])
        at += r
    assert n_rows <= at
    return out


# ------------------------------------------------------------------------------------------------ reference
def ln_reference(x64, g64, b64, eps) -> np.ndarray:
    """float64 LayerNorm of each row of x64 [R, dim]: (x - mean) / sqrt(var + eps) gamma + beta with the biased
    variance; ``eps`` is taken as the float32 the kernel receives."""
    eps = float(np.float32(eps))
    x64 = np.asarray(x64, dtype=np.float64)
    mu = x64.mean(axis=1, keepdims=True)
    t = x64 - mu
    var = (t * t).mean(axis=1, keepdims=True)
    return t / np.sqrt(var + eps) * np.asarray(g64, dtype=np.float64)[None, :] + np.asarray(b64, dtype=np.float64)[None, :]


def _g(n):
    return n * U / (1.0 - n * U)


def _iters(stream: str, dim: int) -> int:
    """The loop iterations in which a lane holds elements: 64 lanes of 4 (f32 stream) or 8 (bf16 stream) each."""
    return -(-dim // (256 if stream == F32 else 512))


def sum_depth(stream: str, dim: int) -> int:
    """The most float32 additions one element passes through on its way into wave_sum(s)'s result.
    layernorm_kernel: ``s += (v.x + v.y) + (v.z + v.w)`` is two additions inside the group and one into s per
    iteration from the element's own on; the first, into s = 0, is exact: n + 1 for n iterations.
    layernorm_bf16res_kernel: ``for e: s += v[i][e]`` is one addition per element from its own on, the first into 0
    exact: 8 n - 1.  wave_sum (kw_common.h) adds six butterfly levels."""
    n = _iters(stream, dim)
    return (n + 1 if stream == F32 else 8 * n - 1) + 6


def sq_depth(stream: str, dim: int) -> int:
    """The same for wave_sum(q), the squaring included.  layernorm_kernel: ``q += (a * a + b * b) + (cc * cc + d * d)``
    is the product, two additions inside the group, then as the sum: n + 2.  layernorm_bf16res_kernel:
    ``q = fmaf(a, a, q)`` is one rounding per element from its own on: 8 n.  Six butterfly levels on top.  (A
    compiler that contracts a * a + b * b into an fma drops a rounding.)"""
    n = _iters(stream, dim)
    return (n + 2 if stream == F32 else 8 * n) + 6


def sum_is_exact(x64) -> np.ndarray:
    """[R] bool: the row's values are multiples of one power of two 2^-k, k <= 40, and sum |x| stays below 2^24 of
    them.  Then every partial sum, in any order, is a float32 number and the kernel's sum of the row is exact."""
    x64 = np.asarray(x64, dtype=np.float64)
    exact = np.zeros(x64.shape[0], dtype=bool)
    for k in range(41):
        scaled = np.ldexp(x64, k)
        exact |= (scaled == np.rint(scaled)).all(axis=1) & (np.abs(scaled).sum(axis=1) < 2.0 ** 24)
    return exact


def ln_bound(x64, g64, b64, eps, out_dtype: str, stream: str = F32) -> np.ndarray:
    """Elementwise acceptance bound of a row kernel's result against ``ln_reference``, x64 being the values the row
    holds after the residual add (float32 / bf16 numbers: the add itself is checked bit for bit).  Derived from the
    operations of layernorm_kernel and layernorm_bf16res_kernel (csrc/norm.hip); every rounded float32 operation is
    charged half an ulp (relative u = 2^-24; the divisions compile to the correctly rounded v_div_scale / v_div_fmas /
    v_div_fixup sequence), rsqrtf one ulp, the allowance of _declin_ref.ln_bound.  g(n) = n u / (1 - n u) bounds n
    compounded roundings.  mu, t_j = x_j - mu, var = mean t_j^2, E = var + eps, R = E^-1/2 are the true values, Ds =
    ``sum_depth`` and Dq = ``sq_depth`` the depths of the two summation trees.

      mean = wave_sum(s) / (float)dim       the sum is sum x_j (1 + th_j), |th_j| <= g(Ds), the division one more:
                                            |mean - mu| <= g(Ds + 1) mean|x_j|.  Where ``sum_is_exact`` (the dyadic
                                            families) the sum has no rounding at all: |mean - mu| <= u |mu|   =: dmu
      d_j  = v - mean                       d_j = t_j + c + rho_j, c = mu - mean, |rho_j| <= u (|t_j| + dmu) =: r_j
                                            (computed twice, in the q loop and in the output loop: the same value)
      q    = wave_sum(q) / (float)dim       sum d_j^2 = sum t_j^2 + dim c^2 + sum (2 (t_j + c) rho_j + rho_j^2), the
                                            cross term 2 c sum t_j being zero; each d_j^2 enters with (1 + th_j),
                                            |th_j| <= g(Dq + 1) with the division:
                                            |q - var| <= dmu^2 + mean(2 (|t_j| + dmu) r_j + r_j^2)
                                                         + g(Dq + 1) mean((|t_j| + dmu + r_j)^2)              =: dv
      e    = q + eps                        |e - E| <= dv + u (E + dv);  rel(e) = that / E
      rstd = rsqrtf(e)                      (1 + r)^-1/2 - 1 is within |r| / 2 + r^2 for |r| <= 0.1 (asserted):
                                            rel(rstd) = rel(e) / 2 + rel(e)^2 + 2 u (1 + rel(e))
      p1   = (v - mean) * rstd              |d_j rstd - t_j R| <= R (|t_j| rel(rstd) + (dmu + r_j) (1 + rel(rstd))) =: a1
                                            |p1 - t_j R| <= a1 + u (|t_j| R + a1)                              =: a2
      p2   = p1 * gg                        |p2 - t_j R g| <= |g| a2 + u |g| (|t_j| R + a2)                    =: a3
      out  = p2 + bb                        |out - ref| <= a3 + u (|ref| + a3)                                 =: a4
                                            (contracted into one fma the last two lose a rounding and stay inside)
      f2bf / pack_bf16x2 (bf16 y)           round to nearest even: half a bf16 ulp of the float32 result, whose
                                            magnitude is at most |ref| + a4: + ulp_bf16(|ref| + a4) / 2

    Constant rows (t = 0, the sum exact) have mean = mu exactly, d = 0 and out = fl(0 + bb) = bb: the tests ask for
    beta bit for bit there, on top of this bound."""
    eps = float(np.float32(eps))
    x64 = np.asarray(x64, dtype=np.float64)
    g64 = np.asarray(g64, dtype=np.float64)[None, :]
    b64 = np.asarray(b64, dtype=np.float64)[None, :]
    dim = x64.shape[1]
    mu = x64.mean(axis=1, keepdims=True)
    t = np.abs(x64 - mu)
    var = (t * t).mean(axis=1, keepdims=True)
    E = var + eps
    R = 1.0 / np.sqrt(E)
    dmu = np.where(sum_is_exact(x64)[:, None], U * np.abs(mu),
                   _g(sum_depth(stream, dim) + 1) * np.abs(x64).mean(axis=1, keepdims=True))
    at = t + dmu
    r = U * at
    dv = dmu ** 2 + (2 * at * r + r * r).mean(axis=1, keepdims=True) \
        + _g(sq_depth(stream, dim) + 1) * ((at + r) ** 2).mean(axis=1, keepdims=True)
    rel_e = (dv + U * (E + dv)) / E
    assert float(rel_e.max()) <= 0.1, f"rel(e) = {float(rel_e.max()):.3g}: the rsqrt expansion needs <= 0.1"
    rel_r = rel_e / 2 + rel_e * rel_e + 2 * U * (1 + rel_e)
    a1 = R * (t * rel_r + (dmu + r) * (1 + rel_r))
    a2 = a1 + U * (t * R + a1)
    a3 = np.abs(g64) * a2 + U * np.abs(g64) * (t * R + a2)
    ref = np.abs((x64 - mu) * R * g64 + b64)
    a4 = a3 + U * (ref + a3)
    if out_dtype == BF16:
        a4 = a4 + ulp_bf16(ref + a4) / 2
    return a4


def ratio(got64, ref64, bound64) -> np.ndarray:
    """|got - ref| / bound, 0 where the result is the reference itself, inf where it is not finite."""
    err = np.abs(np.asarray(got64, dtype=np.float64) - ref64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / bound64)
    return np.where(np.isfinite(q), q, np.inf)


# ------------------------------------------------------------------------------------------------ f32 emulation
MUTANTS = ("one_pass", "drop_eps", "eps_outside", "dim_minus_1", "padded_dim", "swap_gamma", "bf16_truncate",
           "stats_before_delta", "unrounded_residual")


def _wave_tree(lane_vals: np.ndarray) -> np.ndarray:
    """wave_sum's xor butterfly over [R, 64] float32 lane values -> [R]."""
    idx = np.arange(64)
    v = lane_vals
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, idx ^ o]).astype(np.float32)
    return v[:, 0]


def tree_sum(a, stream: str, square: bool = False) -> np.ndarray:
    """The kernels' sum of each row of a [R, dim] float32 (of its squares with ``square``), addition by addition in
    float32: element 4 (64 i + lane) + k (f32 stream) or 8 (64 i + lane) + e (bf16 stream) belongs to lane ``lane``
    in iteration i; the tail of the last iteration is zeros, which change no sum."""
    f = np.float32
    a = np.asarray(a, dtype=f)
    R, dim = a.shape
    w = 4 if stream == F32 else 8
    n = _iters(stream, dim)
    p = np.zeros((R, n * 64 * w), dtype=f)
    p[:, :dim] = a
    p = p.reshape(R, n, 64, w)
    s = np.zeros((R, 64), dtype=f)
    for i in range(n):
        c = p[:, i]
        if stream == F32:
            if square:
                c = (c * c).astype(f)
            s = (s + ((c[..., 0] + c[..., 1]).astype(f) + (c[..., 2] + c[..., 3]).astype(f)).astype(f)).astype(f)
        else:
            for e in range(8):
                if square:  # fmaf(a, a, q): the product is exact in float64, one rounding to float32
                    s = (c[..., e].astype(np.float64) ** 2 + s.astype(np.float64)).astype(f)
                else:
                    s = (s + c[..., e]).astype(f)
    return _wave_tree(s)


def emulate_ln_f32(x, g, b, eps, *, stream: str = F32, delta=None, out_dtype: str = F32, one_pass=False,
                   drop_eps=False, eps_outside=False, dim_minus_1=False, padded_dim=False, swap_gamma=False,
                   bf16_truncate=False, stats_before_delta=False, unrounded_residual=False):
    """layernorm_kernel / layernorm_bf16res_kernel in numpy float32, operation by operation: returns (x after the
    launch, y as it reads back), both float32 arrays.  rsqrtf is the correctly rounded 1 / sqrt.  The keyword
    switches are the corruptions that tests/test_rowk_ref_cpu.py expects ``ln_bound`` to refuse:
      one_pass             var = E[x^2] - mean^2 (clamped at 0) in place of mean((x - mean)^2)
      drop_eps             rsqrt(var)
      eps_outside          rsqrt(var) + eps
      dim_minus_1          the unbiased variance, sum / (dim - 1)
      padded_dim           mean and variance divided by dim rounded up to 256
      swap_gamma           gamma of the neighbouring column (j ^ 1) inside each 4-group
      bf16_truncate        a bf16 y cut instead of rounded
      stats_before_delta   mean and rstd of x, applied to x + delta
      unrounded_residual   bf16 stream: x + delta written back rounded, but normalised before the rounding"""
    f = np.float32
    x = np.asarray(x, dtype=f)
    g = np.asarray(g, dtype=f)
    b = np.asarray(b, dtype=f)
    dim = x.shape[1]
    v = x_after = x
    if delta is not None:
        v = (x + np.asarray(delta, dtype=f)).astype(f)
        x_after = rne_bf16(v) if stream == BF16 else v
        if not unrounded_residual:
            v = x_after
    sv = x if (stats_before_delta and delta is not None) else v
    n = f(-(-dim // 256) * 256 if padded_dim else dim)
    mean = (tree_sum(sv, stream) / n).astype(f)[:, None]
    if one_pass:
        msq = (tree_sum(sv, stream, square=True) / n).astype(f)[:, None]
        var = np.maximum((msq - (mean * mean).astype(f)).astype(f), f(0.0))
    else:
        nv = f(dim - 1) if dim_minus_1 else n
        var = (tree_sum((sv - mean).astype(f), stream, square=True) / nv).astype(f)[:, None]
    with np.errstate(divide="ignore"):
        if eps_outside:
            rstd = ((1.0 / np.sqrt(var.astype(np.float64))).astype(f) + f(eps)).astype(f)
        else:
            e = var if drop_eps else (var + f(eps)).astype(f)
            rstd = (1.0 / np.sqrt(e.astype(np.float64))).astype(f)
    if swap_gamma:
        g = g[np.arange(dim) ^ 1]
    with np.errstate(invalid="ignore", over="ignore"):
        o = ((((v - mean).astype(f) * rstd).astype(f) * g[None, :]).astype(f) + b[None, :]).astype(f)
    if out_dtype == BF16:
        o = trunc_bf16(o) if bf16_truncate else rne_bf16(o)
    return x_after, o
