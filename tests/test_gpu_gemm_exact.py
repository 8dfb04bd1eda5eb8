"""kw_gemm on the MI355X against an exact reference, bit for bit, at every tile and batch seam.

Inputs come from the dyadic recipe of tests/_gemm_ref.py: every product and partial sum is a float32 number, so a
result without GELU has one right f32 and one right bf16 bit pattern and the comparison is bitwise (the only
tolerances are the two GELU bounds of family 7).  Every case launches twice into two freshly guarded buffers (C sits
among sentinel NaNs: before, after, between batches, right of column N, one spare head-split part): both images must
hold the expected bits and every guard element must still hold the sentinel.  The reference is float64,
A.double() @ W.double().T on the device (exact for these inputs in any order) and the float64 restatement of
``epi_one``.  One accumulation per shape is shared by every epilogue run on it.

Families (the case table with the measured GELU numbers: profiles/gemm_exact.md):
 1 gemm_bf16_kernel (128x128)        2 gemm256_kernel, one tile per workgroup     3 gemm256_kernel, persistent walk
 4 either side of use256()           5 A rows 4 GiB past the base                 6 gemm_f32_kernel
 7 GELU bounds                       8 rejections and M = 0                       9 mel_to_time_major
"""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _gemm_ref as R  # noqa: E402
from kwhisper import _lib as L  # noqa: E402
from kwhisper import ops  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
GELU_REPORT = []  # (kernel, K, C dtype, measured, bound or torch's own error): printed, and written where
#                   KW_GEMM_EXACT_REPORT names a file


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    yield
    path = os.environ.get("KW_GEMM_EXACT_REPORT")
    if path and GELU_REPORT:
        with open(path, "w") as f:
            f.write("| kernel | K | C | measured | reference figure |\n|---|---|---|---|---|\n")
            for row in GELU_REPORT:
                f.write("| " + " | ".join(str(c) for c in row) + " |\n")


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def _backend(name):
    old = ops.set_backend(name)
    try:
        yield
    finally:
        ops.set_backend(old)


class Epi:
    """One epilogue configuration of kw_gemm."""

    def __init__(self, name, c_dtype, *, epilogue=R.STORE, gelu=False, scale=1.0, scale_cols=0, bias=True, period=0,
                 ra_shift=0, hs=None):
        self.name, self.c_dtype, self.epilogue, self.gelu = name, c_dtype, epilogue, gelu
        self.scale, self.scale_cols, self.bias, self.period, self.ra_shift, self.hs = scale, scale_cols, bias, period, ra_shift, hs


class Problem:
    """The inputs of one shape and their exact accumulation A . W^T (float64), shared by every epilogue run on it.
    The A buffer is recipe values throughout, gaps between rows included, so a row read from the wrong place shows."""

    def __init__(self, M, N, K, in_dtype=BF, al=None, seed=0, abuf=None):
        self.M, self.N, self.K, self.in_dtype = M, N, K, in_dtype
        self.al = al or R.ALayout(K)
        self.rng = np.random.default_rng([seed, M, N, K])
        if abuf is None:
            abuf = R.to_device(R.recipe_a(self.rng, self.al.span(M, K) + 8), in_dtype, DEV)
        self.abuf = abuf
        self.W = R.to_device(R.recipe_w(self.rng, (N, K)), in_dtype, DEV)
        self.bias = R.to_device(R.recipe_g(self.rng, N), F32, DEV)
        A = R.gather_rows(self.abuf, self.al, M, K)
        R.assert_exact(A, self.W)
        self.acc = A.double() @ self.W.double().t()
        self._ra, self._base = {}, None

    def row_add(self, period, shift=0):
        """The [period, N] f32 table, ``shift`` floats past a 16-B aligned address (the same values at any shift)."""
        if (period, shift) not in self._ra:
            if (period, 0) not in self._ra:
                self._ra[(period, 0)] = R.to_device(R.recipe_g(self.rng, (period, self.N)), F32, DEV)
            t = torch.zeros(shift + period * self.N, dtype=F32, device=DEV)
            t[shift:] = self._ra[(period, 0)].reshape(-1)
            self._ra[(period, shift)] = t[shift:].view(period, self.N)
        return self._ra[(period, shift)]

    def base(self):
        if self._base is None:
            self._base = R.to_device(R.recipe_g(self.rng, (self.M, self.N)), F32, DEV).double()
        return self._base


def pick_seq(M, limit=100):
    """The largest divisor of M up to ``limit``: a head-split sequence length with several batches inside a tile."""
    return max(d for d in range(1, min(M, limit) + 1) if M % d == 0)


def all_epilogues(M, N, *, hs=None):
    """The epilogue set every family runs (GELU apart): STORE f32, STORE bf16 without bias, a column scale whose
    boundary is no multiple of 8 (one 8-column store piece of the 256 kernel straddles it), row_add with period 7
    (divides neither 128 nor 256), RESID, HEADSPLIT with scale_cols = heads * head_dim."""
    hs = hs or (pick_seq(M), 2, 64)
    sc = 100 if N > 100 else 37
    return [
        Epi("store_f32", F32),
        Epi("store_bf16_nobias", BF, bias=False),
        Epi(f"scale{sc}_bf16", BF, scale=0.125, scale_cols=sc),
        Epi("rowadd7_f32", F32, period=7),
        Epi("resid", F32, epilogue=R.RESID),
        Epi("headsplit_bf16", BF, epilogue=R.HEADSPLIT, scale=0.5, scale_cols=hs[1] * hs[2], hs=hs),
    ]


def layout_for(e, N, *, pad=8, rpb=0, gap=0, front=64, back=64):
    """C's guarded layout for an epilogue: ldc = N + pad, and with ``rpb`` rows per batch ``gap`` extra elements
    between batches.  pad / gap / front in multiples of 8 keep the call eligible for the 256 kernel."""
    if e.epilogue == R.HEADSPLIT:
        return R.CLayout(seq=e.hs[0], heads=e.hs[1], hd=e.hs[2], front=front, back=back)
    ldc = N + pad
    return R.CLayout(ldc=ldc, rpb=rpb, bs=(rpb * ldc + gap) if rpb else 0, front=front, back=back)


def launch(p, e, lay, *, backends=("torch",), tag=""):
    """Run epilogue ``e`` of problem ``p`` twice per backend into fresh guarded buffers; assert the bits (exact
    cases) and the guards.  Returns (first buffer, element offsets, pre-activation, float64 result)."""
    M, N, K = p.M, p.N, p.K
    idx, total = R.element_offsets(lay, M, N, DEV)
    bias = p.bias if e.bias else None
    ra = p.row_add(e.period, e.ra_shift) if e.period else None
    base = p.base() if e.epilogue == R.RESID else None
    pre, val = R.reference(p.acc, bias=bias, epilogue=e.epilogue, gelu=e.gelu, scale=e.scale, scale_cols=e.scale_cols,
                           row_add=ra, row_add_period=e.period, base=base)
    want = None
    if e.gelu:
        R.assert_gelu_share(pre)
    else:
        want = R.expected_bits(val, e.c_dtype)
    outs = []
    for be in backends:
        with _backend(be):
            for _ in range(2):
                buf = R.guarded(total, e.c_dtype, DEV)
                if base is not None:
                    R.plant(buf, idx, base)
                ops.GemmPlan(p.abuf, p.W, buf, M, N, K, bias=bias, lda=p.al.lda, a_rows_per_batch=p.al.rpb,
                             a_batch_stride=p.al.bs, a_offset=p.al.front, ldc=lay.ldc or N, c_rows_per_batch=lay.rpb,
                             c_batch_stride=lay.bs, c_offset=lay.front, epilogue=e.epilogue, gelu=e.gelu, scale=e.scale,
                             scale_cols=e.scale_cols, row_add=ra, row_add_period=e.period, hs_seq=lay.seq,
                             hs_heads=lay.heads, hs_head_dim=lay.hd)()
                outs.append(buf)
    torch.cuda.synchronize()
    what = f"{tag} M={M} N={N} K={K} {e.name}"
    for i, buf in enumerate(outs):
        stray, wrong = R.check_guarded(buf, idx, want)
        assert stray.numel() == 0 and wrong.shape[0] == 0, f"{what} launch {i}: " + R.describe(stray, wrong)
        if i:  # GELU cases carry no expected bits: the launches must still agree with each other
            assert torch.equal(R.bits_of(buf), R.bits_of(outs[0])), f"{what}: launch {i} differs from launch 0"
    return outs[0], idx, pre, val


def run_all(p, *, backends=("torch",), tag="", rpb=0, gap=0, hs=None, skip=()):
    for e in all_epilogues(p.M, p.N, hs=hs):
        if e.name in skip:
            continue
        launch(p, e, layout_for(e, p.N, rpb=rpb, gap=gap), backends=backends, tag=tag)


# ---------------------------------------------------------------------------------------------- 1: the 128x128 kernel
# M < 1024: use256() refuses every one of these.  Row tiles x column tiles = 1 .. 24 workgroups: the XCD remap with
# q8 = 0 (fewer than 8), r8 != 0 and r8 = 0; K = 64 / 128 / 192: 1, 2, 3 K-tiles, both parities of the two-stage ring.
@pytest.mark.parametrize("K", [64, 128, 192])
@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("M", [1, 127, 128, 129, 600, 1023])
def test_128_kernel(M, N, K):
    both = (M, N, K) == (600, 384, 192)
    run_all(Problem(M, N, K), backends=("torch", "ctypes") if both else ("torch",), tag="128")


def test_128_kernel_lda_wider_than_k():
    run_all(Problem(129, 128, 128, al=R.ALayout(128 + 8, front=16)), tag="128 lda>K")


def test_128_kernel_stride2_conv_rowmap():
    """conv2 of the stem as a GEMM: row (b, t) reads 3 d contiguous elements from time row 2 t of batch b's T + 2
    padded rows (lda = 2 d, a_rows_per_batch = T / 2, a_batch_stride = (T + 2) d); T = 10, d = 64, 26 batches."""
    d, T, B = 64, 10, 26
    p = Problem(B * (T // 2), 128, 3 * d, al=R.ALayout(2 * d, rpb=T // 2, bs=(T + 2) * d))
    run_all(p, tag="128 conv2 rowmap", hs=(T // 2, 2, 64))


def test_128_kernel_seven_rows_per_batch():
    run_all(Problem(600, 128, 64), tag="128 c_rpb=7", rpb=7, gap=24, skip=("headsplit_bf16",))
    run_all(Problem(602, 128, 64), tag="128 hs_seq=7", hs=(7, 2, 64), skip=("store_f32", "store_bf16_nobias", "resid"))


# ---------------------------------------------------------------------------------------------- 2: 256 kernel, one tile per WG
# M >= 1024, N % 256 == 0, 16-B aligned C: use256() takes them.  5 row tiles, the last with 0 / 1 / 127 / 129 / 255 live
# rows (at 1 and 127 group 1 of the workgroup stores nothing); K-tile counts 1 .. 5 (both ring parities, nk = 1 and 2
# take the short prologue).
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320])
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("M", [1024, 1025, 1151, 1153, 1279])
def test_256_kernel(M, N, K):
    both = (M, N, K) == (1153, 768, 192)
    run_all(Problem(M, N, K), backends=("torch", "ctypes") if both else ("torch",), tag="256")


def test_256_kernel_k1280():
    run_all(Problem(1153, 256, 1280), tag="256 K=1280")


@pytest.mark.parametrize("rpb", [7, 100, 255, 256, 300])
def test_256_kernel_batch_seams(rpb):
    """Rows per batch below 256 take the epilogue's per-row division (``!linear``); 256 and 300 take the
    one-boundary-per-tile shortcut with the boundary inside a tile (300: inside the ragged tile 1024 .. 1278 as
    well).  c_batch_stride != rows * ldc.  Head split: 4 parts, 2 heads of 64, into bf16 and into f32."""
    p = Problem(1279, 256, 128)
    run_all(p, tag=f"256 c_rpb={rpb}", rpb=rpb, gap=40, skip=("headsplit_bf16",))
    Mh = {7: 1099, 100: 1100, 255: 1275, 256: 1280, 300: 1500}[rpb]
    ph = Problem(Mh, 512, 128)
    for c_dtype in (BF, F32):
        e = Epi(f"headsplit4_{'bf16' if c_dtype == BF else 'f32'}", c_dtype, epilogue=R.HEADSPLIT, scale=0.5,
                scale_cols=128, hs=(rpb, 2, 64))
        launch(ph, e, layout_for(e, 512), tag=f"256 hs_seq={rpb}")


def test_256_kernel_conv_stem_layout():
    """conv1 of the stem writes its T rows between the two zero pad rows of each batch (c_offset = d, ldc = d,
    c_rows_per_batch = T, c_batch_stride = (T + 2) d): the guards are the pad rows."""
    d, T, B, c_pad = 256, 600, 2, 128
    p = Problem(B * T, d, 3 * c_pad, al=R.ALayout(c_pad, rpb=T, bs=(T + 2) * c_pad))
    for e in (Epi("store_bf16", BF), Epi("rowadd7_f32", F32, period=7)):
        lay = R.CLayout(ldc=d, rpb=T, bs=(T + 2) * d, front=d, back=d)
        launch(p, e, lay, tag="256 conv1 layout")


# ---------------------------------------------------------------------------------------------- 3: 256 kernel, persistent
@pytest.mark.parametrize("K,bias", [(64, True), (128, False), (192, True), (64, False)])
def test_256_kernel_persistent(K, bias):
    """33 row tiles (33 % 4 != 0: the last row-tile group of the grouped order holds one ragged tile row) by enough
    column tiles for at least 2.5 tiles per CU: every workgroup hands over at least once, most twice.  STORE bf16 /
    f32 and HEADSPLIT overlap the next tile's prologue with this tile's epilogue; RESID and row_add hand over
    serially.  M = 8260 = 7 * 1180: head-split batches end inside tiles."""
    M = 32 * 256 + 68
    N = 256 * -(-5 * _cus() // (2 * 33))
    assert 33 * (N // 256) >= 2.5 * _cus()
    p = Problem(M, N, K)
    both = (K, bias) == (64, True)
    for e in (Epi("store_bf16", BF, bias=bias), Epi("store_f32", F32, bias=bias),
              Epi("headsplit_bf16", BF, epilogue=R.HEADSPLIT, scale=0.5, scale_cols=128, bias=bias, hs=(1180, 2, 64)),
              Epi("resid", F32, epilogue=R.RESID, bias=bias), Epi("rowadd7_f32", F32, period=7, bias=bias)):
        launch(p, e, layout_for(e, N), backends=("torch", "ctypes") if both and e.name == "store_bf16" else ("torch",),
               tag="256 persistent")


@pytest.mark.parametrize("K", [64, 128])
def test_256_kernel_two_ragged_tiles_in_a_row(K):
    """M = 1025, N = 16384: 5 x 64 = 320 tiles, the last 64 (row tile 4, one live row) ragged.  On 256 CUs:
    nwg = 320, q8 = 40, r8 = 0, so every XCD's run_len is 40 and XCD x's run starts at 40 x; the grid is 256, so
    per = 32 workgroups per XCD and workgroup loc takes run positions loc and loc + 32 (loc < 8).  The grouped order
    puts tiles 0 .. 255 in row tiles 0 .. 3 and tiles 256 .. 319 in row tile 4: XCD 7's run (280 .. 319) is all
    ragged, so its workgroups 0 .. 7 walk two ragged tiles in a row -- prologue_wait(false) with the next tile's
    loads behind fewer stores than a full tile issues, at nk = 1 (K = 64) and nk > 1 (K = 128); XCD 6's workgroups
    0 .. 7 go from a full tile (240 .. 247) to a ragged one (272 .. 279)."""
    ragged, full = R.ragged_handoffs(1025, 16384, _cus())
    if ragged == 0:
        pytest.skip(f"with {_cus()} CUs no workgroup takes a tile after a ragged one at this shape")
    p = Problem(1025, 16384, K)
    for e in (Epi("store_bf16", BF), Epi("store_f32", F32)):
        launch(p, e, layout_for(e, 16384), tag=f"256 ragged->next x{ragged}")


# ---------------------------------------------------------------------------------------------- 4: either side of use256()
USE256_SHAPE = (1153, 512, 192)


def _fallback_layout(e, N, trigger):
    if trigger == "aligned":
        return layout_for(e, N, rpb=300, gap=40)
    if trigger == "c_offset=1":
        return layout_for(e, N, rpb=300, gap=40, front=65)
    if trigger == "ldc=N+1":
        return layout_for(e, N, pad=1, rpb=300, gap=40)
    if trigger == "c_batch_stride odd":
        return layout_for(e, N, rpb=300, gap=41)
    raise AssertionError(trigger)


@pytest.mark.parametrize("trigger", ["aligned", "c_offset=1", "ldc=N+1", "c_batch_stride odd", "row_add+1", "M=1023"])
def test_use256_fallbacks_are_exact(trigger):
    """One 256-eligible shape, then each thing use256() refuses: a C base, ldc or c_batch_stride that is no whole
    16-B piece, a row_add table one float off, and M one row short of 1024.  Either kernel must give the expected
    bits."""
    M, N, K = USE256_SHAPE
    p = Problem(1023 if trigger == "M=1023" else M, N, K)
    for e in all_epilogues(p.M, N, hs=(pick_seq(p.M), 2, 64)):
        name = "aligned" if trigger in ("row_add+1", "M=1023") else trigger
        if e.epilogue == R.HEADSPLIT and name not in ("aligned", "c_offset=1"):
            continue  # ldc and c_batch_stride do not apply to a head-split store
        if trigger == "row_add+1":
            if not e.period:
                continue
            e.ra_shift = 1
        launch(p, e, _fallback_layout(e, N, name), backends=("torch", "ctypes") if trigger == "aligned" else ("torch",),
               tag=f"use256 {trigger}")


def test_use256_gelu_f32_bitwise_across_kernels():
    """GELU into f32: both kernels call gelu_erf on identical pre-activations (the accumulation is exact) and apply
    the column scale and row_add in the same order, so the 256 kernel (aligned) and the 128 kernel (each fallback)
    must agree bit for bit."""
    M, N, K = USE256_SHAPE
    p = Problem(M, N, K)

    def image(trigger, shift=0):
        e = Epi("gelu_f32", F32, gelu=True, scale=0.5, scale_cols=100, period=7, ra_shift=shift)
        buf, idx, _, _ = launch(p, e, _fallback_layout(e, N, trigger), tag=f"use256 gelu {trigger}")
        return R.bits_of(buf)[idx]

    want = image("aligned")
    for trigger in ("c_offset=1", "ldc=N+1", "c_batch_stride odd"):
        assert torch.equal(image(trigger), want), trigger
    assert torch.equal(image("aligned", shift=1), want), "row_add+1"


# ---------------------------------------------------------------------------------------------- 5: 4 GiB offsets
def test_a_rows_4gib_past_the_base():
    """A: 2100 bf16 rows with lda = 2^20, so row 2048 starts 4 GiB past the base (4.4 GB, zero but for K = 64 live
    columns).  gemm256_kernel keeps 32-bit byte offsets: it would multiply rows 0 .. 51 again for rows 2048 .. 2099.
    use256() must hand the call to the 128x128 kernel, whose row pointers are 64-bit.  The only test here that
    allocates more than 100 MB."""
    M, N, K, lda = 2100, 256, 64, 2 ** 20
    rng = np.random.default_rng(5)
    abuf = torch.zeros(M * lda, dtype=BF, device=DEV)
    abuf.view(M, lda)[:, :K] = R.to_device(R.recipe_a(rng, (M, K)), BF, DEV)
    p = Problem(M, N, K, al=R.ALayout(lda), abuf=abuf)
    e = Epi("store_f32", F32)
    launch(p, e, layout_for(e, N), backends=("torch", "ctypes"), tag="A rows past 4 GiB")
    del p, abuf
    torch.cuda.empty_cache()  # hand the 4.4 GB back before the next test


# ---------------------------------------------------------------------------------------------- 6: the f32 kernel
# v_mfma_f32_32x32x2_f32 is an fmaf chain: exact on the recipe.  64x64 tiles: M and N below, at and above one tile, N no
# multiple of anything; K = 16 / 48: 1 and 3 K-steps.
F32_HS = {64: (2, 8), 100: (5, 5), 129: (1, 43)}  # heads, head_dim: 4, 4 and 3 head-split parts


@pytest.mark.parametrize("K", [16, 48])
@pytest.mark.parametrize("N", [64, 100, 129])
@pytest.mark.parametrize("M", [1, 63, 65])
def test_f32_kernel(M, N, K):
    both = (M, N, K) == (65, 100, 48)
    run_all(Problem(M, N, K, in_dtype=F32), backends=("torch", "ctypes") if both else ("torch",), tag="f32",
            hs=(pick_seq(M, 16),) + F32_HS[N])


def test_f32_kernel_rowmaps():
    d, T, B = 16, 10, 13
    p = Problem(B * (T // 2), 64, 3 * d, in_dtype=F32, al=R.ALayout(2 * d, rpb=T // 2, bs=(T + 2) * d))
    run_all(p, tag="f32 conv2 rowmap", hs=(T // 2, 2, 8))
    run_all(Problem(65, 100, 48, in_dtype=F32, al=R.ALayout(52, front=4)), tag="f32 c_rpb=7", rpb=7, gap=3,
            skip=("headsplit_bf16",))


# ---------------------------------------------------------------------------------------------- 7: GELU
@pytest.mark.parametrize("K", [64, 1280])
@pytest.mark.parametrize("kernel,M,N", [("128", 600, 384), ("256", 1153, 768), ("f32", 65, 129)])
def test_gelu_bounds(kernel, M, N, K):
    """GELU with a column scale and row_add on top, the only cases with a tolerance.

    bf16 C (gemm256_kernel: gelu_bf16out, A&S 7.1.26; the others: erff): |got - ref64| <= ulp_bf16(ref64) / 2 +
    1e-6 max(1, |x|), x the exact pre-activation (tests/_gemm_ref.py derives the second term).
    f32 C: the error relative to max(1, |x|) is at most 4 x that of torch's own float32 GELU (an independent
    implementation, same column scale and row_add applied in float32) on the same pre-activations, measured here.
    Measured on the MI355X (profiles/gemm_exact.md): bf16 excess over the half ulp at most 6.3e-8 max(1, |x|) on
    all three kernels; every f32 kernel at 1.74e-7, the same figure as torch's float32 GELU."""
    p = Problem(M, N, K, in_dtype=F32 if kernel == "f32" else BF)
    for c_dtype in (BF, F32):
        e = Epi("gelu_" + ("bf16" if c_dtype == BF else "f32"), c_dtype, gelu=True, scale=0.5, scale_cols=100, period=7)
        both = (kernel, K) == ("256", 64)
        buf, idx, pre, val = launch(p, e, layout_for(e, N), backends=("torch", "ctypes") if both else ("torch",),
                                    tag=f"gelu {kernel}")
        got = buf[idx].double()
        err = (got - val).abs()
        if c_dtype == BF:
            excess = float(((err - R.ulp_bf16(val) / 2) / pre.abs().clamp_min(1.0)).max())
            print(f"gelu {kernel} K={K} bf16: worst excess over half a bf16 ulp {excess:.3g} x max(1, |x|) (bound 1e-6)")
            GELU_REPORT.append((kernel, K, "bf16", f"{excess:.3g}", "1e-6"))
            assert bool((err <= R.gelu_bf16_bound(val, pre)).all()), f"{kernel} K={K}: excess {excess:.3g}"
        else:
            t = torch.nn.functional.gelu(pre.float())
            t[:, :e.scale_cols] *= e.scale
            t += p.row_add(7)[torch.arange(M, device=DEV) % 7]
            torch_err = float(R.gelu_rel_err(t.double(), val, pre).max())
            kern_err = float(R.gelu_rel_err(got, val, pre).max())
            print(f"gelu {kernel} K={K} f32: kernel {kern_err:.3g}, torch float32 {torch_err:.3g} (x max(1, |x|))")
            GELU_REPORT.append((kernel, K, "f32", f"{kern_err:.3g}", f"torch {torch_err:.3g}"))
            assert kern_err <= 4 * torch_err, f"{kernel} K={K}: {kern_err:.3g} > 4 x {torch_err:.3g}"


# ---------------------------------------------------------------------------------------------- 8: rejections, M = 0
def _reject_case(name):
    kw = dict(M=128, N=128, K=64, in_dtype=BF, c_dtype=BF, over={})
    kw.update({
        "bf16 N % 128": dict(N=130),
        "bf16 K % 64": dict(K=72),
        "bf16 lda % 8": dict(over=dict(lda=68)),
        "f32 K % 16": dict(in_dtype=F32, c_dtype=F32, K=24),
        "f32 lda % 4": dict(in_dtype=F32, c_dtype=F32, K=16, over=dict(lda=18)),
        "RESID into bf16": dict(over=dict(epilogue=L.KW_EPI_RESID)),
        "HEADSPLIT M % hs_seq": dict(M=10, over=dict(epilogue=L.KW_EPI_HEADSPLIT, hs_seq=3, hs_heads=2, hs_head_dim=64)),
        "HEADSPLIT N % width": dict(over=dict(epilogue=L.KW_EPI_HEADSPLIT, hs_seq=64, hs_heads=3, hs_head_dim=10)),
        "epilogue 3": dict(over=dict(epilogue=3)),
        "M = 0": dict(M=0),
    }[name])
    return kw


@pytest.mark.parametrize("name", ["bf16 N % 128", "bf16 K % 64", "bf16 lda % 8", "f32 K % 16", "f32 lda % 4",
                                  "RESID into bf16", "HEADSPLIT M % hs_seq", "HEADSPLIT N % width", "epilogue 3", "M = 0"])
def test_rejections_write_nothing(name):
    """Each call kw_gemm must refuse returns KW_EINVAL (a ValueError through the ctypes binding) and leaves the
    guarded C all sentinel; M = 0 returns KW_OK and writes nothing either."""
    c = _reject_case(name)
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.default_rng(8)
    A = R.to_device(R.recipe_a(rng, (max(M, 1) + 1) * (K + 8)), c["in_dtype"], DEV)
    W = R.to_device(R.recipe_w(rng, (N, K)), c["in_dtype"], DEV)
    bias = R.to_device(R.recipe_g(rng, N), F32, DEV)
    buf = R.guarded(64 + 2 * max(M, 1) * N + 64, c["c_dtype"], DEV)
    plan = ops.GemmPlan(A, W, buf, M, N, K, bias=bias, c_offset=64, **c["over"])
    with _backend("ctypes"):
        if name == "M = 0":
            plan()
        else:
            with pytest.raises(ValueError):
                plan()
    torch.cuda.synchronize()
    stray, _ = R.check_guarded(buf, torch.zeros((0, 1), dtype=torch.int64, device=DEV))
    assert stray.numel() == 0, f"{name}: " + R.describe(stray, torch.zeros((0, 2)))


# ---------------------------------------------------------------------------------------------- 9: mel_to_time_major
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("T", [1, 31, 33, 3000])
@pytest.mark.parametrize("C,c_pad", [(80, 128), (128, 128), (3, 8)])
def test_mel_to_time_major(C, c_pad, T, dtype):
    """[B][C][T] f32 -> [B][T + 2][c_pad]: out[b][1 + t][c] = mel[b][c][t] (bf16: rounded to nearest even), time
    rows 0 and T + 1 and the channels C .. c_pad - 1 zero, nothing written around the buffer."""
    B, front = 2, 64
    g = torch.Generator(device="cpu").manual_seed(9)
    mel = torch.randn(B, C, T, generator=g).to(DEV)
    want = torch.zeros(B, T + 2, c_pad, dtype=F32, device=DEV)
    want[:, 1:T + 1, :C] = mel.permute(0, 2, 1)
    want_bits = R.bits_of(want.to(dtype)).reshape(1, -1)
    n = B * (T + 2) * c_pad
    idx = front + torch.arange(n, device=DEV).reshape(1, -1)
    backends = ("torch", "ctypes") if (C, T) == (80, 33) else ("torch",)
    for be in backends:
        with _backend(be):
            for _ in range(2):
                buf = R.guarded(front + n + 64, dtype, DEV)
                ops.mel_to_time_major(mel, c_pad, dtype, out=buf[front:front + n].view(B, T + 2, c_pad))
                torch.cuda.synchronize()
                stray, wrong = R.check_guarded(buf, idx, want_bits)
                assert stray.numel() == 0 and wrong.shape[0] == 0, f"{be}: " + R.describe(stray, wrong)
                out = buf[front:front + n].view(B, T + 2, c_pad)
                assert bool((R.bits_of(out[:, 0]) == 0).all()) and bool((R.bits_of(out[:, T + 1]) == 0).all())
                assert bool((R.bits_of(out[:, :, C:]) == 0).all())
