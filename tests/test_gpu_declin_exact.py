"""kw_pack_weight and kw_dec_linear on the MI355X against an exact reference, on every launch path.

Inputs come from the dyadic recipe of tests/_gemm_ref.py (through tests/_declin_ref.py): every product and partial sum
is a float32 number, so a result without LayerNorm or GELU has one right f32 and one right bf16 bit pattern and the
comparison is bitwise.  The fused LayerNorm's sums (sum x, sum x^2, the accumulator, ln_colsum) are exact too, which
leaves about ten rounded f32 operations between exact inputs and the result: it is held to ``ln_bound``, a derived
bound of a few f32 ulp.  GELU is held to the two bounds of the GEMM file's family 7.

Every case: x row-major lies in a buffer of NaNs (ldx = K + 8; the gaps and 64 elements before and after are poison),
a fragment-major x carries NaN in its rows M .. 16 T - 1; C, h, hb lie in guarded buffers (ldc = ldh = N + 8; a
fragment-major hb's rows >= M are guards); two launches into two fresh sets of buffers must both hold the expected
bits with every guard intact.  One workspace serves the module: after every call its arrival counters are zero, and
for a shape without a K split all of it is.  (A K-split call leaves its partial slabs behind: they are scratch,
written before they are read -- the second launch of such a case starts from a slab region full of NaN.)

The shape table is that of tests/test_gpu_declin_pin.py, one shape per path of choose() / launch_one() (its
docstring has the geometry of each).  (64, 2560) at M <= 16 from a row-major x is not called: the 32-row launch
asks for more LDS than a workgroup has and the runtime refuses it.  KW_EHIP for a shape the library could have
refused itself is a known wart; those row counts run from a fragment-major x here.

Families (case table and measured ratios: profiles/declin_exact.md):
 A kw_pack_weight, bitwise            B no LayerNorm, no GELU: bitwise        C fused LayerNorm: ln_bound
 D the LM head's four kernels         E GELU bounds                           F rejections and M = 0
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _declin_ref as D  # noqa: E402
from kwhisper import _lib as L  # noqa: E402
from kwhisper import ops  # noqa: E402

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
ROWS = (1, 16, 17, 32, 33, 70)
SHAPES = {
    "n40_k160": (40, 160, ROWS),
    "n48_k384": (48, 384, ROWS),
    "n48_k2592": (48, 2592, ROWS + (257,)),
    "n64_k2560": (64, 2560, ROWS),
    "n4112_k2560": (4112, 2560, ROWS),
    "n5120_k384": (5120, 384, ROWS),
    "n5120_k512": (5120, 512, ROWS),
    "n8192_k384": (8192, 384, ROWS),
}
LM = "lm_n8200_k256"
LM_SHAPE = (8200, 256, (1, 32, 33, 40, 129, 300, 321))
ALL_SHAPES = dict(SHAPES, **{LM: LM_SHAPE})
KSPLIT = "n48_k2592"
EPS = (1e-5, 2.0 ** -6)
FRONT = 64  # guard / poison elements in front of every operand
CNT = 4096  # the workspace's arrival counters (declin.hip CNT_MAX), in 4-byte words
REPORT = {}  # (family, kernel path, C dtype) -> worst measured ratio
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    yield
    for key in sorted(REPORT):
        print("declin exact:", " | ".join(str(c) for c in key), "|", REPORT[key])
    path = os.environ.get("KW_DECLIN_EXACT_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("| family | kernel path | C | measured |\n|---|---|---|---|\n")
            for key in sorted(REPORT):
                f.write("| " + " | ".join(str(c) for c in key) + f" | {REPORT[key]} |\n")
    _CACHE.clear()
    torch.cuda.empty_cache()


@contextlib.contextmanager
def _backend(name):
    old = ops.set_backend(name)
    try:
        yield
    finally:
        ops.set_backend(old)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------------------------- workspace
def _ws():
    def make():
        need = max(ops.dec_linear_workspace_bytes(N, K) for N, K, _ in ALL_SHAPES.values())
        return torch.zeros(need // 4 + 1, device=DEV, dtype=torch.int32)
    return _cached("ws", make)


def _is_split(N, K):
    return ops.dec_linear_workspace_bytes(N, K) > CNT * 4


def _check_ws(split, what):
    """After a call: the counters are zero; without a K split nothing else was touched either.  A K-split call's
    slabs are scratch: zeroed again here, so that the next shape's check still means "this call wrote nothing"."""
    torch.cuda.synchronize()
    w = _ws()
    assert not bool(w[:CNT].any()), f"{what}: arrival counters not left zero"
    if split:
        REPORT[("workspace", "K-split call leaves its slabs non-zero", "-")] = bool(w[CNT:].any())
        w[CNT:].zero_()
    else:
        assert not bool(w[CNT:].any()), f"{what}: workspace written by a call without a K split"


# ---------------------------------------------------------------------------------------------- problems
class Shape:
    """One (N, K): the weight, its packed form, bias and the exact float32 column sums."""

    def __init__(self, name):
        self.name = name
        self.N, self.K, _ = ALL_SHAPES[name]
        rng = np.random.default_rng([sum(name.encode()), self.N, self.K])
        self.W = D.to_device(D.recipe_w(rng, (self.N, self.K)), BF, DEV)
        self.bias = D.to_device(D.recipe_g(rng, self.N), F32, DEV)
        self.W64 = self.W.double()
        cs64 = self.W64.sum(dim=1)
        self.cs = cs64.float()
        assert torch.equal(self.cs.double(), cs64)
        self.Wp = ops.pack_weight(self.W)
        self.split = _is_split(self.N, self.K)


def shape(name):
    return _cached(("shape", name), lambda: Shape(name))


class Problem:
    """The rows of one (shape, M): the recipe's x and the LayerNorm family's x, each row-major among NaNs and
    fragment-major, with their exact accumulations (float64, computed once and shared by every mode)."""

    def __init__(self, name, M):
        self.s, self.M = shape(name), M
        N, K = self.s.N, self.s.K
        rng = np.random.default_rng([11, M, N, K])
        self.x = D.to_device(D.recipe_a(rng, (M, K)), BF, DEV)
        self.xl = D.to_device(D.ln_rows(rng, M, K), BF, DEV)
        self.base = D.to_device(D.recipe_g(rng, (M, N)), F32, DEV).double()
        D.assert_exact(self.x, self.s.W)
        D.assert_ln_exact(self.xl, self.s.W)
        self.acc = self.x.double() @ self.s.W64.t()
        self.acc_ln = self.xl.double() @ self.s.W64.t()
        self._in = {}

    def operand(self, ln, tiled):
        """(buffer, ldx): x starts FRONT elements into the buffer."""
        if (ln, tiled) not in self._in:
            x = self.xl if ln else self.x
            if tiled:
                pad = torch.full((FRONT,), D.POISON, dtype=torch.int16, device=DEV).view(BF)
                self._in[(ln, tiled)] = (torch.cat([pad, D.tile_x(x), pad]), ops.KW_LD_TILED)
            else:
                self._in[(ln, tiled)] = (D.poisoned_rows(x, self.s.K + 8, FRONT, FRONT), self.s.K + 8)
        return self._in[(ln, tiled)]


def problem(name, M):
    return _cached(("problem", name, M), lambda: Problem(name, M))


def _offsets(M, N, pad):
    return _cached(("idx", M, N, pad), lambda: D.element_offsets(D.CLayout(ldc=N + pad, front=FRONT), M, N, DEV))


def _tiled_hb_offsets(M, N):
    return _cached(("hbt", M, N), lambda: (FRONT + D.tiled_offsets(M, N)[:M].to(DEV), FRONT + D.tiled_elems(M, N) + 64))


class Mode:
    def __init__(self, name, *, c_dtype=F32, resid=False, bias=True, scale=1.0, scale_cols=0, hbt=False, xt=False, pad=8,
                 eps=None, gelu=False):
        self.name, self.c_dtype, self.resid, self.bias, self.scale, self.scale_cols = name, c_dtype, resid, bias, scale, scale_cols
        self.hbt, self.xt, self.pad, self.eps, self.gelu = hbt, xt, pad, eps, gelu


def launch(p, mode, *, backends=("torch",), tag=""):
    """Run ``mode`` on problem ``p`` twice per backend into fresh guarded buffers.  Exact modes: asserts the bits.
    Always: the guards, the workspace, and that the launches agree bit for bit.  Returns (float64 results read back
    from the first launch, reference, pre-activation)."""
    s, M = p.s, p.M
    N, K = s.N, s.K
    what = f"{tag} {s.name} M={M} {mode.name}"
    ln = mode.eps is not None
    xbuf, ldx = p.operand(ln, mode.xt)
    bias = s.bias if mode.bias else None
    idx, total = _offsets(M, N, mode.pad)
    if ln:
        pre = D.ln_reference(p.acc_ln, p.xl.double(), s.cs.double(), None if bias is None else bias.double(), mode.eps)
        val = D.gelu64(pre) if mode.gelu else pre.clone()
        val[:, :mode.scale_cols] *= mode.scale
    else:
        pre, val = D.reference(p.acc, bias=bias, epilogue=D.RESID if mode.resid else D.STORE, gelu=mode.gelu,
                               scale=mode.scale, scale_cols=mode.scale_cols, base=p.base if mode.resid else None)
    exact = not ln and not mode.gelu
    outs = []
    for be in backends:
        with _backend(be):
            for i in range(2):
                if s.split and i:  # the slabs are scratch: whatever they hold must not reach a result
                    _ws()[CNT:].fill_(D.SENTINEL[F32])
                if mode.resid:
                    h = D.guarded(total, F32, DEV)
                    D.plant(h, idx, p.base)
                    idx_hb, total_hb = _tiled_hb_offsets(M, N) if mode.hbt else (idx, total)
                    hb = D.guarded(total_hb, BF, DEV)
                    ops.DecLinearPlan(xbuf, s.Wp, M, N, K, ldx=ldx, x_offset=FRONT, bias=bias,
                                      resid=(h[FRONT:], hb[FRONT:], N + mode.pad, 0), workspace=_ws(), hb_tiled=mode.hbt)()
                    outs.append(((h, idx, F32), (hb, idx_hb, BF)))
                else:
                    C = D.guarded(total, mode.c_dtype, DEV)
                    ops.DecLinearPlan(xbuf, s.Wp, M, N, K, ldx=ldx, x_offset=FRONT,
                                      ln=(mode.eps, s.cs) if ln else None, bias=bias, C=C, ldc=N + mode.pad, c_offset=FRONT,
                                      gelu=mode.gelu, scale=mode.scale, scale_cols=mode.scale_cols, workspace=_ws())()
                    outs.append(((C, idx, mode.c_dtype),))
                _check_ws(s.split, what)
    for i, images in enumerate(outs):
        for j, (buf, ix, dt) in enumerate(images):
            want = D.expected_bits(val, dt) if exact else None
            stray, wrong = D.check_guarded(buf, ix, want)
            assert stray.numel() == 0 and wrong.shape[0] == 0, f"{what} launch {i} image {j}: " + D.describe(stray, wrong)
            if i:
                assert torch.equal(D.bits_of(buf), D.bits_of(outs[0][j][0])), f"{what}: launch {i} differs from launch 0"
    buf, ix, _ = outs[0][0]
    return buf[ix].double(), val, pre


def _row_major_ok(name, M):
    return not (name == "n64_k2560" and M <= 16)  # (the runtime refuses that launch: the docstring)


def _x_forms(name, M):
    return ([False] if _row_major_ok(name, M) else []) + ([True] if M <= 32 else [])


def _cases(table):
    return [(name, M) for name, (_, _, rows) in table.items() for M in rows]


def _path(name, M, mode):
    """The kernel a call takes (kw_dec_linear's dispatch and launch_one, restated for the report's row names)."""
    N, K, _ = ALL_SHAPES[name]
    nkt = K // 32
    lm_shape = mode.eps is not None and mode.c_dtype == F32 and N >= 8192 and not mode.gelu and mode.scale_cols == 0
    if lm_shape and 32 < M <= 320 and nkt % 8 == 0:
        return "lm_head_rows_kernel<8,%d,%d>" % {1: (1, 4), 2: (2, 8), 3: (3, 10)}[(M + 127) // 128]
    if lm_shape and M <= 32:
        return "lm_head_kernel"
    if _is_split(N, K):
        return "dec_linear_kernel, K split"
    if M > 32:
        return "dec_linear_rows_kernel"
    ncg = -(-N // (32 if -(-N // 16) >= 320 else 16))
    if 16 < M <= 32 and 2 * ncg <= _cus():
        return "dec_linear_kernel, 16-row chunks"
    return "dec_linear_kernel"


def _note(family, path, dtype, ratio):
    key = (family, path, "bf16" if dtype == BF else "f32")
    REPORT[key] = max(REPORT.get(key, 0.0), round(float(ratio), 4))


# ---------------------------------------------------------------------------------------------- A: kw_pack_weight
@pytest.mark.parametrize("name", list(ALL_SHAPES))
def test_pack_weight_bitwise(name):
    """kw_pack_weight against ``packed_offsets``, into a buffer full of the sentinel: every element of
    kw_packed_weight_bytes is written (the padding columns with zeros) and nothing past it.  (4112, 2560) is
    1.3 M 16-B pieces against a grid of 1024 x 256 threads: the grid-stride loop runs five times."""
    s = shape(name)
    n = int(L.load().kw_packed_weight_bytes(s.N, s.K)) // 2
    assert n == (s.N + 31) // 32 * 32 * s.K
    want = D.packed_image(s.W).reshape(1, -1)
    idx = FRONT + torch.arange(n, device=DEV).reshape(1, -1)
    for be in ("torch", "ctypes") if name == "n48_k384" else ("torch",):
        for _ in range(2):
            buf = D.guarded(FRONT + n + 64, BF, DEV)
            if be == "torch":
                L.load_torch_ops().pack_weight(s.W, buf[FRONT:FRONT + n])
            else:
                L.check(L.load().kw_pack_weight(ctypes.c_void_p(s.W.data_ptr()), s.N, s.K,
                                                ctypes.c_void_p(buf.data_ptr() + 2 * FRONT),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "kw_pack_weight")
            torch.cuda.synchronize()
            stray, wrong = D.check_guarded(buf, idx, want)
            assert stray.numel() == 0 and wrong.shape[0] == 0, f"{name} {be}: " + D.describe(stray, wrong)
    assert torch.equal(D.bits_of(s.Wp), want.reshape(-1))  # (what every other family multiplies by)


# ---------------------------------------------------------------------------------------------- B: bitwise
def _b_modes(name, M):
    N = ALL_SHAPES[name][0]
    out = []
    for xt in _x_forms(name, M):
        sfx = "/xt" if xt else ""
        out += [Mode("store_f32" + sfx, xt=xt),
                Mode("store_bf16_nobias" + sfx, c_dtype=BF, bias=False, xt=xt),
                Mode(f"scale{N // 2 + 3}_bf16" + sfx, c_dtype=BF, scale=0.125, scale_cols=N // 2 + 3, xt=xt),
                Mode("resid" + sfx, resid=True, xt=xt)]
        if M <= 32 and N % 32 == 0:
            out.append(Mode("resid_hbt" + sfx, resid=True, hbt=True, xt=xt))
        if name in ("n48_k384", "n5120_k512"):  # the element-wise epilogue forced by alignment, not by N
            out.append(Mode("store_f32_ldc=N+3" + sfx, pad=3, xt=xt))
    return out


@pytest.mark.parametrize("name,M", _cases(SHAPES))
def test_linear_bitwise(name, M):
    """STORE f32 with bias, STORE bf16 without, STORE bf16 with a column scale whose boundary N / 2 + 3 straddles a
    16-column block and an 8-column store piece, RESID (h and hb), RESID with a fragment-major hb -- each from a
    row-major x and from a fragment-major one.  The K-split shape at 257 rows: the second 32 * ZMAX window's
    rows_window arithmetic.  (48, 384) runs under both bindings."""
    p = problem(name, M)
    for mode in _b_modes(name, M):
        launch(p, mode, backends=("torch", "ctypes") if name == "n48_k384" else ("torch",), tag="B")


# ---------------------------------------------------------------------------------------------- C, D: LayerNorm
def _ln_check(family, name, M, dtypes):
    p = problem(name, M)
    s = p.s
    for xt in _x_forms(name, M):
        for dtype in dtypes:
            for eps in EPS:
                mode = Mode(f"ln_{'bf16' if dtype == BF else 'f32'}_eps{eps:.3g}" + ("/xt" if xt else ""), c_dtype=dtype,
                            eps=eps, xt=xt)
                got, ref, _ = launch(p, mode, tag=family)
                bound = D.ln_bound(p.acc_ln, p.xl.double(), s.cs.double(), s.bias.double(), eps, dtype)
                assert bool(torch.isfinite(got).all()), f"{name} M={M} {mode.name}: not finite"
                err = (got - ref).abs()
                ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # (0 / 0 where the result is an exact 0)
                worst = float(ratio.max())
                at = divmod(int(ratio.argmax()), s.N)
                print(f"{family} {name} M={M} {mode.name} [{_path(name, M, mode)}]: worst |got - ref| / bound {worst:.3f} at {at}")
                _note(family, _path(name, M, mode), dtype, worst)
                if dtype == BF:  # the store's half ulp dominates that figure: also the excess over it, in f32 bounds
                    f32b = D.ln_bound(p.acc_ln, p.xl.double(), s.cs.double(), s.bias.double(), eps, F32)
                    key = (family + " excess over half a bf16 ulp / f32 bound", _path(name, M, mode), "bf16")
                    REPORT[key] = max(REPORT.get(key, -1.0), round(float(((err - D.ulp_bf16(ref) / 2) / f32b).max()), 4))
                assert worst <= 1.0, f"{name} M={M} {mode.name}: {worst:.3f} x the bound at (m, n) = {at}"
                if M >= 2:  # the constant row: variance 0, the reference is the bias itself
                    assert torch.equal(ref[M - 1], s.bias.double())


@pytest.mark.parametrize("name,M", [c for c in _cases(SHAPES) if c[0] != KSPLIT])
def test_layernorm_within_derived_bound(name, M):
    """The fused LayerNorm into f32 and bf16, from a row-major and a fragment-major x, eps 1e-5 and 2^-6, held to
    ``ln_bound``.  Row m is the recipe plus {-1, -1/2, 0, 1/2, 1}[m % 5] (mean * colsum as large as the result); with
    M >= 2 the last row is constant (variance 0: sq / K - mean^2 may round below 0), where the result must be finite
    and within the bound of the bias.  (8192, 384) into f32 is an LM-head shape: lm_head_kernel up to 32 rows, and at
    33 and 70 rows -- 12 k-tiles, no multiple of 8 -- dec_linear_rows_kernel, not lm_head_rows_kernel.
    Measured on the MI355X (profiles/declin_exact.md): into f32 at most 0.87 (32-row tile), 0.54 (16-row chunks),
    0.92 (rows kernel) of the bound; into bf16 the excess over the store's half ulp at most 0.46 of the f32 bound."""
    _ln_check("C", name, M, (F32, BF))


def test_ksplit_layernorm_is_unsupported_and_writes_nothing():
    p = problem(KSPLIT, 17)
    s = p.s
    xbuf, ldx = p.operand(True, False)
    idx, total = _offsets(17, s.N, 8)
    C = D.guarded(total, F32, DEV)
    with _backend("ctypes"):
        with pytest.raises(L.KWError, match=rf"code {L.KW_EUNSUPPORTED}\b"):
            ops.DecLinearPlan(xbuf, s.Wp, 17, s.N, s.K, ldx=ldx, x_offset=FRONT, ln=(1e-5, s.cs), bias=s.bias, C=C,
                              ldc=s.N + 8, c_offset=FRONT, workspace=_ws())()
    torch.cuda.synchronize()
    stray, _ = D.check_guarded(C, torch.zeros((0, 1), dtype=torch.int64, device=DEV))
    assert stray.numel() == 0 and not bool(_ws().any())


@pytest.mark.parametrize("M", LM_SHAPE[2])
def test_lm_head_within_derived_bound(M):
    """The LM head (LayerNorm, f32 logits, no scale, no GELU) at 8,200 columns, every one compared (the last column
    group is partial): lm_head_kernel<false> (1, 32), lm_head_rows_kernel<8,1,4> (33, 40), <8,2,8> (129),
    <8,3,10> (300) and the fall-through to dec_linear_rows_kernel (321).  Measured on the MI355X: 0.79, 0.90, 0.93,
    0.95 and 0.91 of the bound."""
    _ln_check("D", LM, M, (F32,))


# ---------------------------------------------------------------------------------------------- E: GELU
@pytest.mark.parametrize("M", [17, 70])
@pytest.mark.parametrize("name", ["n5120_k384", KSPLIT])
def test_gelu_bounds(name, M):
    """STORE with GELU.  bf16 C: |got - ref64| <= ulp_bf16(ref64) / 2 + 1e-6 max(1, |x|), x the exact
    pre-activation.  f32 C: the error relative to max(1, |x|) at most 4 x that of torch's own float32 GELU on the
    same pre-activations (tests/test_gpu_gemm_exact.py family 7)."""
    p = problem(name, M)
    for dtype in (BF, F32):
        mode = Mode("gelu_" + ("bf16" if dtype == BF else "f32"), c_dtype=dtype, gelu=True)
        got, val, pre = launch(p, mode, tag="E")
        D.assert_gelu_share(pre)
        err = (got - val).abs()
        path = _path(name, M, mode)
        if dtype == BF:
            excess = float(((err - D.ulp_bf16(val) / 2) / pre.abs().clamp_min(1.0)).max())
            print(f"E {name} M={M} bf16 [{path}]: worst excess over half a bf16 ulp {excess:.3g} x max(1, |x|) (bound 1e-6)")
            REPORT[("E excess / max(1, |x|)", f"{path} {name} M={M}", "bf16")] = f"{excess:.3g} (bound 1e-6)"
            assert bool((err <= D.gelu_bf16_bound(val, pre)).all()), f"{name} M={M}: excess {excess:.3g}"
        else:
            t = torch.nn.functional.gelu(pre.float())
            torch_err = float(D.gelu_rel_err(t.double(), val, pre).max())
            kern_err = float(D.gelu_rel_err(got, val, pre).max())
            print(f"E {name} M={M} f32 [{path}]: kernel {kern_err:.3g}, torch float32 {torch_err:.3g} (x max(1, |x|))")
            REPORT[("E error / max(1, |x|)", f"{path} {name} M={M}", "f32")] = f"{kern_err:.3g} (torch {torch_err:.3g})"
            assert kern_err <= 4 * torch_err, f"{name} M={M}: {kern_err:.3g} > 4 x {torch_err:.3g}"


@pytest.mark.parametrize("M", [17, 70])
def test_layernorm_gelu_scale_bf16(M):
    """fc1 as the engine calls it, and the pin file's ln_gelu_scale_bf16 mode: LayerNorm, GELU, a column scale, bf16
    C, on (5120, 384).  The bound composes the two derived ones: the pre-activation is within ``ln_bound`` (f32) of the
    true one, GELU's slope is at most 1.13 (its maximum, 1.1290 at x = 1.41), its f32 evaluation costs
    1e-6 max(1, |x|) (``gelu_bf16_bound``), the scale 0.125 is exact, the store half a bf16 ulp."""
    name = "n5120_k384"
    p = problem(name, M)
    s = p.s
    mode = Mode("ln_gelu_scale_bf16", c_dtype=BF, eps=EPS[0], gelu=True, scale=0.125, scale_cols=s.N // 2)
    got, val, pre = launch(p, mode, tag="E")
    D.assert_gelu_share(pre)
    sc = torch.ones(s.N, dtype=torch.float64, device=DEV)
    sc[:mode.scale_cols] = mode.scale
    f32_part = sc[None, :] * (1.13 * D.ln_bound(p.acc_ln, p.xl.double(), s.cs.double(), s.bias.double(), mode.eps, F32)
                              + 1e-6 * pre.abs().clamp_min(1.0))
    err = (got - val).abs()
    worst = float(((err - D.ulp_bf16(val) / 2) / f32_part).max())
    print(f"E {name} M={M} ln_gelu_scale_bf16 [{_path(name, M, mode)}]: worst excess over half a bf16 ulp {worst:.3f} x the f32 part")
    REPORT[("E excess / f32 part, ln + gelu + scale", f"{_path(name, M, mode)} {name} M={M}", "bf16")] = f"{worst:.3f}"
    assert bool(torch.isfinite(got).all()) and bool((err <= D.ulp_bf16(val) / 2 + f32_part).all()), f"M={M}: {worst:.3f}"


# ---------------------------------------------------------------------------------------------- F: rejections, M = 0
REJECTIONS = {
    "K % 32": (L.KW_EINVAL, dict(K=72)),
    "ldx < K": (L.KW_EINVAL, dict(ldx=56)),
    "ldx % 8": (L.KW_EINVAL, dict(ldx=68)),
    "tiled x, M = 33": (L.KW_EINVAL, dict(M=33, ldx=ops.KW_LD_TILED)),
    "HB_TILED, N = 40": (L.KW_EINVAL, dict(N=40, epilogue=L.KW_EPI_RESID | ops.KW_EPI_HB_TILED)),
    "HB_TILED with STORE": (L.KW_EINVAL, dict(epilogue=L.KW_EPI_STORE | ops.KW_EPI_HB_TILED)),
    "ln with RESID": (L.KW_EINVAL, dict(ln=True, epilogue=L.KW_EPI_RESID)),
    "ln without colsum": (L.KW_EINVAL, dict(ln=True, colsum=False)),
    "split-K, short workspace": (L.KW_EINVAL, dict(N=48, K=2592, ws_short=4)),
    "M = 0": (L.KW_OK, dict(M=0)),
}


@pytest.mark.parametrize("what", list(REJECTIONS))
def test_rejections_write_nothing(what):
    """Calls kw_dec_linear refuses before any launch, through the C ABI as it is: each returns its code and leaves
    the guarded C, h and hb all sentinel and the workspace zero; M = 0 returns KW_OK and writes nothing either."""
    code, over = REJECTIONS[what]
    c = dict(M=17, N=64, K=64, ldx=None, epilogue=L.KW_EPI_STORE, ln=False, colsum=True, ws_short=0)
    c.update(over)
    M, N, K = c["M"], c["N"], c["K"]
    rng = np.random.default_rng(8)
    Kp = (K + 31) // 32 * 32
    x = D.to_device(D.recipe_a(rng, 64 * (Kp + 8)), BF, DEV)  # 64 rows' worth, row-major or fragment-major
    Wp = ops.pack_weight(D.to_device(D.recipe_w(rng, (N, Kp)), BF, DEV))
    bias = D.to_device(D.recipe_g(rng, N), F32, DEV)
    cs = torch.zeros(N, dtype=F32, device=DEV)
    bufs = [D.guarded(FRONT + 64 * (N + 8) + 64, dt, DEV) for dt in (F32, F32, BF)]
    C, h, hb = bufs
    a = L.DecLinearArgs()
    a.x, a.ldx = x.data_ptr(), (K if c["ldx"] is None else c["ldx"])
    a.ln, a.ln_eps = int(c["ln"]), 1e-5
    a.ln_colsum = cs.data_ptr() if c["colsum"] else None
    a.W, a.bias, a.epilogue = Wp.data_ptr(), bias.data_ptr(), c["epilogue"]
    a.C, a.ldc, a.c_dtype = C.data_ptr() + 4 * FRONT, N + 8, L.KW_DT_F32
    a.scale = 1.0
    a.h, a.hb, a.ldh = h.data_ptr() + 4 * FRONT, hb.data_ptr() + 2 * FRONT, N + 8
    a.M, a.N, a.K = M, N, K
    a.workspace = _ws().data_ptr()
    a.ws_bytes = ops.dec_linear_workspace_bytes(N, Kp) - c["ws_short"]
    rc = L.load().kw_dec_linear(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == code, f"{what}: returned {rc}, expected {code}"
    none = torch.zeros((0, 1), dtype=torch.int64, device=DEV)
    for buf in bufs:
        stray, _ = D.check_guarded(buf, none)
        assert stray.numel() == 0, f"{what}: " + D.describe(stray, torch.zeros((0, 2)))
    assert not bool(_ws().any()), f"{what}: workspace written"
