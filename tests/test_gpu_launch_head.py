"""dec_linear_kernel behind its launch head, on the MI355X: exact bits on every path of choose() / launch_one().

dec_linear_kernel takes what its first loads need as leading scalar parameters (the weight and activation pointers,
the elements x advances per z-chunk, K / 32, the fragment-major tile count, the K splits, the waves per workgroup and
the multiplier that replaces the division by K splits x waves) and its descriptor behind them; the weight and
fragment-major activation loads are issued before the descriptor is read.  Every value that moved is exercised here,
on the machinery and the shape table of tests/test_gpu_declin_exact.py (one shape per path; the dyadic recipe of
tests/_gemm_ref.py, so a result without LayerNorm has one right bit pattern and is compared bit for bit against
float64; guards around every operand, two launches, the workspace checked after each):

 * the k-tile range of a (split, wave) slice without a division: 1 slice (K = 160), 3 (K = 384), 4 (K = 512),
   8 slices of 10 k-tiles (K = 2560) and the K split's 3 x 6 (K = 2592: 81 k-tiles, ranges of 4 and 5);
 * x advanced per z-chunk: the 16-row chunks of a row split at M = 17 and 32, row-major (16 ldx elements) and
   fragment-major (one row tile), from an x that starts 64 elements into its buffer (x_offset);
 * the waves per workgroup as a parameter: 1, 3, 4, 6 and 8 waves;
 * the descriptor read after the loads: null and non-null bias, LayerNorm on and off, RESID with a row-major and a
   fragment-major hb, f32 and bf16 C, the K split's per-chunk counters and slabs;
 * M = 1, 16, 17, 32.
The fused LayerNorm is held to ``ln_bound`` as in the exact file (its epilogue rounds about ten f32 operations).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_declin_exact as E  # noqa: E402
from kwhisper import _lib as L  # noqa: E402

ROWS = (1, 16, 17, 32)


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    yield
    E._CACHE.clear()
    torch.cuda.empty_cache()


def _modes(name, M):
    N = E.ALL_SHAPES[name][0]
    out = []
    for xt in E._x_forms(name, M):
        sfx = "/xt" if xt else ""
        out += [E.Mode("store_f32" + sfx, xt=xt),
                E.Mode("store_bf16_nobias" + sfx, c_dtype=E.BF, bias=False, xt=xt),
                E.Mode("resid" + sfx, resid=True, xt=xt),
                E.Mode("resid_nobias" + sfx, resid=True, bias=False, xt=xt)]
        if N % 32 == 0:
            out.append(E.Mode("resid_hbt" + sfx, resid=True, hbt=True, xt=xt))
    return out


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("name", list(E.SHAPES))
def test_launch_head_bitwise(name, M):
    """STORE (f32 with bias, bf16 without) and RESID (with and without bias, row-major and fragment-major hb), from a
    row-major and a fragment-major x: bit for bit the float64 result, guards intact, two launches alike."""
    p = E.problem(name, M)
    for mode in _modes(name, M):
        E.launch(p, mode, tag="launch head")


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("name", [n for n in E.SHAPES if n != E.KSPLIT])
def test_launch_head_layernorm(name, M):
    """The fused LayerNorm (whose column sums, eps and bias are read from the descriptor behind the head) into f32 and
    bf16 from both forms of x, within ``ln_bound``."""
    E._ln_check("launch head", name, M, (E.F32, E.BF))


def test_ksplit_paths_named():
    """The table still holds a K-split shape and a row-split one (the paths whose head arithmetic moved to the host)."""
    big = E.Mode("store_f32")
    assert E._path(E.KSPLIT, 32, big) == "dec_linear_kernel, K split"
    assert any(E._path(n, 17, big) == "dec_linear_kernel, 16-row chunks" for n in E.SHAPES)
