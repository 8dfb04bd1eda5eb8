"""Fragment-major bf16 activations (KW_LD_TILED, include/kwhisper.h): the Python index permutation, on the CPU."""
import pytest
import torch

from kwhisper import ops


def _piece(m, k, T):
    return ((k // 32) * T + m // 16) * 64 + m % 16 + 16 * ((k % 32) // 8)


@pytest.mark.parametrize("M", [1, 15, 16, 17, 32])
@pytest.mark.parametrize("K", [32, 96, 1280])
def test_tile_untile_round_trip(M, K):
    x = torch.arange(M * K, dtype=torch.float32).view(M, K).bfloat16()
    t = ops.act_tile(x)
    T = (M + 15) // 16
    assert t.shape == (K // 32 * T * 512,) and t.dtype == x.dtype
    assert torch.equal(ops.act_untile(t, M, K), x)
    # every element where the formula puts it (int32 keeps the check exact), the padding rows zero
    xi = torch.arange(1, M * K + 1, dtype=torch.int32).view(M, K)
    ti = ops.act_tile(xi)
    m = torch.arange(M).view(M, 1).expand(M, K)
    k = torch.arange(K).view(1, K).expand(M, K)
    pos = _piece(m, k, T) * 8 + k % 8
    assert torch.equal(ti[pos.reshape(-1)], xi.reshape(-1))
    assert int((ti != 0).sum()) == M * K


def test_piece_index_by_hand():
    """A few elements worked out by hand from the formula in include/kwhisper.h."""
    M, K = 17, 96  # T = 2 row tiles, 3 k-tiles
    x = torch.arange(M * K, dtype=torch.int32).view(M, K)
    t = ops.act_tile(x)
    for (m, k), piece in {(0, 0): 0, (0, 7): 0, (0, 8): 16, (15, 31): 63, (16, 0): 64, (16, 24): 112,
                          (0, 32): 128, (3, 40): 147, (16, 95): 368}.items():
        assert _piece(m, k, 2) == piece
        assert int(t[piece * 8 + k % 8]) == int(x[m, k]), (m, k)


def test_tile_rejects_what_it_does_not_cover():
    with pytest.raises(ValueError):
        ops.act_tile(torch.zeros(33, 32))
    with pytest.raises(ValueError):
        ops.act_tile(torch.zeros(4, 48))
