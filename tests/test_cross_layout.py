"""The cross-attention workspace layout and chunk geometry, through the C ABI's size / offset / supported queries
(no GPU needed, no compute calls).  attention.hip derives every one of them from one geometry and one layout struct;
the numbers below were recorded from the library before that code was shared (ABI 112) and must not move: callers
allocate and zero workspaces by them, and read the status and fault-injection words at the offsets."""
import os
import subprocess

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "kotoba-whisper_amd", "kwhisper", "libkwhisper.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "kotoba-whisper_amd", "csrc"), "-j8"], check=True)
    from kwhisper import _lib

    return _lib.load()


# (B, q_len, H, S), hd = 64 -> (kw_cross_attn_workspace, kw_cross_attn_status_offset)
STEP = {
    (1, 1, 6, 1500): (85568, 9528),
    (32, 1, 20, 1500): (9126464, 1016320),
    (2, 3, 20, 1500): (1711232, 190560),
    (1, 1, 6, 77): (14336, 1608),
    (3, 1, 6, 256): (42880, 4824),
    (1, 1, 2, 2048): (38080, 4232),
    (2, 1, 6, 1350): (171136, 19056),
}

# (M, d, H, S) -> (kw_dec_xq_cross_workspace, kw_dec_xq_cross_status_offset, kw_dec_xq_cross_supported)
FUSED = {
    (1, 384, 6, 1500): (87104, 9528, 1),
    (17, 384, 6, 1500): (1480640, 161976, 1),
    (32, 1280, 20, 1500): (9290304, 1016320, 1),
    (2, 384, 6, 256): (31680, 3216, 1),
    (2, 384, 6, 1350): (174208, 19056, 1),
}


@pytest.mark.parametrize("shape", sorted(STEP))
def test_cross_attn_workspace_and_status_offset(lib, shape):
    B, q_len, H, S = shape
    assert (lib.kw_cross_attn_workspace(B, q_len, H, 64, S), lib.kw_cross_attn_status_offset(B, q_len, H, 64, S)) == STEP[shape]


@pytest.mark.parametrize("shape", sorted(FUSED))
def test_xq_cross_workspace_status_offset_and_supported(lib, shape):
    got = (lib.kw_dec_xq_cross_workspace(*shape), lib.kw_dec_xq_cross_status_offset(*shape),
           lib.kw_dec_xq_cross_supported(*shape))
    assert got == FUSED[shape]


def test_layout_by_hand():
    """The recorded values of the bench shape from the layout's definition: f32 partials [rows][ns][66] | counters
    [rows] | status word | fault word | pad to 64 B | 8-byte wave granules [rows][ns][4][66] | pad to 64 B | query
    granules [M][d / 2]."""
    rows, ns = 32 * 20, 6
    part = rows * ns * 66 * 4
    status = part + rows * 4
    gran = (status + 8 + 63) // 64 * 64
    assert status == 1016320 == STEP[(32, 1, 20, 1500)][1]
    assert gran + 8 * part == 9126464 == STEP[(32, 1, 20, 1500)][0]
    assert (gran + 8 * part + 63) // 64 * 64 + 32 * 640 * 8 == FUSED[(32, 1280, 20, 1500)][0]


# kw_dec_xq_cross covers S whose ceil(S / 256) chunks of ceil(S / chunks) keys all hold 225..256 keys, the last too
@pytest.mark.parametrize("S,want", [(256, 1),    # one chunk of 256
                                    (257, 0),    # two chunks of 129
                                    (1350, 1),   # six chunks of 225
                                    (1345, 0),   # chunk 225, last 220
                                    (1344, 0),   # chunk 224
                                    (1536, 1),   # six chunks of 256
                                    (2049, 0)])  # more than 2048 keys
def test_xq_cross_supported_at_the_chunk_boundaries(lib, S, want):
    assert lib.kw_dec_xq_cross_supported(2, 384, 6, S) == want


def test_xq_cross_supported_rows_and_heads(lib):
    assert lib.kw_dec_xq_cross_supported(32, 384, 6, 1500) == 1
    assert lib.kw_dec_xq_cross_supported(33, 384, 6, 1500) == 0  # more rows than the projection's 32-row tile
    assert lib.kw_dec_xq_cross_supported(2, 384, 5, 1500) == 0   # d != 64 H
