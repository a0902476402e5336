"""The host-only queries that read the row kernels' launch geometry (no GPU): callers size workspaces by them, so a change of
the geometry table in stin_graph.hip must not move them."""
import pytest

from surface_texture_inpainting_net_amd import _lib

BLOCK, TI_ITER = 256, 4
MASK_W = (128, 256, 512, 1024, 2048)


def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize('H', MASK_W)
def test_ti_colsum_rows_at_the_saved_mask_widths(H):
    """one partial row per block of TI_ITER row groups; a row group is 256 / g rows, g = 32 lanes for H = 128 and a wave beyond"""
    lib = _lib.load()
    g = 32 if H == 128 else 64
    for N in (0, 1, 4, 5, 16, 17, 32, 33, 301, 200_704):
        assert lib.stin_edge_bwd_ti_colsum_rows(N, H) == _ceil(_ceil(N, BLOCK // g), TI_ITER), (N, H)


@pytest.mark.parametrize('H', [0, -128, 4, 64, 96, 132, 260, 384, 4096])
def test_ti_colsum_rows_is_zero_elsewhere(H):
    lib = _lib.load()
    for N in (1, 301, 200_704):
        assert lib.stin_edge_bwd_ti_colsum_rows(N, H) == 0


@pytest.mark.parametrize('C', [4, 128, 1024, 1028, 12])
def test_stats_groups_at_their_thresholds(C):
    lib = _lib.load()
    ok = C > 0 and C % 4 == 0 and C <= 1024 and BLOCK % (C // 4) == 0
    for N in (0, 1, 1023, 1024, 1025, 4095, 4096, 4097, 200_704, 5_000_000):
        # gather-add: from 4096 rows, blocks of the one-pass form (4 rows per thread), at most 1024
        want = min(_ceil(_ceil(N, 4) * (C // 4), BLOCK), 1024) if ok and N >= 4096 else 0
        assert lib.stin_gather_add_rows_stats_groups(N, C) == want, (N, C)
        # segment mean: from 1024 rows, one block per 256 / (C / 4) rows, at most 2048
        want = min(_ceil(N, BLOCK // (C // 4)), 2048) if ok and N >= 1024 else 0
        assert lib.stin_segment_mean_stats_groups(N, C) == want, (N, C)
