"""The geometry of the weight-gradient products, asked of the host-only query stin_gemm_tn_geometry (no GPU): every point of the
sweep in tests/_tn_table.py must reach the tile class, chunk count, load width and kernel family its line names, and the
workspace the caller is told to allocate must hold the slabs of that geometry.  tests/test_wgrad_exact.py runs the same table on
the GPU; this file is the check that it aims where it says - a change of a tile or chunk rule shows up here first."""
import pytest

import _tn_table as T
from surface_texture_inpainting_net_amd import _lib

_C = _lib.CONSTANTS


def _check(lib, p, g):
    assert g['tile'] == p.tile, (p.id, g)
    assert g['chunks'] == p.chunks, (p.id, g)
    assert g['vec'] == p.vec and g['ws'] == p.ws, (p.id, g)
    if p.tiles is not None:
        assert g['tiles'] == p.tiles, (p.id, g)
    if p.rows is not None:
        assert g['rows'] == p.rows, (p.id, g)
    assert g['rows'] % 32 == 0 and g['rows'] >= 128
    assert g['chunks'] * g['rows'] >= p.M and (g['chunks'] - 1) * g['rows'] < max(p.M, 1)
    if p.tile != T.SKINNY:
        assert g['tiles'] == ((p.Nc + p.tile[0] - 1) // p.tile[0], (p.K + p.tile[1] - 1) // p.tile[1])


def test_precision_constants_of_the_table():
    assert (T.F32, T.X3, T.X6) == (_C['STIN_GEMM_F32'], _C['STIN_GEMM_BF16X3'], _C['STIN_GEMM_BF16X6'])


@pytest.mark.parametrize('p', T.POINTS + T.BN_POINTS, ids=lambda p: p.id)
def test_point_reaches_its_geometry_and_fits_its_workspace(p, monkeypatch):
    lib = _lib.load()
    T.set_env(monkeypatch, p.env)
    for ones in (0, 1):
        g = T.point_geometry(lib, p, ones)
        _check(lib, p, g)
        # the host check of gemm_tn_*_impl: chunks x (Nc Kq + roundup4(Nc)) floats + 256 bytes of alignment slack
        stride = p.Nc * ((p.K + 3) & ~3) + ((p.Nc + 3) & ~3)
        assert lib.stin_gemm_tn_workspace_bytes(p.M, p.Nc, p.K, ones) >= g['chunks'] * stride * 4 + 256, (p.id, g)


def test_sweep_covers_every_chunk_count_on_every_route():
    want = {(c, last) for c in T.CHUNK_COUNTS for last in ('full', 'one')}
    for name, *_ in T.SWEEP_ROUTES:
        got = {(p.chunks, 'full' if p.M == 128 * p.chunks else 'one') for p in T.POINTS if p.id.startswith(name + '-c')}
        assert got == want, name
        assert all(p.M - 128 * (p.chunks - 1) in (1, 128) for p in T.POINTS if p.id.startswith(name + '-c'))
    assert {p.tile for p in T.POINTS} == {(64, 64), (64, 128), (128, 64), (128, 128), (256, 256), T.SKINNY}
    assert {p.K for p in T.POINTS if p.tile == T.SKINNY} == {4, 8, 12, 16}
    # (Not checked here, because the query cannot see them: the round-up of the grid to 8 chunks per XCD round - 9 chunks = 16 block
    # slots of which 7 write nothing, stin_tn_slabs - and the trip thresholds of the slab fold - four in flight up to 64 chunks,
    # sixteen from 241, k_reduce_slabs / fn_partial.  The counts 8, 9, 63 .. 65, 240, 241 are in the table for them; their
    # protection is the equality on the GPU at those counts.)


def test_one_block_per_cu_rule_at_its_boundary(monkeypatch):
    """bf16x3 products of fp32 rows on 128 x 128 tiles want 256 blocks up to 32 768 rows and 384 beyond: visible with four tiles."""
    lib = _lib.load()
    T.set_env(monkeypatch, {})
    a = T.geometry(lib, 0, 32768, 256, 256, 256, 256, 1, 1, T.X3)
    b = T.geometry(lib, 0, 32769, 256, 256, 256, 256, 1, 1, T.X3)
    assert (a['chunks'], a['rows']) == (64, 512) and (b['chunks'], b['rows']) == (94, 352)
    assert a['chunks'] * 4 == 256 and 96 * 4 == 384
    # one tile: 128-row chunks on both sides of the boundary (256 and 257 of them)
    assert T.geometry(lib, 0, 32768, 128, 128, 128, 128, 1, 1, T.X3)['chunks'] == 256
    assert T.geometry(lib, 0, 32769, 128, 128, 128, 128, 1, 1, T.X3)['chunks'] == 257
    assert T.geometry(lib, 0, 32896, 128, 128, 128, 128, 1, 1, T.X3)['chunks'] == 257
    assert T.geometry(lib, 0, 32897, 128, 128, 128, 128, 1, 1, T.X3)['chunks'] == 258


def test_query_argument_errors_and_no_write_on_error():
    import ctypes
    lib = _lib.load()
    out = (ctypes.c_int32 * 8)(*([77] * 8))
    at = ctypes.addressof(out)
    assert lib.stin_gemm_tn_geometry(0, 100, 64, 64, 63, 64, 1, 0, T.X3, at) == _C['STIN_E_SIZE']          # ldg < Nc
    assert lib.stin_gemm_tn_geometry(0, -1, 64, 64, 64, 64, 1, 0, T.X3, at) == _C['STIN_E_SIZE']
    assert lib.stin_gemm_tn_geometry(2, 100, 64, 64, 64, 64, 1, 0, T.X3, at) == _C['STIN_E_UNSUPPORTED']
    assert lib.stin_gemm_tn_geometry(0, 100, 64, 64, 64, 64, 1, 0, T.X3, None) == _C['STIN_E_NULL']
    assert list(out) == [77] * 8


@pytest.mark.parametrize('case', list(T.block_cases()), ids=lambda c: '%s-sc%d-ti%d-st%d-p%d-n%d' % ('x'.join(map(str, c[0])), *c[1:]))
def test_block_products_geometry(case, monkeypatch):
    """The two products of every block case: a one-tile product has ceil(N / 128) chunks (1, 1, 1, 2, 9, 10, 257, 258 for the row
    counts of the table); the first shape's packed product is skinny; the second shape's products share one producer / consumer grid."""
    lib = _lib.load()
    T.set_env(monkeypatch, {})
    shape, shortcut, ti, storage, prec, N = case
    ga, gb = (T.geometry(lib, *args) for args in T.block_products(shape, shortcut, ti, storage, N, prec))
    for g in (ga, gb):
        assert g['chunks'] * g['rows'] >= N > (g['chunks'] - 1) * g['rows']
        if g['tiles'] == (1, 1):
            assert g['rows'] == 128 and g['chunks'] == (N + 127) // 128
    if N in T.BLOCK_NS:
        one_tile = dict(zip(T.BLOCK_NS, (1, 1, 1, 2, 9, 10, 257, 258)))[N]
        assert ga['chunks'] == one_tile or ga['tiles'] != (1, 1)
    Cin, Cp, H, Cout = shape
    if shape == (10, 12, 64, 32):
        assert gb['tile'] == (T.SKINNY if storage == 0 else (128, 64))
        assert ga['tile'] == ((128, 128) if storage == 0 and prec == T.X3 else (64, 64)) and ga['tiles'] == (1, 1)
    if shape == (64, 64, 128, 64) and storage == 0 and prec == T.X3:
        assert ga['ws'] == 1 and gb['ws'] == 1 and ga['tiles'] == (1, 1)
        if shortcut and ti != 2:
            assert gb['tiles'] == (3, 1)                              # Yw = 320: a ragged third tile
    if shape == (36, 36, 72, 40):
        assert ga['vec'] == (1 if storage == 0 else 0)                # 36 and 76 columns: 16-byte rows of fp32, not of bf16
    if storage == 0 and ti != 2:
        assert lib.stin_edgeconv_wgrad_map_supported(N, Cp, H, Cout, shortcut, prec) == gb['ws']
    ws_bytes = lib.stin_edgeconv_wgrad_workspace_bytes(N, Cp, H, Cout, shortcut)
    need = 0
    for g, (nc, k) in ((ga, (Cout, H)), (gb, (T.block_yw(H, Cout, shortcut, ti), Cp))):
        need += (g['chunks'] * (nc * ((k + 3) & ~3) + ((nc + 3) & ~3)) * 4 + 255) // 256 * 256
    assert ws_bytes >= need + 256


def test_mapped_entry_point_serves_every_block_shape_but_the_skinny_one(monkeypatch):
    """stin_edgeconv_wgrad_map_supported at the row counts of the mapped GPU cases: 1 for the shapes they run, 0 where the packed
    product is skinny (K = Cp = 12) - that shape keeps the gather and has no mapped case."""
    lib = _lib.load()
    T.set_env(monkeypatch, {})
    assert T.BLOCK_MAP_SHAPES == T.BLOCK_SHAPES[1:] and T.BLOCK_SHAPES[0] == (10, 12, 64, 32)
    for Cin, Cp, H, Cout in T.BLOCK_SHAPES:
        for shortcut in (0, 1):
            for N in T.BLOCK_MAP_NS:
                assert N % 4 != 0
                assert lib.stin_edgeconv_wgrad_map_supported(N, Cp, H, Cout, shortcut, T.X3) == int(Cp != 12), (Cp, H, Cout, shortcut, N)
