"""The geometry of the weight-gradient products, asked of the host-only query stin_gemm_tn_route (no GPU): every point of the
sweep in tests/_tn_table.py must reach the tile class, chunk count, load width and kernel family its line names, and the
workspace the caller is told to allocate must hold the slabs of that geometry.  tests/test_wgrad_exact.py runs the same table on
the GPU; this file is the check that it aims where it says - a change of a tile or chunk rule shows up here first."""
import pytest

import _tn_table as T
from surface_texture_inpainting_net_amd import _lib

_C = _lib.CONSTANTS


def _check(lib, p, g):
    assert g['family'] == p.family, (p.id, g)
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
    # the grid: nothing without rows | one block per chunk (skinny) | from 8 chunks on whole rounds of 8 chunks, times the tiles
    rounds = g['chunks'] if g['chunks'] < 8 else (g['chunks'] + 7) // 8 * 8
    assert g['grid'] == {T.NONE: 0, T.SKINNY_K: g['chunks']}.get(p.family, rounds * g['tiles'][0] * g['tiles'][1]), (p.id, g)


def test_precision_constants_of_the_table():
    assert (T.F32, T.X3, T.X6) == (_C['STIN_GEMM_F32'], _C['STIN_GEMM_BF16X3'], _C['STIN_GEMM_BF16X6'])
    assert (T.NONE, T.SKINNY_K, T.EXACT, T.FOUR_WAVE, T.PC, T.B16_REG, T.B16_TR) == tuple(
        _C['STIN_TN_FAMILY_' + n] for n in ('NONE', 'SKINNY', 'F32', 'BF16S', 'PC', 'B16_REG', 'B16_TR'))


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
    assert {p.family for p in T.POINTS} == {T.NONE, T.SKINNY_K, T.EXACT, T.FOUR_WAVE, T.PC, T.B16_REG, T.B16_TR}
    # (Not checked here, because the query cannot see them: the trip thresholds of the slab fold - four in flight up to 64 chunks,
    # sixteen from 241, fn_partial.  The counts 63 .. 65, 240, 241 are in the table for them; their protection is the equality on
    # the GPU at those counts.)


def test_grid_blocks_at_seven_eight_and_nine_chunks(monkeypatch):
    """128-row chunks (M = 128 c on at most 6 tiles): 7 chunks in plain order, 8 = one whole round of the 8 XCDs, 9 = two rounds
    (16 block slots per tile, of which 7 write nothing); the skinny kernel has one block per chunk."""
    lib = _lib.load()
    T.set_env(monkeypatch, {})
    for storage, prec, Nc, K, tiles, family in ((0, T.F32, 64, 64, 1, T.EXACT), (0, T.X3, 320, 128, 3, T.PC), (0, T.X6, 132, 260, 6, T.FOUR_WAVE),
                                                (1, T.X3, 320, 128, 3, T.B16_REG), (1, T.X3, 512, 512, 4, T.B16_TR), (1, T.X3, 128, 128, 1, T.B16_TR)):
        for chunks, slots in ((7, 7), (8, 8), (9, 16)):
            g = T.geometry(lib, storage, 128 * chunks, Nc, K, Nc, K, 1, 1, prec)
            assert (g['family'], g['chunks'], g['tiles'][0] * g['tiles'][1], g['grid']) == (family, chunks, tiles, slots * tiles), (Nc, K, g)
    for chunks in (7, 8, 9):
        g = T.geometry(lib, 0, 128 * chunks, 320, 12, 320, 12, 1, 1, T.X3)
        assert (g['family'], g['chunks'], g['grid']) == (T.SKINNY_K, chunks, chunks)


def test_the_eight_value_query_writes_eight_values_equal_to_the_route(monkeypatch):
    """stin_gemm_tn_geometry keeps the contract its callers allocate for: eight int32 and not one more, the first eight of the route"""
    import ctypes
    lib = _lib.load()
    T.set_env(monkeypatch, {})
    for p in T.CLASS_POINTS:
        g = T.point_geometry(lib, p)
        out8 = (ctypes.c_int32 * 10)(*([-7] * 10))
        assert lib.stin_gemm_tn_geometry(p.storage, p.M, p.Nc, p.K, p.Nc + p.padg, p.K + p.padx, int(p.off == 0), 1, p.prec, ctypes.addressof(out8)) == 0
        if not p.env:
            assert list(out8) == [*g['tile'], *g['tiles'], g['rows'], g['chunks'], g['vec'], g['ws'], -7, -7], p.id


def test_block_workspace_holds_the_compact_layout_where_it_takes_more_chunks(monkeypatch):
    """The compact trans-inv layout runs the packed product with Yw = H (+ Cout) rows inside the workspace of
    stin_edgeconv_wgrad_workspace_bytes, which takes no layout.  With Cp <= 16 and H (+ Cout) <= 1024 < 2 H (+ Cout) the compact
    product is the skinny kernel's (about 1024 chunks) and the wide one is not (about 384 / tiles): slab B must hold the larger of
    the two, slab A (rounded up to 256 bytes) lies in front of it - what the entry points' guard requires."""
    lib = _lib.load()
    T.set_env(monkeypatch, {})
    for N in (60211, 200704):
        for Cp, H, Cout, sc in ((12, 768, 64, 0), (12, 512, 512, 1), (16, 520, 64, 0), (4, 1024, 64, 0), (12, 64, 32, 1)):
            ws_bytes = lib.stin_edgeconv_wgrad_workspace_bytes(N, Cp, H, Cout, sc)
            off_b = (lib.stin_gemm_tn_workspace_bytes(N, Cout, H, 1) + 255) // 256 * 256
            ga = T.geometry(lib, 0, N, Cout, H, Cout, H + 4, 1, 1, T.X3)
            assert ga['chunks'] * (Cout * H + Cout) * 4 <= off_b
            chunks = {}
            for ti in (0, 2):
                yw = T.block_yw(H, Cout, sc, ti)
                gb = T.geometry(lib, 0, N, yw, Cp, yw, Cp, 1, 1, T.X3)
                chunks[ti] = gb['chunks']
                assert off_b + gb['chunks'] * (yw * ((Cp + 3) & ~3) + ((yw + 3) & ~3)) * 4 + 256 <= ws_bytes, (N, Cp, H, Cout, sc, ti, gb)
            if H == 768:
                assert T.geometry(lib, 0, N, 768, Cp, 768, Cp, 1, 1, T.X3)['family'] == T.SKINNY_K and chunks[2] > 10 * chunks[0]


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
    out = (ctypes.c_int32 * 10)(*([77] * 10))
    at = ctypes.addressof(out)
    assert lib.stin_gemm_tn_route(0, 100, 64, 64, 63, 64, 1, 0, T.X3, at) == _C['STIN_E_SIZE']             # ldg < Nc
    assert lib.stin_gemm_tn_route(0, -1, 64, 64, 64, 64, 1, 0, T.X3, at) == _C['STIN_E_SIZE']
    assert lib.stin_gemm_tn_route(2, 100, 64, 64, 64, 64, 1, 0, T.X3, at) == _C['STIN_E_UNSUPPORTED']
    assert lib.stin_gemm_tn_route(0, 100, 64, 64, 64, 64, 1, 0, T.X3, None) == _C['STIN_E_NULL']
    assert lib.stin_gemm_tn_geometry(0, 100, 64, 64, 63, 64, 1, 0, T.X3, at) == _C['STIN_E_SIZE']          # ldg < Nc
    assert lib.stin_gemm_tn_geometry(0, -1, 64, 64, 64, 64, 1, 0, T.X3, at) == _C['STIN_E_SIZE']
    assert lib.stin_gemm_tn_geometry(2, 100, 64, 64, 64, 64, 1, 0, T.X3, at) == _C['STIN_E_UNSUPPORTED']
    assert lib.stin_gemm_tn_geometry(0, 100, 64, 64, 64, 64, 1, 0, T.X3, None) == _C['STIN_E_NULL']
    assert list(out) == [77] * 10


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
