"""The sweep of the transposed (weight-gradient) products dW = G^T [X | w]: ONE table of points, shared by
tests/test_tn_geometry.py (CPU: every point reaches the geometry its line names, asked of stin_gemm_tn_route) and
tests/test_wgrad_exact.py (GPU: every point gives the exact integer product).  The expectations are written down here by hand
from the host rules of csrc/gemm_tn_route.inc (tn_route) - they are NOT computed by a copy of those rules: a rule
change makes test_tn_geometry.py fail on a machine without a GPU and says which point no longer aims where its line says.

With ONE output tile the chunk rule gives 128 rows per chunk for every M <= 49 152 (384 wanted chunks, at least 4 slabs of 32
rows each; the one-block-per-CU form wants 256 and holds for M <= 32 768), and the skinny kernel's rule gives 128 up to 131 072
rows: chunks = ceil(M / 128) on every one-tile route, which is what the chunk sweep below uses.
"""
import collections

F32, X3, X6 = 0, 2, 3                 # STIN_GEMM_F32 / _BF16X3 / _BF16X6 (checked against the header by test_tn_geometry.py)
SKINNY = (0, 0)                       # TI == 0: k_gemm_tn_skinny
# STIN_TN_FAMILY_* (checked against the header by test_tn_geometry.py): the kernel that runs the point
NONE, SKINNY_K, EXACT, FOUR_WAVE, PC, B16_REG, B16_TR = range(7)

# storage 0 = fp32 rows, 1 = bf16 rows; operands are views of width Nc / K in rows of ldg = Nc + padg / ldx = K + padx elements
# whose base is `off` elements behind a 16-byte boundary; env = the A/B switches set for the point; then the geometry it must
# reach: the kernel family, tile (TI, TJ), chunks, vec, ws (= ws_eligible) and, where the line is about them, tiles (tiles_i,
# tiles_j) and rows.  A point without rows has the family NONE (only the fold is launched) and the tile of its shape.
Point = collections.namedtuple('Point', 'id storage prec M Nc K padg padx off env family tile chunks vec ws tiles rows')


def _pt(id, storage, prec, M, Nc, K, family, tile, chunks, vec=1, ws=0, padg=8, padx=16, off=0, env=None, tiles=None, rows=None):
    assert (ws == 1) == (family == PC) and (family == NONE) == (M == 0) and (M == 0 or (tuple(tile) == SKINNY) == (family == SKINNY_K))
    return Point(id, storage, prec, M, Nc, K, padg, padx, off, dict(env or {}), family, tuple(tile), chunks, vec, ws, tiles, rows)


# chunk counts: 1 | 2 | 7, 8, 9 (8 = the first grid rounded to XCD rounds; 9 = 16 block slots of which 7 write nothing) | 15, 16, 17 |
# 63, 64, 65 (the four-in-flight loop of the slab fold ends / starts another trip) | 240, 241 (241 = the first count that enters
# its sixteen-in-flight loop) | 256, 257 (32 768 / 32 769 rows: the last / first size beside the one-block-per-CU rule)
CHUNK_COUNTS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 240, 241, 256, 257)
# per count: one M that fills the last chunk and one that leaves ONE row in it
CHUNK_MS = [(m, c) for c in CHUNK_COUNTS for m in (128 * c, 128 * (c - 1) + 1)]

# the one-tile routes of the chunk sweep: (name, storage, precision, Nc, K, family, tile, ws_eligible, env)
SWEEP_ROUTES = [
    ('f32-64x64', 0, F32, 64, 64, EXACT, (64, 64), 0, {}),                        # k_gemm_tn<64, 64>
    ('x3-ws', 0, X3, 128, 128, PC, (128, 128), 1, {}),                          # k_gemm_tn_ws
    ('x3-4wave', 0, X3, 128, 128, FOUR_WAVE, (128, 128), 0, {'STIN_TN_WS': '0'}),      # k_gemm_tn_bf16s<128, 128, 2>
    ('x6-128x64', 0, X6, 128, 64, FOUR_WAVE, (128, 64), 0, {}),                        # k_gemm_tn_bf16s<128, 64, 3>
    ('f32-128x128', 0, F32, 128, 128, EXACT, (128, 128), 0, {}),                   # k_gemm_tn<128, 128>
    ('x6-64x64', 0, X6, 64, 64, FOUR_WAVE, (64, 64), 0, {}),                           # k_gemm_tn_bf16s<64, 64, 3>
    ('x3-ws-64x64', 0, X3, 64, 64, PC, (128, 128), 1, {}),                      # k_gemm_tn_ws on a tile that is three quarters empty
    ('skinny-k12', 0, X3, 64, 12, SKINNY_K, SKINNY, 0, {}),                           # k_gemm_tn_skinny<12>
    ('skinny-k4-f32', 0, F32, 320, 4, SKINNY_K, SKINNY, 0, {}),                       # k_gemm_tn_skinny<4>: 80 column lanes, 3 row lanes
    ('b16-tr', 1, X3, 128, 128, B16_TR, (128, 128), 0, {}),                         # k_gemm_tn_b16_tr<2, 2, 2, 2>
    ('b16-reg', 1, X3, 128, 128, B16_REG, (128, 128), 0, {'STIN_TN_TR': '0'}),       # k_gemm_tn_b16<128, 128>
    ('b16-64x128', 1, X3, 64, 128, B16_REG, (64, 128), 0, {}),                       # k_gemm_tn_b16<64, 128>
]


def _sweep():
    for name, storage, prec, Nc, K, family, tile, ws, env in SWEEP_ROUTES:
        for M, c in CHUNK_MS:
            yield _pt('%s-c%d-m%d' % (name, c, M), storage, prec, M, Nc, K, family, tile, c, ws=ws, env=env, tiles=(1, 1), rows=128)


# M = 1153: 10 chunks of 128 rows with ONE row in the last, on every tiling below (at most 38 tiles)
_M = 1153
CLASS_POINTS = [
    # ---- the tile classes, fp32 rows.  exact fp32 / bf16x6: tile = 64 up to 64 columns, 128 beyond, per side
    _pt('f32-64x128-ragged', 0, F32, _M, 36, 72, EXACT, (64, 128), 10, tiles=(1, 1)),
    _pt('f32-128x64-ragged', 0, F32, _M, 72, 40, EXACT, (128, 64), 10, tiles=(1, 1)),
    _pt('f32-128x128-2x3-ragged', 0, F32, _M, 132, 260, EXACT, (128, 128), 10, tiles=(2, 3)),
    _pt('x6-64x64', 0, X6, _M, 64, 64, FOUR_WAVE, (64, 64), 10),
    _pt('x6-64x128', 0, X6, _M, 36, 72, FOUR_WAVE, (64, 128), 10),
    _pt('x6-128x128-2x3-ragged', 0, X6, _M, 132, 260, FOUR_WAVE, (128, 128), 10, tiles=(2, 3)),
    _pt('x6-128x64-3x1', 0, X6, _M, 320, 64, FOUR_WAVE, (128, 64), 10, tiles=(3, 1)),
    # bf16x3 on 16-byte rows with both sides >= 32 columns: ALWAYS the 128 x 128 producer / consumer kernel ...
    _pt('x3-ws-320x128', 0, X3, _M, 320, 128, PC, (128, 128), 10, ws=1, tiles=(3, 1)),
    _pt('x3-ws-40x36', 0, X3, _M, 40, 36, PC, (128, 128), 10, ws=1, tiles=(1, 1)),
    _pt('x3-ws-32x32', 0, X3, _M, 32, 32, PC, (128, 128), 10, ws=1),
    _pt('x3-ws-132x260', 0, X3, 4097, 132, 260, PC, (128, 128), 33, ws=1, tiles=(2, 3)),
    # ... and with STIN_TN_WS=0 the four-wave kernel on the tiles of the width rule
    _pt('x3-4wave-320x128', 0, X3, _M, 320, 128, FOUR_WAVE, (128, 128), 10, env={'STIN_TN_WS': '0'}, tiles=(3, 1)),
    _pt('x3-4wave-40x36', 0, X3, _M, 40, 36, FOUR_WAVE, (64, 64), 10, env={'STIN_TN_WS': '0'}),
    _pt('x3-4wave-64x128', 0, X3, _M, 64, 128, FOUR_WAVE, (64, 128), 10, env={'STIN_TN_WS': '0'}),
    _pt('x3-4wave-128x64', 0, X3, _M, 128, 64, FOUR_WAVE, (128, 64), 10, env={'STIN_TN_WS': '0'}),
    _pt('x3-narrow-28x64', 0, X3, _M, 28, 64, FOUR_WAVE, (64, 64), 10),                # Nc < 32: not the producer / consumer kernel
    # ---- bf16 rows: the width rule, 256 x 256 from 512 x 512 up (16-byte rows only), STIN_TN_BIG / STIN_TN_TR
    _pt('b16-64x64', 1, X3, _M, 64, 64, B16_REG, (64, 64), 10),
    _pt('b16-128x64', 1, X3, _M, 72, 40, B16_REG, (128, 64), 10),
    _pt('b16-128x128-ragged', 1, X3, _M, 320, 128, B16_REG, (128, 128), 10, tiles=(3, 1)),                          # register transpose
    _pt('b16-128x128-ragged-tr', 1, X3, _M, 320, 128, B16_TR, (128, 128), 10, env={'STIN_TN_TR': '1'}, tiles=(3, 1)),   # transposed reads
    _pt('b16-256x256', 1, X3, _M, 512, 512, B16_TR, (256, 256), 10, tiles=(2, 2)),
    _pt('b16-256x256-ragged', 1, X3, _M, 520, 512, B16_TR, (256, 256), 10, tiles=(3, 2)),
    _pt('b16-512-big0-tr', 1, X3, _M, 512, 512, B16_TR, (128, 128), 10, env={'STIN_TN_BIG': '0'}, tiles=(4, 4)),
    _pt('b16-512-big0-reg', 1, X3, _M, 512, 512, B16_REG, (128, 128), 10, env={'STIN_TN_BIG': '0', 'STIN_TN_TR': '0'}, tiles=(4, 4)),
    _pt('b16-256-default', 1, X3, _M, 256, 256, B16_TR, (128, 128), 10, tiles=(2, 2)),                      # whole tiles: transposed reads
    _pt('b16-256-tr0-reg', 1, X3, _M, 256, 256, B16_REG, (128, 128), 10, env={'STIN_TN_TR': '0'}, tiles=(2, 2)),
    _pt('b16-256-big1', 1, X3, _M, 256, 256, B16_TR, (256, 256), 10, env={'STIN_TN_BIG': '1'}, tiles=(1, 1)),
    # ---- the skinny kernel: K in {4, 8, 12, 16}, Nc % 4 == 0, 64 <= Nc <= 1024, 16-byte rows - any precision
    _pt('skinny-64x4', 0, X3, _M, 64, 4, SKINNY_K, SKINNY, 10),
    _pt('skinny-320x8', 0, F32, _M, 320, 8, SKINNY_K, SKINNY, 10),
    _pt('skinny-320x12', 0, X3, _M, 320, 12, SKINNY_K, SKINNY, 10),
    _pt('skinny-1024x16', 0, X6, _M, 1024, 16, SKINNY_K, SKINNY, 10),
    _pt('skinny-68x16', 0, X3, _M, 68, 16, SKINNY_K, SKINNY, 10),
    # ... and its near misses
    _pt('not-skinny-nc1028', 0, X3, _M, 1028, 12, FOUR_WAVE, (128, 64), 10, tiles=(9, 1)),
    _pt('not-skinny-nc60', 0, X3, _M, 60, 12, FOUR_WAVE, (64, 64), 10),
    _pt('not-skinny-k20', 0, X3, _M, 64, 20, FOUR_WAVE, (64, 64), 10),
    _pt('not-skinny-ldx', 0, X3, _M, 64, 12, FOUR_WAVE, (64, 64), 10, vec=0, padx=9),
    # ---- vec == 0 (no 16-byte loads): K = 10 | Nc = 3 | ld % 4 != 0 | base one element behind a 16-byte boundary
    _pt('vec0-k10-f32', 0, F32, _M, 64, 10, EXACT, (64, 64), 10, vec=0),
    _pt('vec0-k10-x3', 0, X3, _M, 128, 10, FOUR_WAVE, (128, 64), 10, vec=0),
    _pt('vec0-k10-x6', 0, X6, _M, 64, 10, FOUR_WAVE, (64, 64), 10, vec=0),
    _pt('vec0-nc3-f32', 0, F32, _M, 3, 64, EXACT, (64, 64), 10, vec=0),
    _pt('vec0-nc3-x3', 0, X3, _M, 3, 128, FOUR_WAVE, (64, 128), 10, vec=0),
    _pt('vec0-ld-f32', 0, F32, _M, 128, 128, EXACT, (128, 128), 10, vec=0, padg=9),
    _pt('vec0-ld-x3', 0, X3, _M, 128, 128, FOUR_WAVE, (128, 128), 10, vec=0, padg=9, padx=7),
    _pt('vec0-base-f32', 0, F32, _M, 64, 128, EXACT, (64, 128), 10, vec=0, off=1),
    _pt('vec0-base-x3', 0, X3, _M, 128, 128, FOUR_WAVE, (128, 128), 10, vec=0, off=1),
    _pt('vec0-base-x6', 0, X6, _M, 128, 64, FOUR_WAVE, (128, 64), 10, vec=0, off=1),
    _pt('vec0-k10-b16', 1, X3, _M, 64, 10, B16_REG, (64, 64), 10, vec=0),
    _pt('vec0-ld-b16', 1, X3, _M, 128, 128, B16_REG, (128, 128), 10, vec=0, padg=12),     # ld % 8 != 0: no 16-byte row of bf16
    _pt('vec0-base-b16', 1, X3, _M, 128, 128, B16_REG, (128, 128), 10, vec=0, off=1),
    _pt('vec0-b16-512', 1, X3, _M, 512, 512, B16_REG, (128, 128), 10, vec=0, off=1, tiles=(4, 4)),   # and so no 256 x 256 tile either
    # ---- several tiles: fewer wanted chunks, longer chunks.  bf16x3 on 128 x 128 tiles: 256 wanted blocks up to 32 768 rows
    # (4 tiles: 64 chunks of 512 rows), 384 beyond (96 chunks: ceil(32 769 / 96) = 342 -> 352 rows, 94 chunks)
    _pt('one-per-cu-32768', 0, X3, 32768, 256, 256, PC, (128, 128), 64, ws=1, tiles=(2, 2), rows=512),
    _pt('not-one-per-cu-32769', 0, X3, 32769, 256, 256, PC, (128, 128), 94, ws=1, tiles=(2, 2), rows=352),
    _pt('largest-32896', 0, X3, 32896, 256, 256, PC, (128, 128), 94, ws=1, tiles=(2, 2), rows=352),
    _pt('largest-32896-f32', 0, F32, 32896, 256, 256, EXACT, (128, 128), 94, tiles=(2, 2), rows=352),
    _pt('largest-32896-b16', 1, X3, 32896, 256, 256, B16_TR, (128, 128), 94, tiles=(2, 2), rows=352),
    # ---- no rows: no chunk, nothing launched but the fold, zeros
    _pt('m0-f32', 0, F32, 0, 64, 64, NONE, (64, 64), 0),
    _pt('m0-x3', 0, X3, 0, 128, 128, NONE, (128, 128), 0),
    _pt('m0-skinny', 0, X3, 0, 64, 12, NONE, SKINNY, 0),
    _pt('m0-b16', 1, X3, 0, 128, 128, NONE, (128, 128), 0),
]

POINTS = list(_sweep()) + CLASS_POINTS
assert len({p.id for p in POINTS}) == len(POINTS)

# stin_gemm_tn_bn_f32 (X read as relu(bn(X)); contiguous fp32 operands, not the skinny kernel): one point per tile class and
# the chunk counts 9 (7 idle block slots) and 241 (the sixteen-in-flight fold), full and with one row in the last chunk
BN_POINTS = [
    _pt('bn-f32-64x64', 0, F32, _M, 64, 64, EXACT, (64, 64), 10, padg=0, padx=0),
    _pt('bn-f32-64x128', 0, F32, _M, 36, 72, EXACT, (64, 128), 10, padg=0, padx=0),
    _pt('bn-f32-128x64', 0, F32, _M, 72, 40, EXACT, (128, 64), 10, padg=0, padx=0),
    _pt('bn-f32-128x128', 0, F32, _M, 132, 260, EXACT, (128, 128), 10, padg=0, padx=0, tiles=(2, 3)),
    _pt('bn-x6-128x64', 0, X6, _M, 128, 64, FOUR_WAVE, (128, 64), 10, padg=0, padx=0),
    _pt('bn-x3-ws', 0, X3, _M, 128, 128, PC, (128, 128), 10, ws=1, padg=0, padx=0),
    _pt('bn-x3-ws-ragged', 0, X3, _M, 320, 132, PC, (128, 128), 10, ws=1, padg=0, padx=0, tiles=(3, 2)),
    _pt('bn-x3-4wave', 0, X3, _M, 128, 128, FOUR_WAVE, (128, 128), 10, padg=0, padx=0, env={'STIN_TN_WS': '0'}),
    _pt('bn-x3-4wave-64x64', 0, X3, _M, 64, 64, FOUR_WAVE, (64, 64), 10, padg=0, padx=0, env={'STIN_TN_WS': '0'}),
    _pt('bn-vec0-k10', 0, X3, _M, 64, 10, FOUR_WAVE, (64, 64), 10, vec=0, padg=0, padx=0),
] + [_pt('bn-%s-c%d-m%d' % (name, c, m), 0, prec, m, Nc, K, family, tile, c, ws=ws, padg=0, padx=0, tiles=(1, 1), rows=128)
     for name, prec, Nc, K, family, tile, ws in (('x3-ws', X3, 128, 128, PC, (128, 128), 1), ('f32', F32, 64, 64, EXACT, (64, 64), 0))
     for c in (9, 241) for m in (128 * c, 128 * (c - 1) + 1)]
# ... and the one route the query cannot be asked for (it takes no transform): the four transform vectors one element behind a
# 16-byte boundary, operands aligned.  The product keeps the tile and the chunks of the aligned form ('bn-x3-ws': 128 x 128, 10
# chunks) and runs the four-wave kernel without 16-byte loads, k_gemm_tn_bf16s<128, 128, 2, false>.
BN_UNALIGNED_TF_POINT = _pt('bn-x3-tf-unaligned', 0, X3, _M, 128, 128, FOUR_WAVE, (128, 128), 10, vec=0, padg=0, padx=0)

# ------------------------------------------------------------------------------------------------ the block entry points
# (Cin, Cp, H, Cout): x is [N, Cp], zero-padded from Cin; Yw = 2 H (+ Cout), compact trans-inv layout H (+ Cout)
BLOCK_SHAPES = [
    (10, 12, 64, 32),        # the packed product is skinny (K = 12), dW2 = 32 x 64 - bf16x3: one 128 x 128 producer / consumer tile
    (64, 64, 128, 64),       # Yw = 320 with shortcut: three 128-tiles, the last ragged; both products in ONE producer / consumer grid
    (128, 128, 256, 128),
    (36, 36, 72, 40),        # generic widths
]
# 1 | 1 (one row short of full) | 1 (full) | 2 | 9 | 10 | 257 | 258 chunks of 128 rows where a product has ONE tile
BLOCK_NS = (1, 127, 128, 129, 1025, 1153, 32896, 32897)
# the mapped entry point serves the shapes whose packed product runs on the producer / consumer kernel: not the first (skinny) one
BLOCK_MAP_SHAPES = BLOCK_SHAPES[1:]
BLOCK_MAP_NS = (129, 1025, 4099)          # no multiples of 4: the guarded last slabs of the mapped producer
COLSUM_ROWS = (1, 16, 17, 65, 257)        # rows of ti_colsum (compact layout): one lane | all 16 lanes once | a second trip | 4-in-flight | 16-in-flight


def block_yw(H, Cout, shortcut, ti):
    return (H if ti == 2 else 2 * H) + (Cout if shortcut else 0)


def block_products(shape, shortcut, ti, storage, N, prec):
    """The two TN products of one block as stin_gemm_tn_route arguments (storage, M, Nc, K, ldg, ldx, aligned16, ones, precision):
    A: dW2 | db2 = dagg^T [hE[:, :H] | hE[:, H]] (hE has H + 4 columns), B: the packed product dY^T [x | 1]."""
    Cin, Cp, H, Cout = shape
    Yw = block_yw(H, Cout, shortcut, ti)
    return (storage, N, Cout, H, Cout, H + 4, 1, 1, prec), (storage, N, Yw, Cp, Yw, Cp, 1, 1, prec)


def block_cases():
    """(shape, shortcut, trans_inv, storage, precision, N): every shape x shortcut x trans_inv x storage the entry points accept at
    the backward precision of the network (bf16x3), and exact fp32 / bf16x6 at two row counts."""
    for shape in BLOCK_SHAPES:
        for shortcut in (0, 1):
            for ti in (0, 1, 2):
                for storage in (0, 1):
                    if storage == 1 and ti == 2:
                        continue                           # (the compact layout is fp32 rows only)
                    for N in BLOCK_NS:
                        yield shape, shortcut, ti, storage, X3, N
                    if storage == 0:
                        for prec in (F32, X6):
                            for N in (129, 1153):
                                yield shape, shortcut, ti, storage, prec, N


SWITCHES = ('STIN_TN_WS', 'STIN_TN_TR', 'STIN_TN_BIG')      # the A/B switches that pick a TN route


def set_env(monkeypatch, env):
    """exactly the switches of `env`: a value inherited from the environment would change the route a case aims at"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def geometry(lib, storage, M, Nc, K, ldg, ldx, aligned16, ones, prec):
    """stin_gemm_tn_route -> dict(tile, tiles, rows, chunks, vec, ws, family, grid)"""
    import ctypes
    out = (ctypes.c_int32 * 10)()
    rc = lib.stin_gemm_tn_route(storage, M, Nc, K, ldg, ldx, aligned16, ones, prec, ctypes.addressof(out))
    assert rc == 0, rc
    return dict(tile=(out[0], out[1]), tiles=(out[2], out[3]), rows=out[4], chunks=out[5], vec=out[6], ws=out[7], family=out[8], grid=out[9])


def point_geometry(lib, p, ones=1):
    return geometry(lib, p.storage, p.M, p.Nc, p.K, p.Nc + p.padg, p.K + p.padx, int(p.off == 0), ones, p.prec)
