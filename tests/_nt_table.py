"""The routes of the forward / input-gradient (NT) products C = A W^T (+ epilogue): ONE table of points, shared by
tests/test_nt_geometry.py (CPU: every point reaches the kernel family, tile and parameters its line names, asked of
stin_gemm_nt_geometry) and tests/test_nt_routes_gpu.py (GPU: every launchable point gives the exact integer product through the
public entry point).  The expectations are written down here by hand from the host rules of csrc/gemm_nt_route.inc - they are NOT
computed by a copy of those rules: a rule change makes test_nt_geometry.py fail on a machine without a GPU and says which point no
longer aims where its line says.  Every point states its switches and the CU count it is asked for (256 = MI355X).
"""
import collections

# STIN_GEMM_* (checked against the header by test_nt_geometry.py)
F32, X3, X6, F16, PRE, FRAG, WB16 = 0, 2, 3, 4, 0x100, 0x400, 0x200
XF, HF = X3 | PRE | FRAG, F16 | PRE | FRAG           # pre-split weights in fragment order where the shape takes it
# STIN_NT_*: the families
NONE, TILED, STREAM, STRIP, WIDE, PANEL, B16_TILED, B16_GLDS = range(8)
# STIN_NT_PART_*
BIAS, MASK, RES, COLSTATS, DOTELU, BN_TF, BWD_STATS, BWD_APPLY, OUT_F32, STREAM_ONLY = (1 << i for i in range(10))
# STIN_NT_ALIGN_*
A_IN, A_OUT, A_TF, A_BIAS = 1, 2, 4, 8
E_ALIGN, E_UNSUPPORTED = -3, -5

# storage 0 = fp32 rows, 1 = bf16 rows.  A and W are views of width K in rows of K + padk elements whose base is `off` elements behind
# a 16-byte boundary; C (and the residual) are views of width Nc in rows of Nc + padc elements.  env = the switches set for the
# point (all others unset).  Then what the point must reach: rc (0, or the refusal), family, tile (BM, BN), param, vec, vec_out
# and, where the line is about them, grid (x, y), lds and groups.
Point = collections.namedtuple('Point', 'id storage prec M Nc K parts env cu padk off padc rc family tile param vec vec_out grid lds groups')


def _pt(id, storage, prec, M, Nc, K, family, tile=None, param=0, vec=1, vec_out=0, grid=None, lds=None, groups=0, parts=0, env=None,
        cu=256, padk=None, off=0, padc=8, rc=0):
    padk = (8 if storage else 4) if padk is None else padk
    return Point(id, storage, prec, M, Nc, K, parts, dict(env or {}), cu, padk, off, padc, rc, family, tile, param, vec, vec_out, grid, lds,
                 groups)


def _no(id, storage, prec, M, Nc, K, rc, **kw):
    return _pt(id, storage, prec, M, Nc, K, None, rc=rc, **kw)


P0, P1 = {'STIN_NT_PANEL': '0'}, {'STIN_NT_PANEL': '1'}

POINTS = [
    # ---- tiled kernels, fp32 rows.  Nc <= 32: 128 x 32; else 64 x 64; 128 x 128 for Nc % 128 == 0, K >= 512 and >= 500 tiles of 128 x 128
    _pt('tiled-128x32-f32', 0, F32, 1000, 32, 64, TILED, (128, 32), grid=(8, 1)),
    _pt('tiled-128x32-x3', 0, X3, 1000, 24, 64, TILED, (128, 32), grid=(8, 1)),
    _pt('tiled-64x64-x3', 0, X3, 1000, 64, 128, TILED, (64, 64), grid=(16, 1)),
    _pt('tiled-64x64-x6', 0, X6, 1000, 96, 64, TILED, (64, 64), grid=(32, 1)),
    _pt('tiled-64x64-f16-epi', 0, F16, 1000, 64, 64, TILED, (64, 64), grid=(16, 1), parts=BIAS | MASK | RES),
    # Nc = 512, K = 512: 4 column tiles; 124 row tiles = 496 tiles, 125 = 500
    _pt('tiled-big-496-f32', 0, F32, 15872, 512, 512, TILED, (64, 64), grid=(248 * 8, 1)),
    _pt('tiled-big-500-f32', 0, F32, 15873, 512, 512, TILED, (128, 128), grid=(128 * 4, 1)),
    _pt('tiled-big-496-pre', 0, X3 | PRE, 15872, 512, 512, TILED, (64, 64), grid=(248 * 8, 1)),
    _pt('tiled-big-500-pre', 0, X3 | PRE, 15873, 512, 512, TILED, (128, 128), grid=(128 * 4, 1)),
    _pt('tiled-pre-f16', 0, F16 | PRE, 1000, 24, 64, TILED, (64, 64), grid=(16, 1)),      # pre-split W: no 128 x 32 tile
    # vec = 0 from each cause: K % 4 | ld % 4 | base 4 bytes behind a 16-byte boundary
    _pt('tiled-vec0-k', 0, X3, 300, 64, 66, TILED, (64, 64), vec=0, grid=(5, 1), padk=2),
    _pt('tiled-vec0-ld', 0, X3, 300, 64, 64, TILED, (64, 64), vec=0, grid=(5, 1), padk=2),
    _pt('tiled-vec0-base', 0, F32, 300, 64, 64, TILED, (64, 64), vec=0, grid=(5, 1), off=1),
    _no('pre-vec0-refused', 0, X3 | PRE, 300, 64, 64, E_ALIGN, off=1),
    # the grid: plain block order below 16 row tiles, whole rounds of 8 row tiles (one per XCD) from 16 on; 2 column tiles
    _pt('tiled-grid-15', 0, X3, 960, 128, 64, TILED, (64, 64), grid=(30, 1)),
    _pt('tiled-grid-16', 0, X3, 961, 128, 64, TILED, (64, 64), grid=(32, 1)),
    _pt('tiled-grid-17', 0, X3, 1025, 128, 64, TILED, (64, 64), grid=(48, 1)),

    # ---- resident-strip kernel (fragment order, Nc >= 320, K = 128 .. 256; Nc % 128 != 0 or STIN_NT_PANEL=0 keeps the panel kernel off)
    # LDS = 2 (KC / 32) BM 64 + panels x 512 + 4 BM, + 2 KB per wave of restage area where min(2, blocks per CU) stays
    # cfg 21 (BM 64, 4 waves), K = 128, 3 panels: 32 768 + 1536 + 256 = 34 560 (4 per CU), restaged 42 752 (3): both capped at 2 -> on
    _pt('strip-21-k128-units', 0, XF, 1000, 320, 128, STRIP, (64, 128), 21, vec_out=1, grid=(48, 1), lds=42752),     # 16 x 3 units < 512
    _pt('strip-21-k128-cus', 0, HF, 20000, 320, 128, STRIP, (64, 128), 21, vec_out=1, grid=(512, 1), lds=42752),     # 939 units > 256 x 2
    _pt('strip-21-k256', 0, XF, 1000, 320, 256, STRIP, (64, 128), 21, vec_out=1, grid=(48, 1), lds=75520),           # 67 328 + 8192: 2 -> 2
    _pt('strip-21-nc608', 0, XF, 1000, 608, 192, STRIP, (64, 128), 21, vec_out=1, grid=(80, 1), lds=60160),          # 49 152 + 2560 + 256 + 8192
    # cfg 22 (BM 128, 8 waves, one block per CU) from Nc = 640: K = 128, 6 panels: 65 536 + 3072 + 512 = 69 120 (2), + 16 384 (1) -> off
    _pt('strip-22-nc672-k128', 0, XF, 2000, 672, 128, STRIP, (128, 128), 22, vec_out=0, grid=(96, 1), lds=69120),
    _pt('strip-22-nc640-k128', 0, XF, 20000, 640, 128, STRIP, (128, 128), 22, vec_out=0, grid=(256, 1), lds=68608, env=P0),
    _pt('strip-22-nc640-k256', 0, HF, 20000, 640, 256, STRIP, (128, 128), 22, vec_out=1, grid=(256, 1), lds=150528, env=P0),   # 134 144 (1) + 16 384 (1)
    # cfg 41 (BM 128, 4 waves) by switch only
    _pt('strip-41-k256', 0, XF, 1000, 320, 256, STRIP, (128, 128), 41, vec_out=1, grid=(24, 1), lds=141312, env={'STIN_STRIP_CFG': '41'}),
    _pt('strip-41-k128', 0, XF, 1000, 320, 128, STRIP, (128, 128), 41, vec_out=1, grid=(24, 1), lds=75776, env={'STIN_STRIP_CFG': '41'}),
    _pt('strip-22-switch', 0, XF, 1000, 320, 128, STRIP, (128, 128), 22, vec_out=0, grid=(24, 1), lds=67584, env={'STIN_STRIP_CFG': '22'}),
    _no('strip-unaligned-c', 0, XF, 1000, 320, 128, E_ALIGN, padc=2),

    # ---- all-columns kernel (fragment order, Nc = 128 with K >= 256, Nc = 256 with K >= 512): param = waves along M
    _pt('wide-nc128-4waves', 0, XF, 5000, 128, 256, WIDE, (128, 128), 2, vec_out=1, grid=(40, 1), env=P0),
    _pt('wide-nc256-8waves', 0, XF, 32768, 256, 512, WIDE, (128, 256), 2, vec_out=1, grid=(256, 1), env=P0),          # 256 blocks of 128 rows: one round
    _pt('wide-nc256-4waves', 0, HF, 32769, 256, 512, WIDE, (64, 256), 1, vec_out=1, grid=(513, 1), env=P0),
    _pt('wide-vecout0', 0, XF, 5000, 128, 256, WIDE, (128, 128), 2, vec_out=0, grid=(40, 1), padc=2),                # C rows not 16-byte: no panel either
    _pt('wide-colstats', 0, HF, 5000, 128, 256, WIDE, (128, 128), 2, vec_out=1, grid=(40, 1), groups=79, parts=COLSTATS | BIAS | MASK, env=P0),
    _pt('wide-colstats-res', 0, XF, 130, 256, 512, WIDE, (128, 256), 2, vec_out=0, grid=(2, 1), groups=3, parts=COLSTATS | RES, env=P0),

    # ---- panel kernel: tiles per block = ceil(ceil(M / 32) / (cu / panels)), 2 .. 9 in one round.  Nc = 256: 128 slots
    _pt('panel-m1', 0, XF, 1, 256, 512, PANEL, (64, 128), 2, vec_out=1, grid=(2, 1), lds=33024),
] + [
    _pt('panel-%d' % k, 0, XF if k % 2 else HF, 4096 * k - 5, 256, 512, PANEL, (32 * k, 128), k, vec_out=1, grid=(256, 1),
        lds=33024 if k == 2 else 16384 * k) for k in range(2, 10)
] + [
    _pt('panel-10-falls-back', 0, XF, 36865, 256, 512, WIDE, (64, 256), 1, vec_out=1, grid=(577, 1)),
    _pt('panel-switch-0', 0, XF, 8187, 256, 512, WIDE, (128, 256), 2, vec_out=1, grid=(64, 1), env=P0),
    _pt('panel-switch-1', 0, XF, 40000, 256, 512, PANEL, (160, 128), 5, vec_out=1, grid=(512, 1), lds=81920, env=P1),   # two rounds: 1250 groups / 256
    _pt('panel-cu64', 0, XF, 4091, 256, 512, PANEL, (128, 128), 4, vec_out=1, grid=(64, 1), lds=65536, cu=64),          # 32 slots, 128 row groups
    _pt('panel-cu64-falls-back', 0, XF, 10000, 256, 512, WIDE, (64, 256), 1, vec_out=1, grid=(157, 1), cu=64),          # 313 groups / 32 = 10
    _pt('panel-colstats', 0, XF, 8187, 256, 512, PANEL, (64, 128), 2, vec_out=1, grid=(256, 1), groups=256, parts=COLSTATS | BIAS | MASK),
    _pt('panel-dotelu', 0, XF, 8187, 256, 512, PANEL, (64, 128), 2, vec_out=1, grid=(256, 1), groups=256, parts=COLSTATS | DOTELU | RES),
    _pt('panel-dotelu-nc512', 0, XF, 8190, 512, 256, PANEL, (128, 128), 4, vec_out=1, grid=(256, 1), groups=128, parts=COLSTATS | DOTELU),
    _no('panel-colstats-residual', 0, XF, 4091, 256, 512, E_ALIGN, parts=COLSTATS | RES),        # not the launch the group count was for
    _no('colstats-nc512', 0, XF, 8190, 512, 256, E_UNSUPPORTED, parts=COLSTATS),
    _no('colstats-plain-w', 0, X3, 5000, 128, 256, E_UNSUPPORTED, parts=COLSTATS),
    _no('dotelu-switch-0', 0, XF, 8187, 256, 512, E_UNSUPPORTED, parts=COLSTATS | DOTELU, env={'STIN_DOTELU_FUSED': '0'}),
    _no('dotelu-no-panel', 0, XF, 8187, 256, 512, E_UNSUPPORTED, parts=COLSTATS | DOTELU, env=P0),

    # ---- streaming kernel: K = 64 .. 512 in steps of 64, Nc % 4 == 0; 128 rows per block x param column tiles of 32
    # LDS = piece bytes (4; bf16x6: 6) x (K x 32 x tiles + 128 x 64) (+ 8 K with the operand transform, + 768 x tiles under a BatchNorm backward)
    _pt('stream-65535-tiled', 0, X3, 65535, 64, 64, TILED, (64, 64), grid=(1024, 1)),
    _pt('stream-65536', 0, X3, 65536, 64, 64, STREAM, (128, 64), 2, grid=(512, 1), lds=49152),
    _pt('stream-65536-x6', 0, X6, 65536, 64, 64, STREAM, (128, 64), 2, grid=(512, 1), lds=73728),
    _pt('stream-65536-x6-epi', 0, X6, 65536, 64, 64, TILED, (64, 64), grid=(1024, 1), parts=BIAS),       # the epilogue: 2-piece only
    _pt('stream-65536-epi', 0, F16, 65536, 64, 64, STREAM, (128, 64), 2, grid=(512, 1), lds=49152, parts=BIAS | MASK | RES),
    _pt('stream-65536-bn', 0, X3, 65536, 64, 64, STREAM, (128, 64), 2, grid=(512, 1), lds=49664, parts=BN_TF),
    _pt('stream-switch-0', 0, X3, 65536, 64, 64, TILED, (64, 64), grid=(1024, 1), env={'STIN_NT_STREAM': '0'}),
    _pt('stream-f32-never', 0, F32, 65536, 64, 64, TILED, (64, 64), grid=(1024, 1)),
    _pt('stream-pre-499999-tiled', 0, X3 | PRE, 499999, 64, 64, TILED, (64, 64), grid=(7816, 1)),
    _pt('stream-pre-500000', 0, X3 | PRE, 500000, 64, 64, STREAM, (128, 64), 2, grid=(512, 1), lds=49152, parts=BIAS),
    _pt('stream-pre-rows-switch', 0, F16 | PRE, 2000, 64, 64, STREAM, (128, 64), 2, grid=(16, 1), lds=49152, env={'STIN_NT_STREAM_PRE_ROWS': '1000'}),
    _pt('stream-4-tiles', 0, X3, 65536, 128, 64, STREAM, (128, 128), 4, grid=(512, 1), lds=65536),
    _pt('stream-2-tiles-switch', 0, X3, 65536, 128, 64, STREAM, (128, 64), 2, grid=(256, 2), lds=49152, env={'STIN_NT_STREAM_NT': '2'}),
    _pt('stream-4-tiles-switch', 0, X3, 65536, 64, 64, STREAM, (128, 128), 4, grid=(512, 1), lds=65536, env={'STIN_NT_STREAM_NT': '4'}),
    # asked for by name (stin_gemm_nt_stream_f32): any row count.  The LDS fallbacks: 4 tiles while they fit 160 KB, else 2, else not served
    _pt('stream-x3-k256-4', 0, X3, 3000, 128, 256, STREAM, (128, 128), 4, grid=(24, 1), lds=163840, parts=STREAM_ONLY),
    _pt('stream-x3-k320-2', 0, X3, 3000, 128, 320, STREAM, (128, 64), 2, grid=(24, 2), lds=114688, parts=STREAM_ONLY),
    _pt('stream-x6-k128-4', 0, X6, 3000, 128, 128, STREAM, (128, 128), 4, grid=(24, 1), lds=147456, parts=STREAM_ONLY),
    _pt('stream-x6-k192-2', 0, X6, 3000, 128, 192, STREAM, (128, 64), 2, grid=(24, 2), lds=122880, parts=STREAM_ONLY),
    _no('stream-x6-k320', 0, X6, 3000, 128, 320, E_UNSUPPORTED, parts=STREAM_ONLY),
    _pt('stream-x3-k512', 0, X3, 3000, 64, 512, STREAM, (128, 64), 2, grid=(24, 1), lds=163840, parts=STREAM_ONLY),
    _no('stream-k576', 0, X3, 3000, 64, 576, E_UNSUPPORTED, parts=STREAM_ONLY),
    _no('stream-nc66', 0, X3, 3000, 66, 64, E_UNSUPPORTED, parts=STREAM_ONLY),
    _no('stream-f32', 0, F32, 3000, 64, 64, E_UNSUPPORTED, parts=STREAM_ONLY),
    _no('stream-unaligned', 0, X3, 3000, 64, 64, E_UNSUPPORTED, parts=STREAM_ONLY, off=1),
    # the BatchNorm backward pair: K <= 128 only; the statistics pass on two column tiles, one group of sums per row walker
    _pt('bnbwd-stats-k64', 0, X3, 5000, 128, 64, STREAM, (128, 64), 2, grid=(40, 2), lds=50688, groups=40, parts=BWD_STATS),
    _pt('bnbwd-stats-k128', 0, X6, 5000, 256, 128, STREAM, (128, 64), 2, grid=(40, 4), lds=99840, groups=40, parts=BWD_STATS),
    _pt('bnbwd-apply-k64', 0, X3, 5000, 128, 64, STREAM, (128, 128), 4, grid=(40, 1), lds=68608, parts=BWD_APPLY),
    _no('bnbwd-stats-k192', 0, X3, 5000, 128, 192, E_UNSUPPORTED, parts=BWD_STATS),
    _no('bnbwd-apply-k256', 0, X3, 5000, 128, 256, E_UNSUPPORTED, parts=BWD_APPLY),

    # ---- bf16 rows: 128 x 32 for Nc <= 32, else 64 x 64; 128 x 64 for K >= 512 and >= 1000 tiles of 128 x 64
    _pt('b16-128x32', 1, 0, 1000, 32, 64, B16_TILED, (128, 32), vec_out=1, grid=(8, 1)),
    _pt('b16-64x64', 1, 0, 1000, 64, 64, B16_TILED, (64, 64), vec_out=1, grid=(16, 1), parts=BIAS | MASK | RES),
    _pt('b16-64x64-f32-out', 1, 0, 1000, 64, 64, B16_TILED, (64, 64), vec_out=0, grid=(16, 1), parts=OUT_F32),
    _pt('b16-vec0', 1, 0, 1000, 64, 68, B16_TILED, (64, 64), vec=0, vec_out=1, grid=(16, 1), padk=4),
    _pt('b16-999-tiles', 1, 0, 127872, 64, 512, B16_TILED, (64, 64), vec_out=1, grid=(2000, 1)),
    _pt('b16-1000-tiles', 1, 0, 127873, 64, 512, B16_TILED, (128, 64), vec_out=1, grid=(1000, 1)),
    _pt('b16-wb-tiled', 1, WB16, 1000, 64, 64, B16_TILED, (64, 64), vec_out=1, grid=(16, 1)),
    _no('b16-wb-unaligned', 1, WB16, 1000, 64, 68, E_ALIGN, padk=4),
    # the LDS-DMA kernel (bf16 weights, K % 64 == 0): K >= 1024, Nc >= 256 and >= 128 tiles of 128 x 128; 256 x 256 tiles for
    # Nc >= 512 and >= 200 of them (two column tiles: 99 rows = 198, 100 rows = 200)
    _pt('glds-126-tiles-off', 1, WB16, 8064, 256, 1024, B16_TILED, (64, 64), vec_out=1, grid=(512, 1)),
    _pt('glds-128-tiles-on', 1, WB16, 8192, 256, 1024, B16_GLDS, (128, 128), vec_out=1, grid=(128, 1), lds=65536),
    _pt('glds-198-big-off', 1, WB16, 25344, 512, 1024, B16_GLDS, (128, 128), vec_out=1, grid=(800, 1), lds=65536),
    _pt('glds-200-big-on', 1, WB16, 25600, 512, 1024, B16_GLDS, (256, 256), vec_out=1, grid=(208, 1), lds=147456),
    _pt('glds-switch-1', 1, WB16, 1000, 64, 64, B16_GLDS, (128, 128), vec_out=0, grid=(8, 1), lds=65536, parts=OUT_F32, env={'STIN_NT_GLDS': '1'}),
    _pt('glds-switch-0', 1, WB16, 8192, 256, 1024, B16_TILED, (64, 64), vec_out=1, grid=(512, 1), env={'STIN_NT_GLDS': '0'}),
    _pt('glds-big-switch-1', 1, WB16, 8192, 256, 1024, B16_GLDS, (256, 256), vec_out=1, grid=(32, 1), lds=147456, env={'STIN_NT_BIG': '1'}),
    _pt('glds-big-switch-0', 1, WB16, 25600, 512, 1024, B16_GLDS, (128, 128), vec_out=1, grid=(800, 1), lds=65536, env={'STIN_NT_BIG': '0'}),
    _pt('glds-fp32-w-never', 1, 0, 8192, 256, 1024, B16_TILED, (64, 64), vec_out=1, grid=(512, 1)),

    # ---- no rows: nothing launched
    _pt('m0-f32', 0, X3, 0, 64, 64, NONE, (0, 0), vec=0),
    _pt('m0-b16', 1, 0, 0, 64, 64, NONE, (0, 0), vec=0),
]
assert len({p.id for p in POINTS}) == len(POINTS)

SWITCHES = ('STIN_NT_STREAM', 'STIN_NT_STREAM_NT', 'STIN_NT_STREAM_PRE_ROWS', 'STIN_NT_BNBWD', 'STIN_DOTELU_FUSED', 'STIN_NT_PANEL',
            'STIN_STRIP_CFG', 'STIN_NT_GLDS', 'STIN_NT_BIG')


def set_env(monkeypatch, env):
    """exactly the switches of `env`: a value inherited from the environment would change the route a point aims at"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def launchable(p):
    """the points the GPU test runs: served, with rows, and asked for the CU count of the device it runs on (MI355X: 256)"""
    return p.rc == 0 and p.family != NONE and p.cu == 256


def align_of(p):
    """STIN_NT_ALIGN_* of the operand layout of a point (the transform and bias vectors are whole allocations: aligned)"""
    a = 8 if p.storage else 4                        # elements per 16 bytes of the rows
    wa = 8 if (p.storage and p.prec & WB16) else 4   # ... of the weight rows
    in16 = (p.K + p.padk) % a == 0 and (p.K + p.padk) % wa == 0 and p.off % a == 0 and p.off % wa == 0
    out16 = (p.Nc + p.padc) % a == 0
    return (A_IN if in16 else 0) | (A_OUT if out16 else 0) | A_TF | A_BIAS


def geometry(lib, p):
    """stin_gemm_nt_geometry of a point -> (rc, dict)"""
    import ctypes
    out = (ctypes.c_int32 * 10)(*([-77] * 10))
    rc = lib.stin_gemm_nt_geometry(p.storage, p.M, p.Nc, p.K, p.prec, p.parts, align_of(p), p.cu, ctypes.addressof(out))
    keys = ('family', 'bm', 'bn', 'param', 'vec', 'vec_out', 'lds', 'gx', 'gy', 'groups')
    return rc, dict(zip(keys, out))
