// Host only: WHICH kernel runs a TN product dW = G^T [X | w], on what tile, chunks, grid and LDS.  One pure function, tn_route, asked
// by every TN entry point of stin_gemm.hip and (through stin_common.h, which holds the three records) of stin_wgrad.hip, by
// stin_gemm_tn_workspace_bytes, stin_edgeconv_wgrad_map_supported, stin_gemm_tn_geometry and stin_gemm_tn_route (tests/_tn_table.py: the points it must
// reach).  Of the kernel files it names only constants (BLOCK, TN_R, TrGeom).  The NT rules: gemm_nt_route.inc.
// The A/B switches of the TN routes, read ONCE per entry-point call (tests flip them between calls) - the only getenv of TN host code.
inline TnSwitches tn_switches() {
    auto flag = [](const char* e) { return e == nullptr ? -1 : (atoi(e) != 0 ? 1 : 0); };
    TnSwitches s;
    s.pc = flag(getenv("STIN_TN_WS")) != 0;
    s.big = flag(getenv("STIN_TN_BIG"));
    s.tr = flag(getenv("STIN_TN_TR"));
    return s;
}

inline int tn_tile(int n) {
    return n > 64 ? 128 : 64;    // (measured: 64x64 wgrad tiles are 2-5 % slower end to end at any slab count)
}
inline int tn_rows_per_chunk(int64_t M, int tiles, bool one_per_cu) {
    // ~384 blocks (up to 2 resident per CU, one round), chunks a multiple of the LDS slab.  Round 1 measured 512 best of
    // 256..1536; with loads two slabs ahead a block hides more latency by itself and fewer chunks mean fewer partial slabs to
    // store and reduce: 384 is 0.3-0.5 % faster on the step than 512 (256: 0.4 % slower)
    // one_per_cu (round 3: fp32 bf16x3 products on 128 x 128 tiles with M <= 32 k rows, the shapes of the bottleneck level):
    // 256 blocks - the producer / consumer kernel's fixed cost per block (first-load latency ~5 k cycles, slab store ~9 k) is
    // a sixth of a 750-row chunk; measured 18 063 x 1024 x 256 49.7 -> 45.7 us, block weight gradients 69 -> 62 us, while the
    // 60 k-row products lose 10 % with 256 blocks and keep 384
    const int want = one_per_cu ? 256 : 384;
    int64_t chunks = (want + tiles - 1) / tiles;
    if (chunks > 8) chunks = (chunks + 7) / 8 * 8;          // whole rounds of 8 chunks (one per XCD, see tn_block_map)
    int64_t rows = (M + chunks - 1) / chunks;
    if (rows < 4 * TN_R) rows = 4 * TN_R;
    constexpr int max_rows = 128 * TN_R;
    if (rows > max_rows) rows = max_rows;
    rows = (rows + TN_R - 1) / TN_R * TN_R;
    return (int)rows;
}
inline bool tn_one_per_cu(const TnProblem& p, int TI, int TJ) {
    return p.storage == 0 && p.precision == STIN_GEMM_BF16X3 && TI == 128 && TJ == 128 && p.M <= 32768;
}
// bf16-storage TN: 256 x 256 tiles (k_gemm_tn_b16_tr<2, 4, 4, 2>) for the fat products.  STIN_TN_BIG = 0 | 1 forces (the workspace
// bound covers both choices).
inline bool tn_b16_big_tile(int Nc, int K, int forced) {
    if (forced >= 0) return forced != 0 && Nc >= 256 && K >= 256;
    return Nc >= 512 && K >= 512;
}
// bf16-storage TN, 128 x 128 tiles: the transposed-read kernel (k_gemm_tn_b16_tr); STIN_TN_TR=0 keeps the register-transpose
// kernel (A/B switch).
inline bool tn_b16_tr_enabled(int Nc, int K, int forced) {
    if (forced >= 0) return forced != 0;
    // whole tiles only: with a ragged third tile (161 362 x 320 x 128, the level-0 product of the crop batches) the 64 KB of LDS
    // (two blocks per CU instead of four) cost more than the transposes: 54.6 -> 68.6 us; whole-tile shapes gain 5-17 %
    return Nc % 128 == 0 && K % 128 == 0;
}
// k_gemm_tn_skinny (gemm_tn_skinny.inc): fp32 rows, K <= 16, a block owns all Nc columns of its row chunk
inline bool tn_skinny_shape(const TnProblem& p) {
    return p.storage == 0 && p.K <= 16 && p.K % 4 == 0 && p.Nc % 4 == 0 && p.Nc >= 64 && p.Nc <= 4 * BLOCK && p.ldg % 4 == 0 &&
           p.ldx % 4 == 0 && p.aligned16;
}
inline int tn_skinny_rows(int64_t M) {                                         // ~1024 chunks, a multiple of 32 rows, at least 128
    constexpr int want = 1024;                                                  // measured: 256 / 512 / 1024 / 2048 chunks: 106 / 75 / 72 / 79 us at 200 704 x 320 x 12
    int64_t rows = (M + want - 1) / want;
    rows = (rows + 31) / 32 * 32;
    // the chunk's [X | w] image is rows x (KP + 4 <= 20) floats of dynamic LDS: capped at 512 rows = 40 KB (below the 64 KB a
    // launch gets without hipFuncSetAttribute) - beyond ~0.5 M rows the chunk COUNT grows instead of the chunk
    if (rows > 512) rows = 512;
    return (int)(rows < 128 ? 128 : rows);
}
// blocks of a tiled grid: plain order below 8 chunks, else whole rounds of 8 chunks (one per XCD: tn_block_map)
inline int64_t tn_grid(int64_t chunks, int tiles) { return (chunks >= 8 ? ((chunks + 7) / 8) * 8 : chunks) * (int64_t)tiles; }

// THE decision.  Pure: no getenv, no HIP call, no statics, no pointers.  Precedence: the tile of the width rule (bf16 rows with
// 16-byte vectors: 256 x 256 for the fat products); bf16x3 on 16-byte fp32 rows with both widths >= 32: the 128 x 128 tile of the
// producer / consumer kernel, while that kernel is enabled; the chunk rule on that tile; last, the skinny shape overrides all of it.
inline TnRoute tn_route(const TnProblem& p, const TnSwitches& sw) {
    TnRoute r = {};
    r.family = STIN_TN_FAMILY_NONE;
    if (!(p.M >= 0 && p.Nc > 0 && p.K > 0 && p.ldg >= p.Nc && p.ldx >= p.K)) { r.status = STIN_E_SIZE; return r; }
    const int a16 = p.storage ? 8 : 4;                             // elements per 16-byte vector
    const bool vec16 = (p.Nc % a16 == 0) && (p.K % a16 == 0) && (p.ldg % a16 == 0) && (p.ldx % a16 == 0) && p.aligned16;
    const bool big = p.storage == 1 && vec16 && tn_b16_big_tile(p.Nc, p.K, sw.big);
    r.TI = big ? 256 : tn_tile(p.Nc);
    r.TJ = big ? 256 : tn_tile(p.K);
    // (round 5) fp32 bf16x3 products whose narrow side is <= 64 columns (the level-0 dW2 = dagg^T h: 64 x 128; SingleConvMeshNet's
    // per-edge dW2) ran on the four-wave kernel (its 64-wide tiles) at ~3 TB/s; on the producer / consumer kernel the same
    // product is a 128 x 128 tile that is half or a quarter empty - the wasted MFMAs are free beside the operand stream
    // (200 704 x 64 x 128: 50 -> 3x us; 1.2 M x 64 x 128: 267 -> 1xx us).  One tile either way: same chunks, same slabs.
    // 128 x 128 tiles of the width rule (both widths > 64) are a subset: this is the whole condition of the producer / consumer kernel.
    const bool pc = p.storage == 0 && p.precision == STIN_GEMM_BF16X3 && vec16 && p.M > 0 && p.Nc >= 32 && p.K >= 32 && sw.pc;
    if (pc) r.TI = r.TJ = 128;
    r.tiles_i = (p.Nc + r.TI - 1) / r.TI;
    r.tiles_j = (p.K + r.TJ - 1) / r.TJ;
    r.rows_per_chunk = tn_rows_per_chunk(p.M, r.tiles_i * r.tiles_j, big || tn_one_per_cu(p, r.TI, r.TJ));
    const bool skinny = tn_skinny_shape(p);
    if (skinny) {
        r.TI = r.TJ = 0;
        r.tiles_i = r.tiles_j = 1;
        r.rows_per_chunk = tn_skinny_rows(p.M);
    }
    r.chunks = p.M > 0 ? (p.M + r.rows_per_chunk - 1) / r.rows_per_chunk : 0;
    r.Kq = (p.K + 3) & ~3;
    // X read as relu(bn(X)): the tiled kernels and the producer / consumer kernel.  Transform vectors that are no 16-byte vectors
    // keep the tile and the chunks found above and run the four-wave kernel without 16-byte loads.
    r.vec = (vec16 && (!p.bn_tf || p.bn_tf_aligned16)) ? 1 : 0;
    if (p.bn_tf && skinny) { r.status = STIN_E_UNSUPPORTED; return r; }
    if (p.M == 0) return r;
    r.threads = BLOCK;
    r.grid = tn_grid(r.chunks, r.tiles_i * r.tiles_j);
    if (skinny) {                                                  // exact fp32 on the VALU, whatever the precision asked for
        const int kp = r.Kq;                                       // the chunk's [X | w] image, later the block's column sums
        const int64_t lds_x = (int64_t)r.rows_per_chunk * (kp + 4) * 4, lds_o = (int64_t)p.Nc * (kp + 1) * 4;
        r.family = STIN_TN_FAMILY_SKINNY, r.lds = lds_x > lds_o ? lds_x : lds_o, r.grid = r.chunks;
    } else if (p.storage == 1) {
        if (big) r.family = STIN_TN_FAMILY_B16_TR, r.threads = TrGeom<2, 4, 4, 2>::THREADS, r.lds = TrGeom<2, 4, 4, 2>::LDS;
        else if (r.TI == 128 && r.TJ == 128 && r.vec && tn_b16_tr_enabled(p.Nc, p.K, sw.tr))
            r.family = STIN_TN_FAMILY_B16_TR, r.threads = TrGeom<2, 2, 2, 2>::THREADS, r.lds = TrGeom<2, 2, 2, 2>::LDS;
        else r.family = STIN_TN_FAMILY_B16_REG;
    } else if (pc && r.vec) {
        r.family = STIN_TN_FAMILY_PC, r.threads = 2 * BLOCK;       // (four producer and four consumer waves: stin_wgrad.hip)
    } else {
        r.family = (p.precision == STIN_GEMM_BF16X3 || p.precision == STIN_GEMM_BF16X6) ? STIN_TN_FAMILY_BF16S : STIN_TN_FAMILY_F32;
    }
    if (p.x_row_map && r.family != STIN_TN_FAMILY_PC) r.status = STIN_E_UNSUPPORTED;   // only that kernel reads X through a map
    return r;
}
