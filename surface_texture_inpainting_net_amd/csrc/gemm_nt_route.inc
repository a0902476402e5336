// Host only: WHICH kernel runs an NT product C = A W^T (+ epilogue), on what tile, grid and LDS.  One pure function, nt_route, asked
// by every NT entry point of stin_gemm.hip, the three *_groups queries and stin_gemm_nt_geometry (tests/_nt_table.py: the points it
// must reach).  Of the kernel files it names only constants (ST_PANEL, WD_KC, BKB, GlGeom).  The TN rules: gemm_tn_route.inc.
// The A/B switches of the NT routes, read ONCE per entry-point call (tests flip them between calls) - the only getenv of NT host code.
struct NtSwitches {
    bool stream;               // STIN_NT_STREAM=0: never the streaming kernel on its own account (rows >= a threshold)
    int stream_nt;             // STIN_NT_STREAM_NT = 2 | 4: column tiles per block of the streaming kernel (else: the rule)
    int64_t stream_pre_rows;   // STIN_NT_STREAM_PRE_ROWS: row threshold of the streaming kernel for pre-split weights
    bool bnbwd;                // STIN_NT_BNBWD=0: stin_gemm_nt_bn_bwd_groups answers 0 (the caller keeps its three launches)
    bool dotelu;               // STIN_DOTELU_FUSED=0: no dot-ELU statistics on the panel kernel's epilogue
    int panel;                 // STIN_NT_PANEL: 0 = never the panel kernel, 1 = for every fragment-order shape, -1 (unset) = the rule
    int strip_cfg;             // STIN_STRIP_CFG = 21 | 22 | 41: strip-kernel configuration (else: the rule)
    int glds, big;             // STIN_NT_GLDS / STIN_NT_BIG = 0 | 1 force the bf16-row rules, -1 (unset) = the rule
};
inline NtSwitches nt_switches() {
    auto num = [](const char* e, int64_t unset) { return e != nullptr ? atoll(e) : unset; };
    auto flag = [](const char* e) { return e == nullptr ? -1 : (atoi(e) != 0 ? 1 : 0); };
    NtSwitches s;
    s.stream = num(getenv("STIN_NT_STREAM"), 1) != 0;
    s.stream_nt = (int)num(getenv("STIN_NT_STREAM_NT"), 0);
    // in-step A/B (profiles/r05_experiments_not_shipped.md): at 200 704 rows the headline step is 0.03 ms SLOWER with the streaming
    // kernel on pre-split weights (7.36-7.39 against 7.34 ms), at 1 M rows (config 5 in fp32) 0.35 ms faster (41.45 against
    // 41.81 ms) - the default sits between
    s.stream_pre_rows = num(getenv("STIN_NT_STREAM_PRE_ROWS"), 500000);
    s.bnbwd = num(getenv("STIN_NT_BNBWD"), 1) != 0;
    s.dotelu = num(getenv("STIN_DOTELU_FUSED"), 1) != 0;
    s.panel = (int)num(getenv("STIN_NT_PANEL"), -1);
    s.strip_cfg = (int)num(getenv("STIN_STRIP_CFG"), 0);
    s.glds = flag(getenv("STIN_NT_GLDS"));
    s.big = flag(getenv("STIN_NT_BIG"));
    return s;
}

struct NtProblem {
    int storage;               // 0 = fp32 rows, 1 = bf16 rows
    int64_t M;
    int Nc, K;
    int precision;             // fp32 rows: STIN_GEMM_* with its W_PRESPLIT / W_FRAG flags; bf16 rows: 0 or STIN_GEMM_W_BF16
    int parts;                 // STIN_NT_PART_*: the epilogue parts present (stin_hip.h)
    int align;                 // STIN_NT_ALIGN_*: the 16-byte facts of the operands (stin_hip.h)
    bool null_operand;         // a required pointer is NULL (the refusal keeps its place among the others)
    bool has(int part) const { return (parts & part) != 0; }
    bool aligned(int what) const { return (align & what) == what; }
};
struct NtRoute {
    int status;                // STIN_OK, or why this call cannot be served
    int family;                // STIN_NT_* (stin_hip.h); STIN_NT_NONE: no rows, nothing to launch
    int bm, bn;                // output tile of a block
    int param;                 // panel: 32-row tiles per block | strip: 21 / 22 / 41 | all-columns: waves along M | stream: column tiles per block
    int vec;                   // 16-byte operand loads
    int vec_out;               // 16-byte stores (all-columns, bf16 rows) / the strip kernel's restaged epilogue
    int64_t lds;               // dynamic LDS bytes
    int64_t grid;              // blocks along x
    int grid_y;                // blocks along y (the streaming kernel's column blocks; 1 elsewhere)
    int64_t groups;            // statistics groups of a fused epilogue, 0 without one
};

// blocks of a tiled grid: plain order below 16 row tiles, else whole rounds of 8 row tiles (one per XCD: nt_block_tile)
inline int64_t nt_grid(int64_t M, int Nc, int BM, int BN) {
    const int64_t nrow = (M + BM - 1) / BM, ncol = (Nc + BN - 1) / BN;
    return (nrow < 16 ? nrow : ((nrow + 7) / 8) * 8) * ncol;
}

// Balanced column-panel kernel (k_gemm_nt_panel): 32-row tiles per block (MT0 + MT1, 2 .. 9) so that (row blocks) x (128-column
// panels) fills the chip in ONE round, or 0 = this shape stays on the strip / all-columns kernels.  Measured (MI355X, round 4,
// strip / all-columns -> panel, bf16x3): 18 063 x 256 x 1024 43.4 -> 36.7-38.8 us, x 256 x 512 26.4 -> 23.3, x 512 x 256 31.3 -> 24.2,
// x 128 x 1280 35.1 -> 28.8; grids of two and more rounds (one 147 KB block per CU at a time: nothing overlaps a block's
// prologue and its 5 us store phase) are no faster than the strip kernel (18 063 x 1024 x 256 44.0 -> 42.9-46.7, 60 211 x 640 x 256
// 80.6 -> 93.1) and stay there.  forced (STIN_NT_PANEL) = 0 disables, = 1 takes it for every fragment-order shape whatever the
// number of rounds.
inline int panel_tiles(int64_t M, int Nc, int K, int forced, int cu) {
    if (forced == 0 || Nc % 128 != 0 || K % WD_KC != 0 || M <= 0) return 0;
    const int P = Nc / 128;
    const int64_t rg = (M + 31) / 32;
    const int max_rounds = forced == 1 ? 64 : 1;
    for (int rounds = 1; rounds <= max_rounds; ++rounds) {
        const int64_t slots = (int64_t)cu * rounds / P;
        if (slots < 1) continue;
        const int64_t mts = (rg + slots - 1) / slots;
        // (fewer row groups than slots - the coarse levels of a small crop, 1 806 x 256 x 1024: the finest blocks, 64 rows; the
        // all-columns kernel ran that shape on 15 workgroups, 41.8 us)
        if (mts <= 9) return mts < 2 ? 2 : (int)mts;
    }
    return 0;
}
// all-columns NT kernel: waves along the rows of a block (see k_gemm_nt_wide).  8 waves per block (128 rows) for Nc = 256
// while the 128-row blocks fit the chip in one round: 18 063 x 256 x 1024 41.6 -> 36.7 us, x 512 29.3 -> 27.7; slower for 60 k
// rows (471 blocks: 59 -> 64 us) and for Nc = 128 (256-row blocks: 71 of them at 18 k rows, 34 -> 52 us), which keep 4 waves.
inline int wide_waves_m(int64_t M, int Nc, int cu) { return (Nc == 256 && (M + 127) / 128 > (int64_t)cu) ? 1 : 2; }
// Resident-strip kernel (k_gemm_nt_strip).  Configuration 21 = (MT 2, one quad), 22 = two quads, 41 = MT 4; STIN_STRIP_CFG forces one.
inline void strip_route(const NtProblem& p, const NtSwitches& sw, int cu, NtRoute* r) {
    const int KC = p.K < 256 ? p.K : 256;                         // resident K chunk: 64 rows x 256 k x 4 B = 64 KB -> 2 blocks per CU
    const int P = (p.Nc + ST_PANEL - 1) / ST_PANEL, forced = sw.strip_cfg;
    // measured (profiles/r03_strip_cfg.md): two quads gain 2-5 % where a strip has many panels (18 063 x 1024 x 256: 46.6 -> 44.4 us,
    // x 1280 x 128 43.3 -> 42.1, 60 211 x 640 x 256 79.7 -> 77.8, 200 704 x 320 x 128 135.5 -> 133.2) and lose 3 % at Nc = 512
    // (30.2 -> 31.2); MT = 4 on one quad (one wave per SIMD) is 25-40 % slower everywhere and stays a tested tuning variant
    r->param = (forced == 21 || forced == 22 || forced == 41) ? forced : (p.Nc >= 640 ? 22 : 21);
    r->bm = r->param == 21 ? 64 : 128;
    r->bn = ST_PANEL;
    const int waves = r->param == 22 ? 8 : 4;
    r->lds = (int64_t)2 * (KC / 32) * r->bm * 64 + (int64_t)P * ST_PANEL * 4 + r->bm * 4;
    // the epilogue's restage area (2 KB per wave) only where it does not cost a resident block (K chunks of 256: 2 blocks
    // per CU either way; chunks of 128 would drop from 4 to 3 and lose more than the wide stores gain: 130 -> 155 us at
    // 200 704 x 320 x 128)
    const int64_t occ_plain = 160 * 1024 / r->lds, occ_rest = 160 * 1024 / (r->lds + waves * 2048);
    r->vec_out = ((occ_rest > 2 ? 2 : occ_rest) == (occ_plain > 2 ? 2 : occ_plain)) ? 1 : 0;     // (occupancy is capped at 2 below)
    if (r->vec_out) r->lds += waves * 2048;
    int occ = (int)(160 * 1024 / r->lds);
    // (round 4) at most two resident blocks per CU: with three or four (K chunks of 128: 32-44 KB of LDS per block) the blocks
    // of a CU re-stream the W panels against each other - 200 704 x 320 x 128: 136.6 us at four / three, 126.5 at two, 124 at one
    // two-quad block (profiles/probes/nt_probe.py, an occupancy sweep)
    if (occ > 2) occ = 2;
    if (r->param == 22) occ = 1;                                  // eight-wave blocks: one per CU (18 063 x 1280 x 128: 39.2 -> 35.6 us)
    if (occ < 1) occ = 1;
    const int64_t units = ((p.M + r->bm - 1) / r->bm) * P;
    r->grid = (int64_t)cu * occ < units ? (int64_t)cu * occ : units;
}
// The streaming kernel for a shape: NT (32-column tiles per block), LDS bytes, blocks (gx row walkers x ncb column blocks)
constexpr int64_t STREAM_MIN_ROWS = 65536;      // below this the tiling's many short blocks fill the chip better than 32-row wave tiles
inline bool stream_geo(const NtProblem& p, int precision, int mode, int nt, int cu, NtRoute* r) {
    const int K = p.K, Nc = p.Nc;
    if (p.M <= 0 || Nc <= 0 || Nc % 4 != 0 || K < 64 || K > 512 || K % 64 != 0) return false;
    // staged chunk: 64 columns (8 KB per wave in flight, 32 KB of staging per block: two blocks per CU up to K = 128 -
    // 1 200 642 x 64 x 128 with the BatchNorm transform: 184 us against 212 with 128-column chunks, profiles/probes/kc_probe.sh)
    constexpr int KC = 64;
    // (the statistics pass is faster with two column tiles although the A rows then come from L2 a second time: 207 against 232 us at
    // 1 200 642 x 128 x 64, 178 against 277 at 361 000 x 256 x 128)
    if (nt != 2 && nt != 4) nt = (Nc <= 64 || mode == 1) ? 2 : 4;
    const int64_t esz = precision == STIN_GEMM_BF16X6 ? 6 : 4;                   // bytes per operand element in LDS: 2 or 3 pieces of 16 bits
    auto lds_of = [&](int nt_) {
        return esz * ((int64_t)K * 32 * nt_ + 128 * KC) + (p.has(STIN_NT_PART_BN_TF) ? 8 * K : 0) + (mode != 0 ? 24 * 32 * nt_ : 0);
    };
    if (lds_of(nt) > 160 * 1024) nt = 2;
    if (lds_of(nt) > 160 * 1024) return false;
    r->param = nt, r->bm = 128, r->bn = 32 * nt, r->lds = lds_of(nt);
    if (r->lds < 4 * 2 * 32 * nt * (int64_t)sizeof(double)) r->lds = 4 * 2 * 32 * nt * (int64_t)sizeof(double);
    r->grid_y = (Nc + 32 * nt - 1) / (32 * nt);
    int bpc = (int)((160 * 1024) / r->lds);
    if (bpc > 2) bpc = 2;
    int64_t gx = (int64_t)cu * bpc / r->grid_y;
    if (gx < 1) gx = 1;
    const int64_t need = ((p.M + 31) / 32 + 3) / 4;                               // blocks that have a tile for every wave
    r->grid = need < gx ? need : gx;
    return true;
}
// does the streaming kernel serve this product?  `precision` without its flags; the bf16 / fp16 split precisions only, 16-byte rows
inline bool stream_serves(const NtProblem& p, int precision, int mode, const NtSwitches& sw, int cu, NtRoute* r) {
    const bool epi = p.has(STIN_NT_PART_BIAS | STIN_NT_PART_ROW_MASK | STIN_NT_PART_RESIDUAL) || (p.precision & STIN_GEMM_W_PRESPLIT);
    if (!(precision == STIN_GEMM_BF16X3 || precision == STIN_GEMM_F16X3 || (precision == STIN_GEMM_BF16X6 && !epi))) return false;
    if (!p.aligned(STIN_NT_ALIGN_IN | STIN_NT_ALIGN_OUT) || (p.has(STIN_NT_PART_BIAS) && !p.aligned(STIN_NT_ALIGN_BIAS))) return false;
    if (!stream_geo(p, precision, mode, sw.stream_nt, cu, r)) return false;
    r->family = STIN_NT_STREAM, r->vec = 1, r->groups = mode == 1 ? r->grid : 0;
    return true;
}
// the tiled kernels of fp32 rows.  Tile choice, from per-shape sweeps on MI355X (profiles/gemm_tiles.py) and whole-step A/B runs: the
// skinny GEMMs of the shipped 3-level network (K <= 256, or K >= 512 with only 256 output columns) are latency-bound, so the 64x64
// tile (4x the blocks in flight) wins there.  Long reductions with enough tiles (the 1024..4096-wide layers of a 5-level network:
// K >= 512, >= 500 tiles of 128x128) are 1.15-1.35x faster on 128x128.  Pre-split W: one data layout per network, no 128x32 tile.
inline void tiled_route(const NtProblem& p, bool wpre, int vec, NtRoute* r) {
    constexpr int64_t min_blocks = 500;
    r->family = STIN_NT_TILED, r->vec = vec, r->bm = r->bn = 64;
    if (!wpre && p.Nc <= 32) r->bm = 128, r->bn = 32;
    else if (p.Nc % 128 == 0 && p.K >= 512 && ((p.M + 127) / 128) * (p.Nc / 128) >= min_blocks) r->bm = r->bn = 128;
    r->grid = nt_grid(p.M, p.Nc, r->bm, r->bn);
}
// bf16 rows
inline void b16_route(const NtProblem& p, const NtSwitches& sw, NtRoute* r) {
    const int64_t M = p.M, Nc = p.Nc, K = p.K;
    const bool wb = (p.precision & STIN_GEMM_W_BF16) != 0;
    r->vec = (K % 8 == 0 && p.aligned(STIN_NT_ALIGN_IN)) ? 1 : 0;
    if (wb && !r->vec) { r->status = STIN_E_ALIGN; return; }
    r->vec_out = (!p.has(STIN_NT_PART_OUT_F32) && Nc % 8 == 0 && p.aligned(STIN_NT_ALIGN_OUT)) ? 1 : 0;
    // fat shapes with bf16 weights: the 128 x 128 LDS-DMA kernel (k_gemm_nt_b16_glds) replaces the register-staged tiles.  It needs
    // enough k-tiles to amortise its prologue and enough 128 x 128 tiles to fill the chip; the tall-skinny level-0 / level-1 shapes
    // (K <= 128, bound by their output bytes) stay on the small tiles.  Measured (profiles/r03_nt_bf16_fat.md): +10..25 % from
    // K = 1024 up (8 100 x 4096 x 1024: 124 -> 110 us, x 1024 x 4096: 104 -> 82), a loss at K <= 512 where four to eight k-tiles do
    // not amortise the two-buffer prologue and the output bytes dominate.  STIN_NT_GLDS = 0 | 1 forces (tuning aid / A-B).
    const bool pays = sw.glds >= 0 ? sw.glds != 0 : (K >= 1024 && Nc >= 256 && ((M + 127) / 128) * ((Nc + 127) / 128) >= 128);
    if (wb && K % BKB == 0 && pays) {
        // 256 x 256 tiles when they still fill the chip (>= 200 tiles).  STIN_NT_BIG = 0 | 1 forces.
        const bool big = sw.big >= 0 ? sw.big != 0 : (Nc >= 512 && ((M + 255) / 256) * ((Nc + 255) / 256) >= 200);
        r->family = STIN_NT_B16_GLDS, r->bm = r->bn = big ? 256 : 128;
        r->lds = big ? GlGeom<2, 4, 4, 2>::LDS : GlGeom<2, 2, 2, 2>::LDS;
        const int64_t nrow = (M + r->bm - 1) / r->bm, ncol = (Nc + r->bn - 1) / r->bn;
        r->grid = ncol % 8 == 0 ? nrow * ncol : nt_grid(M, Nc, r->bm, r->bn);
        return;
    }
    // 64x64 is the best tile for every shape of the shipped 3-level network; long reductions with enough tiles (the wide
    // layers of a 5-level network) are 1.1-1.5x faster on 128x64 (profiles/gemm_tiles.py)
    r->family = STIN_NT_B16_TILED, r->bm = r->bn = 64;
    if (Nc <= 32) r->bm = 128, r->bn = 32;
    else if (K >= 512 && ((M + 127) / 128) * ((Nc + 63) / 64) >= 1000) r->bm = 128;
    r->grid = nt_grid(M, Nc, r->bm, r->bn);
}

// THE decision.  Pure: no getenv, no HIP call, no statics.  Precedence for fp32 rows: the streaming kernel where it was asked for by
// name (stin_gemm_nt_stream_f32, the BatchNorm-backward pair); then, for fragment-order weights, panel, all-columns, strip; for
// pre-split weights streaming (very tall) or tiled; for plain weights streaming (tall) or tiled.
inline NtRoute nt_route(const NtProblem& p, const NtSwitches& sw, int cu) {
    NtRoute r = {};
    r.grid_y = 1;
    auto refuse = [&](int code) { r.status = code; r.family = STIN_NT_NONE; return r; };
    if (p.storage == 1) {
        if (p.M == 0) return r;
        if (p.null_operand) return refuse(STIN_E_NULL);
        b16_route(p, sw, &r);
        return r;
    }
    const bool colstats = p.has(STIN_NT_PART_COLSTATS), dotelu = p.has(STIN_NT_PART_DOTELU), tf = p.has(STIN_NT_PART_BN_TF);
    const bool residual = p.has(STIN_NT_PART_RESIDUAL);
    const int bn_bwd = p.has(STIN_NT_PART_BN_BWD_STATS) ? 1 : p.has(STIN_NT_PART_BN_BWD_APPLY) ? 2 : 0;
    if (bn_bwd != 0 || p.has(STIN_NT_PART_STREAM_ONLY)) {
        // K = 256 under the BatchNorm backward (Nc = 512, the 18 063-vertex level of SingleConvMeshNet): the weight slice leaves room
        // for two column tiles per block, so the A rows are re-read by 8 column blocks and the two passes (436 us) lose to the three
        // launches (377 us, profiles/probes/bnbwd_probe.py)
        if ((bn_bwd != 0 && p.K > 128) || !stream_serves(p, p.precision, bn_bwd, sw, cu, &r)) return refuse(STIN_E_UNSUPPORTED);
        return p.null_operand ? refuse(STIN_E_NULL) : r;
    }
    const bool wpre = (p.precision & STIN_GEMM_W_PRESPLIT) != 0;
    const bool wfrag = wpre && (p.precision & STIN_GEMM_W_FRAG) != 0 && stin_w_frag_shape(p.Nc, p.K);
    const int precision = p.precision & ~(STIN_GEMM_W_PRESPLIT | STIN_GEMM_W_FRAG);
    if (!(precision == STIN_GEMM_F32 || precision == STIN_GEMM_BF16X3 || precision == STIN_GEMM_BF16X6 || precision == STIN_GEMM_F16X3))
        return refuse(STIN_E_UNSUPPORTED);
    if (wpre && !(precision == STIN_GEMM_BF16X3 || precision == STIN_GEMM_F16X3)) return refuse(STIN_E_UNSUPPORTED);
    if (tf && (wpre || colstats || dotelu)) return refuse(STIN_E_UNSUPPORTED);             // (the tiled and streaming kernels only)
    if (p.M == 0) return r;
    if (p.null_operand) return refuse(STIN_E_NULL);
    const int vec = (p.K % 4 == 0 && p.aligned(STIN_NT_ALIGN_IN) && (!tf || p.aligned(STIN_NT_ALIGN_TF))) ? 1 : 0;
    // column statistics: a kernel whose blocks own whole rows (all-columns), or the panel kernel's two-stage epilogue
    if (colstats && !(wfrag && (p.Nc <= 256 || dotelu))) return refuse(STIN_E_UNSUPPORTED);
    if (dotelu && !sw.dotelu) return refuse(STIN_E_UNSUPPORTED);
    const bool out16 = p.aligned(STIN_NT_ALIGN_OUT);
    const int promised = wfrag ? panel_tiles(p.M, p.Nc, p.K, sw.panel, cu) : 0;          // what the shape alone gives: the *_groups answer
    const int pmts = (vec && out16 && !(colstats && residual && !dotelu)) ? promised : 0;
    if (dotelu && !(pmts > 0 && colstats)) return refuse(STIN_E_UNSUPPORTED);            // (the panel kernel's epilogue only)
    if (colstats && pmts == 0 && promised > 0) return refuse(STIN_E_ALIGN);              // the launch is not the one the group count was for
    if (pmts > 0) {
        r.family = STIN_NT_PANEL, r.param = pmts, r.vec = r.vec_out = 1, r.bm = 32 * pmts, r.bn = 128;
        const int64_t nrb = (p.M + r.bm - 1) / r.bm;
        r.grid = (nrb >= 16 ? ((nrb + 7) / 8) * 8 : nrb) * (p.Nc / 128);
        r.lds = (int64_t)r.bm * 512 > 8 * 4096 + r.bm * 4 ? (int64_t)r.bm * 512 : 8 * 4096 + r.bm * 4;
        if (colstats) r.groups = 2 * nrb;                         // two row groups (MT0 | MT1 tiles) per row block
    } else if (wfrag && p.Nc <= 256) {
        // Nc = 128 / 256: the fragment-order weight operand cannot be read by any other kernel
        if (!vec) return refuse(STIN_E_ALIGN);
        r.family = STIN_NT_WIDE, r.param = wide_waves_m(p.M, p.Nc, cu), r.vec = 1;
        // the LDS-restaged epilogue stores 16 bytes per lane: C (and the residual) rows must allow it
        r.vec_out = (out16 && !(colstats && residual)) ? 1 : 0;
        r.bm = 64 * r.param, r.bn = p.Nc, r.grid = (p.M + r.bm - 1) / r.bm;
        if (colstats) r.groups = (p.M + 63) / 64;                 // one statistics group per wave row group (64 rows)
    } else if (wfrag) {
        if (!(vec && out16)) return refuse(STIN_E_ALIGN);         // (as above: no other kernel reads this operand)
        r.family = STIN_NT_STRIP, r.vec = 1;
        strip_route(p, sw, cu, &r);
    } else if (wpre) {
        // pre-split W: the 16-byte vector path only (K % 4 == 0, aligned rows); (round 5) very tall products: the streaming-rows
        // kernel, bit-identical
        if (!vec) return refuse(STIN_E_ALIGN);
        if (!(p.M >= sw.stream_pre_rows && sw.stream && stream_serves(p, precision, 0, sw, cu, &r))) tiled_route(p, true, 1, &r);
    } else if (!(p.M >= STREAM_MIN_ROWS && sw.stream && stream_serves(p, p.precision, 0, sw, cu, &r))) {
        tiled_route(p, false, vec, &r);                           // (plain fp32 weights, K = 64 .. 512, tall: the streaming kernel)
    }
    return r;
}
