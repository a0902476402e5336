// GEMMs of bf16-STORAGE rows: NT tiled / LDS-DMA, TN register-transpose / hardware-transposed reads
// Part of stin_gemm.hip (included inside its anonymous namespace; not a translation unit of its own).
// =================================================================== bf16-STORAGE GEMMs
// Operands already live in HBM as bf16 rows (the *_bf16 pipeline): no split, ONE v_mfma_f32_32x32x16_bf16 per
// k-step, fp32 accumulation.  The weight operand W stays fp32 in memory (it is tiny) and is rounded to bf16 while
// it is staged.  LDS tiles are [rows][64 bf16] = 128-byte rows, the 16-byte chunk c of row r stored at chunk
// position c ^ ((r >> 1) & 7): conflict-free ds_write_b128 staging (8 lanes = one row) and ds_read_b128 fragments
// (the 16-lane read groups {0-3,12-15,20-27}, {4-11,16-19,28-31} hit 16 distinct 16-byte slots of the 256-byte
// bank span).  bf16 output tiles go through LDS so that the global stores are 16 bytes per lane, row-contiguous.
constexpr int BKB = 64;

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    b2 h = {(__bf16)lo, (__bf16)hi};
    return *reinterpret_cast<uint32_t*>(&h);
}
__device__ __forceinline__ uint4 f8_to_bf16x8(float4 a, float4 b) {
    return make_uint4(pack_bf16x2(a.x, a.y), pack_bf16x2(a.z, a.w), pack_bf16x2(b.x, b.y), pack_bf16x2(b.z, b.w));
}
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }

// Epilogue shared by the bf16-storage NT kernels: + bias * row_mask + residual in fp32, one rounding; bf16 tiles leave through
// LDS (smem: the operand tiles, free once every wave has passed the caller's last barrier) as 16-byte row-contiguous stores.
template <int BM, int BN, int WM, int WN, typename OUT, int THREADS = BLOCK>
__device__ __forceinline__ void nt_b16_epilogue(f32x16 (&acc)[BM / WM / 32][BN / WN / 32], unsigned char* smem, int64_t m0, int n0,
                                                const float* __restrict__ bias, const stin_bf16* __restrict__ row_mask,
                                                int64_t ld_mask, const stin_bf16* __restrict__ res, int64_t ld_res, int64_t M,
                                                int Nc, OUT* __restrict__ C, int64_t ldc, int vec_out) {
    constexpr int TM = BM / WM, TN = BN / WN, MT = TM / 32, NT = TN / 32;
    constexpr int CPITCH = BN + 32;                               // output staging pitch (bf16): rows r, r+1 on disjoint banks
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int kh = lane >> 5, li = lane & 31;
    // ---- epilogue: + bias * row_mask + residual in fp32, one rounding
    constexpr bool OUT_BF16 = sizeof(OUT) == 2;
    const bool staged = OUT_BF16 && vec_out;
    if (staged) __syncthreads();                                  // every wave is done with the operand tiles
    stin_bf16(*Cs)[CPITCH] = reinterpret_cast<stin_bf16(*)[CPITCH]>(smem);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int lcol = wn * TN + j * 32 + li;
        const int col = n0 + lcol;
        const bool col_ok = col < Nc;
        const float bv = (bias != nullptr && col_ok) ? bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lrow = wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const int64_t row = m0 + lrow;
                float t = acc[i][j][r];
                if (row < M && col_ok) {
                    if (bias != nullptr) t += row_mask != nullptr ? bv * (float)row_mask[row * ld_mask] : bv;
                    if (res != nullptr) t += (float)res[row * ld_res + col];
                }
                v[r] = t;
            }
            if (staged) {
                // lanes (li, li^1) trade one value per register pair so that each writes two adjacent columns of ONE row
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const bool odd = li & 1;
                    const float got = __shfl_xor(odd ? v[2 * q] : v[2 * q + 1], 1);
                    const int lrow = wm * TM + i * 32 + ((2 * q) & 3) + 8 * ((2 * q) >> 2) + 4 * kh + (odd ? 1 : 0);
                    const uint32_t pr = odd ? pack_bf16x2(got, v[2 * q + 1]) : pack_bf16x2(v[2 * q], got);
                    *reinterpret_cast<uint32_t*>(&Cs[lrow][lcol & ~1]) = pr;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                    if (row < M && col_ok) st1(C + row * ldc + col, v[r]);
                }
            }
        }
    }
    if (staged) {
        __syncthreads();
        constexpr int CHUNKS = BM * BN / 8;                       // 16-byte chunks of the output tile
#pragma unroll
        for (int s = 0; s < CHUNKS / THREADS; ++s) {
            const int c = tid + s * THREADS;
            const int lrow = c / (BN / 8), lc = (c % (BN / 8)) * 8;
            const int64_t row = m0 + lrow;
            const int col = n0 + lc;
            if (row < M && col < Nc)
                *reinterpret_cast<uint4*>(reinterpret_cast<stin_bf16*>(C) + row * ldc + col) =
                    *reinterpret_cast<const uint4*>(&Cs[lrow][lc]);
        }
    }
}

template <int BM, int BN, int WM, int WN, typename OUT, bool VEC, bool WB = false>   // WB: W already holds bf16 (ldw in bf16 elements)
__global__ __launch_bounds__(BLOCK) void k_gemm_nt_b16(const stin_bf16* __restrict__ A, int64_t lda,
                                                       const float* __restrict__ W, int64_t ldw,
                                                       const float* __restrict__ bias,
                                                       const stin_bf16* __restrict__ row_mask, int64_t ld_mask,
                                                       const stin_bf16* __restrict__ res, int64_t ld_res, int64_t M,
                                                       int Nc, int K, OUT* __restrict__ C, int64_t ldc, int vec_out) {
    constexpr int TM = BM / WM, TN = BN / WN, MT = TM / 32, NT = TN / 32;
    constexpr int A_CH = BM * 8 / BLOCK, W_CH = BN * 8 / BLOCK;   // 16-byte (8 x bf16) chunks per thread per tile
    static_assert(A_CH >= 1 && W_CH >= 1, "tile too small for 256 threads");
    constexpr int CPITCH = BN + 32;                               // output staging pitch (bf16): rows r, r+1 on disjoint banks
    constexpr int TILE_BYTES = (BM + BN) * BKB * 2, OUT_BYTES = BM * CPITCH * 2;
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_BYTES > OUT_BYTES ? TILE_BYTES : OUT_BYTES];
    stin_bf16(*As)[BKB] = reinterpret_cast<stin_bf16(*)[BKB]>(smem);
    stin_bf16(*Ws)[BKB] = reinterpret_cast<stin_bf16(*)[BKB]>(smem + BM * BKB * 2);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int64_t m0;
    int n0;
    if (!nt_block_tile(M, Nc, BM, BN, m0, n0)) return;                 // block-uniform
    const int ch = tid & 7, r0 = tid >> 3;                       // staging: chunk along k, first row (32 rows per pass)
    auto swz = [](int row, int chunk) { return (chunk ^ ((row >> 1) & 7)) << 3; };   // bf16 offset of a 16-byte chunk

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    uint4 ra[A_CH], rw[W_CH];
    auto load_tiles = [&](int k0) {
        const int k = k0 + ch * 8;
#pragma unroll
        for (int s = 0; s < A_CH; ++s) {
            const int64_t row = m0 + r0 + s * 32;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row < M) {
                const stin_bf16* p = A + row * lda + k;
                if (VEC) {
                    if (k < K) v = *reinterpret_cast<const uint4*>(p);
                } else {
                    uint32_t h[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) h[e] = (k + e < K) ? (uint32_t)*reinterpret_cast<const uint16_t*>(p + e) : 0u;
                    v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
                }
            }
            ra[s] = v;
        }
#pragma unroll
        for (int s = 0; s < W_CH; ++s) {
            const int row = n0 + r0 + s * 32;
            if constexpr (WB) {                                   // pre-converted weights: 16 bytes = 8 k-values, no conversion
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (row < Nc && k < K) v = *reinterpret_cast<const uint4*>(reinterpret_cast<const stin_bf16*>(W) + (int64_t)row * ldw + k);
                rw[s] = v;
                continue;
            }
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (row < Nc) {
                const float* p = W + (int64_t)row * ldw + k;
                if (VEC) {
                    if (k < K) {
                        a = ld4(p);
                        b = ld4(p + 4);
                    }
                } else {
                    if (k + 0 < K) a.x = p[0];
                    if (k + 1 < K) a.y = p[1];
                    if (k + 2 < K) a.z = p[2];
                    if (k + 3 < K) a.w = p[3];
                    if (k + 4 < K) b.x = p[4];
                    if (k + 5 < K) b.y = p[5];
                    if (k + 6 < K) b.z = p[6];
                    if (k + 7 < K) b.w = p[7];
                }
            }
            rw[s] = f8_to_bf16x8(a, b);
        }
    };
    auto store_tiles = [&]() {
#pragma unroll
        for (int s = 0; s < A_CH; ++s) {
            const int row = r0 + s * 32;
            *reinterpret_cast<uint4*>(&As[row][swz(row, ch)]) = ra[s];
        }
#pragma unroll
        for (int s = 0; s < W_CH; ++s) {
            const int row = r0 + s * 32;
            *reinterpret_cast<uint4*>(&Ws[row][swz(row, ch)]) = rw[s];
        }
    };

    const int kh = lane >> 5, li = lane & 31;
    load_tiles(0);
    for (int k0 = 0; k0 < K; k0 += BKB) {
        __syncthreads();
        store_tiles();
        __syncthreads();
        if (k0 + BKB < K) load_tiles(k0 + BKB);
#pragma unroll
        for (int ks = 0; ks < BKB / 16; ++ks) {
            bf16x8 a[MT], b[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int row = wm * TM + i * 32 + li;
                a[i] = *reinterpret_cast<const bf16x8*>(&As[row][swz(row, 2 * ks + kh)]);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int row = wn * TN + j * 32 + li;
                b[j] = *reinterpret_cast<const bf16x8*>(&Ws[row][swz(row, 2 * ks + kh)]);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }

    nt_b16_epilogue<BM, BN, WM, WN, OUT>(acc, smem, m0, n0, bias, row_mask, ld_mask, res, ld_res, M, Nc, C, ldc, vec_out);
}

// Fat shapes of the deep hierarchies (BASELINE config 5: 8 100 rows x 1024..4096 channels, 27 k x 512..2048): both operands
// bf16, K a multiple of 64, where the register-staged 64 x 64 / 128 x 64 tiles above ran at 0.11-0.18 of the MFMA peak (one
// LDS buffer: load -> wait -> write -> barrier per k-tile).  128 x 128 tile, 4 waves of 64 x 64, the two operand tiles of a
// k-step (2 x 16 KB) staged by LDS-DMA (global_load_lds_dwordx4: 1 KB per wave-instruction = 8 rows x 128 B, no VGPRs, no
// ds_write) into one of TWO buffers while the MFMAs of the previous k-tile run; one barrier per k-tile.  An LDS-DMA writes
// wave-linear (base + lane * 16), so the bank swizzle of the image - the 16-byte chunk c of row r sits at position
// c ^ ((r >> 1) & 7), the image k_gemm_nt_b16 reads conflict-free - is applied to the per-lane SOURCE address.  Rows past M
// / Nc are clamped to the last valid row (their products are never stored).  Same MFMA sequence per output element as
// k_gemm_nt_b16 (k ascending in steps of 16): bit-identical results.
// Block -> tile: with a multiple of 8 column tiles every XCD owns Nc / 8 columns (its W panel, 1 MB at K = 1024 and Nc = 4096,
// stays in that XCD's L2 while the A row tiles stream through, each read by the XCD's consecutive blocks); otherwise the
// row-tile-per-XCD order of nt_block_tile.
// Tile = (WM MT 32) x (WN NT 32): 128 x 128 on 2 x 2 waves of 64 x 64 (static 64 KB, two blocks per CU) or 256 x 256 on 2 x 4 waves
// of 128 x 64 (one block per CU; halves the operand re-reads through L2 and reads 6 KB of LDS per 8 MFMAs instead of 4 per 4).
template <int WM, int WN, int MT, int NT>
struct GlGeom {
    static constexpr int BM = WM * MT * 32, BN = WN * NT * 32, THREADS = 64 * WM * WN;
    static constexpr int BUF = (BM + BN) * BKB * 2;               // one k-tile of both operands
    static constexpr int OUT_BYTES = BM * (BN + 32) * 2;          // the epilogue's bf16 staging image
    static constexpr int LDS = 2 * BUF > OUT_BYTES ? 2 * BUF : OUT_BYTES;
    static constexpr int RPP = THREADS / 8;                       // rows per staging pass (8 lanes = one 128-byte row)
    static constexpr int NSA = BM / RPP, NSW = BN / RPP;
};

template <typename OUT, int WM, int WN, int MT, int NT>
__global__ __launch_bounds__(64 * WM * WN, 2) void k_gemm_nt_b16_glds(const stin_bf16* __restrict__ A, int64_t lda,
                                                                   const stin_bf16* __restrict__ W, int64_t ldw,
                                                                   const float* __restrict__ bias,
                                                                   const stin_bf16* __restrict__ row_mask, int64_t ld_mask,
                                                                   const stin_bf16* __restrict__ res, int64_t ld_res, int64_t M,
                                                                   int Nc, int K, OUT* __restrict__ C, int64_t ldc, int vec_out) {
    typedef GlGeom<WM, WN, MT, NT> Geo;
    constexpr int BM = Geo::BM, BN = Geo::BN, TM = MT * 32, TN = NT * 32, BUF = Geo::BUF;
    extern __shared__ __attribute__((aligned(1024))) unsigned char gl_smem[];
    unsigned char* smem = gl_smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int64_t m0;
    int n0;
    const int ncol = (Nc + BN - 1) / BN;
    if (ncol % 8 == 0) {
        const int cpx = ncol / 8;
        const int64_t j = blockIdx.x >> 3;
        m0 = (j / cpx) * BM;
        n0 = (int)((blockIdx.x & 7) * cpx + j % cpx) * BN;
    } else if (!nt_block_tile(M, Nc, BM, BN, m0, n0)) {
        return;                                                   // block-uniform
    }
    // staging: lane -> LDS position (row tid >> 3 of a pass of RPP rows, 16-byte slot tid & 7), source chunk = slot ^ swizzle(row)
    const int slot = tid & 7, r0 = tid >> 3;
    const stin_bf16* asrc[Geo::NSA];
    const stin_bf16* wsrc[Geo::NSW];
#pragma unroll
    for (int s = 0; s < Geo::NSA; ++s) {
        const int row = r0 + Geo::RPP * s;
        const int64_t ar = m0 + row < M ? m0 + row : M - 1;
        asrc[s] = A + ar * lda + (slot ^ ((row >> 1) & 7)) * 8;
    }
#pragma unroll
    for (int s = 0; s < Geo::NSW; ++s) {
        const int row = r0 + Geo::RPP * s;
        const int wr = n0 + row < Nc ? n0 + row : Nc - 1;
        wsrc[s] = W + (int64_t)wr * ldw + (slot ^ ((row >> 1) & 7)) * 8;
    }
    auto stage = [&](int buf, int k0) {
        unsigned char* base = smem + buf * BUF + wave * 1024;     // this wave's 8 rows of every pass
#pragma unroll
        for (int s = 0; s < Geo::NSA; ++s)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[s] + k0),
                                             (__attribute__((address_space(3))) void*)(base + s * (Geo::RPP * 128)), 16, 0, 0);
#pragma unroll
        for (int s = 0; s < Geo::NSW; ++s)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[s] + k0),
                                             (__attribute__((address_space(3))) void*)(base + BM * 128 + s * (Geo::RPP * 128)), 16, 0, 0);
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int kh = lane >> 5, li = lane & 31;
    // fragment byte offsets inside a tile: row * 128 + ((2 ks + kh) ^ ((row >> 1) & 7)) * 16
    int aoff[MT], boff[NT], asw[MT], bsw[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int row = wm * TM + i * 32 + li;
        aoff[i] = row * 128;
        asw[i] = (row >> 1) & 7;
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int row = wn * TN + j * 32 + li;
        boff[j] = BM * 128 + row * 128;
        bsw[j] = (row >> 1) & 7;
    }
    const int nt = K / BKB;
    stage(0, 0);
    __syncthreads();                                              // (hipcc drains the LDS-DMAs before the barrier)
    for (int t = 0; t < nt; ++t) {
        const unsigned char* tile = smem + (t & 1) * BUF;
        if (t + 1 < nt) stage((t + 1) & 1, (t + 1) * BKB);        // the buffer every wave finished reading before the last barrier
#pragma unroll
        for (int ks = 0; ks < BKB / 16; ++ks) {
            bf16x8 a[MT], b[NT];
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = *reinterpret_cast<const bf16x8*>(tile + aoff[i] + (((2 * ks + kh) ^ asw[i]) << 4));
#pragma unroll
            for (int j = 0; j < NT; ++j) b[j] = *reinterpret_cast<const bf16x8*>(tile + boff[j] + (((2 * ks + kh) ^ bsw[j]) << 4));
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();                                          // next tile landed (vmcnt(0) of the DMAs) and this one is free
    }
    nt_b16_epilogue<BM, BN, WM, WN, OUT, Geo::THREADS>(acc, smem, m0, n0, bias, row_mask, ld_mask, res, ld_res, M, Nc, C, ldc, vec_out);
}

// dW[Nc, K(+1)] = G^T [X | w] with G, X (and the optional row weight w) stored as bf16; fp32 slabs as k_gemm_tn.
// The reduction index is the ROW m: each staging thread loads a 4(rows) x 8(cols) bf16 patch (4 x 16-byte loads),
// transposes it in registers (v_perm byte selects) and writes one 8-byte run (4 consecutive m) per column into
// Gt[col][m] / Xt[col][m] (row pitch 144 B: conflict-free ds_write_b64 across 16 row groups and ds_read_b128).
constexpr int TNK_R = 64;                  // rows (m) per LDS slab = four MFMA k-steps
constexpr int TNK_PITCH = TNK_R + 8;

template <int TI, int TJ, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_gemm_tn_b16(const stin_bf16* __restrict__ G, int64_t ldg,
                                                       const stin_bf16* __restrict__ X, int64_t ldx, int64_t M, int Nc,
                                                       int K, int Kq, int has_bias, const stin_bf16* __restrict__ row_w, int64_t ld_w,
                                                       int rows_per_chunk, int tiles_i, int tiles_j, int64_t chunks,
                                                       float* __restrict__ slab) {
    constexpr int MT = TI / 64, NT = TJ / 64;
    constexpr int ITEMS = 2 * (TI + TJ);                           // 4x8 patches per 64-row slab (G then X): 16 row groups x T/8
    constexpr int NPASS = (ITEMS + BLOCK - 1) / BLOCK;
    __shared__ __attribute__((aligned(16))) stin_bf16 Gt[TI][TNK_PITCH];
    __shared__ __attribute__((aligned(16))) stin_bf16 Xt[TJ][TNK_PITCH];
    __shared__ float bsum[16][TI + 4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int tiles = tiles_i * tiles_j;
    int64_t chunk;
    int tile;
    if (!tn_block_map(blockIdx.x, chunks, tiles, chunk, tile)) return;   // block-uniform
    const int tj = tile % tiles_j, ti = tile / tiles_j;
    const int i0 = ti * TI, j0 = tj * TJ;
    const int64_t mb = chunk * rows_per_chunk;
    const int64_t me = (mb + rows_per_chunk < M) ? mb + rows_per_chunk : M;
    const bool want_bias = has_bias && (tj == 0);

    f32x16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
    float bs[8];                                                    // bias-gradient partial: the 8 columns of this thread's G patches
#pragma unroll
    for (int e = 0; e < 8; ++e) bs[e] = 0.f;

    uint4 patch[NPASS][4];
    uint16_t pw[NPASS][4];
    bool pv[NPASS][4];
    auto load_slab = [&](int64_t m0) {
#pragma unroll
        for (int s = 0; s < NPASS; ++s) {
            const int item = tid + s * BLOCK;
            const bool isG = item < 2 * TI;
            const int it = isG ? item : item - 2 * TI;
            const int rg = it % 16, c8 = it / 16;
            const bool live = item < ITEMS;
            const stin_bf16* base = isG ? G : X;
            const int64_t ld = isG ? ldg : ldx;
            const int col = (isG ? i0 : j0) + c8 * 8;
            const int lim = isG ? Nc : K;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + rg * 4 + r;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (live && row < me) {
                    const stin_bf16* p = base + row * ld + col;
                    if (VEC) {
                        if (col < lim) v = *reinterpret_cast<const uint4*>(p);
                    } else {
                        uint32_t h[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) h[e] = (col + e < lim) ? (uint32_t)*reinterpret_cast<const uint16_t*>(p + e) : 0u;
                        v = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
                    }
                }
                patch[s][r] = v;
                const int64_t rc = row < me ? row : me - 1;        // plain load, masked in store_slab (see k_gemm_tn_bf16s)
                const stin_bf16* wp = (want_bias && row_w != nullptr) ? row_w + rc * ld_w : G;   // always a valid address
                pw[s][r] = *reinterpret_cast<const uint16_t*>(wp);   // raw bits: widened in store_slab, no use of the value here
                pv[s][r] = isG && live && row < me;
            }
        }
    };
    auto store_slab = [&]() {
#pragma unroll
        for (int s = 0; s < NPASS; ++s) {
            const int item = tid + s * BLOCK;
            if (item >= ITEMS) continue;
            const bool isG = item < 2 * TI;
            const int it = isG ? item : item - 2 * TI;
            const int rg = it % 16, c8 = it / 16;
            if (isG && want_bias) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint4 v = patch[s][r];
                    const float w = pv[s][r] ? (row_w != nullptr ? bf16_lo(pw[s][r]) : 1.f) : 0.f;
                    bs[0] += w * bf16_lo(v.x); bs[1] += w * bf16_hi(v.x);
                    bs[2] += w * bf16_lo(v.y); bs[3] += w * bf16_hi(v.y);
                    bs[4] += w * bf16_lo(v.z); bs[5] += w * bf16_hi(v.z);
                    bs[6] += w * bf16_lo(v.w); bs[7] += w * bf16_hi(v.w);
                }
            }
            stin_bf16* dst = isG ? &Gt[c8 * 8][rg * 4] : &Xt[c8 * 8][rg * 4];
            const uint32_t w[4][4] = {{patch[s][0].x, patch[s][0].y, patch[s][0].z, patch[s][0].w},
                                      {patch[s][1].x, patch[s][1].y, patch[s][1].z, patch[s][1].w},
                                      {patch[s][2].x, patch[s][2].y, patch[s][2].z, patch[s][2].w},
                                      {patch[s][3].x, patch[s][3].y, patch[s][3].z, patch[s][3].w}};
#pragma unroll
            for (int d = 0; d < 4; ++d) {                          // dword d of a row = columns 2d, 2d+1
                // column 2d: low halves of rows 0..3; column 2d+1: high halves
                const uint32_t lo01 = __builtin_amdgcn_perm(w[1][d], w[0][d], 0x05040100u);
                const uint32_t lo23 = __builtin_amdgcn_perm(w[3][d], w[2][d], 0x05040100u);
                const uint32_t hi01 = __builtin_amdgcn_perm(w[1][d], w[0][d], 0x07060302u);
                const uint32_t hi23 = __builtin_amdgcn_perm(w[3][d], w[2][d], 0x07060302u);
                *reinterpret_cast<uint2*>(dst + (2 * d) * TNK_PITCH) = make_uint2(lo01, lo23);
                *reinterpret_cast<uint2*>(dst + (2 * d + 1) * TNK_PITCH) = make_uint2(hi01, hi23);
            }
        }
    };

    const int kh = lane >> 5, li = lane & 31;
    load_slab(mb);
    for (int64_t m0 = mb; m0 < me; m0 += TNK_R) {
        __syncthreads();                                           // previous slab's fragment reads are done
        store_slab();
        __syncthreads();
        if (m0 + TNK_R < me) load_slab(m0 + TNK_R);                // next slab's global loads in flight during the MFMAs
#pragma unroll
        for (int ks = 0; ks < TNK_R; ks += 16) {
            bf16x8 a[MT], c[NT];
#pragma unroll
            for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const bf16x8*>(&Gt[wi * (TI / 2) + t * 32 + li][ks + 8 * kh]);
#pragma unroll
            for (int t = 0; t < NT; ++t) c[t] = *reinterpret_cast<const bf16x8*>(&Xt[wj * (TJ / 2) + t * 32 + li][ks + 8 * kh]);
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[t], c[u], acc[t][u], 0, 0, 0);
        }
    }

    float* out = slab + chunk * tn_chunk_stride(Nc, Kq);
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int col = j0 + wj * (TJ / 2) + u * 32 + li;
        if (col >= K) continue;
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wi * (TI / 2) + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (row < Nc) out[(int64_t)row * Kq + col] = acc[t][u][r];
            }
    }
    if (want_bias) {                                              // block-uniform
        // G patches are items [0, 2*TI): item = tid (2*TI <= 256), row group tid % 16, column group tid / 16
        if (tid < 2 * TI) {
#pragma unroll
            for (int e = 0; e < 8; ++e) bsum[tid % 16][(tid / 16) * 8 + e] = bs[e];
        }
        __syncthreads();
        if (tid < TI) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) t += bsum[r][tid];
            if (i0 + tid < Nc) out[(int64_t)Nc * Kq + i0 + tid] = t;
        }
    }
}

// ------------------------------------------------------------ TN, bf16 storage, hardware-transposed LDS reads (round 3)
// dW tile [128 x 128] += G[m, i]^T X[m, j] over a chunk of rows m.  The reduction index is the ROW of both operands, so the
// MFMA fragments (8 consecutive k per lane) run DOWN the columns of the row-major tiles.  k_gemm_tn_b16 transposes 4 x 8
// patches in registers (v_perm) and scatters 8-byte runs into a k-major LDS image; gfx950 reads the transpose for free:
// the tiles are staged as they lie in memory ([64 rows][128 cols] bf16 = 256-byte rows, one ds_write_b128 per 16-byte chunk,
// no shuffles) and ds_read_b64_tr_b16 hands each lane of a 16-lane group one COLUMN of a 4-row x 16-column block - two of
// them are the 32x32x16 operand of the transposed tile.  Image: chunk ch of row r at position ch ^ (((r & 3) << 2) |
// ((r >> 2) & 3)) (conflict-free for the row writes and for the transposed reads; addressing checked on the device by
// profiles/micro/tr_read_check.hip).  Two LDS buffers, ONE barrier per 64-row slab: the next slab's global loads are issued
// before the MFMAs of the current one and written to the other buffer after them.  Same products in the same k order
// as k_gemm_tn_b16 (bit-identical slabs); the bias column (sum_m w[m] G[m, i]) is accumulated from the A fragments in fp32
// (other association than the staged form: equal to rounding).  128 x 128 tiles, 16-byte rows (Nc, K, ldg, ldx % 8 == 0).
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* lo, const unsigned char* hi) {
    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)lo);
    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)hi);
    const s16x8 v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}
// Tile = (WI MT 32) x (WJ NT 32) on WI x WJ waves: 128 x 128 on 2 x 2 waves of 64 x 64 (two blocks per CU), or 256 x 256 on
// 2 x 4 waves of 128 x 64 (one block per CU).  The big tile is what the fat shapes need: with 128 x 128 tiles every operand
// element is re-read Nc / 128 (K / 128) times - 1.06 GB through the L2 -> CU paths for the 8 100 x 4096 x 1024 product, more
// time than its MFMAs - the 256 x 256 tile halves that and reads 6 KB of LDS per 8 MFMAs instead of 4 KB per 4.
template <int WI, int WJ, int MT, int NT>
struct TrGeom {
    static constexpr int TI = WI * MT * 32, TJ = WJ * NT * 32, THREADS = 64 * WI * WJ;
    static constexpr int ROWB_G = TI * 2, ROWB_X = TJ * 2;                      // bytes of a tile row
    static constexpr int TILE_G = 64 * ROWB_G, TILE_X = 64 * ROWB_X, BUF = TILE_G + TILE_X;
    static constexpr int LDS = 2 * BUF + 2 * 64 * 4;                            // two buffers + two slabs of row weights
    static_assert(TI == TJ, "the staging map assumes square tiles");
    static_assert((64 * (TI / 8)) % THREADS == 0, "whole staging passes");
};
template <int ROWB>
__device__ __forceinline__ int tr_offw(int row, int ch) { return ROWB * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))); }

template <int WI, int WJ, int MT, int NT>
__global__ __launch_bounds__(64 * WI * WJ) void k_gemm_tn_b16_tr(const stin_bf16* __restrict__ G, int64_t ldg,
                                                                 const stin_bf16* __restrict__ X, int64_t ldx, int64_t M, int Nc,
                                                                 int K, int Kq, int has_bias, const stin_bf16* __restrict__ row_w,
                                                                 int64_t ld_w, int rows_per_chunk, int tiles_i, int tiles_j,
                                                                 int64_t chunks, float* __restrict__ slab) {
    typedef TrGeom<WI, WJ, MT, NT> Geo;
    constexpr int TI = Geo::TI, TJ = Geo::TJ, THREADS = Geo::THREADS, CI = TI / 8;
    constexpr int NS = 64 * CI / THREADS;                                      // staging passes (16 rows each)
    constexpr int RPP = THREADS / CI;                                          // rows per pass
    extern __shared__ __attribute__((aligned(16))) unsigned char tr_smem[];
    float* wrow = reinterpret_cast<float*>(tr_smem + 2 * Geo::BUF);            // [2][64]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wi = wave / WJ, wj = wave % WJ;
    const int tiles = tiles_i * tiles_j;
    int64_t chunk;
    int tile;
    if (!tn_block_map(blockIdx.x, chunks, tiles, chunk, tile)) return;   // block-uniform
    const int tj = tile % tiles_j, ti = tile / tiles_j;
    const int i0 = ti * TI, j0 = tj * TJ;
    const int64_t mb = chunk * rows_per_chunk;
    const int64_t me = (mb + rows_per_chunk < M) ? mb + rows_per_chunk : M;
    const bool want_bias = has_bias && (tj == 0);

    f32x16 acc[MT][NT];
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int c = 0; c < NT; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
    float bias[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) bias[t] = 0.f;

    // staging: chunk idx = tid + THREADS s of the 64 x CI chunk grid of a tile -> row idx / CI, chunk idx % CI (whole rows per wave)
    const int sch = tid % CI, srow = tid / CI;                                 // rows srow + RPP s
    const bool g_ok = i0 + sch * 8 < Nc, x_ok = j0 + sch * 8 < K;
    const stin_bf16* gsrc = G + i0 + (g_ok ? sch * 8 : 0);
    const stin_bf16* xsrc = X + j0 + (x_ok ? sch * 8 : 0);
    int soff[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) soff[s] = tr_offw<Geo::ROWB_G>(srow + RPP * s, sch);
    uint4 rg[NS], rx[NS];
    float rw = 0.f;
    auto load_slab = [&](int64_t m0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int64_t row = m0 + srow + RPP * s;
            const int64_t rc = row < me ? row : me - 1;                         // clamped address, masked value
            const uint4 vg = *reinterpret_cast<const uint4*>(gsrc + rc * ldg);
            const uint4 vx = *reinterpret_cast<const uint4*>(xsrc + rc * ldx);
            const bool live = row < me;
            rg[s] = (live && g_ok) ? vg : make_uint4(0u, 0u, 0u, 0u);
            rx[s] = (live && x_ok) ? vx : make_uint4(0u, 0u, 0u, 0u);
        }
        if (want_bias && tid < 64) {
            const int64_t row = m0 + tid;
            rw = row < me ? (row_w != nullptr ? (float)row_w[row * ld_w] : 1.f) : 0.f;
        }
    };
    auto store_slab = [&](int buf) {
        unsigned char* base = tr_smem + buf * Geo::BUF;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            *reinterpret_cast<uint4*>(base + soff[s]) = rg[s];
            *reinterpret_cast<uint4*>(base + Geo::TILE_G + soff[s]) = rx[s];
        }
        if (want_bias && tid < 64) wrow[buf * 64 + tid] = rw;
    };

    // transposed-read addresses of this lane for k-step 0 (a k-step further down = + 16 rows)
    const int g16 = lane >> 4, tl = lane & 15, tq = tl >> 2, tp = tl & 3;
    int aoff[MT][2], boff[NT][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = 8 * (g16 >> 1) + 4 * h + tq;
#pragma unroll
        for (int t = 0; t < MT; ++t)
            aoff[t][h] = tr_offw<Geo::ROWB_G>(row, (wi * (MT * 32) + t * 32 + 16 * (g16 & 1)) / 8 + (tp >> 1)) + 8 * (tp & 1);
#pragma unroll
        for (int u = 0; u < NT; ++u)
            boff[u][h] = Geo::TILE_G + tr_offw<Geo::ROWB_X>(row, (wj * (NT * 32) + u * 32 + 16 * (g16 & 1)) / 8 + (tp >> 1)) + 8 * (tp & 1);
    }
    const int kh = lane >> 5, li = lane & 31;

    load_slab(mb);
    store_slab(0);
    __syncthreads();
    int buf = 0;
    for (int64_t m0 = mb; m0 < me; m0 += TNK_R) {
        const bool more = m0 + TNK_R < me;
        if (more) load_slab(m0 + TNK_R);                                       // in flight during the MFMAs below
        const unsigned char* base = tr_smem + buf * Geo::BUF;
#pragma unroll
        for (int ks = 0; ks < TNK_R / 16; ++ks) {
            bf16x8 a[MT], c[NT];
#pragma unroll
            for (int t = 0; t < MT; ++t)
                a[t] = tr_frag(base + ks * 16 * Geo::ROWB_G + aoff[t][0], base + ks * 16 * Geo::ROWB_G + aoff[t][1]);
#pragma unroll
            for (int u = 0; u < NT; ++u)
                c[u] = tr_frag(base + ks * 16 * Geo::ROWB_X + boff[u][0], base + ks * 16 * Geo::ROWB_X + boff[u][1]);
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[t], c[u], acc[t][u], 0, 0, 0);
            if (want_bias && wj == 0) {                                        // wave-uniform
                const float* w = wrow + buf * 64 + ks * 16 + 8 * kh;
#pragma unroll
                for (int t = 0; t < MT; ++t)
#pragma unroll
                    for (int e = 0; e < 8; ++e) bias[t] += w[e] * (float)a[t][e];
            }
        }
        if (more) store_slab(buf ^ 1);                                         // the buffer nobody reads in this iteration
        __syncthreads();
        buf ^= 1;
    }

    float* out = slab + chunk * tn_chunk_stride(Nc, Kq);
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int col = j0 + wj * (NT * 32) + u * 32 + li;
        if (col >= K) continue;
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wi * (MT * 32) + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (row < Nc) out[(int64_t)row * Kq + col] = acc[t][u][r];
            }
    }
    if (want_bias && wj == 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const float tot = bias[t] + __shfl_xor(bias[t], 32);               // the two k-halves of the wave
            const int row = i0 + wi * (MT * 32) + t * 32 + li;
            if (kh == 0 && row < Nc) out[(int64_t)Nc * Kq + row] = tot;
        }
    }
}

