// TN products with K <= 16 (k_gemm_tn_skinny), the slab reduction and the host-side tile / chunk rules
// Part of stin_gemm.hip (included inside its anonymous namespace; not a translation unit of its own).
// ----------------------------------------------------------------------------- TN, skinny K (round 4)
// dW[Nc, K] = G^T [X | w] with K <= 16 (the first block of the network: [dA | dB | g] against the 12 padded input channels,
// 200 704 x 320 x 12).  On the MFMA kernels above this shape stages 128 x 64 tiles that are four fifths empty and streams G at
// 2.5 TB/s (102 us for 267 MB).  It is pure streaming with 13 multiply-adds per G element, so: no matrix cores, no LDS staging -
// a block owns ALL Nc columns of a chunk of rows; thread (row lane, column lane) holds 4 columns x (KP + 1) fp32 accumulators,
// loads one 16-byte piece of a G row and the row's K values of X (the same addresses for every column lane of the row lane: L1
// hits) per trip, UR rows in flight; rows ascending per thread, then the row lanes in order through LDS - fixed order, exact fp32
// products (precision >= every split mode).  Partial results go to the usual slab layout ([Nc][Kq] + bias [Nc] per chunk), so
// k_reduce_slabs / k_wgrad_finalize fold them unchanged.
template <int KP>
__global__ __launch_bounds__(BLOCK) void k_gemm_tn_skinny(const float* __restrict__ G, int64_t ldg, const float* __restrict__ X, int64_t ldx,
                                                         int64_t M, int Nc, int K, int Kq, int has_bias,
                                                         const float* __restrict__ row_weight, int64_t ld_weight, int rows_per_chunk,
                                                         float* __restrict__ slab) {
    constexpr int UR = 8;
    const int CL = Nc / 4, RL = BLOCK / CL;                                   // column lanes per row, row lanes (BLOCK - CL RL threads idle)
    const int cl = threadIdx.x % CL, rl = threadIdx.x / CL;
    const bool live = rl < RL;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < M ? r0 + rows_per_chunk : M;
    const int nrows = (int)(r1 - r0);
    // the chunk's [X | w] rows once into LDS ((KP + 4) floats per row: K values, the row weight, padding to 16 bytes): the inner
    // loop then issues ONE global load per row (the G piece) and reads its X row as LDS broadcasts
    extern __shared__ __attribute__((aligned(16))) float sk_smem[];           // [rows_per_chunk][KP + 4], later [Nc][KP + 1]
    constexpr int XP = KP + 4;
    for (int i = threadIdx.x; i < nrows * (KP / 4); i += BLOCK) {
        const int r = i / (KP / 4), q = i % (KP / 4);
        *reinterpret_cast<float4*>(sk_smem + r * XP + q * 4) = ld4(X + (r0 + r) * ldx + q * 4);
    }
    for (int r = threadIdx.x; r < nrows; r += BLOCK) sk_smem[r * XP + KP] = row_weight != nullptr ? row_weight[(r0 + r) * ld_weight] : 1.f;
    __syncthreads();
    float acc[4][KP + 1];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k <= KP; ++k) acc[c][k] = 0.f;
    if (live) {
        const float* Gp = G + r0 * ldg + cl * 4;
        for (int rb = rl; rb < nrows; rb += UR * RL) {
            float4 g[UR];
#pragma unroll
            for (int u = 0; u < UR; ++u) {
                const int r = rb + u * RL;
                g[u] = ld4(Gp + (int64_t)(r < nrows ? r : rb) * ldg);
            }
#pragma unroll
            for (int u = 0; u < UR; ++u) {
                const int r = rb + u * RL;
                if (r >= nrows) continue;
                const float* xr = sk_smem + r * XP;
                const float gv[4] = {g[u].x, g[u].y, g[u].z, g[u].w};
                const float w = xr[KP];
#pragma unroll
                for (int q = 0; q < KP / 4; ++q) {
                    const float4 xv = *reinterpret_cast<const float4*>(xr + q * 4);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        acc[c][4 * q + 0] += gv[c] * xv.x;
                        acc[c][4 * q + 1] += gv[c] * xv.y;
                        acc[c][4 * q + 2] += gv[c] * xv.z;
                        acc[c][4 * q + 3] += gv[c] * xv.w;
                    }
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c][KP] += gv[c] * w;
            }
        }
    }
    __syncthreads();                                                          // (the X image is dead: its space takes the column sums)
    // row lanes in order: row lane 0 stores its sums into the block's [Nc][KP + 1] image, 1 .. RL - 1 add in turn (fixed order)
    for (int t = 0; t < RL; ++t) {
        if (live && rl == t) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int k = 0; k <= KP; ++k) {
                    float* dst = sk_smem + (cl * 4 + c) * (KP + 1) + k;
                    *dst = t == 0 ? acc[c][k] : *dst + acc[c][k];
                }
        }
        __syncthreads();
    }
    float* out = slab + (int64_t)blockIdx.x * tn_chunk_stride(Nc, Kq);
    for (int i = threadIdx.x; i < Nc * Kq; i += BLOCK) {
        const int c = i / Kq, k = i % Kq;
        out[i] = k < K ? sk_smem[c * (KP + 1) + k] : 0.f;
    }
    if (has_bias)
        for (int c = threadIdx.x; c < Nc; c += BLOCK) out[(int64_t)Nc * Kq + c] = sk_smem[c * (KP + 1) + KP];
}
inline bool tn_skinny_shape(int storage, int Nc, int K, int64_t ldg, int64_t ldx, const void* G, const void* X) {
    return storage == 0 && K <= 16 && K % 4 == 0 && Nc % 4 == 0 && Nc >= 64 && Nc <= 4 * BLOCK && ldg % 4 == 0 && ldx % 4 == 0 &&
           stin_aligned16(G) && stin_aligned16(X);
}
inline int tn_skinny_rows(int64_t M) {                                         // ~1024 chunks, a multiple of 32 rows, at least 128
    constexpr int want = 1024;                                                  // measured: 256 / 512 / 1024 / 2048 chunks: 106 / 75 / 72 / 79 us at 200 704 x 320 x 12
    int64_t rows = (M + want - 1) / want;
    rows = (rows + 31) / 32 * 32;
    // the chunk's [X | w] image is rows x (KP + 4 <= 20) floats of dynamic LDS: capped at 512 rows = 40 KB (below the 64 KB a
    // launch gets without hipFuncSetAttribute) - beyond ~0.5 M rows the chunk COUNT grows instead of the chunk
    // (stin_gemm_tn_workspace_bytes sizes the slab from the same function)
    if (rows > 512) rows = 512;
    return (int)(rows < 128 ? 128 : rows);
}

// dW[row][col] = sum_c slab[c][row][col] (and the bias column from the chunk's bias block): 16 chunk-lanes x 16 float4
// groups per block, each chunk-lane walks the chunk list with stride 16 (4 x 16-byte loads in flight), then a
// fixed-order LDS reduction over the chunk-lanes -> deterministic.
constexpr int RS_COLS = 16, RS_KL = 16;
__device__ __forceinline__ void add4(float4& a, const float4 b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__global__ __launch_bounds__(BLOCK) void k_reduce_slabs(const float* __restrict__ slab, int64_t chunks, int Nc, int K, int Kq,
                                                        int has_bias, float* __restrict__ out, int64_t ldo,
                                                        float* __restrict__ bias_out) {
    __shared__ float4 sm[RS_KL][RS_COLS + 1];
    const int tx = threadIdx.x % RS_COLS, ty = threadIdx.x / RS_COLS;
    const int64_t cs = tn_chunk_stride(Nc, Kq);
    const int64_t nw4 = (int64_t)Nc * Kq / 4, nb4 = has_bias ? (Nc + 3) / 4 : 0;
    const int64_t g = (int64_t)blockIdx.x * RS_COLS + tx;          // float4 group: weight block first, then the bias block
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
    if (g < nw4 + nb4) {
        const float* p = slab + 4 * g;
        int64_t c = ty;
        for (; c + 15 * RS_KL < chunks; c += 16 * RS_KL) {          // (sixteen loads in flight on long chunk lists; same addition order)
            float4 v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = ld4(p + (c + u * RS_KL) * cs);
#pragma unroll
            for (int u = 0; u < 16; u += 4) {
                add4(s0, v[u]);
                add4(s1, v[u + 1]);
                add4(s2, v[u + 2]);
                add4(s3, v[u + 3]);
            }
        }
        for (; c + 3 * RS_KL < chunks; c += 4 * RS_KL) {
            add4(s0, ld4(p + c * cs));
            add4(s1, ld4(p + (c + RS_KL) * cs));
            add4(s2, ld4(p + (c + 2 * RS_KL) * cs));
            add4(s3, ld4(p + (c + 3 * RS_KL) * cs));
        }
        for (; c < chunks; c += RS_KL) add4(s0, ld4(p + c * cs));
    }
    add4(s0, s1);
    add4(s2, s3);
    add4(s0, s2);
    sm[ty][tx] = s0;
    __syncthreads();
    if (ty == 0 && g < nw4 + nb4) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < RS_KL; ++k) add4(s, sm[k][tx]);
        const float v[4] = {s.x, s.y, s.z, s.w};
        if (g < nw4) {
            const int64_t row = (4 * g) / Kq;
            const int col = (int)((4 * g) % Kq);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (col + e < K) out[row * ldo + col + e] = v[e];
        } else {
            const int64_t i = 4 * (g - nw4);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < Nc) {
                    if (bias_out != nullptr) bias_out[i + e] = v[e];          // (stin_gemm_tn_wb_*: db as its own vector)
                    else out[(i + e) * ldo + K] = v[e];
                }
        }
    }
}

inline int tn_tile(int n) {
    return n > 64 ? 128 : 64;    // (measured: 64x64 wgrad tiles are 2-5 % slower end to end at any slab count)
}

inline int stin_cu_count() { return stin_cu_count_dev(); }          // (per device: stin_common.h)

inline int tn_rows_per_chunk(int64_t M, int tiles, bool one_per_cu = false) {
    // ~384 blocks (up to 2 resident per CU, one round), chunks a multiple of the LDS slab.  Round 1 measured 512 best of
    // 256..1536; with loads two slabs ahead a block hides more latency by itself and fewer chunks mean fewer partial slabs to
    // store and reduce: 384 is 0.3-0.5 % faster on the step than 512 (256: 0.4 % slower)
    // one_per_cu (round 3: fp32 bf16x3 products on 128 x 128 tiles with M <= 32 k rows, the shapes of the bottleneck level):
    // 256 blocks - the producer / consumer kernel's fixed cost per block (first-load latency ~5 k cycles, slab store ~9 k) is
    // a sixth of a 750-row chunk; measured 18 063 x 1024 x 256 49.7 -> 45.7 us, block weight gradients 69 -> 62 us, while the
    // 60 k-row products lose 10 % with 256 blocks and keep 384
    const int want = one_per_cu ? 256 : 384;
    int64_t chunks = (want + tiles - 1) / tiles;
    if (chunks > 8) chunks = (chunks + 7) / 8 * 8;          // whole rounds of 8 chunks (one per XCD, see the kernels' block map)
    int64_t rows = (M + chunks - 1) / chunks;
    if (rows < 4 * TN_R) rows = 4 * TN_R;
    constexpr int max_rows = 128 * TN_R;
    if (rows > max_rows) rows = max_rows;
    rows = (rows + TN_R - 1) / TN_R * TN_R;
    return (int)rows;
}
// bf16-storage TN: 256 x 256 tiles (k_gemm_tn_b16_tr<2, 4, 4, 2>) for the fat products.  STIN_TN_BIG = 0 | 1 forces (re-read per call;
// the workspace bound covers both choices).
inline bool tn_b16_big_tile(int Nc, int K) {
    const char* e = getenv("STIN_TN_BIG");
    if (e) return atoi(e) != 0 && Nc >= 256 && K >= 256;
    return Nc >= 512 && K >= 512;
}
// bf16-storage TN, 128 x 128 tiles: the transposed-read kernel (k_gemm_tn_b16_tr); STIN_TN_TR=0 keeps the register-transpose
// kernel (A/B switch, re-read per call).
inline bool tn_b16_tr_enabled(int Nc, int K) {
    const char* e = getenv("STIN_TN_TR");
    if (e) return atoi(e) != 0;
    // whole tiles only: with a ragged third tile (161 362 x 320 x 128, the level-0 product of the crop batches) the 64 KB of LDS
    // (two blocks per CU instead of four) cost more than the transposes: 54.6 -> 68.6 us; whole-tile shapes gain 5-17 %
    return Nc % 128 == 0 && K % 128 == 0;
}
inline bool tn_one_per_cu(int storage, int precision, int TI, int TJ, int64_t M) {
    return storage == 0 && precision == STIN_GEMM_BF16X3 && TI == 128 && TJ == 128 && M <= 32768;
}

