// TN products with K <= 16 (k_gemm_tn_skinny) and the slab reduction (k_reduce_slabs).  The host rules: gemm_tn_route.inc.
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

// dW[row][col] = sum_c slab[c][row][col] (and the bias column from the chunk's bias block): 16 chunk-lanes x 16 float4
// groups per block, each chunk-lane folds its share of the chunk list (fn_partial, stin_common.h: the fold of k_wgrad_finalize),
// then a fixed-order LDS reduction over the chunk-lanes -> deterministic.
__global__ __launch_bounds__(BLOCK) void k_reduce_slabs(const float* __restrict__ slab, int64_t chunks, int Nc, int K, int Kq,
                                                        int has_bias, float* __restrict__ out, int64_t ldo,
                                                        float* __restrict__ bias_out) {
    __shared__ float4 sm[FN_KL][FN_COLS + 1];
    const int tx = threadIdx.x % FN_COLS, ty = threadIdx.x / FN_COLS;
    const int64_t nw4 = (int64_t)Nc * Kq / 4, nb4 = has_bias ? (Nc + 3) / 4 : 0;
    const int64_t g = (int64_t)blockIdx.x * FN_COLS + tx;          // float4 group: weight block first, then the bias block
    sm[ty][tx] = fn_partial(g < nw4 + nb4 ? slab + 4 * g : nullptr, tn_chunk_stride(Nc, Kq), chunks, ty);
    __syncthreads();
    if (ty == 0 && g < nw4 + nb4) {
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int k = 0; k < FN_KL; ++k) add4(s, sm[k][tx]);
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
