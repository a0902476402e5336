// TN (weight-gradient) products of fp32 rows: exact-fp32 and split-bf16 tilings (k_gemm_tn, k_gemm_tn_bf16s)
// Part of stin_gemm.hip (included inside its anonymous namespace; not a translation unit of its own).
// ----------------------------------------------------------------------------- TN
// dW tile TI x TJ per 256-thread block, reduction over a chunk of rows m.  Both operands are
// row-major with m as the slow index, so a 32-row slab of G (TI columns) and X (TJ columns) is staged
// in LDS exactly as it lies in memory (16-byte global loads, ds_write_b128, double buffered, the next
// slab's loads in flight during the MFMAs) and the MFMA fragments are stride-1 ds_read_b32:
// A[i][k] = Gs[k][i], B[k][j] = Xs[k][j] with k = the row inside the slab.  4 waves as 2 x 2, each
// (TI/2) x (TJ/2).  The bias gradient sum_m w[m] G[m, :] is accumulated on the VALU by the staging
// threads of the j-tile-0 blocks.  Partial tiles go to the chunk block of the slab workspace (tn_chunk_stride); k_reduce_slabs adds them
// in a fixed order.  Blocks are numbered so that all tiles of one row chunk share an XCD
// (blockIdx % 8 is the observed XCD round-robin): the chunk's rows are re-read from that L2.
constexpr int TN_R = 32;   // rows per LDS slab
// One chunk's partial result in the slab workspace: the weight block [Nc][Kq] (Kq = K rounded up to 4: rows stay
// 16-byte aligned, and 128-byte aligned for the usual K % 32 == 0, so the tile stores are whole cache lines) followed
// by the bias-gradient partials [Nc] - NOT an odd-pitched [Nc][K + 1] matrix.
__host__ __device__ __forceinline__ int64_t tn_chunk_stride(int Nc, int Kq) { return (int64_t)Nc * Kq + ((Nc + 3) & ~3); }

template <int TI, int TJ, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_gemm_tn(const float* __restrict__ G, int64_t ldg,
                                                   const float* __restrict__ X, int64_t ldx, int64_t M, int Nc,
                                                   int K, int Kq, int has_bias, const float* __restrict__ row_w, int64_t ld_w,
                                                   int rows_per_chunk, int tiles_i, int tiles_j, int64_t chunks,
                                                   float* __restrict__ slab, const stin_bn_tf xtf) {
    constexpr int MT = TI / 64, NT = TJ / 64;                    // 32x32 MFMA tiles per wave
    constexpr int GF4 = TN_R * TI / 4 / BLOCK, XF4 = TN_R * TJ / 4 / BLOCK;   // float4 per thread per slab
    constexpr int GC4 = TI / 4, XC4 = TJ / 4;                    // float4 columns
    __shared__ float Gs[2][TN_R][TI];
    __shared__ float Xs[2][TN_R][TJ];
    __shared__ float bsum[BLOCK / GC4][TI + 4];

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
    float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);

    const int gc = tid % GC4, gr = tid / GC4;    // staging coordinates in the G slab (rows gr + s * BLOCK/GC4)
    const int xc = tid % XC4, xr = tid / XC4;
    float4 rg[GF4], rx[XF4];
    float rwt[GF4];

    stin_bn_coef4 xq;                                                  // (s, t) of this thread's fixed X columns (transform at STORE time)
    xq.s = xq.t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (xtf.mean != nullptr) {
        float* sp = reinterpret_cast<float*>(&xq.s);
        float* tp = reinterpret_cast<float*>(&xq.t);
#pragma unroll
        for (int e = 0; e < 4; ++e) stin_bn_st(xtf, j0 + xc * 4 + e < K ? j0 + xc * 4 + e : 0, sp[e], tp[e]);
    }
    auto load_slab = [&](int64_t m0) {
#pragma unroll
        for (int s = 0; s < GF4; ++s) {
            const int64_t row = m0 + gr + s * (BLOCK / GC4);
            const int col = i0 + gc * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            float w = 0.f;
            if (row < me) {
                const float* p = G + row * ldg + col;
                if (VEC) {
                    if (col < Nc) v = ld4(p);
                } else {
                    if (col + 0 < Nc) v.x = p[0];
                    if (col + 1 < Nc) v.y = p[1];
                    if (col + 2 < Nc) v.z = p[2];
                    if (col + 3 < Nc) v.w = p[3];
                }
                if (want_bias) w = row_w != nullptr ? row_w[row * ld_w] : 1.f;
            }
            rg[s] = v;
            rwt[s] = w;
        }
#pragma unroll
        for (int s = 0; s < XF4; ++s) {
            const int64_t row = m0 + xr + s * (BLOCK / XC4);
            const int col = j0 + xc * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < me) {
                const float* p = X + row * ldx + col;
                if (VEC) {
                    if (col < K) v = ld4(p);
                } else {
                    if (col + 0 < K) v.x = p[0];
                    if (col + 1 < K) v.y = p[1];
                    if (col + 2 < K) v.z = p[2];
                    if (col + 3 < K) v.w = p[3];
                }
            }
            rx[s] = v;
        }
    };
    auto store_slab = [&](int buf) {
#pragma unroll
        for (int s = 0; s < GF4; ++s) {
            st4(&Gs[buf][gr + s * (BLOCK / GC4)][gc * 4], rg[s]);
            bs.x += rwt[s] * rg[s].x;
            bs.y += rwt[s] * rg[s].y;
            bs.z += rwt[s] * rg[s].z;
            bs.w += rwt[s] * rg[s].w;
        }
#pragma unroll
        for (int s = 0; s < XF4; ++s) st4(&Xs[buf][xr + s * (BLOCK / XC4)][xc * 4], xtf.mean != nullptr ? stin_bn_relu4(rx[s], xq) : rx[s]);
    };

    const int kh = lane >> 5, li = lane & 31;
    load_slab(mb);
    store_slab(0);
    __syncthreads();
    int buf = 0;
    for (int64_t m0 = mb; m0 < me; m0 += TN_R) {
        const bool more = m0 + TN_R < me;
        if (more) load_slab(m0 + TN_R);                           // in flight during the MFMAs
#pragma unroll
        for (int kk = 0; kk < TN_R; kk += 2) {
            float a[MT], c[NT];
#pragma unroll
            for (int t = 0; t < MT; ++t) a[t] = Gs[buf][kk + kh][wi * (TI / 2) + t * 32 + li];
#pragma unroll
            for (int t = 0; t < NT; ++t) c[t] = Xs[buf][kk + kh][wj * (TJ / 2) + t * 32 + li];
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], c[u], acc[t][u], 0, 0, 0);
        }
        if (more) store_slab(buf ^ 1);                            // the other buffer: last read one iteration ago
        __syncthreads();
        buf ^= 1;
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
    if (want_bias) {                                              // block-uniform branch
        st4(&bsum[gr][gc * 4], bs);
        __syncthreads();
        if (tid < TI) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < BLOCK / GC4; ++r) t += bsum[r][tid];
            if (i0 + tid < Nc) out[(int64_t)Nc * Kq + i0 + tid] = t;
        }
    }
}

// ------------------------------------------------------------------- TN, split-bf16
// Same contract as k_gemm_tn on the bf16 matrix cores.  The reduction index is the ROW m, so the MFMA
// fragments need 8 consecutive m for one column: each staging thread loads a 4(rows) x 4(cols) fp32 patch
// (4 x 16-byte loads), splits it into NS bf16 pieces, transposes it in registers and writes one 8-byte
// (4 consecutive m) run per column into Gt[piece][col][m] / Xt[piece][col][m] (row pitch 80 B; lanes of a
// 16-lane group differ in the row group first => conflict-free ds_write_b64 and ds_read_b128).
constexpr int TNB_R = 32;                  // rows (m) per LDS slab = two MFMA k-steps of 16
constexpr int TNB_PITCH = TNB_R + 8;       // bf16 per LDS row (80 bytes)

template <int TI, int TJ, int NS, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_gemm_tn_bf16s(const float* __restrict__ G, int64_t ldg,
                                                         const float* __restrict__ X, int64_t ldx, int64_t M,
                                                         int Nc, int K, int Kq, int has_bias, const float* __restrict__ row_w,
                                                         int64_t ld_w, int rows_per_chunk, int tiles_i, int tiles_j,
                                                         int64_t chunks, float* __restrict__ slab, const stin_bn_tf xtf) {
    constexpr int MT = TI / 64, NT = TJ / 64;
    constexpr int ITEMS = 2 * (TI + TJ);                          // 4x4 patches per slab (G then X)
    constexpr int PASSES = ITEMS / BLOCK;                          // 1, 1.5 -> handled as 2 with a guard, or 2
    constexpr int NPASS = (ITEMS + BLOCK - 1) / BLOCK;
    __shared__ __attribute__((aligned(16))) __bf16 Gt[NS][TI][TNB_PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 Xt[NS][TJ][TNB_PITCH];
    __shared__ float bsum[8][TI + 4];
    (void)PASSES;

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
    float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);                  // bias-gradient partial (columns of this thread's G patch)

    // Two register sets (128x128 tiles): the loads of slab s + 2 are issued while slab s multiplies - one slab of cover (24 MFMAs
    // = 0.35 us per wave) is less than an HBM / Infinity-Cache load takes under load.  Pays for M >= 60 k; at M = 18 k the
    // kernel is bound by the LDS round trip of the transposing split (2 barriers, 32 KB written + 64 KB read per slab), not by loads.
    struct Slab {
        float4 patch[NPASS][4];
        float pw[4];
        bool pv[4];
    };
    Slab S0, S1;
    stin_bn_coef4 xq[NPASS];                                       // (s, t) of the X patches' columns: fixed per thread and pass
    if (xtf.mean != nullptr) {                                     // (the transform itself runs at STORE time, see k_gemm_nt_bf16s)
#pragma unroll
        for (int s = 0; s < NPASS; ++s) {
            const int item = tid + s * BLOCK;
            const int c = j0 + ((item >= 2 * TI ? item - 2 * TI : 0) / 8) * 4;
            float* sp = reinterpret_cast<float*>(&xq[s].s);
            float* tp = reinterpret_cast<float*>(&xq[s].t);
#pragma unroll
            for (int e = 0; e < 4; ++e) stin_bn_st(xtf, c + e < K ? c + e : 0, sp[e], tp[e]);
        }
    }
    auto load_slab = [&](Slab& P, int64_t m0) {
#pragma unroll
        for (int s = 0; s < NPASS; ++s) {
            const int item = tid + s * BLOCK;
            const bool isG = item < 2 * TI;
            const int it = isG ? item : item - 2 * TI;
            const int rg = it % 8, c4 = it / 8;
            const bool live = item < ITEMS;
            const float* base = isG ? G : X;
            const int64_t ld = isG ? ldg : ldx;
            const int col = (isG ? i0 : j0) + c4 * 4;
            const int lim = isG ? Nc : K;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = m0 + rg * 4 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live && row < me) {
                    const float* p = base + row * ld + col;
                    if (VEC) {
                        if (col < lim) v = ld4(p);
                    } else {
                        if (col + 0 < lim) v.x = p[0];
                        if (col + 1 < lim) v.y = p[1];
                        if (col + 2 < lim) v.z = p[2];
                        if (col + 3 < lim) v.w = p[3];
                    }
                }
                P.patch[s][r] = v;
                // row weight of the bias-gradient column: a PLAIN load (clamped row, no select on the loaded value), so that
                // the compiler does not have to drain the prefetched patch loads before the MFMAs; masked in store_slab
                if (s == 0) {
                    const int64_t rc = row < me ? row : me - 1;
                    const float* wp = (want_bias && row_w != nullptr) ? row_w + rc * ld_w : G;   // always a valid address
                    P.pw[r] = *wp;
                    P.pv[r] = row < me;
                }
            }
        }
    };
    auto store_slab = [&](const Slab& P) {
#pragma unroll
        for (int s = 0; s < NPASS; ++s) {
            const int item = tid + s * BLOCK;
            if (item >= ITEMS) continue;
            const bool isG = item < 2 * TI;
            const int it = isG ? item : item - 2 * TI;
            const int rg = it % 8, c4 = it / 8;
            if (s == 0 && isG) {                                   // 2*TI >= 128: pass 0 holds every G patch of TI=128; see below for TI=64
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float w = (want_bias && P.pv[r]) ? (row_w != nullptr ? P.pw[r] : 1.f) : 0.f;
                    bs.x += w * P.patch[s][r].x;
                    bs.y += w * P.patch[s][r].y;
                    bs.z += w * P.patch[s][r].z;
                    bs.w += w * P.patch[s][r].w;
                }
            }
            __bf16* dst = isG ? &Gt[0][c4 * 4][rg * 4] : &Xt[0][c4 * 4][rg * 4];
            const int plane = (isG ? TI : TJ) * TNB_PITCH;
            float4 pr[4] = {P.patch[s][0], P.patch[s][1], P.patch[s][2], P.patch[s][3]};
            if (!isG && xtf.mean != nullptr) {
#pragma unroll
                for (int r = 0; r < 4; ++r) pr[r] = stin_bn_relu4(pr[r], xq[s]);
            }
            float col[4][4] = {{pr[0].x, pr[1].x, pr[2].x, pr[3].x},
                               {pr[0].y, pr[1].y, pr[2].y, pr[3].y},
                               {pr[0].z, pr[1].z, pr[2].z, pr[3].z},
                               {pr[0].w, pr[1].w, pr[2].w, pr[3].w}};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
#pragma unroll
                for (int p = 0; p < NS; ++p) {
                    bf16x4 h;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        h[r] = (__bf16)col[c][r];
                        col[c][r] -= (float)h[r];
                    }
                    *reinterpret_cast<bf16x4*>(dst + p * plane + c * TNB_PITCH) = h;
                }
            }
        }
    };

    const int kh = lane >> 5, li = lane & 31;
    auto multiply = [&]() {
#pragma unroll
        for (int ks = 0; ks < TNB_R; ks += 16) {
            bf16x8 a[NS][MT], c[NS][NT];
#pragma unroll
            for (int p = 0; p < NS; ++p) {
#pragma unroll
                for (int t = 0; t < MT; ++t)
                    a[p][t] = *reinterpret_cast<const bf16x8*>(&Gt[p][wi * (TI / 2) + t * 32 + li][ks + 8 * kh]);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    c[p][t] = *reinterpret_cast<const bf16x8*>(&Xt[p][wj * (TJ / 2) + t * 32 + li][ks + 8 * kh]);
            }
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    if (NS == 3) {
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][t], c[1][u], acc[t][u], 0, 0, 0);
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][t], c[2][u], acc[t][u], 0, 0, 0);
                        acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2][t], c[0][u], acc[t][u], 0, 0, 0);
                    }
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][t], c[1][u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1][t], c[0][u], acc[t][u], 0, 0, 0);
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][t], c[0][u], acc[t][u], 0, 0, 0);
                }
        }
    };
    // 128x128 tiles only: the second register set costs the narrower tiles a wave of occupancy (measured: 200 704 x 320 x 12
    // 91 -> 118 us with it, while 60 211 x 640 x 256 goes 161 -> 139 and 200 704 x 320 x 128 186 -> 143)
    constexpr bool DEEP = (TI == 128 && TJ == 128);
    load_slab(S0, mb);
    if (DEEP) {
        load_slab(S1, mb + TNB_R);                                 // (rows >= me load nothing)
        // (branch-free body: with an odd slab count the last half-iteration multiplies a slab of zeros)
        auto step = [&](Slab& P, int64_t m0) {
            __syncthreads();                                       // previous slab's fragment reads are done
            store_slab(P);
            __syncthreads();
            load_slab(P, m0 + 2 * TNB_R);                          // two slabs ahead
            multiply();
        };
        for (int64_t m0 = mb; m0 < me; m0 += 2 * TNB_R) {
            step(S0, m0);
            step(S1, m0 + TNB_R);
        }
    } else {
        for (int64_t m0 = mb; m0 < me; m0 += TNB_R) {
            __syncthreads();
            store_slab(S0);
            __syncthreads();
            if (m0 + TNB_R < me) load_slab(S0, m0 + TNB_R);        // next slab's global loads in flight during the MFMAs
            multiply();
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
        // pass-0 G patches: item = tid < 2*TI, row group tid % 8, column group tid / 8
        if (tid < 2 * TI) st4(&bsum[tid % 8][(tid / 8) * 4], bs);
        __syncthreads();
        if (tid < TI) {
            float t = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) t += bsum[r][tid];
            if (i0 + tid < Nc) out[(int64_t)Nc * Kq + i0 + tid] = t;
        }
    }
}

